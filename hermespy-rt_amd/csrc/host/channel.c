/* channel.c -- channel frequency responses, impulse responses, power statistics and the strongest paths from traced
 * paths, on the device (include/hrt_device.h: hrt_channel, hrt_array_channel, hrt_taps, hrt_array_taps,
 * hrt_power_profiles, hrt_dominant_paths, hrt_beam_channel, hrt_beam_taps, hrt_array_covariance, hrt_propagate,
 * hrt_channel_svd, hrt_channel_equalizer, hrt_channel_precoder, hrt_codebook_select, hrt_channel_detect, hrt_channel_kbest, hrt_sparse_array_channel, hrt_sparse_array_taps, hrt_sparse_beam_channel,
 * hrt_sparse_beam_taps;
 * include/hermespy_rt.h: hrt_compute_array_covariance, hrt_compute_received_signal, hrt_compute_channel,
 * hrt_compute_array_channel, hrt_compute_taps, hrt_compute_array_taps, hrt_compute_power_profiles,
 * hrt_compute_dominant_paths, hrt_compute_beam_channel, hrt_compute_beam_taps, hrt_compute_sparse_array_channel,
 * hrt_compute_sparse_array_taps, hrt_compute_sparse_beam_channel, hrt_compute_sparse_beam_taps).
 *
 *     H[rx, tx, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p))
 *
 * over the LoS entry and the scatter records of every (rx, tx) -- the sum a HermesPy caller forms on the host
 * from compute_paths()'s per-path arrays, formed where the records already are: of C3's 2.3 GB of dense host
 * arrays only nrx * ntx * 2 * T * K complex values leave the device.  The kernels are in csrc/hrt_channel.hip,
 * csrc/hrt_array_channel.hip, csrc/hrt_taps.hip, csrc/hrt_array_taps.hip, csrc/hrt_power.hip,
 * csrc/hrt_dominant.hip, csrc/hrt_beam_channel.hip, csrc/hrt_beam_taps.hip and csrc/hrt_covariance.hip, over the workspace view of
 * csrc/hrt_pathsum.h.  The two pair
 * families (hrt_array_channel: element pairs, hrt_beam_channel: beam pairs) share one grid (hrt_kgrid, pair_grid) as
 * their kernels share one GEMM body (csrc/hrt_pair_gemm.inc), and the array and beam drop-ins one packing of the
 * element offsets (ac_pack_offsets).  The drop-in entries run the batch loop of batch.c, with one device output
 * accumulated over the batches and one small download at the end.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "hrt_internal.h"
#include "../hrt_array_channel.h"
#include "../hrt_array_taps.h"
#include "../hrt_beam_channel.h"
#include "../hrt_beam_taps.h"
#include "../hrt_channel.h"
#include "../hrt_codebook.h"
#include "../hrt_covariance.h"
#include "../hrt_detect.h"
#include "../hrt_dominant.h"
#include "../hrt_equalizer.h"
#include "../hrt_kbest.h"
#include "../hrt_pathsum.h"
#include "../hrt_patterns.h"
#include "../hrt_power.h"
#include "../hrt_precoder.h"
#include "../hrt_propagate.h"
#include "../hrt_sparse_beam.h"
#include "../hrt_sparse_beam_taps.h"
#include "../hrt_sparse_channel.h"
#include "../hrt_sparse_taps.h"
#include "../hrt_svd.h"
#include "../hrt_taps.h"

/* ------------------------------------------------------------------ what the path-sum families share (hrt_pathsum.h) */

#define HRT_CH_MIN_CHUNK 512u                /* records of one TX segment per chunk, at least */

static int parts_check(uint32_t parts, const char *who)
{
    if (parts == 0 || (parts & ~(uint32_t)(HRT_CHANNEL_LOS | HRT_CHANNEL_SCATTER)))
        return hrt_fail(HRT_E_INVALID, "%s: parts 0x%x (HRT_CHANNEL_LOS | HRT_CHANNEL_SCATTER)", who, parts);
    return HRT_OK;
}

/* the workspace view of one call: the layout of the shard, the counts and the LoS rule (shard rank 0 adds the LoS
 * term, so the shards of one launch set sum to the whole response); nchunks 0 */
static int ps_view(const hrt_problem *p, const hrt_shard *s, uint32_t parts, const char *who, hrt_kview *v)
{
    if (!p || !s) return hrt_fail(HRT_E_INVALID, "%s: NULL argument", who);
    hrt_layout L;
    int rc = hrt_layout_query(p, s, &L);
    if (rc) return rc;
    const uint64_t links = (uint64_t)p->num_rx * p->num_tx;
    if (links > 65535u)
        return hrt_fail(HRT_E_INVALID, "%s: num_rx * num_tx = %llu > 65535", who, (unsigned long long)links);
    memset(v, 0, sizeof *v);
    v->cap = L.cap; v->off_counts = L.off_counts; v->off_los = L.off_los; v->off_hits = L.off_hits;
    v->hit_block_bytes = L.hit_block_bytes; v->off_recs = L.off_recs; v->rec_block_bytes = L.rec_block_bytes;
    v->off_masks = L.off_masks;
    v->nb = s->num_bounces; v->nrx = p->num_rx; v->ntx = p->num_tx;
    v->num_local = (uint32_t)hrt_shard_num_local(s);
    v->los = (parts & HRT_CHANNEL_LOS) && s->rank == 0;
    return HRT_OK;
}

/* the shard of the trace, for the kernels that form a record's departure direction from its global path */
static void ps_shard(const hrt_shard *s, hrt_kshard *k)
{
    k->num_paths = s->num_paths;
    k->rank = s->rank; k->count = s->count; k->chunk = s->chunk ? s->chunk : 4096u;
}

/* the scratch of one call: seg, then nchunks * per_chunk bytes of partial sums */
static uint64_t ps_seg_bytes(const hrt_kview *v)
{
    return ((uint64_t)v->nb * (v->ntx + 1u) * 4u + 255u) / 256u * 256u;
}

/* The record chunks per (link, block) of the scatter part, where the call has one (v->nchunks stays 0 otherwise):
 * enough of the `groups` blocks per chunk to reach target_groups, chunks of at least HRT_CH_MIN_CHUNK records,
 * partial sums of at most partial_max bytes (but one chunk always), and at most y_max (the chunks' grid dimension).
 * Returns the scratch of the call: seg, then the partial sums. */
static uint64_t ps_chunks(hrt_kview *v, uint32_t parts, uint64_t groups, uint64_t target_groups, uint64_t per_chunk,
                          uint64_t partial_max, uint64_t y_max)
{
    if ((parts & HRT_CHANNEL_SCATTER) && v->nb > 0) {
        uint64_t nch = (target_groups + groups - 1) / groups;
        const uint64_t by_recs = v->num_local / HRT_CH_MIN_CHUNK;
        if (nch > by_recs) nch = by_recs;
        if (nch > partial_max / per_chunk) nch = partial_max / per_chunk;
        if (nch > y_max) nch = y_max;
        if (nch < 1) nch = 1;
        v->nchunks = (uint32_t)nch;
    }
    return ps_seg_bytes(v) + v->nchunks * per_chunk;
}

static int ps_scratch_out(int rc, uint64_t bytes, uint64_t *out, const char *query)
{
    if (rc) return rc;
    if (!out) return hrt_fail(HRT_E_INVALID, "%s: NULL out", query);
    *out = bytes;
    return HRT_OK;
}

/* the device buffers of one call, once its plan needs `need` bytes of scratch (`query` names the size query) */
static int ps_bind(hrt_kview *v, uint64_t need, const void *d_workspace, void *d_scratch, uint64_t scratch_bytes,
                   const void *d_out, int accumulate, const char *who, const char *query, float **partial)
{
    if (!d_workspace || !d_out || !d_scratch)
        return hrt_fail(HRT_E_INVALID, "%s: NULL workspace, scratch or output", who);
    if (scratch_bytes < need)
        return hrt_fail(HRT_E_INVALID, "%s: scratch of %llu bytes, %llu needed (%s)", who,
                        (unsigned long long)scratch_bytes, (unsigned long long)need, query);
    if (accumulate != 0 && accumulate != 1) return hrt_fail(HRT_E_INVALID, "%s: accumulate must be 0 or 1", who);
    v->ws = (const uint8_t *)d_workspace;
    v->accumulate = (uint32_t)accumulate;
    v->seg = (uint32_t *)d_scratch;
    *partial = (float *)((uint8_t *)d_scratch + ps_seg_bytes(v));
    return HRT_OK;
}

/* ------------------------------------------------------------------ frequency responses (hrt_channel) */

#define HRT_CH_MAX_POINTS (1u << 20)         /* num_freqs * num_times */
#define HRT_CH_TARGET_GROUPS 8192u           /* waves of the partial kernel worth launching (32 per CU) */
#define HRT_CH_PARTIAL_MAX (512ull << 20)    /* partial sums beyond one chunk per tile: at most this */

static int spec_check(const hrt_channel_spec *spec)
{
    if (!spec) return hrt_fail(HRT_E_INVALID, "hrt_channel: NULL spec");
    if (spec->num_freqs == 0 || spec->num_times == 0)
        return hrt_fail(HRT_E_INVALID, "hrt_channel: num_freqs and num_times must be > 0");
    if ((uint64_t)spec->num_freqs * spec->num_times > HRT_CH_MAX_POINTS)
        return hrt_fail(HRT_E_INVALID, "hrt_channel: num_freqs * num_times = %llu > 2^20",
                        (unsigned long long)spec->num_freqs * spec->num_times);
    int rc = parts_check(spec->parts, "hrt_channel");
    if (rc) return rc;
    if (!isfinite(spec->f0_hz) || !isfinite(spec->df_hz) || !isfinite(spec->t0_s) || !isfinite(spec->dt_s))
        return hrt_fail(HRT_E_INVALID, "hrt_channel: f0, df, t0 and dt must be finite");
    return HRT_OK;
}

/* the tiling of one call: a pure function of the problem, the shard and the spec (so the sums, and their
 * order, do not depend on anything else) */
static int ch_plan(const hrt_problem *p, const hrt_shard *s, const hrt_channel_spec *spec, hrt_kchannel *K,
                   uint64_t *bytes)
{
    int rc = spec_check(spec);
    if (rc) return rc;
    memset(K, 0, sizeof *K);
    if ((rc = ps_view(p, s, spec->parts, "hrt_channel", &K->v))) return rc;
    K->K = spec->num_freqs; K->T = spec->num_times;
    K->K1 = (spec->num_freqs + HRT_CH_K2 - 1) / HRT_CH_K2;
    K->rows = K->K1 * K->T;
    K->tiles = (K->rows + HRT_CH_ROWS - 1) / HRT_CH_ROWS;
    K->f0 = spec->f0_hz; K->df = spec->df_hz; K->t0 = spec->t0_s; K->dt = spec->dt_s;
    const uint64_t links = (uint64_t)K->v.nrx * K->v.ntx;
    const uint64_t per_chunk = links * K->tiles * HRT_CH_TILE_FLOATS * 4u;
    /* (the chunks are grid x: no cap; HRT_CH_MIN_CHUNK keeps them below 2^23) */
    *bytes = ps_chunks(&K->v, spec->parts, links * K->tiles, HRT_CH_TARGET_GROUPS, per_chunk, HRT_CH_PARTIAL_MAX,
                       UINT32_MAX);
    return HRT_OK;
}

int hrt_channel_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_channel_spec *spec, uint64_t *out)
{
    hrt_kchannel K;
    uint64_t bytes = 0;
    const int rc = ch_plan(p, s, spec, &K, &bytes);
    return ps_scratch_out(rc, bytes, out, "hrt_channel_scratch_bytes");
}

int hrt_channel(const hrt_problem *p, const hrt_shard *s, const void *d_workspace, const hrt_channel_spec *spec,
                void *d_scratch, uint64_t scratch_bytes, float *d_out, int accumulate, void *stream)
{
    hrt_kchannel K;
    uint64_t need = 0;
    int rc = ch_plan(p, s, spec, &K, &need);
    if (rc) return rc;
    if ((rc = ps_bind(&K.v, need, d_workspace, d_scratch, scratch_bytes, d_out, accumulate, "hrt_channel",
                      "hrt_channel_scratch_bytes", &K.partial)))
        return rc;
    K.out = d_out;
    HRT_HIP(hrt_hip_set_device(p->device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_channel(&K, stream), "channel kernels");
    return HRT_OK;
}

/* ------------------------------------------------------------------ antenna patterns (hrt_apply_patterns) */

/* the checks of one side's pattern (`side`: "rx" or "tx") of a call (`who`); the table pointer is tested for NULL only */
static int pattern_check(const hrt_pattern *f, const char *side, const char *who)
{
    if (f->kind > HRT_PATTERN_TABLE)
        return hrt_fail(HRT_E_INVALID, "%s: %s kind = %u (HRT_PATTERN_ISOTROPIC .. HRT_PATTERN_TABLE)", who, side, f->kind);
    if (f->kind == HRT_PATTERN_TABLE) {
        if (!f->d_table) return hrt_fail(HRT_E_INVALID, "%s: NULL %s table", who, side);
        if (f->num_zenith < 2 || f->num_zenith > HRT_PT_MAX_ZENITH)
            return hrt_fail(HRT_E_INVALID, "%s: %s num_zenith = %u (2 .. %u)", who, side, f->num_zenith, HRT_PT_MAX_ZENITH);
        if (f->num_azimuth < 1 || f->num_azimuth > HRT_PT_MAX_AZIMUTH)
            return hrt_fail(HRT_E_INVALID, "%s: %s num_azimuth = %u (1 .. %u)", who, side, f->num_azimuth,
                            HRT_PT_MAX_AZIMUTH);
    }
    if (!isfinite(f->gain_db) || fabsf(f->gain_db) > HRT_PT_MAX_GAIN_DB)
        return hrt_fail(HRT_E_INVALID, "%s: %s gain_db must be finite and within +-200 dB", who, side);
    return HRT_OK;
}

static void pattern_fields(const hrt_pattern *f, uint32_t side, hrt_kpatterns *K)
{
    K->kind[side] = f->kind;
    K->g[side] = (float)pow(10.0, (double)f->gain_db / 20.0);
    if (f->kind == HRT_PATTERN_TABLE) {
        K->nz[side] = f->num_zenith; K->na[side] = f->num_azimuth;
        K->table[side] = f->d_table;
    }
}

int hrt_apply_patterns(const hrt_problem *p, const hrt_shard *s, void *d_workspace, uint64_t workspace_bytes,
                       const hrt_pattern_spec *spec, void *stream)
{
    if (!spec) return hrt_fail(HRT_E_INVALID, "hrt_apply_patterns: NULL spec");
    int rc = pattern_check(&spec->rx, "rx", "hrt_apply_patterns");
    if (rc) return rc;
    if ((rc = pattern_check(&spec->tx, "tx", "hrt_apply_patterns"))) return rc;
    if (!p || !s || !d_workspace) return hrt_fail(HRT_E_INVALID, "hrt_apply_patterns: NULL argument");
    hrt_kpatterns K;
    memset(&K, 0, sizeof K);
    if ((rc = ps_view(p, s, HRT_CHANNEL_LOS | HRT_CHANNEL_SCATTER, "hrt_apply_patterns", &K.v))) return rc;
    hrt_layout L;
    if ((rc = hrt_layout_query(p, s, &L))) return rc;
    if (workspace_bytes < L.total_bytes)
        return hrt_fail(HRT_E_INVALID, "hrt_apply_patterns: workspace of %llu bytes, %llu needed (hrt_layout_query)",
                        (unsigned long long)workspace_bytes, (unsigned long long)L.total_bytes);
    ps_shard(s, &K.sh);
    pattern_fields(&spec->rx, 0u, &K);
    pattern_fields(&spec->tx, 1u, &K);
    K.rot[0] = spec->d_rx_rot; K.rot[1] = spec->d_tx_rot;
    K.v.ws = (const uint8_t *)d_workspace;
    HRT_HIP(hrt_hip_set_device(p->device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_patterns(&K, stream), "pattern kernels");
    return HRT_OK;
}

/* the patterns the path-sum drop-ins of this thread apply (hermespy_rt.h: hrt_compute_set_patterns); NULL: none */
static __thread const hrt_patterns_host *g_patterns;

void hrt_compute_set_patterns(const hrt_patterns_host *patterns)
{
    g_patterns = patterns;
}

static uint64_t pattern_table_floats(const hrt_pattern *f)
{
    return f->kind == HRT_PATTERN_TABLE ? (uint64_t)f->num_zenith * f->num_azimuth : 0u;
}

/* the checks of the patterns of a drop-in call with nrx x ntx links: host arrays, so their contents too */
static int patterns_host_check(const hrt_patterns_host *h, size_t nrx, size_t ntx)
{
    const char *who = "hrt_compute_set_patterns";
    int rc = pattern_check(&h->rx, "rx", who);
    if (rc) return rc;
    if ((rc = pattern_check(&h->tx, "tx", who))) return rc;
    for (int side = 0; side < 2; ++side) {
        const hrt_pattern *f = side ? &h->tx : &h->rx;
        for (uint64_t i = 0, n = pattern_table_floats(f); i < n; ++i)
            if (!isfinite(f->d_table[i]) || f->d_table[i] < 0.f)
                return hrt_fail(HRT_E_INVALID, "%s: %s table value %llu is not finite and >= 0", who, side ? "tx" : "rx",
                                (unsigned long long)i);
    }
    if (h->rx_rot && h->num_rx != nrx)
        return hrt_fail(HRT_E_INVALID, "%s: %zu rx rotations, but the call has num_rx = %zu", who, h->num_rx, nrx);
    if (h->tx_rot && h->num_tx != ntx)
        return hrt_fail(HRT_E_INVALID, "%s: %zu tx rotations, but the call has num_tx = %zu", who, h->num_tx, ntx);
    for (size_t i = 0; h->rx_rot && i < 9u * nrx; ++i)
        if (!isfinite(h->rx_rot[i])) return hrt_fail(HRT_E_INVALID, "%s: rx rotation %zu is not finite", who, i / 9u);
    for (size_t i = 0; h->tx_rot && i < 9u * ntx; ++i)
        if (!isfinite(h->tx_rot[i])) return hrt_fail(HRT_E_INVALID, "%s: tx rotation %zu is not finite", who, i / 9u);
    return HRT_OK;
}

/* the patterns of a drop-in call on its device: tables and rotations uploaded to one buffer (*d_buf, the caller's to
 * free), rx table, tx table, rx rotations, tx rotations */
static int patterns_upload(const hrt_patterns_host *h, int device, size_t nrx, size_t ntx, void **d_buf,
                           hrt_pattern_spec *spec)
{
    const uint64_t n[4] = {pattern_table_floats(&h->rx), pattern_table_floats(&h->tx), h->rx_rot ? 9u * nrx : 0u,
                           h->tx_rot ? 9u * ntx : 0u};
    const float *src[4] = {h->rx.d_table, h->tx.d_table, h->rx_rot, h->tx_rot};
    const float *dst[4] = {NULL, NULL, NULL, NULL};
    int rc = hrt_device_malloc(device, d_buf, (n[0] + n[1] + n[2] + n[3] + 1u) * 4u);
    if (rc) return rc;
    float *at = (float *)*d_buf;
    for (int k = 0; k < 4; ++k) {
        if (!n[k]) continue;
        if ((rc = hrt_device_upload(device, at, src[k], n[k] * 4u))) return rc;
        dst[k] = at;
        at += n[k];
    }
    spec->rx = h->rx; spec->tx = h->tx;
    spec->rx.d_table = dst[0]; spec->tx.d_table = dst[1];
    spec->d_rx_rot = dst[2]; spec->d_tx_rot = dst[3];
    return HRT_OK;
}

/* One drop-in call: what the ten hrt_compute_* entries of this file share.  `scratch_bytes` and `run` are
 * the device entry of the call; h_const (const_bytes, may be 0) is uploaded to the device once before the first
 * batch, and `run` finds it at d_const. */
typedef struct ch_job ch_job;
struct ch_job {
    const void *spec;   /* hrt_channel_spec (hrt_compute_channel, hrt_compute_array_channel), hrt_taps_spec
                           (hrt_compute_taps, hrt_compute_array_taps), hrt_power_spec, hrt_dominant_spec or
                           hrt_covariance_spec */
    uint64_t out_bytes;
    const void *h_const;
    uint64_t const_bytes;
    void *d_const;
    int (*scratch_bytes)(const ch_job *j, const hrt_problem *p, const hrt_shard *s, uint64_t *out);
    int (*run)(const ch_job *j, const hrt_problem *p, const hrt_shard *s, const void *d_ws, void *d_scratch,
               uint64_t scratch_bytes, void *d_out, int accumulate);
    uint32_t nr, nt;   /* the array calls' element counts (hrt_compute_array_channel, hrt_compute_array_taps,
                          hrt_compute_beam_channel) */
    double fa;
    uint32_t nbr, nbt; /* the beam calls' beam counts (hrt_compute_beam_channel, hrt_compute_beam_taps) */
    /* optional: runs on the downloaded output while the problem still exists (NULL: nothing to do) */
    int (*finish)(const ch_job *j, const hrt_problem *p, void *out);
    /* optional: replaces the download of the accumulated output at d_out (out_bytes) after the last batch: what
     * reaches the host `out` is its business (hrt_compute_received_signal: the propagated signal, not the taps) */
    int (*deliver)(const ch_job *j, int device, const void *d_out, void *out);
    const void *aux;   /* what `deliver` needs (hrt_compute_received_signal: its pr_job) */
};

static int ch_compute(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel, const Vec3 *tx_vel,
                      float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb, ch_job *job, void *out,
                      hrt_stats *stats, double t_begin)
{
    /* the thread's patterns, read once: what the call applies after each batch's trace (NULL: nothing) */
    const hrt_patterns_host *const pat = g_patterns;
    if (pat) {
        const int prc = patterns_host_check(pat, nrx, ntx);
        if (prc) return prc;
    }
    hrt_pattern_spec pat_spec;
    void *d_pat = NULL;
    hrt_stats st;
    memset(&st, 0, sizeof st);
    st.num_devices = 1;
    void *d_out = NULL, *d_scratch = NULL;
    uint64_t scratch_bytes = 0;
    const uint64_t out_bytes = job->out_bytes;
    double t_dev = 0.0, t_dirs = 0.0;
    job->d_const = NULL;
    hrt_solo so;   /* device, problem, batch count and the drop-in's worker buffers, pooled between calls (batch.c) */
    int rc = hrt_solo_begin(&so, scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &st, t_begin);
    if (rc) goto done;
    hrt_problem *prob = so.prob;
    work_t *w = &so.wc.w;
    const int device = so.wc.device;
    const uint32_t G = so.wc.G;
    hrt_layout L;
    if (job->const_bytes) {
        if ((rc = hrt_device_malloc(device, &job->d_const, job->const_bytes))) goto done;
        if ((rc = hrt_device_upload(device, job->d_const, job->h_const, job->const_bytes))) goto done;
    }
    if (pat && (rc = patterns_upload(pat, device, nrx, ntx, &d_pat, &pat_spec))) goto done;
    /* scratch: the largest any batch needs (batch 0 has the most local rays) */
    for (uint32_t g = 0; g < G; ++g) {
        hrt_shard s = {np, g, G, 0, (uint32_t)nb};
        if (hrt_shard_num_local(&s) == 0) continue;
        uint64_t b = 0;
        if ((rc = job->scratch_bytes(job, prob, &s, &b))) goto done;
        if (b > scratch_bytes) scratch_bytes = b;
    }
    if ((rc = hrt_device_malloc(device, &d_out, out_bytes))) goto done;
    if ((rc = hrt_device_malloc(device, &d_scratch, scratch_bytes))) goto done;

    for (uint32_t g = 0, first = 1; g < G; ++g) {
        hrt_shard s = {np, g, G, 0, (uint32_t)nb};
        if (hrt_shard_num_local(&s) == 0) continue;
        if ((rc = hrt_layout_query(prob, &s, &L))) goto done;
        double t0 = hrt_now_s();
        if ((rc = hrt_launch_dirs_device(&s, (float *)w->d_dirs, device, NULL, NULL))) goto done;
        if ((rc = hrt_launch_order_device(&s, (uint32_t *)w->d_order, device, NULL))) goto done;
        t_dirs += hrt_now_s() - t0;
        t0 = hrt_now_s();
        if ((rc = hrt_trace_batch(prob, &s, &L, w, &st))) goto done;   /* (batch.c) */
        if (pat && (rc = hrt_apply_patterns(prob, &s, w->d_ws, L.total_bytes, &pat_spec, NULL))) goto done;
        /* batch 0 is rank 0 of the launch set: it adds the LoS term; the others add their records */
        if ((rc = job->run(job, prob, &s, w->d_ws, d_scratch, scratch_bytes, d_out, first ? 0 : 1)))
            goto done;
        first = 0;
        if ((rc = hrt_device_sync(device, NULL))) goto done;
        t_dev += hrt_now_s() - t0;
    }
    {
        const double t0 = hrt_now_s();
        if (job->deliver) {
            if ((rc = job->deliver(job, device, d_out, out))) goto done;
        } else if ((rc = hrt_device_download(device, out, d_out, out_bytes))) goto done;
        if (job->finish && (rc = job->finish(job, prob, out))) goto done;
        st.t_readback_s = hrt_now_s() - t0;
    }
    st.num_batches = G;
    st.dev_id[0] = device;
    st.dev_batches[0] = G;
    st.t_launch_dirs_s = t_dirs;
    st.t_device_s = t_dev;
    st.dev_t_device_s[0] = t_dev;
    st.dev_t_readback_s[0] = st.t_readback_s;
    st.t_total_s = hrt_now_s() - t_begin;
    if (stats) *stats = st;
    rc = HRT_OK;

done:
    if (d_scratch) hrt_device_free(st.device, d_scratch);
    if (d_out) hrt_device_free(st.device, d_out);
    if (d_pat) hrt_device_free(st.device, d_pat);
    if (job->d_const) hrt_device_free(st.device, job->d_const);
    job->d_const = NULL;
    hrt_solo_end(&so, rc);
    return rc;
}

static int ch_job_scratch(const ch_job *j, const hrt_problem *p, const hrt_shard *s, uint64_t *out)
{
    return hrt_channel_scratch_bytes(p, s, j->spec, out);
}

static int ch_job_run(const ch_job *j, const hrt_problem *p, const hrt_shard *s, const void *d_ws, void *d_scratch,
                      uint64_t scratch_bytes, void *d_out, int accumulate)
{
    return hrt_channel(p, s, d_ws, j->spec, d_scratch, scratch_bytes, d_out, accumulate, NULL);
}

static int ch_drop_in_check(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                            const Vec3 *tx_vel, size_t nrx, size_t ntx, size_t np, size_t nb, const void *out,
                            const char *who)
{
    if (!scene || !out || !rx_pos || !tx_pos || !rx_vel || !tx_vel) return hrt_fail(HRT_E_INVALID, "%s: NULL argument", who);
    if (nrx == 0 || ntx == 0 || np == 0 || nb == 0)
        return hrt_fail(HRT_E_INVALID, "num_rx, num_tx, num_rays and num_bounces must be > 0");
    if (nb > 65535) return hrt_fail(HRT_E_INVALID, "num_bounces > 65535 is not supported");
    return HRT_OK;
}

int hrt_compute_channel(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                        const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                        const hrt_channel_spec *spec, float *out, hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = spec_check(spec);
    if (rc) return rc;
    if ((rc = ch_drop_in_check(scene, rx_pos, tx_pos, rx_vel, tx_vel, nrx, ntx, np, nb, out, "hrt_compute_channel")))
        return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = spec;
    job.out_bytes = (uint64_t)nrx * ntx * 2u * spec->num_times * spec->num_freqs * 8u;
    job.scratch_bytes = ch_job_scratch;
    job.run = ch_job_run;
    return ch_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, out, stats, t_begin);
}

/* ------------------------------------------------------------------ antenna arrays (hrt_array_channel) */

#define HRT_AC_TARGET_GROUPS 2048u          /* workgroups of the partial kernel worth launching (8 per CU) */
#define HRT_AC_PARTIAL_MAX (512ull << 20)   /* partial sums beyond one chunk: at most this */
#define HRT_SPEED_OF_LIGHT 299792458.0

/* the checks of the arrays of a call (`who`) whose spec has `grid` points per element pair (`axes` names them);
 * device pointers are not read */
static int arrays_check(const hrt_array_spec *a, uint64_t grid, const char *axes, const char *who)
{
    if (!a) return hrt_fail(HRT_E_INVALID, "%s: NULL arrays", who);
    if (a->num_rx_elements < 1 || a->num_rx_elements > HRT_AC_MAX_ELEMENTS || a->num_tx_elements < 1 ||
        a->num_tx_elements > HRT_AC_MAX_ELEMENTS)
        return hrt_fail(HRT_E_INVALID, "%s: %u RX and %u TX elements (1 .. %u each)", who, a->num_rx_elements,
                        a->num_tx_elements, HRT_AC_MAX_ELEMENTS);
    const uint64_t pts = (uint64_t)a->num_rx_elements * a->num_tx_elements * grid;
    if (pts > HRT_AC_MAX_POINTS)
        return hrt_fail(HRT_E_INVALID, "%s: Nr * Nt * %s = %llu > 2^24", who, axes, (unsigned long long)pts);
    if (!isfinite(a->array_frequency_hz) || !(a->array_frequency_hz > 0.0))
        return hrt_fail(HRT_E_INVALID, "%s: the array frequency must be finite and > 0", who);
    if (!a->rx_elements || !a->tx_elements) return hrt_fail(HRT_E_INVALID, "%s: NULL element offsets", who);
    return HRT_OK;
}

/* the checks of an array call that need no problem (device pointers are not read) */
static int array_check(const hrt_channel_spec *spec, const hrt_array_spec *a)
{
    int rc = spec_check(spec);
    if (rc) return rc;
    return arrays_check(a, (uint64_t)spec->num_times * spec->num_freqs, "num_times * num_freqs",
                        "hrt_array_channel");
}

/* the element counts of a drop-in array call (`who`), before they are narrowed to the spec's */
static int ac_counts_check(size_t nr, size_t nt, const char *who)
{
    if (nr > HRT_AC_MAX_ELEMENTS || nt > HRT_AC_MAX_ELEMENTS)
        return hrt_fail(HRT_E_INVALID, "%s: %zu RX and %zu TX elements (1 .. %u each)", who, nr, nt,
                        HRT_AC_MAX_ELEMENTS);
    return HRT_OK;
}

/* the host offsets of a drop-in array call (`who`): finite */
static int ac_offsets_check(const Vec3 *rx_el, size_t nr, const Vec3 *tx_el, size_t nt, const char *who)
{
    for (size_t i = 0; i < nr; ++i)
        if (!isfinite(rx_el[i].x) || !isfinite(rx_el[i].y) || !isfinite(rx_el[i].z))
            return hrt_fail(HRT_E_INVALID, "%s: RX element %zu is not finite", who, i);
    for (size_t j = 0; j < nt; ++j)
        if (!isfinite(tx_el[j].x) || !isfinite(tx_el[j].y) || !isfinite(tx_el[j].z))
            return hrt_fail(HRT_E_INVALID, "%s: TX element %zu is not finite", who, j);
    return HRT_OK;
}

/* the host offsets of a drop-in array or beam call as ch_compute uploads them: [nr + nt][3] floats, rx then tx
 * (ac_job_arrays) */
static void ac_pack_offsets(const Vec3 *rx_el, size_t nr, const Vec3 *tx_el, size_t nt, float *e)
{
    for (size_t i = 0; i < nr; ++i) { e[3 * i] = rx_el[i].x; e[3 * i + 1] = rx_el[i].y; e[3 * i + 2] = rx_el[i].z; }
    for (size_t j = 0; j < nt; ++j) {
        float *q = e + 3u * (nr + j);
        q[0] = tx_el[j].x; q[1] = tx_el[j].y; q[2] = tx_el[j].z;
    }
}

/* the array fields of hrt_karray / hrt_karray_taps (call `who`, `grid` points per element pair and `links` links) and
 * the limit of the output index */
static int ac_fields(const hrt_array_spec *a, uint64_t links, uint64_t grid, const char *who, uint32_t *nr,
                     uint32_t *nt, uint32_t *npairs, double *fa_c)
{
    if (links * 2u * a->num_rx_elements * a->num_tx_elements * grid >= (1ull << 39))
        return hrt_fail(HRT_E_INVALID, "%s: more than 2^39 outputs", who);
    *nr = a->num_rx_elements; *nt = a->num_tx_elements; *npairs = *nr * *nt;
    *fa_c = a->array_frequency_hz / HRT_SPEED_OF_LIGHT;
    return HRT_OK;
}

/* The grid of one call of a pair family (hrt_kgrid, csrc/hrt_pathsum.h: hrt_array_channel's element pairs,
 * hrt_beam_channel's beam pairs) and its record chunks, v->nchunks.  Returns the bytes of one chunk's partial sums;
 * *bytes is the scratch: seg, then the partial sums. */
static uint64_t pair_grid(hrt_kview *v, const hrt_channel_spec *spec, uint32_t npairs, double fa_hz, hrt_kgrid *g,
                          uint64_t *bytes)
{
    g->K = spec->num_freqs; g->T = spec->num_times;
    g->K1 = (spec->num_freqs + HRT_CH_K2 - 1) / HRT_CH_K2;
    g->rows = g->K1 * g->T;
    g->pblocks = (npairs + HRT_AC_PAIRS - 1) / HRT_AC_PAIRS;
    g->cblocks = (g->rows + HRT_AC_GROWS - 1) / HRT_AC_GROWS;
    g->f0 = spec->f0_hz; g->df = spec->df_hz; g->t0 = spec->t0_s; g->dt = spec->dt_s;
    g->fa_c = fa_hz / HRT_SPEED_OF_LIGHT;
    const uint64_t links = (uint64_t)v->nrx * v->ntx;
    const uint64_t per_chunk = links * 2u * npairs * g->T * g->K * 8u;
    *bytes = ps_chunks(v, spec->parts, links * g->pblocks * g->cblocks, HRT_AC_TARGET_GROUPS, per_chunk,
                       HRT_AC_PARTIAL_MAX, 65535u);
    return per_chunk;
}

/* the tiling of one array call: a pure function of the problem, the shard, the spec and the array sizes */
static int ac_plan(const hrt_problem *p, const hrt_shard *s, const hrt_channel_spec *spec, const hrt_array_spec *a,
                   hrt_karray *K, uint64_t *bytes)
{
    int rc = array_check(spec, a);
    if (rc) return rc;
    memset(K, 0, sizeof *K);
    if ((rc = ps_view(p, s, spec->parts, "hrt_array_channel", &K->v))) return rc;
    const uint64_t links = (uint64_t)K->v.nrx * K->v.ntx;
    if ((rc = ac_fields(a, links, (uint64_t)spec->num_times * spec->num_freqs, "hrt_array_channel", &K->nr, &K->nt,
                        &K->npairs, &K->g.fa_c)))
        return rc;
    ps_shard(s, &K->sh);
    (void)pair_grid(&K->v, spec, K->npairs, a->array_frequency_hz, &K->g, bytes);
    return HRT_OK;
}

int hrt_array_channel_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_channel_spec *spec,
                                    const hrt_array_spec *arrays, uint64_t *out)
{
    hrt_karray K;
    uint64_t bytes = 0;
    const int rc = ac_plan(p, s, spec, arrays, &K, &bytes);
    return ps_scratch_out(rc, bytes, out, "hrt_array_channel_scratch_bytes");
}

int hrt_array_channel(const hrt_problem *p, const hrt_shard *s, const void *d_workspace,
                      const hrt_channel_spec *spec, const hrt_array_spec *arrays, void *d_scratch,
                      uint64_t scratch_bytes, float *d_out, int accumulate, void *stream)
{
    hrt_karray K;
    uint64_t need = 0;
    int rc = ac_plan(p, s, spec, arrays, &K, &need);
    if (rc) return rc;
    if ((rc = ps_bind(&K.v, need, d_workspace, d_scratch, scratch_bytes, d_out, accumulate, "hrt_array_channel",
                      "hrt_array_channel_scratch_bytes", &K.partial)))
        return rc;
    K.rx_el = arrays->rx_elements;
    K.tx_el = arrays->tx_elements;
    K.out = d_out;
    HRT_HIP(hrt_hip_set_device(p->device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_array_channel(&K, stream), "array channel kernels");
    return HRT_OK;
}

/* the array spec of a drop-in call: the offsets uploaded by ch_compute (rx then tx) */
static hrt_array_spec ac_job_arrays(const ch_job *j)
{
    hrt_array_spec a;
    a.num_rx_elements = j->nr;
    a.num_tx_elements = j->nt;
    a.rx_elements = (const float *)j->d_const;
    a.tx_elements = (const float *)j->d_const + 3u * j->nr;
    a.array_frequency_hz = j->fa;
    return a;
}

static int ac_job_scratch(const ch_job *j, const hrt_problem *p, const hrt_shard *s, uint64_t *out)
{
    const hrt_array_spec a = ac_job_arrays(j);
    return hrt_array_channel_scratch_bytes(p, s, j->spec, &a, out);
}

static int ac_job_run(const ch_job *j, const hrt_problem *p, const hrt_shard *s, const void *d_ws, void *d_scratch,
                      uint64_t scratch_bytes, void *d_out, int accumulate)
{
    const hrt_array_spec a = ac_job_arrays(j);
    return hrt_array_channel(p, s, d_ws, j->spec, &a, d_scratch, scratch_bytes, d_out, accumulate, NULL);
}

/* What hrt_compute_array_channel and hrt_compute_array_taps (`who`, device entry `dev`) share once the counts and
 * the spec are checked: the remaining checks in their order, the offsets for ch_compute to upload (rx then tx;
 * ac_job_arrays), the call.  `job` has the spec, the output size and the device entry. */
static int ac_compute(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel, const Vec3 *tx_vel,
                      float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb, ch_job *job, const Vec3 *rx_el,
                      size_t nr, const Vec3 *tx_el, size_t nt, double f_a, float *out, hrt_stats *stats,
                      double t_begin, const char *dev, const char *who)
{
    int rc = ac_offsets_check(rx_el, nr, tx_el, nt, dev);
    if (rc) return rc;
    if ((rc = ch_drop_in_check(scene, rx_pos, tx_pos, rx_vel, tx_vel, nrx, ntx, np, nb, out, who))) return rc;
    float *e = (float *)malloc((nr + nt) * 3u * sizeof(float));
    if (!e) return hrt_fail(HRT_E_NOMEM, "out of host memory");
    ac_pack_offsets(rx_el, nr, tx_el, nt, e);
    job->h_const = e;
    job->const_bytes = (nr + nt) * 3u * sizeof(float);
    job->nr = (uint32_t)nr;
    job->nt = (uint32_t)nt;
    job->fa = f_a;
    rc = ch_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, job, out, stats, t_begin);
    free(e);
    return rc;
}

int hrt_compute_array_channel(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                              const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                              const hrt_channel_spec *spec, const Vec3 *rx_el, size_t nr, const Vec3 *tx_el,
                              size_t nt, double f_a, float *out, hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = ac_counts_check(nr, nt, "hrt_array_channel");
    if (rc) return rc;
    /* (the element pointers stand in for the device ones: array_check tests them for NULL only) */
    const hrt_array_spec a = {(uint32_t)nr, (uint32_t)nt, (const float *)rx_el, (const float *)tx_el, f_a};
    if ((rc = array_check(spec, &a))) return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = spec;
    job.out_bytes = (uint64_t)nrx * ntx * nr * nt * 2u * spec->num_times * spec->num_freqs * 8u;
    job.scratch_bytes = ac_job_scratch;
    job.run = ac_job_run;
    return ac_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, rx_el, nr, tx_el, nt, f_a,
                      out, stats, t_begin, "hrt_array_channel", "hrt_compute_array_channel");
}

/* ------------------------------------------------------------------ impulse responses (hrt_taps) */

/* (of the three taps families) */
#define HRT_TP_TARGET_GROUPS 2048u          /* workgroups of the partial kernel worth launching (8 per CU) */
#define HRT_TP_PARTIAL_MAX (512ull << 20)   /* partial sums beyond one chunk: at most this */

/* the checks of a taps spec of a call (`who`) */
static int taps_spec_check(const hrt_taps_spec *spec, const char *who)
{
    if (!spec) return hrt_fail(HRT_E_INVALID, "%s: NULL spec", who);
    if (spec->num_taps == 0 || spec->num_times == 0)
        return hrt_fail(HRT_E_INVALID, "%s: num_taps and num_times must be > 0", who);
    if ((uint64_t)spec->num_taps * spec->num_times > HRT_TP_MAX_POINTS)
        return hrt_fail(HRT_E_INVALID, "%s: num_taps * num_times = %llu > 2^20", who,
                        (unsigned long long)spec->num_taps * spec->num_times);
    if (!isfinite(spec->fs_hz) || !(spec->fs_hz > 0.0))
        return hrt_fail(HRT_E_INVALID, "%s: the sampling rate must be finite and > 0", who);
    if (!isfinite(spec->fc_hz) || !isfinite(spec->t0_s) || !isfinite(spec->dt_s))
        return hrt_fail(HRT_E_INVALID, "%s: fc, t0 and dt must be finite", who);
    const int64_t lo = spec->l_min, hi = (int64_t)spec->l_min + spec->num_taps;
    if (lo < -HRT_TP_MAX_TAP || lo > HRT_TP_MAX_TAP || hi > HRT_TP_MAX_TAP)
        return hrt_fail(HRT_E_INVALID, "%s: tap indices l_min = %lld .. %lld outside +-2^24", who, (long long)lo,
                        (long long)hi);
    return parts_check(spec->parts, who);
}

/* The grid of one call of a taps family (hrt_ktgrid, csrc/hrt_pathsum.h) with npairs * num_times rows, and the record
 * chunks of its scatter part (v->nchunks): returns the scratch of seg and the partial sums, *per_chunk the bytes of
 * one chunk's.  Where the grid has four row tiles (rows >= 13) a wave holds 4 row tiles (U read once per MFMA, V formed
 * once per four) and the `wr` waves of a block that stand along the rows make it 4 wr x 4 tiles: wr = 1 in hrt_taps
 * (4 x 1 tiles a wave), 4 in the array and beam families (4 x 4 tiles a wave: a block of 64 rows, so a staged record
 * serves 64 MFMAs).  Otherwise 1 x 4 tiles a wave, the waves along the columns: a block of 1 x 16 tiles (the rows past
 * 4 rows of the tile are padding). */
static uint64_t taps_grid(hrt_kview *v, const hrt_taps_spec *spec, uint32_t npairs, uint32_t wr, hrt_ktgrid *g,
                          uint64_t *per_chunk)
{
    g->L = spec->num_taps; g->T = spec->num_times; g->l_min = spec->l_min;
    g->rows = npairs * g->T;
    g->rtiles = (4u * g->rows + 15u) / 16u;
    g->ctiles = (g->L + 15u) / 16u;
    g->rt = g->rtiles >= 4u ? 4u : 1u;
    const uint32_t brows = g->rt == 4u ? 4u * wr : 1u, bcols = g->rt == 4u ? 4u : 16u;   /* tiles of a block */
    g->rblocks = (g->rtiles + brows - 1u) / brows;
    g->cblocks = (g->ctiles + bcols - 1u) / bcols;
    g->fs = spec->fs_hz; g->fc = spec->fc_hz; g->t0 = spec->t0_s; g->dt = spec->dt_s;
    const uint64_t links = (uint64_t)v->nrx * v->ntx;
    *per_chunk = links * 2u * npairs * g->T * g->L * 8u;
    return ps_chunks(v, spec->parts, links * g->rblocks * g->cblocks, HRT_TP_TARGET_GROUPS, *per_chunk,
                     HRT_TP_PARTIAL_MAX, 65535u);
}

/* the plan of one taps call: a pure function of the problem, the shard and the spec */
static int taps_plan(const hrt_problem *p, const hrt_shard *s, const hrt_taps_spec *spec, hrt_ktaps *K,
                     uint64_t *bytes)
{
    int rc = taps_spec_check(spec, "hrt_taps");
    if (rc) return rc;
    memset(K, 0, sizeof *K);
    if ((rc = ps_view(p, s, spec->parts, "hrt_taps", &K->v))) return rc;
    hrt_ktgrid g;   /* hrt_ktaps holds these fields written out (csrc/hrt_taps.h) */
    uint64_t per_chunk;
    *bytes = taps_grid(&K->v, spec, 1u, 1u, &g, &per_chunk);
    K->L = g.L; K->T = g.T; K->l_min = g.l_min;
    K->rtiles = g.rtiles; K->ctiles = g.ctiles; K->rt = g.rt; K->rblocks = g.rblocks; K->cblocks = g.cblocks;
    K->fs = g.fs; K->fc = g.fc; K->t0 = g.t0; K->dt = g.dt;
    return HRT_OK;
}

int hrt_taps_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_taps_spec *spec, uint64_t *out)
{
    hrt_ktaps K;
    uint64_t bytes = 0;
    const int rc = taps_plan(p, s, spec, &K, &bytes);
    return ps_scratch_out(rc, bytes, out, "hrt_taps_scratch_bytes");
}

int hrt_taps(const hrt_problem *p, const hrt_shard *s, const void *d_workspace, const hrt_taps_spec *spec,
             void *d_scratch, uint64_t scratch_bytes, float *d_out, int accumulate, void *stream)
{
    hrt_ktaps K;
    uint64_t need = 0;
    int rc = taps_plan(p, s, spec, &K, &need);
    if (rc) return rc;
    if ((rc = ps_bind(&K.v, need, d_workspace, d_scratch, scratch_bytes, d_out, accumulate, "hrt_taps",
                      "hrt_taps_scratch_bytes", &K.partial)))
        return rc;
    K.out = d_out;
    HRT_HIP(hrt_hip_set_device(p->device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_taps(&K, stream), "taps kernels");
    return HRT_OK;
}

static int tp_job_scratch(const ch_job *j, const hrt_problem *p, const hrt_shard *s, uint64_t *out)
{
    return hrt_taps_scratch_bytes(p, s, j->spec, out);
}

static int tp_job_run(const ch_job *j, const hrt_problem *p, const hrt_shard *s, const void *d_ws, void *d_scratch,
                      uint64_t scratch_bytes, void *d_out, int accumulate)
{
    return hrt_taps(p, s, d_ws, j->spec, d_scratch, scratch_bytes, d_out, accumulate, NULL);
}

int hrt_compute_taps(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel, const Vec3 *tx_vel,
                     float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb, const hrt_taps_spec *spec, float *out,
                     hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = taps_spec_check(spec, "hrt_taps");
    if (rc) return rc;
    if ((rc = ch_drop_in_check(scene, rx_pos, tx_pos, rx_vel, tx_vel, nrx, ntx, np, nb, out, "hrt_compute_taps")))
        return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = spec;
    job.out_bytes = (uint64_t)nrx * ntx * 2u * spec->num_times * spec->num_taps * 8u;
    job.scratch_bytes = tp_job_scratch;
    job.run = tp_job_run;
    return ch_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, out, stats, t_begin);
}

/* ------------------------------------------------------------------ antenna-array impulse responses (hrt_array_taps) */

/* the checks of an array taps call that need no problem (device pointers are not read) */
static int at_check(const hrt_taps_spec *spec, const hrt_array_spec *a)
{
    int rc = taps_spec_check(spec, "hrt_array_taps");
    if (rc) return rc;
    return arrays_check(a, (uint64_t)spec->num_times * spec->num_taps, "num_times * num_taps", "hrt_array_taps");
}

/* the plan of one array taps call: a pure function of the problem, the shard, the spec and the array sizes */
static int at_plan(const hrt_problem *p, const hrt_shard *s, const hrt_taps_spec *spec, const hrt_array_spec *a,
                   hrt_karray_taps *K, uint64_t *bytes)
{
    int rc = at_check(spec, a);
    if (rc) return rc;
    memset(K, 0, sizeof *K);
    if ((rc = ps_view(p, s, spec->parts, "hrt_array_taps", &K->v))) return rc;
    const uint64_t links = (uint64_t)K->v.nrx * K->v.ntx;
    if ((rc = ac_fields(a, links, (uint64_t)spec->num_times * spec->num_taps, "hrt_array_taps", &K->nr, &K->nt,
                        &K->npairs, &K->fa_c)))
        return rc;
    ps_shard(s, &K->sh);
    uint64_t per_chunk;
    *bytes = taps_grid(&K->v, spec, K->npairs, 4u, &K->g, &per_chunk);
    return HRT_OK;
}

int hrt_array_taps_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_taps_spec *spec,
                                 const hrt_array_spec *arrays, uint64_t *out)
{
    hrt_karray_taps K;
    uint64_t bytes = 0;
    const int rc = at_plan(p, s, spec, arrays, &K, &bytes);
    return ps_scratch_out(rc, bytes, out, "hrt_array_taps_scratch_bytes");
}

int hrt_array_taps(const hrt_problem *p, const hrt_shard *s, const void *d_workspace, const hrt_taps_spec *spec,
                   const hrt_array_spec *arrays, void *d_scratch, uint64_t scratch_bytes, float *d_out, int accumulate,
                   void *stream)
{
    hrt_karray_taps K;
    uint64_t need = 0;
    int rc = at_plan(p, s, spec, arrays, &K, &need);
    if (rc) return rc;
    if ((rc = ps_bind(&K.v, need, d_workspace, d_scratch, scratch_bytes, d_out, accumulate, "hrt_array_taps",
                      "hrt_array_taps_scratch_bytes", &K.partial)))
        return rc;
    K.rx_el = arrays->rx_elements;
    K.tx_el = arrays->tx_elements;
    K.out = d_out;
    HRT_HIP(hrt_hip_set_device(p->device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_array_taps(&K, stream), "array taps kernels");
    return HRT_OK;
}

static int at_job_scratch(const ch_job *j, const hrt_problem *p, const hrt_shard *s, uint64_t *out)
{
    const hrt_array_spec a = ac_job_arrays(j);
    return hrt_array_taps_scratch_bytes(p, s, j->spec, &a, out);
}

static int at_job_run(const ch_job *j, const hrt_problem *p, const hrt_shard *s, const void *d_ws, void *d_scratch,
                      uint64_t scratch_bytes, void *d_out, int accumulate)
{
    const hrt_array_spec a = ac_job_arrays(j);
    return hrt_array_taps(p, s, d_ws, j->spec, &a, d_scratch, scratch_bytes, d_out, accumulate, NULL);
}

int hrt_compute_array_taps(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                           const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                           const hrt_taps_spec *spec, const Vec3 *rx_el, size_t nr, const Vec3 *tx_el, size_t nt,
                           double f_a, float *out, hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = ac_counts_check(nr, nt, "hrt_array_taps");
    if (rc) return rc;
    /* (the element pointers stand in for the device ones: at_check tests them for NULL only) */
    const hrt_array_spec a = {(uint32_t)nr, (uint32_t)nt, (const float *)rx_el, (const float *)tx_el, f_a};
    if ((rc = at_check(spec, &a))) return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = spec;
    job.out_bytes = (uint64_t)nrx * ntx * nr * nt * 2u * spec->num_times * spec->num_taps * 8u;
    job.scratch_bytes = at_job_scratch;
    job.run = at_job_run;
    return ac_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, rx_el, nr, tx_el, nt, f_a,
                      out, stats, t_begin, "hrt_array_taps", "hrt_compute_array_taps");
}

/* ------------------------------------------------------------------ received signals (hrt_propagate) */

/* the checks of a propagation call (`who`); device pointers are not read */
static int propagate_check(const hrt_propagate_spec *sp, const char *who)
{
    if (!sp) return hrt_fail(HRT_E_INVALID, "%s: NULL spec", who);
    if (sp->num_rx == 0 || sp->num_tx == 0 || sp->nr == 0 || sp->nt == 0 || sp->num_times == 0 || sp->num_taps == 0 ||
        sp->samples_per_block == 0 || sp->num_samples == 0 || sp->num_out == 0)
        return hrt_fail(HRT_E_INVALID, "%s: num_rx, num_tx, nr, nt, num_times, num_taps, samples_per_block, num_samples "
                        "and num_out must be > 0", who);
    if (sp->nr > HRT_PG_MAX_ELEMENTS || sp->nt > HRT_PG_MAX_ELEMENTS)
        return hrt_fail(HRT_E_INVALID, "%s: nr = %u and nt = %u (1 .. %u each)", who, sp->nr, sp->nt,
                        HRT_PG_MAX_ELEMENTS);
    const uint64_t pts = (uint64_t)sp->nr * sp->nt * sp->num_times;   /* <= 2^52 */
    if (pts > HRT_PG_MAX_POINTS || pts * sp->num_taps > HRT_PG_MAX_POINTS)
        return hrt_fail(HRT_E_INVALID, "%s: nr * nt * num_times * num_taps > 2^24", who);
    const int64_t lo = sp->l_min, hi = (int64_t)sp->l_min + sp->num_taps;
    if (lo < -HRT_PG_MAX_TAP || lo > HRT_PG_MAX_TAP || hi < -HRT_PG_MAX_TAP || hi > HRT_PG_MAX_TAP)
        return hrt_fail(HRT_E_INVALID, "%s: tap indices l_min = %lld .. %lld outside +-2^24", who, (long long)lo,
                        (long long)hi);
    if (sp->num_samples > HRT_PG_MAX_SAMPLES || sp->num_out > HRT_PG_MAX_SAMPLES)
        return hrt_fail(HRT_E_INVALID, "%s: num_samples = %llu and num_out = %llu (at most 2^31 each)", who,
                        (unsigned long long)sp->num_samples, (unsigned long long)sp->num_out);
    return HRT_OK;
}

uint64_t hrt_propagate_out_floats(const hrt_propagate_spec *spec)
{
    if (!spec) return 0;
    return (uint64_t)spec->num_rx * spec->nr * 2u * spec->num_out * 2u;
}

int hrt_propagate(int device, const hrt_propagate_spec *spec, const void *d_taps, const void *d_signal, void *d_out,
                  int accumulate, void *stream)
{
    int rc = propagate_check(spec, "hrt_propagate");
    if (rc) return rc;
    if (!d_taps || !d_signal || !d_out) return hrt_fail(HRT_E_INVALID, "hrt_propagate: NULL device pointer");
    if (accumulate != 0 && accumulate != 1)
        return hrt_fail(HRT_E_INVALID, "hrt_propagate: accumulate = %d (0 or 1)", accumulate);
    if ((uint64_t)spec->num_rx * spec->nr * 2u > UINT32_MAX || (uint64_t)spec->num_tx * spec->nt > UINT32_MAX)
        return hrt_fail(HRT_E_INVALID, "hrt_propagate: more than 2^32 rows or TX ports");
    hrt_kpropagate K;
    memset(&K, 0, sizeof K);
    K.R = spec->num_rx * spec->nr * 2u;
    K.P = spec->num_tx * spec->nt;
    K.ntx = spec->num_tx; K.nr = spec->nr; K.nt = spec->nt;
    K.M = spec->num_times; K.L = spec->num_taps; K.S = spec->samples_per_block;
    K.l_min = spec->l_min;
    K.accumulate = (uint32_t)accumulate;
    K.N = spec->num_samples; K.N_out = spec->num_out;
    K.h = (const float *)d_taps; K.x = (const float *)d_signal; K.out = (float *)d_out;
    HRT_HIP(hrt_hip_set_device(device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_propagate(&K, hrt_propagate_form(K.M, K.S), stream), "propagation kernel");
    return HRT_OK;
}

/* what hrt_compute_received_signal's `deliver` needs */
typedef struct {
    hrt_propagate_spec spec;
    const float *x;
} pr_job;

/* after the last batch: the taps stay at d_taps; x goes up, the propagation runs once, only y comes down */
static int pr_job_deliver(const ch_job *j, int device, const void *d_taps, void *out)
{
    const pr_job *pj = (const pr_job *)j->aux;
    const uint64_t x_bytes = (uint64_t)pj->spec.num_tx * pj->spec.nt * pj->spec.num_samples * 8u;
    const uint64_t y_bytes = hrt_propagate_out_floats(&pj->spec) * 4u;
    void *d_x = NULL, *d_y = NULL;
    int rc = hrt_device_malloc(device, &d_x, x_bytes);
    if (!rc) rc = hrt_device_malloc(device, &d_y, y_bytes);
    if (!rc) rc = hrt_device_upload(device, d_x, pj->x, x_bytes);
    if (!rc) rc = hrt_propagate(device, &pj->spec, d_taps, d_x, d_y, 0, NULL);
    if (!rc) rc = hrt_device_sync(device, NULL);
    if (!rc) rc = hrt_device_download(device, out, d_y, y_bytes);
    if (d_y) hrt_device_free(device, d_y);
    if (d_x) hrt_device_free(device, d_x);
    return rc;
}

int hrt_compute_received_signal(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                                const hrt_taps_spec *spec, const Vec3 *rx_el, size_t nr, const Vec3 *tx_el, size_t nt,
                                double f_a, uint32_t samples_per_block, const float *x, uint64_t num_samples,
                                uint64_t num_out, float *y, hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = ac_counts_check(nr, nt, "hrt_array_taps");
    if (rc) return rc;
    /* (the element pointers stand in for the device ones: at_check tests them for NULL only) */
    const hrt_array_spec a = {(uint32_t)nr, (uint32_t)nt, (const float *)rx_el, (const float *)tx_el, f_a};
    if ((rc = at_check(spec, &a))) return rc;
    if (!x || !y) return hrt_fail(HRT_E_INVALID, "hrt_compute_received_signal: NULL argument");
    if (nrx > UINT32_MAX || ntx > UINT32_MAX)
        return hrt_fail(HRT_E_INVALID, "hrt_compute_received_signal: num_rx or num_tx > 2^32");
    pr_job pj;
    memset(&pj, 0, sizeof pj);
    pj.spec.num_rx = (uint32_t)nrx; pj.spec.num_tx = (uint32_t)ntx;
    pj.spec.nr = (uint32_t)nr; pj.spec.nt = (uint32_t)nt;
    pj.spec.num_times = spec->num_times; pj.spec.num_taps = spec->num_taps;
    pj.spec.l_min = spec->l_min;
    pj.spec.samples_per_block = samples_per_block;
    pj.spec.num_samples = num_samples; pj.spec.num_out = num_out;
    pj.x = x;
    /* (num_rx and num_tx 0: ch_drop_in_check's refusal, below, as in hrt_compute_array_taps) */
    if (nrx && ntx && (rc = propagate_check(&pj.spec, "hrt_compute_received_signal"))) return rc;
    if (nrx && ntx && (uint64_t)spec->num_times != (num_out + samples_per_block - 1u) / samples_per_block)
        return hrt_fail(HRT_E_INVALID, "hrt_compute_received_signal: num_times = %u, but ceil(num_out / "
                        "samples_per_block) = %llu", spec->num_times,
                        (unsigned long long)((num_out + samples_per_block - 1u) / samples_per_block));
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = spec;
    job.out_bytes = (uint64_t)nrx * ntx * nr * nt * 2u * spec->num_times * spec->num_taps * 8u;
    job.scratch_bytes = at_job_scratch;
    job.run = at_job_run;
    job.deliver = pr_job_deliver;
    job.aux = &pj;
    return ac_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, rx_el, nr, tx_el, nt, f_a,
                      y, stats, t_begin, "hrt_array_taps", "hrt_compute_received_signal");
}

/* ------------------------------------------------------------------ per-point SVD (hrt_channel_svd) */

/* the checks of an SVD call (`who`); device pointers are not read */
static int svd_check(const hrt_svd_spec *sp, const char *who)
{
    if (!sp) return hrt_fail(HRT_E_INVALID, "%s: NULL spec", who);
    if (sp->num_rx == 0 || sp->num_tx == 0 || sp->num_times == 0 || sp->num_freqs == 0)
        return hrt_fail(HRT_E_INVALID, "%s: num_rx, num_tx, num_times and num_freqs must be > 0", who);
    const uint32_t m = sp->nr > sp->nt ? sp->nr : sp->nt, n = sp->nr > sp->nt ? sp->nt : sp->nr;
    if (n < 1 || n > HRT_SVD_MAX_SHORT || m > HRT_SVD_MAX_LONG)
        return hrt_fail(HRT_E_INVALID, "%s: nr = %u and nt = %u (the smaller 1 .. %u, the larger 1 .. %u)", who, sp->nr,
                        sp->nt, HRT_SVD_MAX_SHORT, HRT_SVD_MAX_LONG);
    const uint64_t grid = (uint64_t)sp->num_times * sp->num_freqs;   /* < 2^64 */
    if (grid > HRT_SVD_MAX_POINTS || (uint64_t)sp->nr * sp->nt * grid > HRT_SVD_MAX_POINTS)
        return hrt_fail(HRT_E_INVALID, "%s: nr * nt * num_times * num_freqs > 2^24", who);
    if (sp->want & ~(HRT_SVD_U | HRT_SVD_V))
        return hrt_fail(HRT_E_INVALID, "%s: want = 0x%x has unknown bits", who, sp->want);
    if ((uint64_t)sp->num_rx * sp->num_tx >= (1ull << 31) / (2u * grid))
        return hrt_fail(HRT_E_INVALID, "%s: 2^31 points or more", who);
    return HRT_OK;
}

/* the regions of the output: byte offsets of sigma, u, v, sweeps and the end (hermespy_rt.h) */
static void svd_regions(const hrt_svd_spec *sp, uint64_t off[5])
{
    const uint64_t points = (uint64_t)sp->num_rx * sp->num_tx * 2u * sp->num_times * sp->num_freqs;
    const uint64_t n = sp->nr > sp->nt ? sp->nt : sp->nr;
    off[0] = 0;
    off[1] = off[0] + points * n * 4u;
    off[2] = off[1] + ((sp->want & HRT_SVD_U) ? points * sp->nr * n * 8u : 0u);
    off[3] = off[2] + ((sp->want & HRT_SVD_V) ? points * sp->nt * n * 8u : 0u);
    off[4] = off[3] + points * 4u;
}

uint64_t hrt_svd_out_bytes(const hrt_svd_spec *spec)
{
    if (!spec) return 0;
    uint64_t off[5];
    svd_regions(spec, off);
    return off[4];
}

int hrt_channel_svd(int device, const hrt_svd_spec *spec, const void *d_H, void *d_out, void *stream)
{
    int rc = svd_check(spec, "hrt_channel_svd");
    if (rc) return rc;
    if (!d_H || !d_out) return hrt_fail(HRT_E_INVALID, "hrt_channel_svd: NULL device pointer");
    uint64_t off[5];
    svd_regions(spec, off);
    hrt_ksvd K;
    memset(&K, 0, sizeof K);
    K.nr = spec->nr; K.nt = spec->nt;
    K.tall = spec->nr >= spec->nt;
    K.m = K.tall ? K.nr : K.nt; K.n = K.tall ? K.nt : K.nr;
    const uint32_t g = hrt_svd_form(K.nr, K.nt);
    K.mk = (K.m + g - 1u) / g; K.nk = (K.n + g - 1u) / g;
    K.pts = 2ull * spec->num_times * spec->num_freqs;
    K.points = (uint64_t)spec->num_rx * spec->num_tx * K.pts;
    K.H = (const float *)d_H;
    K.sigma = (float *)((char *)d_out + off[0]);
    K.u = (spec->want & HRT_SVD_U) ? (float *)((char *)d_out + off[1]) : NULL;
    K.v = (spec->want & HRT_SVD_V) ? (float *)((char *)d_out + off[2]) : NULL;
    K.sweeps = (uint32_t *)((char *)d_out + off[3]);
    HRT_HIP(hrt_hip_set_device(device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_svd(&K, g, stream), "SVD kernel");
    return HRT_OK;
}

/* after the last batch: H stays at d_H; the decomposition runs once, only its result comes down */
static int svd_job_deliver(const ch_job *j, int device, const void *d_H, void *out)
{
    const hrt_svd_spec *sp = (const hrt_svd_spec *)j->aux;
    const uint64_t bytes = hrt_svd_out_bytes(sp);
    void *d_svd = NULL;
    int rc = hrt_device_malloc(device, &d_svd, bytes);
    if (!rc) rc = hrt_channel_svd(device, sp, d_H, d_svd, NULL);
    if (!rc) rc = hrt_device_sync(device, NULL);
    if (!rc) rc = hrt_device_download(device, out, d_svd, bytes);
    if (d_svd) hrt_device_free(device, d_svd);
    return rc;
}

int hrt_compute_channel_svd(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                            const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                            const hrt_channel_spec *spec, const Vec3 *rx_el, size_t nr, const Vec3 *tx_el, size_t nt,
                            double f_a, uint32_t want, void *out, hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = ac_counts_check(nr, nt, "hrt_array_channel");
    if (rc) return rc;
    /* (the element pointers stand in for the device ones: array_check tests them for NULL only) */
    const hrt_array_spec a = {(uint32_t)nr, (uint32_t)nt, (const float *)rx_el, (const float *)tx_el, f_a};
    if ((rc = array_check(spec, &a))) return rc;
    if (!out) return hrt_fail(HRT_E_INVALID, "hrt_compute_channel_svd: NULL argument");
    if (nrx > UINT32_MAX || ntx > UINT32_MAX)
        return hrt_fail(HRT_E_INVALID, "hrt_compute_channel_svd: num_rx or num_tx > 2^32");
    hrt_svd_spec sv;
    memset(&sv, 0, sizeof sv);
    sv.num_rx = (uint32_t)nrx; sv.num_tx = (uint32_t)ntx;
    sv.nr = (uint32_t)nr; sv.nt = (uint32_t)nt;
    sv.num_times = spec->num_times; sv.num_freqs = spec->num_freqs;
    sv.want = want;
    /* (num_rx and num_tx 0: ch_drop_in_check's refusal, below, as in hrt_compute_array_channel) */
    if (nrx && ntx && (rc = svd_check(&sv, "hrt_compute_channel_svd"))) return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = spec;
    job.out_bytes = (uint64_t)nrx * ntx * nr * nt * 2u * spec->num_times * spec->num_freqs * 8u;
    job.scratch_bytes = ac_job_scratch;
    job.run = ac_job_run;
    job.deliver = svd_job_deliver;
    job.aux = &sv;
    return ac_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, rx_el, nr, tx_el, nt, f_a,
                      out, stats, t_begin, "hrt_array_channel", "hrt_compute_channel_svd");
}

/* ------------------------------------------------------------------ per-point equalizers (hrt_channel_equalizer) */

/* the checks of an equalizer call (`who`); device pointers are not read */
static int eq_check(const hrt_equalizer_spec *sp, const char *who)
{
    if (!sp) return hrt_fail(HRT_E_INVALID, "%s: NULL spec", who);
    if (sp->num_rx == 0 || sp->num_tx == 0 || sp->num_times == 0 || sp->num_freqs == 0)
        return hrt_fail(HRT_E_INVALID, "%s: num_rx, num_tx, num_times and num_freqs must be > 0", who);
    if (sp->nt < 1 || sp->nt > HRT_EQ_MAX_NT || sp->nr < 1 || sp->nr > HRT_EQ_MAX_NR)
        return hrt_fail(HRT_E_INVALID, "%s: nr = %u and nt = %u (nr 1 .. %u, nt 1 .. %u)", who, sp->nr, sp->nt,
                        HRT_EQ_MAX_NR, HRT_EQ_MAX_NT);
    if (sp->kind != HRT_EQ_ZF && sp->kind != HRT_EQ_LMMSE)
        return hrt_fail(HRT_E_INVALID, "%s: kind = %u is neither HRT_EQ_ZF nor HRT_EQ_LMMSE", who, sp->kind);
    if (sp->kind == HRT_EQ_ZF && sp->nr < sp->nt)
        return hrt_fail(HRT_E_INVALID, "%s: zero-forcing needs nr >= nt (nr = %u, nt = %u)", who, sp->nr, sp->nt);
    if (sp->flags & ~HRT_EQ_W)
        return hrt_fail(HRT_E_INVALID, "%s: flags = 0x%x has unknown bits", who, sp->flags);
    if (!(sp->noise > 0.f) || !(sp->noise <= 3.402823466e+38f))
        return hrt_fail(HRT_E_INVALID, "%s: noise = %g must be finite and > 0", who, (double)sp->noise);
    const uint64_t grid = (uint64_t)sp->num_times * sp->num_freqs;   /* < 2^64 */
    if (grid > HRT_EQ_MAX_POINTS || (uint64_t)sp->nr * sp->nt * grid > HRT_EQ_MAX_POINTS)
        return hrt_fail(HRT_E_INVALID, "%s: nr * nt * num_times * num_freqs > 2^24", who);
    if ((uint64_t)sp->num_rx * sp->num_tx >= (1ull << 31) / (2u * grid))
        return hrt_fail(HRT_E_INVALID, "%s: 2^31 points or more", who);
    return HRT_OK;
}

/* the regions of the output: byte offsets of W, sinr, status and the end (hermespy_rt.h) */
static void eq_regions(const hrt_equalizer_spec *sp, uint64_t off[4])
{
    const uint64_t points = (uint64_t)sp->num_rx * sp->num_tx * 2u * sp->num_times * sp->num_freqs;
    off[0] = 0;
    off[1] = off[0] + ((sp->flags & HRT_EQ_W) ? points * sp->nt * sp->nr * 8u : 0u);
    off[2] = off[1] + points * sp->nt * 4u;
    off[3] = off[2] + points * 4u;
}

uint64_t hrt_equalizer_out_bytes(const hrt_equalizer_spec *spec)
{
    if (!spec) return 0;
    uint64_t off[4];
    eq_regions(spec, off);
    return off[3];
}

int hrt_channel_equalizer(int device, const hrt_equalizer_spec *spec, const void *d_H, void *d_out, void *stream)
{
    int rc = eq_check(spec, "hrt_channel_equalizer");
    if (rc) return rc;
    if (!d_H || !d_out) return hrt_fail(HRT_E_INVALID, "hrt_channel_equalizer: NULL device pointer");
    uint64_t off[4];
    eq_regions(spec, off);
    hrt_kequalizer K;
    memset(&K, 0, sizeof K);
    K.nr = spec->nr; K.nt = spec->nt;
    const uint32_t g = hrt_equalizer_form(K.nr, K.nt);
    K.mk = (K.nr + g - 1u) / g; K.nk = (K.nt + g - 1u) / g;
    K.lmmse = spec->kind == HRT_EQ_LMMSE;
    K.n0 = spec->noise;
    K.pts = 2ull * spec->num_times * spec->num_freqs;
    K.points = (uint64_t)spec->num_rx * spec->num_tx * K.pts;
    K.H = (const float *)d_H;
    K.W = (spec->flags & HRT_EQ_W) ? (float *)((char *)d_out + off[0]) : NULL;
    K.sinr = (float *)((char *)d_out + off[1]);
    K.status = (uint32_t *)((char *)d_out + off[2]);
    HRT_HIP(hrt_hip_set_device(device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_equalizer(&K, g, stream), "equalizer kernel");
    return HRT_OK;
}

/* after the last batch: H stays at d_H; the equalizer is formed once, only its result comes down */
static int eq_job_deliver(const ch_job *j, int device, const void *d_H, void *out)
{
    const hrt_equalizer_spec *sp = (const hrt_equalizer_spec *)j->aux;
    const uint64_t bytes = hrt_equalizer_out_bytes(sp);
    void *d_eq = NULL;
    int rc = hrt_device_malloc(device, &d_eq, bytes);
    if (!rc) rc = hrt_channel_equalizer(device, sp, d_H, d_eq, NULL);
    if (!rc) rc = hrt_device_sync(device, NULL);
    if (!rc) rc = hrt_device_download(device, out, d_eq, bytes);
    if (d_eq) hrt_device_free(device, d_eq);
    return rc;
}

int hrt_compute_channel_equalizer(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                  const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                                  const hrt_channel_spec *spec, const Vec3 *rx_el, size_t nr, const Vec3 *tx_el,
                                  size_t nt, double f_a, uint32_t kind, uint32_t flags, float noise, void *out,
                                  hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = ac_counts_check(nr, nt, "hrt_array_channel");
    if (rc) return rc;
    /* (the element pointers stand in for the device ones: array_check tests them for NULL only) */
    const hrt_array_spec a = {(uint32_t)nr, (uint32_t)nt, (const float *)rx_el, (const float *)tx_el, f_a};
    if ((rc = array_check(spec, &a))) return rc;
    if (!out) return hrt_fail(HRT_E_INVALID, "hrt_compute_channel_equalizer: NULL argument");
    if (nrx > UINT32_MAX || ntx > UINT32_MAX)
        return hrt_fail(HRT_E_INVALID, "hrt_compute_channel_equalizer: num_rx or num_tx > 2^32");
    hrt_equalizer_spec eq;
    memset(&eq, 0, sizeof eq);
    eq.num_rx = (uint32_t)nrx; eq.num_tx = (uint32_t)ntx;
    eq.nr = (uint32_t)nr; eq.nt = (uint32_t)nt;
    eq.num_times = spec->num_times; eq.num_freqs = spec->num_freqs;
    eq.kind = kind; eq.flags = flags; eq.noise = noise;
    /* (num_rx and num_tx 0: ch_drop_in_check's refusal, below, as in hrt_compute_array_channel) */
    if (nrx && ntx && (rc = eq_check(&eq, "hrt_compute_channel_equalizer"))) return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = spec;
    job.out_bytes = (uint64_t)nrx * ntx * nr * nt * 2u * spec->num_times * spec->num_freqs * 8u;
    job.scratch_bytes = ac_job_scratch;
    job.run = ac_job_run;
    job.deliver = eq_job_deliver;
    job.aux = &eq;
    return ac_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, rx_el, nr, tx_el, nt, f_a,
                      out, stats, t_begin, "hrt_array_channel", "hrt_compute_channel_equalizer");
}

/* ------------------------------------------------------------------ per-point precoders (hrt_channel_precoder) */

static int pc_positive(float v)
{
    return v > 0.f && v <= 3.402823466e+38f;
}

/* the checks of a precoder call (`who`); device pointers are not read */
static int pc_check(const hrt_precoder_spec *sp, const char *who)
{
    if (!sp) return hrt_fail(HRT_E_INVALID, "%s: NULL spec", who);
    if (sp->num_rx == 0 || sp->num_tx == 0 || sp->num_times == 0 || sp->num_freqs == 0)
        return hrt_fail(HRT_E_INVALID, "%s: num_rx, num_tx, num_times and num_freqs must be > 0", who);
    if (sp->nr < 1 || sp->nr > HRT_PC_MAX_NR || sp->nt < 1 || sp->nt > HRT_PC_MAX_NT)
        return hrt_fail(HRT_E_INVALID, "%s: nr = %u and nt = %u (nr 1 .. %u, nt 1 .. %u)", who, sp->nr, sp->nt,
                        HRT_PC_MAX_NR, HRT_PC_MAX_NT);
    if (sp->kind != HRT_PC_MRT && sp->kind != HRT_PC_ZF && sp->kind != HRT_PC_RZF)
        return hrt_fail(HRT_E_INVALID, "%s: kind = %u is none of HRT_PC_MRT, HRT_PC_ZF, HRT_PC_RZF", who, sp->kind);
    if (sp->norm != HRT_PC_TOTAL && sp->norm != HRT_PC_STREAM)
        return hrt_fail(HRT_E_INVALID, "%s: norm = %u is neither HRT_PC_TOTAL nor HRT_PC_STREAM", who, sp->norm);
    if (sp->kind == HRT_PC_ZF && sp->nr > sp->nt)
        return hrt_fail(HRT_E_INVALID, "%s: zero-forcing needs nr <= nt (nr = %u, nt = %u)", who, sp->nr, sp->nt);
    if (sp->flags & ~HRT_PC_P)
        return hrt_fail(HRT_E_INVALID, "%s: flags = 0x%x has unknown bits", who, sp->flags);
    if (!pc_positive(sp->noise))
        return hrt_fail(HRT_E_INVALID, "%s: noise = %g must be finite and > 0", who, (double)sp->noise);
    if (!pc_positive(sp->power))
        return hrt_fail(HRT_E_INVALID, "%s: power = %g must be finite and > 0", who, (double)sp->power);
    if (sp->kind == HRT_PC_RZF && !pc_positive(sp->regularization))
        return hrt_fail(HRT_E_INVALID, "%s: regularization = %g must be finite and > 0", who,
                        (double)sp->regularization);
    const uint64_t grid = (uint64_t)sp->num_times * sp->num_freqs;   /* < 2^64 */
    if (grid > HRT_PC_MAX_POINTS || (uint64_t)sp->nr * sp->nt * grid > HRT_PC_MAX_POINTS)
        return hrt_fail(HRT_E_INVALID, "%s: nr * nt * num_times * num_freqs > 2^24", who);
    if ((uint64_t)sp->num_rx * sp->num_tx >= (1ull << 31) / (2u * grid))
        return hrt_fail(HRT_E_INVALID, "%s: 2^31 points or more", who);
    return HRT_OK;
}

/* the regions of the output: byte offsets of P, sinr, status and the end (hermespy_rt.h) */
static void pc_regions(const hrt_precoder_spec *sp, uint64_t off[4])
{
    const uint64_t points = (uint64_t)sp->num_rx * sp->num_tx * 2u * sp->num_times * sp->num_freqs;
    off[0] = 0;
    off[1] = off[0] + ((sp->flags & HRT_PC_P) ? points * sp->nt * sp->nr * 8u : 0u);
    off[2] = off[1] + points * sp->nr * 4u;
    off[3] = off[2] + points * 4u;
}

uint64_t hrt_precoder_out_bytes(const hrt_precoder_spec *spec)
{
    if (!spec) return 0;
    uint64_t off[4];
    pc_regions(spec, off);
    return off[3];
}

int hrt_channel_precoder(int device, const hrt_precoder_spec *spec, const void *d_H, void *d_out, void *stream)
{
    int rc = pc_check(spec, "hrt_channel_precoder");
    if (rc) return rc;
    if (!d_H || !d_out) return hrt_fail(HRT_E_INVALID, "hrt_channel_precoder: NULL device pointer");
    uint64_t off[4];
    pc_regions(spec, off);
    hrt_kprecoder K;
    memset(&K, 0, sizeof K);
    K.nr = spec->nr; K.nt = spec->nt;
    const uint32_t g = hrt_precoder_form(K.nr, K.nt);
    K.mk = (K.nt + g - 1u) / g; K.nk = (K.nr + g - 1u) / g;
    K.kind = spec->kind;
    K.stream = spec->norm == HRT_PC_STREAM;
    K.alpha = spec->kind == HRT_PC_RZF ? spec->regularization : 0.f;
    K.n0 = spec->noise;
    K.power = K.stream ? spec->power / (float)spec->nr : spec->power;
    K.pts = 2ull * spec->num_times * spec->num_freqs;
    K.points = (uint64_t)spec->num_rx * spec->num_tx * K.pts;
    K.H = (const float *)d_H;
    K.P = (spec->flags & HRT_PC_P) ? (float *)((char *)d_out + off[0]) : NULL;
    K.sinr = (float *)((char *)d_out + off[1]);
    K.status = (uint32_t *)((char *)d_out + off[2]);
    HRT_HIP(hrt_hip_set_device(device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_precoder(&K, g, stream), "precoder kernel");
    return HRT_OK;
}

/* after the last batch: H stays at d_H; the precoder is formed once, only its result comes down */
static int pc_job_deliver(const ch_job *j, int device, const void *d_H, void *out)
{
    const hrt_precoder_spec *sp = (const hrt_precoder_spec *)j->aux;
    const uint64_t bytes = hrt_precoder_out_bytes(sp);
    void *d_pc = NULL;
    int rc = hrt_device_malloc(device, &d_pc, bytes);
    if (!rc) rc = hrt_channel_precoder(device, sp, d_H, d_pc, NULL);
    if (!rc) rc = hrt_device_sync(device, NULL);
    if (!rc) rc = hrt_device_download(device, out, d_pc, bytes);
    if (d_pc) hrt_device_free(device, d_pc);
    return rc;
}

int hrt_compute_channel_precoder(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                 const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                                 const hrt_channel_spec *spec, const Vec3 *rx_el, size_t nr, const Vec3 *tx_el,
                                 size_t nt, double f_a, uint32_t kind, uint32_t norm, uint32_t flags, float noise,
                                 float power, float regularization, void *out, hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = ac_counts_check(nr, nt, "hrt_array_channel");
    if (rc) return rc;
    /* (the element pointers stand in for the device ones: array_check tests them for NULL only) */
    const hrt_array_spec a = {(uint32_t)nr, (uint32_t)nt, (const float *)rx_el, (const float *)tx_el, f_a};
    if ((rc = array_check(spec, &a))) return rc;
    if (!out) return hrt_fail(HRT_E_INVALID, "hrt_compute_channel_precoder: NULL argument");
    if (nrx > UINT32_MAX || ntx > UINT32_MAX)
        return hrt_fail(HRT_E_INVALID, "hrt_compute_channel_precoder: num_rx or num_tx > 2^32");
    hrt_precoder_spec pc;
    memset(&pc, 0, sizeof pc);
    pc.num_rx = (uint32_t)nrx; pc.num_tx = (uint32_t)ntx;
    pc.nr = (uint32_t)nr; pc.nt = (uint32_t)nt;
    pc.num_times = spec->num_times; pc.num_freqs = spec->num_freqs;
    pc.kind = kind; pc.norm = norm; pc.flags = flags;
    pc.noise = noise; pc.power = power; pc.regularization = regularization;
    /* (num_rx and num_tx 0: ch_drop_in_check's refusal, below, as in hrt_compute_array_channel) */
    if (nrx && ntx && (rc = pc_check(&pc, "hrt_compute_channel_precoder"))) return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = spec;
    job.out_bytes = (uint64_t)nrx * ntx * nr * nt * 2u * spec->num_times * spec->num_freqs * 8u;
    job.scratch_bytes = ac_job_scratch;
    job.run = ac_job_run;
    job.deliver = pc_job_deliver;
    job.aux = &pc;
    return ac_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, rx_el, nr, tx_el, nt, f_a,
                      out, stats, t_begin, "hrt_array_channel", "hrt_compute_channel_precoder");
}

/* ------------------------------------------------------------------ codebook selection (hrt_codebook_select) */

/* the checks of a codebook selection call (`who`); device pointers are not read */
static int cs_check(const hrt_codebook_spec *sp, const char *who)
{
    if (!sp) return hrt_fail(HRT_E_INVALID, "%s: NULL spec", who);
    if (sp->num_rx == 0 || sp->num_tx == 0 || sp->num_times == 0 || sp->num_freqs == 0)
        return hrt_fail(HRT_E_INVALID, "%s: num_rx, num_tx, num_times and num_freqs must be > 0", who);
    if (sp->nr < 1 || sp->nr > HRT_CS_MAX_NR || sp->nt < 1 || sp->nt > HRT_CS_MAX_NT)
        return hrt_fail(HRT_E_INVALID, "%s: nr = %u and nt = %u (nr 1 .. %u, nt 1 .. %u)", who, sp->nr, sp->nt,
                        HRT_CS_MAX_NR, HRT_CS_MAX_NT);
    if (sp->layers < 1 || sp->layers > HRT_CS_MAX_L || sp->layers > sp->nt)
        return hrt_fail(HRT_E_INVALID, "%s: layers = %u (1 .. min(%u, nt = %u))", who, sp->layers, HRT_CS_MAX_L,
                        sp->nt);
    if (sp->entries < 1 || sp->entries > HRT_CS_MAX_C)
        return hrt_fail(HRT_E_INVALID, "%s: entries = %u (1 .. %u)", who, sp->entries, HRT_CS_MAX_C);
    if (sp->subband < 1 || sp->subband > sp->num_freqs)
        return hrt_fail(HRT_E_INVALID, "%s: subband = %u (1 .. num_freqs = %u)", who, sp->subband, sp->num_freqs);
    if (sp->metric != HRT_CS_POWER && sp->metric != HRT_CS_CAPACITY)
        return hrt_fail(HRT_E_INVALID, "%s: metric = %u is neither HRT_CS_POWER nor HRT_CS_CAPACITY", who, sp->metric);
    if (sp->flags & ~(HRT_CS_TABLE | HRT_CS_EFFECTIVE))
        return hrt_fail(HRT_E_INVALID, "%s: flags = 0x%x has unknown bits", who, sp->flags);
    if (sp->metric == HRT_CS_CAPACITY && !pc_positive(sp->noise))
        return hrt_fail(HRT_E_INVALID, "%s: noise = %g must be finite and > 0", who, (double)sp->noise);
    const uint64_t grid = (uint64_t)sp->num_times * sp->num_freqs;   /* < 2^64 */
    if (grid >= (1ull << 31) || (uint64_t)sp->num_rx * sp->num_tx >= (1ull << 31) / (2u * grid))
        return hrt_fail(HRT_E_INVALID, "%s: 2^31 points or more", who);
    const uint64_t B = ((uint64_t)sp->num_freqs + sp->subband - 1u) / sp->subband;
    /* (B <= K, so the points check above bounds num_rx num_tx 2 T B by 2^31 and the product by 2^43) */
    if ((uint64_t)sp->num_rx * sp->num_tx * 2u * sp->num_times * B * sp->entries >= (1ull << 31))
        return hrt_fail(HRT_E_INVALID, "%s: 2^31 table entries or more", who);
    return HRT_OK;
}

/* the regions of the output: byte offsets of index, metric, status, table, effective and the end (hermespy_rt.h) */
static void cs_regions(const hrt_codebook_spec *sp, uint64_t off[6])
{
    const uint64_t links = (uint64_t)sp->num_rx * sp->num_tx;
    const uint64_t B = sp->subband ? ((uint64_t)sp->num_freqs + sp->subband - 1u) / sp->subband : 0u;
    const uint64_t sub = links * 2u * sp->num_times * B, points = links * 2u * sp->num_times * sp->num_freqs;
    off[0] = 0;
    off[1] = off[0] + sub * 4u;
    off[2] = off[1] + sub * 4u;
    off[3] = off[2] + sub * 4u;
    off[4] = off[3] + ((sp->flags & HRT_CS_TABLE) ? sub * sp->entries * 4u : 0u);
    off[5] = off[4] + ((sp->flags & HRT_CS_EFFECTIVE) ? points * sp->nr * sp->layers * 8u : 0u);
}

uint64_t hrt_codebook_out_bytes(const hrt_codebook_spec *spec)
{
    if (!spec) return 0;
    uint64_t off[6];
    cs_regions(spec, off);
    return off[5];
}

int hrt_codebook_select(int device, const hrt_codebook_spec *spec, const void *d_H, const void *d_codebook, void *d_out,
                        void *stream)
{
    int rc = cs_check(spec, "hrt_codebook_select");
    if (rc) return rc;
    if (!d_H || !d_codebook || !d_out) return hrt_fail(HRT_E_INVALID, "hrt_codebook_select: NULL device pointer");
    hrt_kcodebook K;
    memset(&K, 0, sizeof K);
    K.nr = spec->nr; K.nt = spec->nt; K.l = spec->layers; K.c = spec->entries;
    K.ct = hrt_codebook_tile(K.nt, K.l);
    K.capacity = spec->metric == HRT_CS_CAPACITY;
    K.T = spec->num_times; K.K = spec->num_freqs; K.S = spec->subband;
    K.B = (K.K + K.S - 1u) / K.S;
    K.n0 = K.capacity ? spec->noise : 1.f;
    K.pts = 2ull * K.T * K.K;
    K.subbands = (uint64_t)spec->num_rx * spec->num_tx * 2u * K.T * K.B;
    K.flags = spec->flags;
    K.out = d_out;                  /* (the kernel places the regions by cs_regions' rule) */
    HRT_HIP(hrt_hip_set_device(device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_codebook(&K, d_H, d_codebook, stream), "codebook selection kernel");
    return HRT_OK;
}

typedef struct {
    hrt_codebook_spec spec;
    const float *codebook;          /* host, complex [entries][nt][layers] */
} cs_job_aux;

/* after the last batch: H stays at d_H; the codebook goes up, selection runs once, only its result comes down */
static int cs_job_deliver(const ch_job *j, int device, const void *d_H, void *out)
{
    const cs_job_aux *a = (const cs_job_aux *)j->aux;
    const uint64_t bytes = hrt_codebook_out_bytes(&a->spec);
    const uint64_t cb_bytes = (uint64_t)a->spec.entries * a->spec.nt * a->spec.layers * 8u;
    void *d_cs = NULL, *d_cb = NULL;
    int rc = hrt_device_malloc(device, &d_cs, bytes);
    if (!rc) rc = hrt_device_malloc(device, &d_cb, cb_bytes);
    if (!rc) rc = hrt_device_upload(device, d_cb, a->codebook, cb_bytes);
    if (!rc) rc = hrt_codebook_select(device, &a->spec, d_H, d_cb, d_cs, NULL);
    if (!rc) rc = hrt_device_sync(device, NULL);
    if (!rc) rc = hrt_device_download(device, out, d_cs, bytes);
    if (d_cb) hrt_device_free(device, d_cb);
    if (d_cs) hrt_device_free(device, d_cs);
    return rc;
}

int hrt_compute_codebook_select(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                                const hrt_channel_spec *spec, const Vec3 *rx_el, size_t nr, const Vec3 *tx_el,
                                size_t nt, double f_a, const float *codebook, uint32_t layers, uint32_t entries,
                                uint32_t subband, uint32_t metric, uint32_t flags, float noise, void *out,
                                hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = ac_counts_check(nr, nt, "hrt_array_channel");
    if (rc) return rc;
    /* (the element pointers stand in for the device ones: array_check tests them for NULL only) */
    const hrt_array_spec a = {(uint32_t)nr, (uint32_t)nt, (const float *)rx_el, (const float *)tx_el, f_a};
    if ((rc = array_check(spec, &a))) return rc;
    if (!out || !codebook) return hrt_fail(HRT_E_INVALID, "hrt_compute_codebook_select: NULL argument");
    if (nrx > UINT32_MAX || ntx > UINT32_MAX)
        return hrt_fail(HRT_E_INVALID, "hrt_compute_codebook_select: num_rx or num_tx > 2^32");
    cs_job_aux aux;
    memset(&aux, 0, sizeof aux);
    aux.codebook = codebook;
    aux.spec.num_rx = (uint32_t)nrx; aux.spec.num_tx = (uint32_t)ntx;
    aux.spec.nr = (uint32_t)nr; aux.spec.nt = (uint32_t)nt;
    aux.spec.num_times = spec->num_times; aux.spec.num_freqs = spec->num_freqs;
    aux.spec.layers = layers; aux.spec.entries = entries; aux.spec.subband = subband;
    aux.spec.metric = metric; aux.spec.flags = flags; aux.spec.noise = noise;
    /* (num_rx and num_tx 0: ch_drop_in_check's refusal, below, as in hrt_compute_array_channel) */
    if (nrx && ntx && (rc = cs_check(&aux.spec, "hrt_compute_codebook_select"))) return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = spec;
    job.out_bytes = (uint64_t)nrx * ntx * nr * nt * 2u * spec->num_times * spec->num_freqs * 8u;
    job.scratch_bytes = ac_job_scratch;
    job.run = ac_job_run;
    job.deliver = cs_job_deliver;
    job.aux = &aux;
    return ac_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, rx_el, nr, tx_el, nt, f_a,
                      out, stats, t_begin, "hrt_array_channel", "hrt_compute_codebook_select");
}

/* ------------------------------------------------------------------ maximum-likelihood detection (hrt_channel_detect) */

/* the checks of a detection call (`who`); device pointers are not read */
static int dt_check(const hrt_detect_spec *sp, const char *who)
{
    if (!sp) return hrt_fail(HRT_E_INVALID, "%s: NULL spec", who);
    if (sp->num_rx == 0 || sp->num_tx == 0 || sp->num_times == 0 || sp->num_freqs == 0)
        return hrt_fail(HRT_E_INVALID, "%s: num_rx, num_tx, num_times and num_freqs must be > 0", who);
    if (sp->nr < 1 || sp->nr > HRT_DT_MAX_NR)
        return hrt_fail(HRT_E_INVALID, "%s: nr = %u (1 .. %u)", who, sp->nr, HRT_DT_MAX_NR);
    if (sp->bits < 1 || sp->bits > HRT_DT_MAX_B)
        return hrt_fail(HRT_E_INVALID, "%s: bits = %u (1 .. %u)", who, sp->bits, HRT_DT_MAX_B);
    if (sp->nt < 1 || sp->nt > HRT_DT_MAX_BITS || sp->nt * sp->bits > HRT_DT_MAX_BITS)
        return hrt_fail(HRT_E_INVALID, "%s: nt = %u streams of %u bits (nt >= 1, nt * bits <= %u)", who, sp->nt,
                        sp->bits, HRT_DT_MAX_BITS);
    if (sp->flags & ~HRT_DT_LLR)
        return hrt_fail(HRT_E_INVALID, "%s: flags = 0x%x has unknown bits", who, sp->flags);
    if (!pc_positive(sp->noise))
        return hrt_fail(HRT_E_INVALID, "%s: noise = %g must be finite and > 0", who, (double)sp->noise);
    const uint64_t grid = (uint64_t)sp->num_times * sp->num_freqs;   /* < 2^64 */
    if (grid > HRT_EQ_MAX_POINTS || (uint64_t)sp->nr * sp->nt * grid > HRT_EQ_MAX_POINTS)
        return hrt_fail(HRT_E_INVALID, "%s: nr * nt * num_times * num_freqs > 2^24", who);
    if ((uint64_t)sp->num_rx * sp->num_tx >= (1ull << 31) / (2u * grid))
        return hrt_fail(HRT_E_INVALID, "%s: 2^31 points or more", who);
    return HRT_OK;
}

uint64_t hrt_detect_out_bytes(const hrt_detect_spec *spec)
{
    if (!spec) return 0;
    const uint64_t points = (uint64_t)spec->num_rx * spec->num_tx * 2u * spec->num_times * spec->num_freqs;
    return points * 12u + ((spec->flags & HRT_DT_LLR) ? points * spec->nt * spec->bits * 4u : 0u);
}

int hrt_channel_detect(int device, const hrt_detect_spec *spec, const void *d_H, const void *d_Y,
                       const void *d_constellation, void *d_out, void *stream)
{
    int rc = dt_check(spec, "hrt_channel_detect");
    if (rc) return rc;
    if (!d_H || !d_Y || !d_constellation || !d_out)
        return hrt_fail(HRT_E_INVALID, "hrt_channel_detect: NULL device pointer");
    hrt_kdetect K;
    memset(&K, 0, sizeof K);
    K.nr = spec->nr; K.nt = spec->nt; K.b = spec->bits;
    K.g = hrt_detect_form(K.nt, K.b);
    K.tiles = hrt_detect_tiles(K.nt, K.b);
    K.llr = (spec->flags & HRT_DT_LLR) != 0u;
    K.n0 = spec->noise;
    K.pts = 2u * spec->num_times * spec->num_freqs;                 /* <= 2^25 */
    K.points = spec->num_rx * spec->num_tx * K.pts;                 /* < 2^31 */
    K.out = d_out;                  /* (the kernel places the regions by hrt_detect_out_bytes' rule) */
    HRT_HIP(hrt_hip_set_device(device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_detect(&K, d_H, d_Y, d_constellation, stream), "detection kernel");
    return HRT_OK;
}

typedef struct {
    hrt_detect_spec spec;
    const float *Y;                 /* host, complex [num_rx][num_tx][nr][2][T][K] */
    const float *constellation;     /* host, complex [2^bits] */
} dt_job_aux;

/* after the last batch: H stays at d_H; Y and the constellation go up, detection runs once, only its result comes
 * down */
static int dt_job_deliver(const ch_job *j, int device, const void *d_H, void *out)
{
    const dt_job_aux *a = (const dt_job_aux *)j->aux;
    const uint64_t bytes = hrt_detect_out_bytes(&a->spec);
    const uint64_t y_bytes = (uint64_t)a->spec.num_rx * a->spec.num_tx * a->spec.nr * 2u * a->spec.num_times
                             * a->spec.num_freqs * 8u;
    const uint64_t s_bytes = 8ull << a->spec.bits;
    void *d_dt = NULL, *d_y = NULL, *d_s = NULL;
    int rc = hrt_device_malloc(device, &d_dt, bytes);
    if (!rc) rc = hrt_device_malloc(device, &d_y, y_bytes);
    if (!rc) rc = hrt_device_malloc(device, &d_s, s_bytes);
    if (!rc) rc = hrt_device_upload(device, d_y, a->Y, y_bytes);
    if (!rc) rc = hrt_device_upload(device, d_s, a->constellation, s_bytes);
    if (!rc) rc = hrt_channel_detect(device, &a->spec, d_H, d_y, d_s, d_dt, NULL);
    if (!rc) rc = hrt_device_sync(device, NULL);
    if (!rc) rc = hrt_device_download(device, out, d_dt, bytes);
    if (d_s) hrt_device_free(device, d_s);
    if (d_y) hrt_device_free(device, d_y);
    if (d_dt) hrt_device_free(device, d_dt);
    return rc;
}

int hrt_compute_channel_detect(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                               const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                               const hrt_channel_spec *spec, const Vec3 *rx_el, size_t nr, const Vec3 *tx_el,
                               size_t nt, double f_a, const float *Y, const float *constellation, uint32_t bits,
                               uint32_t flags, float noise, void *out, hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = ac_counts_check(nr, nt, "hrt_array_channel");
    if (rc) return rc;
    /* (the element pointers stand in for the device ones: array_check tests them for NULL only) */
    const hrt_array_spec a = {(uint32_t)nr, (uint32_t)nt, (const float *)rx_el, (const float *)tx_el, f_a};
    if ((rc = array_check(spec, &a))) return rc;
    if (!out || !Y || !constellation) return hrt_fail(HRT_E_INVALID, "hrt_compute_channel_detect: NULL argument");
    if (nrx > UINT32_MAX || ntx > UINT32_MAX)
        return hrt_fail(HRT_E_INVALID, "hrt_compute_channel_detect: num_rx or num_tx > 2^32");
    dt_job_aux aux;
    memset(&aux, 0, sizeof aux);
    aux.Y = Y;
    aux.constellation = constellation;
    aux.spec.num_rx = (uint32_t)nrx; aux.spec.num_tx = (uint32_t)ntx;
    aux.spec.nr = (uint32_t)nr; aux.spec.nt = (uint32_t)nt;
    aux.spec.num_times = spec->num_times; aux.spec.num_freqs = spec->num_freqs;
    aux.spec.bits = bits; aux.spec.flags = flags; aux.spec.noise = noise;
    /* (num_rx and num_tx 0: ch_drop_in_check's refusal, below, as in hrt_compute_array_channel) */
    if (nrx && ntx && (rc = dt_check(&aux.spec, "hrt_compute_channel_detect"))) return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = spec;
    job.out_bytes = (uint64_t)nrx * ntx * nr * nt * 2u * spec->num_times * spec->num_freqs * 8u;
    job.scratch_bytes = ac_job_scratch;
    job.run = ac_job_run;
    job.deliver = dt_job_deliver;
    job.aux = &aux;
    return ac_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, rx_el, nr, tx_el, nt, f_a,
                      out, stats, t_begin, "hrt_array_channel", "hrt_compute_channel_detect");
}

/* ------------------------------------------------------------------ K-best tree-search detection (hrt_channel_kbest) */

/* the checks of a K-best detection call (`who`); device pointers are not read */
static int kb_check(const hrt_kbest_spec *sp, const char *who)
{
    if (!sp) return hrt_fail(HRT_E_INVALID, "%s: NULL spec", who);
    if (sp->num_rx == 0 || sp->num_tx == 0 || sp->num_times == 0 || sp->num_freqs == 0)
        return hrt_fail(HRT_E_INVALID, "%s: num_rx, num_tx, num_times and num_freqs must be > 0", who);
    if (sp->nr < 1 || sp->nr > HRT_KB_MAX_NR)
        return hrt_fail(HRT_E_INVALID, "%s: nr = %u (1 .. %u)", who, sp->nr, HRT_KB_MAX_NR);
    if (sp->bits < 1 || sp->bits > HRT_KB_MAX_B)
        return hrt_fail(HRT_E_INVALID, "%s: bits = %u (1 .. %u)", who, sp->bits, HRT_KB_MAX_B);
    if (sp->nt < 1 || sp->nt > HRT_KB_MAX_NT || sp->nt * sp->bits > HRT_KB_MAX_BITS)
        return hrt_fail(HRT_E_INVALID, "%s: nt = %u streams of %u bits (1 <= nt <= %u, nt * bits <= %u)", who, sp->nt,
                        sp->bits, HRT_KB_MAX_NT, HRT_KB_MAX_BITS);
    if (!hrt_kbest_k_ok(sp->k))
        return hrt_fail(HRT_E_INVALID, "%s: k = %u (1, 2, 4, .. %u)", who, sp->k, HRT_KB_MAX_K);
    if (sp->flags & ~(HRT_KB_LLR | HRT_KB_SORTED))
        return hrt_fail(HRT_E_INVALID, "%s: flags = 0x%x has unknown bits", who, sp->flags);
    if (!pc_positive(sp->noise))
        return hrt_fail(HRT_E_INVALID, "%s: noise = %g must be finite and > 0", who, (double)sp->noise);
    if (!pc_positive(sp->clip))
        return hrt_fail(HRT_E_INVALID, "%s: clip = %g must be finite and > 0", who, (double)sp->clip);
    const uint64_t grid = (uint64_t)sp->num_times * sp->num_freqs;   /* < 2^64 */
    if (grid > HRT_EQ_MAX_POINTS || (uint64_t)sp->nr * sp->nt * grid > HRT_EQ_MAX_POINTS)
        return hrt_fail(HRT_E_INVALID, "%s: nr * nt * num_times * num_freqs > 2^24", who);
    if ((uint64_t)sp->num_rx * sp->num_tx >= (1ull << 31) / (2u * grid))
        return hrt_fail(HRT_E_INVALID, "%s: 2^31 points or more", who);
    return HRT_OK;
}

uint64_t hrt_kbest_out_bytes(const hrt_kbest_spec *spec)
{
    if (!spec) return 0;
    const uint64_t points = (uint64_t)spec->num_rx * spec->num_tx * 2u * spec->num_times * spec->num_freqs;
    return points * 12u + ((spec->flags & HRT_KB_LLR) ? points * spec->nt * spec->bits * 4u : 0u);
}

int hrt_channel_kbest(int device, const hrt_kbest_spec *spec, const void *d_H, const void *d_Y,
                      const void *d_constellation, void *d_out, void *stream)
{
    int rc = kb_check(spec, "hrt_channel_kbest");
    if (rc) return rc;
    if (!d_H || !d_Y || !d_constellation || !d_out)
        return hrt_fail(HRT_E_INVALID, "hrt_channel_kbest: NULL device pointer");
    hrt_kkbest K;
    memset(&K, 0, sizeof K);
    K.nr = spec->nr; K.nt = spec->nt; K.b = spec->bits; K.k = spec->k;
    K.g = hrt_kbest_form(K.nr, K.nt, K.k);
    K.mk = (K.nr + K.g - 1u) / K.g;
    K.llr = (spec->flags & HRT_KB_LLR) != 0u;
    K.sorted = (spec->flags & HRT_KB_SORTED) != 0u;
    /* (HRT_KBEST_NO_SKIP=1 walks every batch: for measuring the skip, the bytes are the same) */
    const char *ns = getenv("HRT_KBEST_NO_SKIP");
    K.skip = !(ns && ns[0] == '1');
    K.n0 = spec->noise;
    K.clip = spec->clip;
    K.pts = 2u * spec->num_times * spec->num_freqs;                 /* <= 2^25 */
    K.points = spec->num_rx * spec->num_tx * K.pts;                 /* < 2^31 */
    K.out = d_out;                  /* (the kernel places the regions by hrt_kbest_out_bytes' rule) */
    HRT_HIP(hrt_hip_set_device(device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_kbest(&K, d_H, d_Y, d_constellation, stream), "K-best detection kernel");
    return HRT_OK;
}

typedef struct {
    hrt_kbest_spec spec;
    const float *Y;                 /* host, complex [num_rx][num_tx][nr][2][T][K] */
    const float *constellation;     /* host, complex [2^bits] */
} kb_job_aux;

/* after the last batch: H stays at d_H; Y and the constellation go up, detection runs once, only its result comes
 * down */
static int kb_job_deliver(const ch_job *j, int device, const void *d_H, void *out)
{
    const kb_job_aux *a = (const kb_job_aux *)j->aux;
    const uint64_t bytes = hrt_kbest_out_bytes(&a->spec);
    const uint64_t y_bytes = (uint64_t)a->spec.num_rx * a->spec.num_tx * a->spec.nr * 2u * a->spec.num_times
                             * a->spec.num_freqs * 8u;
    const uint64_t s_bytes = 8ull << a->spec.bits;
    void *d_kb = NULL, *d_y = NULL, *d_s = NULL;
    int rc = hrt_device_malloc(device, &d_kb, bytes);
    if (!rc) rc = hrt_device_malloc(device, &d_y, y_bytes);
    if (!rc) rc = hrt_device_malloc(device, &d_s, s_bytes);
    if (!rc) rc = hrt_device_upload(device, d_y, a->Y, y_bytes);
    if (!rc) rc = hrt_device_upload(device, d_s, a->constellation, s_bytes);
    if (!rc) rc = hrt_channel_kbest(device, &a->spec, d_H, d_y, d_s, d_kb, NULL);
    if (!rc) rc = hrt_device_sync(device, NULL);
    if (!rc) rc = hrt_device_download(device, out, d_kb, bytes);
    if (d_s) hrt_device_free(device, d_s);
    if (d_y) hrt_device_free(device, d_y);
    if (d_kb) hrt_device_free(device, d_kb);
    return rc;
}

int hrt_compute_channel_kbest(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                              const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                              const hrt_channel_spec *spec, const Vec3 *rx_el, size_t nr, const Vec3 *tx_el,
                              size_t nt, double f_a, const float *Y, const float *constellation, uint32_t bits,
                              uint32_t flags, uint32_t k, float noise, float clip, void *out, hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = ac_counts_check(nr, nt, "hrt_array_channel");
    if (rc) return rc;
    /* (the element pointers stand in for the device ones: array_check tests them for NULL only) */
    const hrt_array_spec a = {(uint32_t)nr, (uint32_t)nt, (const float *)rx_el, (const float *)tx_el, f_a};
    if ((rc = array_check(spec, &a))) return rc;
    if (!out || !Y || !constellation) return hrt_fail(HRT_E_INVALID, "hrt_compute_channel_kbest: NULL argument");
    if (nrx > UINT32_MAX || ntx > UINT32_MAX)
        return hrt_fail(HRT_E_INVALID, "hrt_compute_channel_kbest: num_rx or num_tx > 2^32");
    kb_job_aux aux;
    memset(&aux, 0, sizeof aux);
    aux.Y = Y;
    aux.constellation = constellation;
    aux.spec.num_rx = (uint32_t)nrx; aux.spec.num_tx = (uint32_t)ntx;
    aux.spec.nr = (uint32_t)nr; aux.spec.nt = (uint32_t)nt;
    aux.spec.num_times = spec->num_times; aux.spec.num_freqs = spec->num_freqs;
    aux.spec.bits = bits; aux.spec.flags = flags; aux.spec.k = k; aux.spec.noise = noise; aux.spec.clip = clip;
    /* (num_rx and num_tx 0: ch_drop_in_check's refusal, below, as in hrt_compute_array_channel) */
    if (nrx && ntx && (rc = kb_check(&aux.spec, "hrt_compute_channel_kbest"))) return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = spec;
    job.out_bytes = (uint64_t)nrx * ntx * nr * nt * 2u * spec->num_times * spec->num_freqs * 8u;
    job.scratch_bytes = ac_job_scratch;
    job.run = ac_job_run;
    job.deliver = kb_job_deliver;
    job.aux = &aux;
    return ac_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, rx_el, nr, tx_el, nt, f_a,
                      out, stats, t_begin, "hrt_array_channel", "hrt_compute_channel_kbest");
}

/* ------------------------------------------------------------------ power statistics (hrt_power_profiles) */

#define HRT_PW_TARGET_GROUPS 2048u          /* workgroups of the moments pass worth launching (8 per CU) */
#define HRT_PW_PARTIAL_MAX (512ull << 20)   /* partial moments beyond one chunk: at most this */

static uint64_t align256(uint64_t n)
{
    return (n + 255u) / 256u * 256u;
}

/* the checks of a power spec that need no problem */
static int power_check(const hrt_power_spec *spec)
{
    if (!spec) return hrt_fail(HRT_E_INVALID, "hrt_power_profiles: NULL spec");
    int rc = parts_check(spec->parts, "hrt_power_profiles");
    if (rc) return rc;
    const uint32_t Ld = spec->num_delay_bins, Nth = spec->num_zenith_bins, Nph = spec->num_azimuth_bins;
    if (Ld > HRT_PW_MAX_DELAY_BINS)
        return hrt_fail(HRT_E_INVALID, "hrt_power_profiles: num_delay_bins = %u > 2^16", Ld);
    if (Ld > 0 && !isfinite(spec->tau0_s))
        return hrt_fail(HRT_E_INVALID, "hrt_power_profiles: tau0 must be finite");
    if (Ld > 0 && (!isfinite(spec->dtau_s) || !(spec->dtau_s > 0.0)))
        return hrt_fail(HRT_E_INVALID, "hrt_power_profiles: dtau must be finite and > 0");
    if ((Nth == 0) != (Nph == 0))
        return hrt_fail(HRT_E_INVALID,
                        "hrt_power_profiles: num_zenith_bins = %u and num_azimuth_bins = %u (both 0 or both >= 1)",
                        Nth, Nph);
    if ((uint64_t)Nth * Nph > HRT_PW_MAX_ANGLE_BINS)
        return hrt_fail(HRT_E_INVALID, "hrt_power_profiles: num_zenith_bins * num_azimuth_bins = %llu > 2^14",
                        (unsigned long long)Nth * Nph);
    return HRT_OK;
}

/* the checks that need the link count */
static int power_links_check(uint64_t nrx, uint64_t ntx, const hrt_power_spec *spec)
{
    if (nrx > 65535u || ntx > 65535u || nrx * ntx > 65535u)
        return hrt_fail(HRT_E_INVALID, "hrt_power_profiles: num_rx * num_tx = %llu > 65535",
                        (unsigned long long)(nrx * ntx));
    const uint64_t bins = nrx * ntx * (spec->num_delay_bins + 2ull * spec->num_zenith_bins * spec->num_azimuth_bins);
    if (bins > HRT_PW_MAX_LINK_BINS)
        return hrt_fail(HRT_E_INVALID,
                        "hrt_power_profiles: num_rx * num_tx * (num_delay_bins + 2 num_zenith_bins num_azimuth_bins)"
                        " = %llu > 2^26", (unsigned long long)bins);
    return HRT_OK;
}

uint64_t hrt_power_out_doubles(size_t num_rx, size_t num_tx, const hrt_power_spec *spec)
{
    if (!spec) return 0;
    const uint64_t per_pol = HRT_POWER_FIELDS + (uint64_t)spec->num_delay_bins +
                             2ull * spec->num_zenith_bins * spec->num_azimuth_bins;
    return (uint64_t)num_rx * num_tx * 2u * per_pol;
}

/* the chunking and scratch of one power call: a pure function of the problem, the shard and the spec */
static int pw_plan(const hrt_problem *p, const hrt_shard *s, const hrt_power_spec *spec, hrt_kpower *K,
                   uint64_t *bytes, uint64_t *off_total, uint64_t *off_hist)
{
    int rc = power_check(spec);
    if (rc) return rc;
    memset(K, 0, sizeof *K);
    if ((rc = ps_view(p, s, spec->parts, "hrt_power_profiles", &K->v))) return rc;
    if ((rc = power_links_check(K->v.nrx, K->v.ntx, spec))) return rc;
    ps_shard(s, &K->sh);
    K->Ld = spec->num_delay_bins; K->Nth = spec->num_zenith_bins; K->Nph = spec->num_azimuth_bins;
    K->nbins = K->Ld + 2u * K->Nth * K->Nph;
    K->tau0 = spec->tau0_s; K->dtau = spec->dtau_s;
    const uint64_t links = (uint64_t)K->v.nrx * K->v.ntx;
    const uint64_t per_chunk = links * 2u * HRT_POWER_FIELDS * 8u;
    (void)ps_chunks(&K->v, spec->parts, links, HRT_PW_TARGET_GROUPS, per_chunk, HRT_PW_PARTIAL_MAX, UINT32_MAX);
    *off_total = align256(K->v.nchunks * per_chunk);
    *off_hist = *off_total + align256(links * 2u * 8u);
    *bytes = ps_seg_bytes(&K->v) + *off_hist + links * 2u * K->nbins * 8u;
    return HRT_OK;
}

int hrt_power_profiles_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_power_spec *spec,
                                     uint64_t *out)
{
    hrt_kpower K;
    uint64_t bytes = 0, ot, oh;
    const int rc = pw_plan(p, s, spec, &K, &bytes, &ot, &oh);
    return ps_scratch_out(rc, bytes, out, "hrt_power_profiles_scratch_bytes");
}

int hrt_power_profiles(const hrt_problem *p, const hrt_shard *s, const void *d_workspace, const hrt_power_spec *spec,
                       void *d_scratch, uint64_t scratch_bytes, double *d_out, int accumulate, void *stream)
{
    hrt_kpower K;
    uint64_t need = 0, off_total = 0, off_hist = 0;
    int rc = pw_plan(p, s, spec, &K, &need, &off_total, &off_hist);
    if (rc) return rc;
    float *partial = NULL;
    if ((rc = ps_bind(&K.v, need, d_workspace, d_scratch, scratch_bytes, d_out, accumulate, "hrt_power_profiles",
                      "hrt_power_profiles_scratch_bytes", &partial)))
        return rc;
    K.partial = (double *)partial;
    K.total = (double *)((uint8_t *)partial + off_total);
    K.hist = (unsigned long long *)((uint8_t *)partial + off_hist);
    K.out = d_out;
    HRT_HIP(hrt_hip_set_device(p->device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_power(&K, stream), "power kernels");
    return HRT_OK;
}

static int pw_job_scratch(const ch_job *j, const hrt_problem *p, const hrt_shard *s, uint64_t *out)
{
    return hrt_power_profiles_scratch_bytes(p, s, j->spec, out);
}

static int pw_job_run(const ch_job *j, const hrt_problem *p, const hrt_shard *s, const void *d_ws, void *d_scratch,
                      uint64_t scratch_bytes, void *d_out, int accumulate)
{
    return hrt_power_profiles(p, s, d_ws, j->spec, d_scratch, scratch_bytes, d_out, accumulate, NULL);
}

int hrt_compute_power_profiles(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                               const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                               const hrt_power_spec *spec, double *out, hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = power_check(spec);
    if (rc) return rc;
    if ((rc = power_links_check(nrx, ntx, spec))) return rc;
    if ((rc = ch_drop_in_check(scene, rx_pos, tx_pos, rx_vel, tx_vel, nrx, ntx, np, nb, out,
                               "hrt_compute_power_profiles")))
        return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = spec;
    job.out_bytes = hrt_power_out_doubles(nrx, ntx, spec) * 8u;
    job.scratch_bytes = pw_job_scratch;
    job.run = pw_job_run;
    return ch_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, out, stats, t_begin);
}

/* ------------------------------------------------------------------ spatial covariance matrices (hrt_array_covariance) */

#define HRT_CV_TARGET_GROUPS 2048u          /* workgroups of the partial kernel worth launching (8 per CU) */
#define HRT_CV_PARTIAL_MAX (512ull << 20)   /* partial sums beyond one chunk: at most this (the pair families' cap) */

/* the checks of a covariance call that need no problem (device pointers are not read); n[0], n[1]: the elements of the
 * RX and the TX side, 0 for a side that is not asked for */
static int cov_check(const hrt_covariance_spec *spec, const hrt_array_spec *a, uint32_t n[2])
{
    if (!spec) return hrt_fail(HRT_E_INVALID, "hrt_array_covariance: NULL spec");
    if (!a) return hrt_fail(HRT_E_INVALID, "hrt_array_covariance: NULL arrays");
    int rc = parts_check(spec->parts, "hrt_array_covariance");
    if (rc) return rc;
    if (spec->sides == 0 || (spec->sides & ~(uint32_t)(HRT_COV_RX | HRT_COV_TX)))
        return hrt_fail(HRT_E_INVALID, "hrt_array_covariance: sides 0x%x (HRT_COV_RX | HRT_COV_TX)", spec->sides);
    n[0] = (spec->sides & HRT_COV_RX) ? a->num_rx_elements : 0u;
    n[1] = (spec->sides & HRT_COV_TX) ? a->num_tx_elements : 0u;
    if ((spec->sides & HRT_COV_RX) && (n[0] < 1 || n[0] > HRT_CV_MAX_ELEMENTS))
        return hrt_fail(HRT_E_INVALID, "hrt_array_covariance: num_rx_elements = %u (1 .. %u)", n[0], HRT_CV_MAX_ELEMENTS);
    if ((spec->sides & HRT_COV_TX) && (n[1] < 1 || n[1] > HRT_CV_MAX_ELEMENTS))
        return hrt_fail(HRT_E_INVALID, "hrt_array_covariance: num_tx_elements = %u (1 .. %u)", n[1], HRT_CV_MAX_ELEMENTS);
    if (!isfinite(a->array_frequency_hz) || !(a->array_frequency_hz > 0.0))
        return hrt_fail(HRT_E_INVALID, "hrt_array_covariance: the array frequency must be finite and > 0");
    if ((spec->sides & HRT_COV_RX) && !a->rx_elements)
        return hrt_fail(HRT_E_INVALID, "hrt_array_covariance: NULL rx_elements");
    if ((spec->sides & HRT_COV_TX) && !a->tx_elements)
        return hrt_fail(HRT_E_INVALID, "hrt_array_covariance: NULL tx_elements");
    return HRT_OK;
}

/* the checks that need the link count */
static int cov_links_check(uint64_t nrx, uint64_t ntx, const uint32_t n[2])
{
    if (nrx > 65535u || ntx > 65535u || nrx * ntx > 65535u)
        return hrt_fail(HRT_E_INVALID, "hrt_array_covariance: num_rx * num_tx = %llu > 65535",
                        (unsigned long long)(nrx * ntx));
    const uint64_t outs = nrx * ntx * 2u * ((uint64_t)n[0] * n[0] + (uint64_t)n[1] * n[1]);
    if (outs > HRT_CV_MAX_OUTPUTS)
        return hrt_fail(HRT_E_INVALID, "hrt_array_covariance: num_rx * num_tx * 2 * (Nr^2 + Nt^2) = %llu > 2^26",
                        (unsigned long long)outs);
    return HRT_OK;
}

uint64_t hrt_covariance_out_floats(size_t num_rx, size_t num_tx, const hrt_array_spec *arrays,
                                   const hrt_covariance_spec *spec)
{
    if (!arrays || !spec) return 0;
    const uint64_t nr = (spec->sides & HRT_COV_RX) ? arrays->num_rx_elements : 0u;
    const uint64_t nt = (spec->sides & HRT_COV_TX) ? arrays->num_tx_elements : 0u;
    return (uint64_t)num_rx * num_tx * 2u * (nr * nr + nt * nt) * 2u;
}

/* the tiling of one covariance call: a pure function of the problem, the shard, the spec and the array sizes */
static int cov_plan(const hrt_problem *p, const hrt_shard *s, const hrt_covariance_spec *spec, const hrt_array_spec *a,
                    hrt_kcov *K, uint64_t *bytes)
{
    uint32_t n[2];
    int rc = cov_check(spec, a, n);
    if (rc) return rc;
    memset(K, 0, sizeof *K);
    if ((rc = ps_view(p, s, spec->parts, "hrt_array_covariance", &K->v))) return rc;
    if ((rc = cov_links_check(K->v.nrx, K->v.ntx, n))) return rc;
    ps_shard(s, &K->sh);
    K->sides = spec->sides;
    for (int q = 0; q < 2; ++q) {
        const uint32_t nb = (n[q] + HRT_CV_BLOCK - 1u) / HRT_CV_BLOCK;
        K->n[q] = n[q];
        K->nblk[q] = nb * (nb + 1u) / 2u;
    }
    K->fa_c = a->array_frequency_hz / HRT_SPEED_OF_LIGHT;
    const uint64_t links = (uint64_t)K->v.nrx * K->v.ntx, blocks = K->nblk[0] + K->nblk[1];
    const uint64_t per_chunk = links * 2u * blocks * HRT_CV_BLOCK * HRT_CV_BLOCK * 8u;
    *bytes = ps_chunks(&K->v, spec->parts, links * blocks, HRT_CV_TARGET_GROUPS, per_chunk, HRT_CV_PARTIAL_MAX, 65535u);
    return HRT_OK;
}

int hrt_array_covariance_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_covariance_spec *spec,
                                       const hrt_array_spec *arrays, uint64_t *out)
{
    hrt_kcov K;
    uint64_t bytes = 0;
    const int rc = cov_plan(p, s, spec, arrays, &K, &bytes);
    return ps_scratch_out(rc, bytes, out, "hrt_array_covariance_scratch_bytes");
}

int hrt_array_covariance(const hrt_problem *p, const hrt_shard *s, const void *d_workspace,
                         const hrt_covariance_spec *spec, const hrt_array_spec *arrays, void *d_scratch,
                         uint64_t scratch_bytes, float *d_out, int accumulate, void *stream)
{
    hrt_kcov K;
    uint64_t need = 0;
    int rc = cov_plan(p, s, spec, arrays, &K, &need);
    if (rc) return rc;
    if ((rc = ps_bind(&K.v, need, d_workspace, d_scratch, scratch_bytes, d_out, accumulate, "hrt_array_covariance",
                      "hrt_array_covariance_scratch_bytes", &K.partial)))
        return rc;
    K.el[0] = K.n[0] ? arrays->rx_elements : NULL;
    K.el[1] = K.n[1] ? arrays->tx_elements : NULL;
    K.out = d_out;
    HRT_HIP(hrt_hip_set_device(p->device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_covariance(&K, stream), "covariance kernels");
    return HRT_OK;
}

static int cv_job_scratch(const ch_job *j, const hrt_problem *p, const hrt_shard *s, uint64_t *out)
{
    const hrt_array_spec a = ac_job_arrays(j);
    return hrt_array_covariance_scratch_bytes(p, s, j->spec, &a, out);
}

static int cv_job_run(const ch_job *j, const hrt_problem *p, const hrt_shard *s, const void *d_ws, void *d_scratch,
                      uint64_t scratch_bytes, void *d_out, int accumulate)
{
    const hrt_array_spec a = ac_job_arrays(j);
    return hrt_array_covariance(p, s, d_ws, j->spec, &a, d_scratch, scratch_bytes, d_out, accumulate, NULL);
}

int hrt_compute_array_covariance(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                 const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                                 const hrt_covariance_spec *spec, const Vec3 *rx_el, size_t nr, const Vec3 *tx_el,
                                 size_t nt, double f_a, float *out, hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    if (!spec) return hrt_fail(HRT_E_INVALID, "hrt_array_covariance: NULL spec");
    /* a side that is not asked for needs no elements: its count and pointer are not looked at */
    if (!(spec->sides & HRT_COV_RX)) { nr = 0; rx_el = NULL; }
    if (!(spec->sides & HRT_COV_TX)) { nt = 0; tx_el = NULL; }
    if (nr > HRT_CV_MAX_ELEMENTS)
        return hrt_fail(HRT_E_INVALID, "hrt_array_covariance: num_rx_elements = %zu (1 .. %u)", nr, HRT_CV_MAX_ELEMENTS);
    if (nt > HRT_CV_MAX_ELEMENTS)
        return hrt_fail(HRT_E_INVALID, "hrt_array_covariance: num_tx_elements = %zu (1 .. %u)", nt, HRT_CV_MAX_ELEMENTS);
    /* (the element pointers stand in for the device ones: cov_check tests them for NULL only) */
    const hrt_array_spec a = {(uint32_t)nr, (uint32_t)nt, (const float *)rx_el, (const float *)tx_el, f_a};
    uint32_t n[2];
    int rc = cov_check(spec, &a, n);
    if (rc) return rc;
    if ((rc = cov_links_check(nrx, ntx, n))) return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = spec;
    job.out_bytes = hrt_covariance_out_floats(nrx, ntx, &a, spec) * 4u;
    job.scratch_bytes = cv_job_scratch;
    job.run = cv_job_run;
    return ac_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, rx_el, nr, tx_el, nt, f_a,
                      out, stats, t_begin, "hrt_array_covariance", "hrt_compute_array_covariance");
}

/* ------------------------------------------------------------------ the K strongest paths per link (hrt_dominant_paths) */

#define HRT_DM_TARGET_GROUPS 2048u          /* workgroups of the partial kernel worth launching (8 per CU) */
#define HRT_DM_PARTIAL_MAX (512ull << 20)   /* candidate lists beyond one chunk: at most this */

/* the checks of a dominant spec that need no problem */
static int dominant_check(const hrt_dominant_spec *spec)
{
    if (!spec) return hrt_fail(HRT_E_INVALID, "hrt_dominant_paths: NULL spec");
    if (spec->max_paths == 0 || spec->max_paths > HRT_DM_MAX_PATHS)
        return hrt_fail(HRT_E_INVALID, "hrt_dominant_paths: max_paths = %u (1 .. %u)", spec->max_paths,
                        HRT_DM_MAX_PATHS);
    return parts_check(spec->parts, "hrt_dominant_paths");
}

/* the checks that need the link count */
static int dominant_links_check(uint64_t nrx, uint64_t ntx, const hrt_dominant_spec *spec)
{
    if (nrx > 65535u || ntx > 65535u || nrx * ntx > 65535u)
        return hrt_fail(HRT_E_INVALID, "hrt_dominant_paths: num_rx * num_tx = %llu > 65535",
                        (unsigned long long)(nrx * ntx));
    if (nrx * ntx * spec->max_paths > HRT_DM_MAX_LINK_PATHS)
        return hrt_fail(HRT_E_INVALID, "hrt_dominant_paths: num_rx * num_tx * max_paths = %llu > 2^22",
                        (unsigned long long)(nrx * ntx * spec->max_paths));
    return HRT_OK;
}

uint64_t hrt_dominant_out_bytes(size_t num_rx, size_t num_tx, const hrt_dominant_spec *spec)
{
    if (dominant_check(spec) || dominant_links_check(num_rx, num_tx, spec)) return 0;
    return (uint64_t)num_rx * num_tx * (16u + (uint64_t)spec->max_paths * sizeof(hrt_dominant_path));
}

/* the chunking and scratch of one dominant call: a pure function of the problem, the shard and the spec; off[0 .. 3]
 * are where la, ca, lb and cb start behind seg (hrt_dominant.h) */
static int dm_plan(const hrt_problem *p, const hrt_shard *s, const hrt_dominant_spec *spec, hrt_kdominant *K,
                   uint64_t *bytes, uint64_t off[4])
{
    int rc = dominant_check(spec);
    if (rc) return rc;
    memset(K, 0, sizeof *K);
    if ((rc = ps_view(p, s, spec->parts, "hrt_dominant_paths", &K->v))) return rc;
    if ((rc = dominant_links_check(K->v.nrx, K->v.ntx, spec))) return rc;
    if (s->num_paths >> HRT_DM_PATH_BITS)
        return hrt_fail(HRT_E_INVALID, "hrt_dominant_paths: num_paths = %llu >= 2^48",
                        (unsigned long long)s->num_paths);
    ps_shard(s, &K->sh);
    K->K = spec->max_paths;
    const uint64_t links = (uint64_t)K->v.nrx * K->v.ntx;
    const uint64_t per_chunk = links * (K->K * sizeof(hrt_dm_cand) + 8u);
    (void)ps_chunks(&K->v, spec->parts, links, HRT_DM_TARGET_GROUPS, per_chunk, HRT_DM_PARTIAL_MAX,
                    HRT_DM_MAX_CHUNKS);
    K->nmid = K->v.nchunks > HRT_DM_FANIN ? (K->v.nchunks + HRT_DM_FANIN - 1u) / HRT_DM_FANIN : 0u;
    off[0] = 0;
    off[1] = off[0] + align256(links * K->v.nchunks * K->K * sizeof(hrt_dm_cand));
    off[2] = off[1] + align256(links * K->v.nchunks * 8u);
    off[3] = off[2] + align256(links * K->nmid * K->K * sizeof(hrt_dm_cand));
    *bytes = ps_seg_bytes(&K->v) + off[3] + align256(links * K->nmid * 8u);
    return HRT_OK;
}

int hrt_dominant_paths_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_dominant_spec *spec,
                                     uint64_t *out)
{
    hrt_kdominant K;
    uint64_t bytes = 0, off[4];
    const int rc = dm_plan(p, s, spec, &K, &bytes, off);
    return ps_scratch_out(rc, bytes, out, "hrt_dominant_paths_scratch_bytes");
}

int hrt_dominant_paths(const hrt_problem *p, const hrt_shard *s, const void *d_workspace,
                       const hrt_dominant_spec *spec, void *d_scratch, uint64_t scratch_bytes, void *d_out,
                       int accumulate, void *stream)
{
    hrt_kdominant K;
    uint64_t need = 0, off[4];
    int rc = dm_plan(p, s, spec, &K, &need, off);
    if (rc) return rc;
    float *partial = NULL;
    if ((rc = ps_bind(&K.v, need, d_workspace, d_scratch, scratch_bytes, d_out, accumulate, "hrt_dominant_paths",
                      "hrt_dominant_paths_scratch_bytes", &partial)))
        return rc;
    K.la = (hrt_dm_cand *)((uint8_t *)partial + off[0]);
    K.ca = (uint64_t *)((uint8_t *)partial + off[1]);
    K.lb = (hrt_dm_cand *)((uint8_t *)partial + off[2]);
    K.cb = (uint64_t *)((uint8_t *)partial + off[3]);
    K.out = (uint8_t *)d_out;
    HRT_HIP(hrt_hip_set_device(p->device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_dominant(&K, stream), "dominant kernels");
    return HRT_OK;
}

static int dm_job_scratch(const ch_job *j, const hrt_problem *p, const hrt_shard *s, uint64_t *out)
{
    return hrt_dominant_paths_scratch_bytes(p, s, j->spec, out);
}

static int dm_job_run(const ch_job *j, const hrt_problem *p, const hrt_shard *s, const void *d_ws, void *d_scratch,
                      uint64_t scratch_bytes, void *d_out, int accumulate)
{
    return hrt_dominant_paths(p, s, d_ws, j->spec, d_scratch, scratch_bytes, d_out, accumulate, NULL);
}

/* the kept records' tri: the row of the device table -> the flat index of the reference's (mesh, face) loop */
static int dm_job_finish(const ch_job *j, const hrt_problem *p, void *out)
{
    const hrt_dominant_spec *spec = j->spec;
    const uint64_t links = (uint64_t)p->num_rx * p->num_tx;
    const uint64_t *hdr = out;
    hrt_dominant_path *recs = (hrt_dominant_path *)((uint8_t *)out + 16u * links);
    for (uint64_t l = 0; l < links; ++l)
        for (uint64_t k = 0; k < hdr[2 * l] && k < spec->max_paths; ++k) {
            hrt_dominant_path *r = recs + l * spec->max_paths + k;
            if (r->bounce >= 0 && r->tri < p->num_tri) r->tri = p->accel.orig[r->tri];
        }
    return HRT_OK;
}

int hrt_compute_dominant_paths(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                               const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                               const hrt_dominant_spec *spec, void *out, hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = dominant_check(spec);
    if (rc) return rc;
    if ((rc = dominant_links_check(nrx, ntx, spec))) return rc;
    if ((rc = ch_drop_in_check(scene, rx_pos, tx_pos, rx_vel, tx_vel, nrx, ntx, np, nb, out,
                               "hrt_compute_dominant_paths")))
        return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = spec;
    job.out_bytes = hrt_dominant_out_bytes(nrx, ntx, spec);
    job.scratch_bytes = dm_job_scratch;
    job.run = dm_job_run;
    job.finish = dm_job_finish;
    return ch_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, out, stats, t_begin);
}

/* ------------------------------------------------------------------ array channels of path lists (hrt_sparse_array_channel) */

/* the checks of a sparse spec (`who`) */
static int sparse_check(const hrt_sparse_spec *sp, const char *who)
{
    if (!sp) return hrt_fail(HRT_E_INVALID, "%s: NULL spec", who);
    const uint64_t links = (uint64_t)sp->num_rx * sp->num_tx;
    if (links == 0 || links > HRT_SP_MAX_LINKS)
        return hrt_fail(HRT_E_INVALID, "%s: num_rx * num_tx = %llu (1 .. 65535)", who, (unsigned long long)links);
    if (sp->max_paths == 0 || sp->max_paths > HRT_DM_MAX_PATHS)
        return hrt_fail(HRT_E_INVALID, "%s: max_paths = %u (1 .. %u)", who, sp->max_paths, HRT_DM_MAX_PATHS);
    if (links * sp->max_paths > HRT_DM_MAX_LINK_PATHS)
        return hrt_fail(HRT_E_INVALID, "%s: num_rx * num_tx * max_paths = %llu > 2^22", who,
                        (unsigned long long)(links * sp->max_paths));
    const hrt_channel_spec grid = {sp->f0_hz, sp->df_hz, sp->num_freqs, sp->t0_s, sp->dt_s, sp->num_times,
                                   HRT_CHANNEL_LOS | HRT_CHANNEL_SCATTER};
    return spec_check(&grid);
}

uint64_t hrt_sparse_paths_bytes(const hrt_sparse_spec *spec)
{
    if (sparse_check(spec, "hrt_sparse_paths_bytes")) return 0;
    return (uint64_t)spec->num_rx * spec->num_tx * (16u + (uint64_t)spec->max_paths * sizeof(hrt_dominant_path));
}

uint64_t hrt_sparse_out_bytes(const hrt_sparse_spec *spec, uint32_t nr, uint32_t nt)
{
    if (sparse_check(spec, "hrt_sparse_out_bytes")) return 0;
    return (uint64_t)spec->num_rx * spec->num_tx * nr * nt * 2u * spec->num_times * spec->num_freqs * 8u;
}

int hrt_sparse_array_channel(int device, const hrt_sparse_spec *spec, const float *d_rx_el, uint32_t nr,
                             const float *d_tx_el, uint32_t nt, double fa_hz, const void *d_paths, float *d_out,
                             int accumulate, void *stream)
{
    _Static_assert(sizeof(hrt_dominant_path) == HRT_SP_SLOT_BYTES &&
                   offsetof(hrt_dominant_path, a_te_re) == HRT_SP_SLOT_FIRST, "hrt_dominant_path: the staged floats");
    int rc = sparse_check(spec, "hrt_sparse_array_channel");
    if (rc) return rc;
    if (!d_paths || !d_out) return hrt_fail(HRT_E_INVALID, "hrt_sparse_array_channel: NULL device pointer");
    const uint64_t grid = (uint64_t)spec->num_times * spec->num_freqs;
    const hrt_array_spec a = {nr, nt, d_rx_el, d_tx_el, fa_hz};
    if ((rc = arrays_check(&a, grid, "num_times * num_freqs", "hrt_sparse_array_channel"))) return rc;
    if ((uintptr_t)d_paths % 8u) return hrt_fail(HRT_E_INVALID, "hrt_sparse_array_channel: d_paths is not 8-byte aligned");
    if (accumulate != 0 && accumulate != 1)
        return hrt_fail(HRT_E_INVALID, "hrt_sparse_array_channel: accumulate must be 0 or 1");
    hrt_ksparse K;
    memset(&K, 0, sizeof K);
    K.links = spec->num_rx * spec->num_tx;
    K.max_paths = spec->max_paths;
    if ((rc = ac_fields(&a, K.links, grid, "hrt_sparse_array_channel", &K.nr, &K.nt, &K.npairs, &K.g.fa_c))) return rc;
    K.g.K = spec->num_freqs; K.g.T = spec->num_times;
    K.g.K1 = (spec->num_freqs + HRT_CH_K2 - 1) / HRT_CH_K2;
    K.g.rows = K.g.K1 * K.g.T;
    K.g.pblocks = (K.npairs + HRT_AC_PAIRS - 1) / HRT_AC_PAIRS;
    K.g.cblocks = (K.g.rows + HRT_AC_GROWS - 1) / HRT_AC_GROWS;
    K.g.f0 = spec->f0_hz; K.g.df = spec->df_hz; K.g.t0 = spec->t0_s; K.g.dt = spec->dt_s;
    K.accumulate = (uint32_t)accumulate;
    K.rx_el = d_rx_el; K.tx_el = d_tx_el;
    K.paths = (const uint8_t *)d_paths;
    K.out = d_out;
    HRT_HIP(hrt_hip_set_device(device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_sparse_channel(&K, stream), "sparse channel kernel");
    return HRT_OK;
}

/* what the deliver and finish hooks of hrt_compute_sparse_array_channel need */
typedef struct {
    hrt_sparse_spec sp;
    void *paths_out;     /* host, hrt_dominant_out_bytes; may be NULL */
} sp_job;

/* after the last batch: the merged lists stay at d_paths; the channel is evaluated once, and only it (and the lists, if
 * asked for) comes down.  The offsets are ch_compute's upload (ac_job_arrays). */
static int sp_job_deliver(const ch_job *j, int device, const void *d_paths, void *out)
{
    const sp_job *sj = (const sp_job *)j->aux;
    const hrt_array_spec a = ac_job_arrays(j);
    const uint64_t bytes = hrt_sparse_out_bytes(&sj->sp, j->nr, j->nt);
    void *d_H = NULL;
    int rc = hrt_device_malloc(device, &d_H, bytes);
    if (!rc)
        rc = hrt_sparse_array_channel(device, &sj->sp, a.rx_elements, j->nr, a.tx_elements, j->nt, j->fa, d_paths,
                                      (float *)d_H, 0, NULL);
    if (!rc) rc = hrt_device_sync(device, NULL);
    if (!rc) rc = hrt_device_download(device, out, d_H, bytes);
    if (!rc && sj->paths_out) rc = hrt_device_download(device, sj->paths_out, d_paths, j->out_bytes);
    if (d_H) hrt_device_free(device, d_H);
    return rc;
}

static int sp_job_finish(const ch_job *j, const hrt_problem *p, void *out)
{
    (void)out;
    const sp_job *sj = (const sp_job *)j->aux;
    return sj->paths_out ? dm_job_finish(j, p, sj->paths_out) : HRT_OK;
}

int hrt_compute_sparse_array_channel(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                     const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                                     const hrt_dominant_spec *dspec, const hrt_channel_spec *grid, const Vec3 *rx_el,
                                     size_t nr, const Vec3 *tx_el, size_t nt, double f_a, float *out, void *paths_out,
                                     hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = dominant_check(dspec);
    if (rc) return rc;
    if ((rc = dominant_links_check(nrx, ntx, dspec))) return rc;
    if (!grid) return hrt_fail(HRT_E_INVALID, "hrt_compute_sparse_array_channel: NULL grid");
    if ((rc = ac_counts_check(nr, nt, "hrt_sparse_array_channel"))) return rc;
    sp_job sj;
    memset(&sj, 0, sizeof sj);
    sj.sp.f0_hz = grid->f0_hz; sj.sp.df_hz = grid->df_hz; sj.sp.num_freqs = grid->num_freqs;
    sj.sp.t0_s = grid->t0_s; sj.sp.dt_s = grid->dt_s; sj.sp.num_times = grid->num_times;
    sj.sp.num_rx = (uint32_t)nrx; sj.sp.num_tx = (uint32_t)ntx;
    sj.sp.max_paths = dspec->max_paths;
    sj.paths_out = paths_out;
    {   /* the grid and the arrays (the element pointers stand in for the device ones: tested for NULL only) */
        const hrt_channel_spec g = {grid->f0_hz, grid->df_hz, grid->num_freqs, grid->t0_s, grid->dt_s,
                                    grid->num_times, dspec->parts};
        if ((rc = spec_check(&g))) return rc;
        const hrt_array_spec a = {(uint32_t)nr, (uint32_t)nt, (const float *)rx_el, (const float *)tx_el, f_a};
        if ((rc = arrays_check(&a, (uint64_t)g.num_times * g.num_freqs, "num_times * num_freqs",
                               "hrt_sparse_array_channel")))
            return rc;
    }
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = dspec;
    job.out_bytes = (uint64_t)nrx * ntx * (16u + (uint64_t)dspec->max_paths * sizeof(hrt_dominant_path));
    job.scratch_bytes = dm_job_scratch;
    job.run = dm_job_run;
    job.deliver = sp_job_deliver;
    job.finish = sp_job_finish;
    job.aux = &sj;
    return ac_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, rx_el, nr, tx_el, nt, f_a,
                      out, stats, t_begin, "hrt_sparse_array_channel", "hrt_compute_sparse_array_channel");
}

/* ------------------------------------------------------------------ array taps of path lists (hrt_sparse_array_taps) */

/* the taps spec of a sparse taps spec: the grid, and both parts (a list has no parts of its own) */
static hrt_taps_spec sparse_taps_grid(const hrt_sparse_taps_spec *sp)
{
    const hrt_taps_spec t = {sp->fs_hz, sp->fc_hz, sp->t0_s, sp->dt_s, sp->l_min, sp->num_taps, sp->num_times,
                             HRT_CHANNEL_LOS | HRT_CHANNEL_SCATTER};
    return t;
}

/* the checks of a sparse taps spec (`who`) */
static int sparse_taps_check(const hrt_sparse_taps_spec *sp, const char *who)
{
    if (!sp) return hrt_fail(HRT_E_INVALID, "%s: NULL spec", who);
    const uint64_t links = (uint64_t)sp->num_rx * sp->num_tx;
    if (links == 0 || links > HRT_SP_MAX_LINKS)
        return hrt_fail(HRT_E_INVALID, "%s: num_rx * num_tx = %llu (1 .. 65535)", who, (unsigned long long)links);
    if (sp->max_paths == 0 || sp->max_paths > HRT_DM_MAX_PATHS)
        return hrt_fail(HRT_E_INVALID, "%s: max_paths = %u (1 .. %u)", who, sp->max_paths, HRT_DM_MAX_PATHS);
    if (links * sp->max_paths > HRT_DM_MAX_LINK_PATHS)
        return hrt_fail(HRT_E_INVALID, "%s: num_rx * num_tx * max_paths = %llu > 2^22", who,
                        (unsigned long long)(links * sp->max_paths));
    const hrt_taps_spec grid = sparse_taps_grid(sp);
    return taps_spec_check(&grid, who);
}

uint64_t hrt_sparse_taps_out_bytes(const hrt_sparse_taps_spec *spec, uint32_t nr, uint32_t nt)
{
    if (sparse_taps_check(spec, "hrt_sparse_taps_out_bytes")) return 0;
    return (uint64_t)spec->num_rx * spec->num_tx * nr * nt * 2u * spec->num_times * spec->num_taps * 8u;
}

int hrt_sparse_array_taps(int device, const hrt_sparse_taps_spec *spec, const float *d_rx_el, uint32_t nr,
                          const float *d_tx_el, uint32_t nt, double fa_hz, const void *d_paths, float *d_out,
                          int accumulate, void *stream)
{
    const char *who = "hrt_sparse_array_taps";
    int rc = sparse_taps_check(spec, who);
    if (rc) return rc;
    if (!d_paths || !d_out) return hrt_fail(HRT_E_INVALID, "%s: NULL device pointer", who);
    const uint64_t grid = (uint64_t)spec->num_times * spec->num_taps;
    const hrt_array_spec a = {nr, nt, d_rx_el, d_tx_el, fa_hz};
    if ((rc = arrays_check(&a, grid, "num_times * num_taps", who))) return rc;
    if ((uintptr_t)d_paths % 8u) return hrt_fail(HRT_E_INVALID, "%s: d_paths is not 8-byte aligned", who);
    if (accumulate != 0 && accumulate != 1) return hrt_fail(HRT_E_INVALID, "%s: accumulate must be 0 or 1", who);
    hrt_ksparse_taps K;
    memset(&K, 0, sizeof K);
    K.links = spec->num_rx * spec->num_tx;
    K.max_paths = spec->max_paths;
    if ((rc = ac_fields(&a, K.links, grid, who, &K.nr, &K.nt, &K.npairs, &K.fa_c))) return rc;
    {   /* the grid of the array taps; a list has no records to chunk (nb = 0: nchunks stays 0) */
        const hrt_taps_spec t = sparse_taps_grid(spec);
        hrt_kview v;
        uint64_t per_chunk;
        memset(&v, 0, sizeof v);
        v.nrx = spec->num_rx; v.ntx = spec->num_tx;
        (void)taps_grid(&v, &t, K.npairs, 4u, &K.g, &per_chunk);
    }
    K.accumulate = (uint32_t)accumulate;
    K.rx_el = d_rx_el; K.tx_el = d_tx_el;
    K.paths = (const uint8_t *)d_paths;
    K.out = d_out;
    HRT_HIP(hrt_hip_set_device(device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_sparse_taps(&K, stream), "sparse taps kernel");
    return HRT_OK;
}

/* what the deliver and finish hooks of hrt_compute_sparse_array_taps need */
typedef struct {
    hrt_sparse_taps_spec sp;
    void *paths_out;     /* host, hrt_dominant_out_bytes; may be NULL */
} spt_job;

/* after the last batch, as sp_job_deliver: the taps are evaluated once, and only they (and the lists, if asked for)
 * come down */
static int spt_job_deliver(const ch_job *j, int device, const void *d_paths, void *out)
{
    const spt_job *sj = (const spt_job *)j->aux;
    const hrt_array_spec a = ac_job_arrays(j);
    const uint64_t bytes = hrt_sparse_taps_out_bytes(&sj->sp, j->nr, j->nt);
    void *d_h = NULL;
    int rc = hrt_device_malloc(device, &d_h, bytes);
    if (!rc)
        rc = hrt_sparse_array_taps(device, &sj->sp, a.rx_elements, j->nr, a.tx_elements, j->nt, j->fa, d_paths,
                                   (float *)d_h, 0, NULL);
    if (!rc) rc = hrt_device_sync(device, NULL);
    if (!rc) rc = hrt_device_download(device, out, d_h, bytes);
    if (!rc && sj->paths_out) rc = hrt_device_download(device, sj->paths_out, d_paths, j->out_bytes);
    if (d_h) hrt_device_free(device, d_h);
    return rc;
}

static int spt_job_finish(const ch_job *j, const hrt_problem *p, void *out)
{
    (void)out;
    const spt_job *sj = (const spt_job *)j->aux;
    return sj->paths_out ? dm_job_finish(j, p, sj->paths_out) : HRT_OK;
}

int hrt_compute_sparse_array_taps(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                  const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                                  const hrt_dominant_spec *dspec, const hrt_taps_spec *grid, const Vec3 *rx_el,
                                  size_t nr, const Vec3 *tx_el, size_t nt, double f_a, float *out, void *paths_out,
                                  hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = dominant_check(dspec);
    if (rc) return rc;
    if ((rc = dominant_links_check(nrx, ntx, dspec))) return rc;
    if (!grid) return hrt_fail(HRT_E_INVALID, "hrt_compute_sparse_array_taps: NULL grid");
    if ((rc = ac_counts_check(nr, nt, "hrt_sparse_array_taps"))) return rc;
    spt_job sj;
    memset(&sj, 0, sizeof sj);
    sj.sp.fs_hz = grid->fs_hz; sj.sp.fc_hz = grid->fc_hz; sj.sp.t0_s = grid->t0_s; sj.sp.dt_s = grid->dt_s;
    sj.sp.l_min = grid->l_min; sj.sp.num_taps = grid->num_taps; sj.sp.num_times = grid->num_times;
    sj.sp.num_rx = (uint32_t)nrx; sj.sp.num_tx = (uint32_t)ntx;
    sj.sp.max_paths = dspec->max_paths;
    sj.paths_out = paths_out;
    {   /* the grid and the arrays (the element pointers stand in for the device ones: tested for NULL only) */
        const hrt_taps_spec g = {grid->fs_hz, grid->fc_hz, grid->t0_s, grid->dt_s, grid->l_min, grid->num_taps,
                                 grid->num_times, dspec->parts};
        if ((rc = taps_spec_check(&g, "hrt_sparse_array_taps"))) return rc;
        const hrt_array_spec a = {(uint32_t)nr, (uint32_t)nt, (const float *)rx_el, (const float *)tx_el, f_a};
        if ((rc = arrays_check(&a, (uint64_t)g.num_times * g.num_taps, "num_times * num_taps",
                               "hrt_sparse_array_taps")))
            return rc;
    }
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = dspec;
    job.out_bytes = (uint64_t)nrx * ntx * (16u + (uint64_t)dspec->max_paths * sizeof(hrt_dominant_path));
    job.scratch_bytes = dm_job_scratch;
    job.run = dm_job_run;
    job.deliver = spt_job_deliver;
    job.finish = spt_job_finish;
    job.aux = &sj;
    return ac_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, rx_el, nr, tx_el, nt, f_a,
                      out, stats, t_begin, "hrt_sparse_array_taps", "hrt_compute_sparse_array_taps");
}

/* ------------------------------------------------------------------ beamformed channel responses (hrt_beam_channel) */

/* (the grid, the chunks and the bound of the partial sums are the array channel's: pair_grid) */

/* the checks of a beam call that need no problem (device pointers are not read).  There is no limit on Nr * Nt: the
 * element-domain matrix is never formed */
static int beam_check(const hrt_channel_spec *spec, const hrt_array_spec *a, const hrt_beam_spec *bm)
{
    const char *who = "hrt_beam_channel";
    int rc = spec_check(spec);
    if (rc) return rc;
    if (!a) return hrt_fail(HRT_E_INVALID, "%s: NULL arrays", who);
    if (!bm) return hrt_fail(HRT_E_INVALID, "%s: NULL beams", who);
    if (a->num_rx_elements < 1 || a->num_rx_elements > HRT_BM_MAX_ELEMENTS || a->num_tx_elements < 1 ||
        a->num_tx_elements > HRT_BM_MAX_ELEMENTS)
        return hrt_fail(HRT_E_INVALID, "%s: %u RX and %u TX elements (1 .. %u each)", who, a->num_rx_elements,
                        a->num_tx_elements, HRT_BM_MAX_ELEMENTS);
    if (bm->num_rx_beams < 1 || bm->num_rx_beams > HRT_BM_MAX_BEAMS || bm->num_tx_beams < 1 ||
        bm->num_tx_beams > HRT_BM_MAX_BEAMS)
        return hrt_fail(HRT_E_INVALID, "%s: %u RX and %u TX beams (1 .. %u each)", who, bm->num_rx_beams,
                        bm->num_tx_beams, HRT_BM_MAX_BEAMS);
    const uint64_t pts = (uint64_t)bm->num_rx_beams * bm->num_tx_beams * spec->num_times * spec->num_freqs;
    if (pts > HRT_BM_MAX_POINTS)
        return hrt_fail(HRT_E_INVALID, "%s: Br * Bt * num_times * num_freqs = %llu > 2^24", who,
                        (unsigned long long)pts);
    if (!isfinite(a->array_frequency_hz) || !(a->array_frequency_hz > 0.0))
        return hrt_fail(HRT_E_INVALID, "%s: the array frequency must be finite and > 0", who);
    if (!a->rx_elements || !a->tx_elements) return hrt_fail(HRT_E_INVALID, "%s: NULL element offsets", who);
    if (!bm->rx_weights || !bm->tx_weights) return hrt_fail(HRT_E_INVALID, "%s: NULL beam weights", who);
    return HRT_OK;
}

/* the counts of a drop-in beam call (`who`), before they are narrowed to the specs' */
static int beam_counts_check(size_t nr, size_t nt, size_t nbr, size_t nbt, const char *who)
{
    if (nr > HRT_BM_MAX_ELEMENTS || nt > HRT_BM_MAX_ELEMENTS)
        return hrt_fail(HRT_E_INVALID, "%s: %zu RX and %zu TX elements (1 .. %u each)", who, nr, nt,
                        HRT_BM_MAX_ELEMENTS);
    if (nbr > HRT_BM_MAX_BEAMS || nbt > HRT_BM_MAX_BEAMS)
        return hrt_fail(HRT_E_INVALID, "%s: %zu RX and %zu TX beams (1 .. %u each)", who, nbr, nbt,
                        HRT_BM_MAX_BEAMS);
    return HRT_OK;
}

/* the host weights of a drop-in beam call (`who`; [beams][elements][2]): finite */
static int beam_weights_check(const float *w, size_t beams, size_t elements, const char *side, const char *who)
{
    for (size_t i = 0; i < beams * elements * 2u; ++i)
        if (!isfinite(w[i]))
            return hrt_fail(HRT_E_INVALID, "%s: %s weight (%zu, %zu) is not finite", who, side,
                            i / (2u * elements), i / 2u % elements);
    return HRT_OK;
}

static uint64_t beam_los_bytes(const hrt_kbeam *K)
{
    return align256((uint64_t)K->v.nrx * K->v.ntx * K->npairs * 8u);
}

/* the tiling of one beam call: a pure function of the problem, the shard, the spec and the array and codebook
 * sizes.  The scratch is seg, the partial sums (*off_los bytes of them) and the LoS gains of every (link, pair) */
static int beam_plan(const hrt_problem *p, const hrt_shard *s, const hrt_channel_spec *spec, const hrt_array_spec *a,
                     const hrt_beam_spec *bm, hrt_kbeam *K, uint64_t *bytes, uint64_t *off_los)
{
    int rc = beam_check(spec, a, bm);
    if (rc) return rc;
    memset(K, 0, sizeof *K);
    if ((rc = ps_view(p, s, spec->parts, "hrt_beam_channel", &K->v))) return rc;
    const uint64_t links = (uint64_t)K->v.nrx * K->v.ntx;
    if (links * 2u * bm->num_rx_beams * bm->num_tx_beams * spec->num_times * spec->num_freqs >= (1ull << 39))
        return hrt_fail(HRT_E_INVALID, "hrt_beam_channel: more than 2^39 outputs");
    ps_shard(s, &K->sh);
    K->nr = a->num_rx_elements; K->nt = a->num_tx_elements;
    K->br = bm->num_rx_beams; K->bt = bm->num_tx_beams; K->npairs = K->br * K->bt;
    uint64_t sums = 0;
    const uint64_t per_chunk = pair_grid(&K->v, spec, K->npairs, a->array_frequency_hz, &K->g, &sums);
    *off_los = align256(K->v.nchunks * per_chunk);
    *bytes = sums - K->v.nchunks * per_chunk + *off_los + beam_los_bytes(K);
    return HRT_OK;
}

int hrt_beam_channel_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_channel_spec *spec,
                                   const hrt_array_spec *arrays, const hrt_beam_spec *beams, uint64_t *out)
{
    hrt_kbeam K;
    uint64_t bytes = 0, off_los = 0;
    const int rc = beam_plan(p, s, spec, arrays, beams, &K, &bytes, &off_los);
    return ps_scratch_out(rc, bytes, out, "hrt_beam_channel_scratch_bytes");
}

int hrt_beam_channel(const hrt_problem *p, const hrt_shard *s, const void *d_workspace, const hrt_channel_spec *spec,
                     const hrt_array_spec *arrays, const hrt_beam_spec *beams, void *d_scratch, uint64_t scratch_bytes,
                     float *d_out, int accumulate, void *stream)
{
    hrt_kbeam K;
    uint64_t need = 0, off_los = 0;
    int rc = beam_plan(p, s, spec, arrays, beams, &K, &need, &off_los);
    if (rc) return rc;
    if ((rc = ps_bind(&K.v, need, d_workspace, d_scratch, scratch_bytes, d_out, accumulate, "hrt_beam_channel",
                      "hrt_beam_channel_scratch_bytes", &K.partial)))
        return rc;
    K.los = (float *)((uint8_t *)K.partial + off_los);
    K.rx_el = arrays->rx_elements;
    K.tx_el = arrays->tx_elements;
    K.rx_w = beams->rx_weights;
    K.tx_w = beams->tx_weights;
    K.out = d_out;
    HRT_HIP(hrt_hip_set_device(p->device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_beam_channel(&K, stream), "beam channel kernels");
    return HRT_OK;
}

/* the beam spec of a drop-in call: the weights uploaded by ch_compute behind the offsets (rx then tx) */
static hrt_beam_spec beam_job_beams(const ch_job *j)
{
    hrt_beam_spec b;
    b.num_rx_beams = j->nbr;
    b.num_tx_beams = j->nbt;
    b.rx_weights = (const float *)j->d_const + 3u * (j->nr + j->nt);
    b.tx_weights = b.rx_weights + 2u * (size_t)j->nbr * j->nr;
    return b;
}

static int beam_job_scratch(const ch_job *j, const hrt_problem *p, const hrt_shard *s, uint64_t *out)
{
    const hrt_array_spec a = ac_job_arrays(j);
    const hrt_beam_spec b = beam_job_beams(j);
    return hrt_beam_channel_scratch_bytes(p, s, j->spec, &a, &b, out);
}

static int beam_job_run(const ch_job *j, const hrt_problem *p, const hrt_shard *s, const void *d_ws, void *d_scratch,
                        uint64_t scratch_bytes, void *d_out, int accumulate)
{
    const hrt_array_spec a = ac_job_arrays(j);
    const hrt_beam_spec b = beam_job_beams(j);
    return hrt_beam_channel(p, s, d_ws, j->spec, &a, &b, d_scratch, scratch_bytes, d_out, accumulate, NULL);
}

/* What hrt_compute_beam_channel and hrt_compute_beam_taps share once everything is checked: the offsets (rx then tx;
 * ac_job_arrays) and behind them the weights (rx then tx; beam_job_beams) for ch_compute to upload, the call.  `job`
 * has the spec, the output size and the device entry. */
static int beam_compute(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel, const Vec3 *tx_vel,
                        float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb, ch_job *job, const Vec3 *rx_el,
                        size_t nr, const Vec3 *tx_el, size_t nt, double f_a, const float *rx_weights,
                        size_t n_rx_beams, const float *tx_weights, size_t n_tx_beams, void *out, hrt_stats *stats,
                        double t_begin)
{
    const size_t n_el = (nr + nt) * 3u, n_wr = n_rx_beams * nr * 2u, n_wt = n_tx_beams * nt * 2u;
    float *e = (float *)malloc((n_el + n_wr + n_wt) * sizeof(float));
    if (!e) return hrt_fail(HRT_E_NOMEM, "out of host memory");
    ac_pack_offsets(rx_el, nr, tx_el, nt, e);
    memcpy(e + n_el, rx_weights, n_wr * sizeof(float));
    memcpy(e + n_el + n_wr, tx_weights, n_wt * sizeof(float));
    job->h_const = e;
    job->const_bytes = (n_el + n_wr + n_wt) * sizeof(float);
    job->nr = (uint32_t)nr; job->nt = (uint32_t)nt;
    job->nbr = (uint32_t)n_rx_beams; job->nbt = (uint32_t)n_tx_beams;
    job->fa = f_a;
    const int rc = ch_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, job, out, stats, t_begin);
    free(e);
    return rc;
}

int hrt_compute_beam_channel(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                             const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                             const hrt_channel_spec *spec, const Vec3 *rx_el, size_t nr, const Vec3 *tx_el, size_t nt,
                             double f_a, const float *rx_weights, size_t n_rx_beams, const float *tx_weights,
                             size_t n_tx_beams, float *out, hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = beam_counts_check(nr, nt, n_rx_beams, n_tx_beams, "hrt_beam_channel");
    if (rc) return rc;
    /* (the host pointers stand in for the device ones: beam_check tests them for NULL only) */
    const hrt_array_spec a = {(uint32_t)nr, (uint32_t)nt, (const float *)rx_el, (const float *)tx_el, f_a};
    const hrt_beam_spec bm = {(uint32_t)n_rx_beams, (uint32_t)n_tx_beams, rx_weights, tx_weights};
    if ((rc = beam_check(spec, &a, &bm))) return rc;
    if ((rc = ac_offsets_check(rx_el, nr, tx_el, nt, "hrt_beam_channel"))) return rc;
    if ((rc = beam_weights_check(rx_weights, n_rx_beams, nr, "RX", "hrt_beam_channel"))) return rc;
    if ((rc = beam_weights_check(tx_weights, n_tx_beams, nt, "TX", "hrt_beam_channel"))) return rc;
    if ((rc = ch_drop_in_check(scene, rx_pos, tx_pos, rx_vel, tx_vel, nrx, ntx, np, nb, out,
                               "hrt_compute_beam_channel")))
        return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = spec;
    job.out_bytes = (uint64_t)nrx * ntx * n_rx_beams * n_tx_beams * 2u * spec->num_times * spec->num_freqs * 8u;
    job.scratch_bytes = beam_job_scratch;
    job.run = beam_job_run;
    return beam_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, rx_el, nr, tx_el, nt, f_a,
                        rx_weights, n_rx_beams, tx_weights, n_tx_beams, out, stats, t_begin);
}

/* ------------------------------------------------------------------ beamformed impulse responses (hrt_beam_taps) */

/* the checks of a beam taps call that need no problem (device pointers are not read).  There is no limit on Nr * Nt:
 * the element-domain taps are never formed */
static int bt_check(const hrt_taps_spec *spec, const hrt_array_spec *a, const hrt_beam_spec *bm)
{
    const char *who = "hrt_beam_taps";
    int rc = taps_spec_check(spec, who);
    if (rc) return rc;
    if (!a) return hrt_fail(HRT_E_INVALID, "%s: NULL arrays", who);
    if (!bm) return hrt_fail(HRT_E_INVALID, "%s: NULL beams", who);
    if (a->num_rx_elements < 1 || a->num_rx_elements > HRT_BM_MAX_ELEMENTS || a->num_tx_elements < 1 ||
        a->num_tx_elements > HRT_BM_MAX_ELEMENTS)
        return hrt_fail(HRT_E_INVALID, "%s: %u RX and %u TX elements (1 .. %u each)", who, a->num_rx_elements,
                        a->num_tx_elements, HRT_BM_MAX_ELEMENTS);
    if (bm->num_rx_beams < 1 || bm->num_rx_beams > HRT_BM_MAX_BEAMS || bm->num_tx_beams < 1 ||
        bm->num_tx_beams > HRT_BM_MAX_BEAMS)
        return hrt_fail(HRT_E_INVALID, "%s: %u RX and %u TX beams (1 .. %u each)", who, bm->num_rx_beams,
                        bm->num_tx_beams, HRT_BM_MAX_BEAMS);
    const uint64_t pts = (uint64_t)bm->num_rx_beams * bm->num_tx_beams * spec->num_times * spec->num_taps;
    if (pts > HRT_BM_MAX_POINTS)
        return hrt_fail(HRT_E_INVALID, "%s: Br * Bt * num_times * num_taps = %llu > 2^24", who,
                        (unsigned long long)pts);
    if (!isfinite(a->array_frequency_hz) || !(a->array_frequency_hz > 0.0))
        return hrt_fail(HRT_E_INVALID, "%s: the array frequency must be finite and > 0", who);
    if (!a->rx_elements || !a->tx_elements) return hrt_fail(HRT_E_INVALID, "%s: NULL element offsets", who);
    if (!bm->rx_weights || !bm->tx_weights) return hrt_fail(HRT_E_INVALID, "%s: NULL beam weights", who);
    return HRT_OK;
}

/* the plan of one beam taps call: a pure function of the problem, the shard, the spec and the array and codebook
 * sizes (taps_grid with Br Bt pairs: a block of 64 rows covers up to 64 beam pairs).  The scratch is seg, the partial
 * sums (*off_los bytes of them) and the LoS gains of every (link, pair) */
static int bt_plan(const hrt_problem *p, const hrt_shard *s, const hrt_taps_spec *spec, const hrt_array_spec *a,
                   const hrt_beam_spec *bm, hrt_kbeam_taps *K, uint64_t *bytes, uint64_t *off_los)
{
    int rc = bt_check(spec, a, bm);
    if (rc) return rc;
    memset(K, 0, sizeof *K);
    if ((rc = ps_view(p, s, spec->parts, "hrt_beam_taps", &K->v))) return rc;
    const uint64_t links = (uint64_t)K->v.nrx * K->v.ntx;
    if (links * 2u * bm->num_rx_beams * bm->num_tx_beams * spec->num_times * spec->num_taps >= (1ull << 39))
        return hrt_fail(HRT_E_INVALID, "hrt_beam_taps: more than 2^39 outputs");
    ps_shard(s, &K->sh);
    K->nr = a->num_rx_elements; K->nt = a->num_tx_elements;
    K->br = bm->num_rx_beams; K->bt = bm->num_tx_beams; K->npairs = K->br * K->bt;
    K->fa_c = a->array_frequency_hz / HRT_SPEED_OF_LIGHT;
    uint64_t per_chunk;
    const uint64_t sums = taps_grid(&K->v, spec, K->npairs, 4u, &K->g, &per_chunk);
    *off_los = align256(K->v.nchunks * per_chunk);
    *bytes = sums - K->v.nchunks * per_chunk + *off_los + align256(links * K->npairs * 8u);
    return HRT_OK;
}

int hrt_beam_taps_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_taps_spec *spec,
                                const hrt_array_spec *arrays, const hrt_beam_spec *beams, uint64_t *out)
{
    hrt_kbeam_taps K;
    uint64_t bytes = 0, off_los = 0;
    const int rc = bt_plan(p, s, spec, arrays, beams, &K, &bytes, &off_los);
    return ps_scratch_out(rc, bytes, out, "hrt_beam_taps_scratch_bytes");
}

int hrt_beam_taps(const hrt_problem *p, const hrt_shard *s, const void *d_workspace, const hrt_taps_spec *spec,
                  const hrt_array_spec *arrays, const hrt_beam_spec *beams, void *d_scratch, uint64_t scratch_bytes,
                  float *d_out, int accumulate, void *stream)
{
    hrt_kbeam_taps K;
    uint64_t need = 0, off_los = 0;
    int rc = bt_plan(p, s, spec, arrays, beams, &K, &need, &off_los);
    if (rc) return rc;
    if ((rc = ps_bind(&K.v, need, d_workspace, d_scratch, scratch_bytes, d_out, accumulate, "hrt_beam_taps",
                      "hrt_beam_taps_scratch_bytes", &K.partial)))
        return rc;
    K.los = (float *)((uint8_t *)K.partial + off_los);
    K.rx_el = arrays->rx_elements;
    K.tx_el = arrays->tx_elements;
    K.rx_w = beams->rx_weights;
    K.tx_w = beams->tx_weights;
    K.out = d_out;
    HRT_HIP(hrt_hip_set_device(p->device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_beam_taps(&K, stream), "beam taps kernels");
    return HRT_OK;
}

static int bt_job_scratch(const ch_job *j, const hrt_problem *p, const hrt_shard *s, uint64_t *out)
{
    const hrt_array_spec a = ac_job_arrays(j);
    const hrt_beam_spec b = beam_job_beams(j);
    return hrt_beam_taps_scratch_bytes(p, s, j->spec, &a, &b, out);
}

static int bt_job_run(const ch_job *j, const hrt_problem *p, const hrt_shard *s, const void *d_ws, void *d_scratch,
                      uint64_t scratch_bytes, void *d_out, int accumulate)
{
    const hrt_array_spec a = ac_job_arrays(j);
    const hrt_beam_spec b = beam_job_beams(j);
    return hrt_beam_taps(p, s, d_ws, j->spec, &a, &b, d_scratch, scratch_bytes, d_out, accumulate, NULL);
}

int hrt_compute_beam_taps(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                          const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                          const hrt_taps_spec *spec, const Vec3 *rx_el, size_t nr, const Vec3 *tx_el, size_t nt,
                          double f_a, const float *rx_weights, size_t n_rx_beams, const float *tx_weights,
                          size_t n_tx_beams, float *out, hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    int rc = beam_counts_check(nr, nt, n_rx_beams, n_tx_beams, "hrt_beam_taps");
    if (rc) return rc;
    /* (the host pointers stand in for the device ones: bt_check tests them for NULL only) */
    const hrt_array_spec a = {(uint32_t)nr, (uint32_t)nt, (const float *)rx_el, (const float *)tx_el, f_a};
    const hrt_beam_spec bm = {(uint32_t)n_rx_beams, (uint32_t)n_tx_beams, rx_weights, tx_weights};
    if ((rc = bt_check(spec, &a, &bm))) return rc;
    if ((rc = ac_offsets_check(rx_el, nr, tx_el, nt, "hrt_beam_taps"))) return rc;
    if ((rc = beam_weights_check(rx_weights, n_rx_beams, nr, "RX", "hrt_beam_taps"))) return rc;
    if ((rc = beam_weights_check(tx_weights, n_tx_beams, nt, "TX", "hrt_beam_taps"))) return rc;
    if ((rc = ch_drop_in_check(scene, rx_pos, tx_pos, rx_vel, tx_vel, nrx, ntx, np, nb, out, "hrt_compute_beam_taps")))
        return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = spec;
    job.out_bytes = (uint64_t)nrx * ntx * n_rx_beams * n_tx_beams * 2u * spec->num_times * spec->num_taps * 8u;
    job.scratch_bytes = bt_job_scratch;
    job.run = bt_job_run;
    return beam_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, rx_el, nr, tx_el, nt, f_a,
                        rx_weights, n_rx_beams, tx_weights, n_tx_beams, out, stats, t_begin);
}

/* ------------------------------------------------------------------ beam channels of path lists (hrt_sparse_beam_channel) */

/* the checks of a sparse beam call (`who`) behind sparse_check that need no device: the counts, the points, f_a.  There
 * is no limit on Nr * Nt: the element-domain matrix is never formed */
static int sparse_beam_check(const hrt_sparse_spec *sp, uint32_t nr, uint32_t nt, uint32_t br, uint32_t bt, double fa_hz,
                             const char *who)
{
    if (nr < 1 || nr > HRT_BM_MAX_ELEMENTS || nt < 1 || nt > HRT_BM_MAX_ELEMENTS)
        return hrt_fail(HRT_E_INVALID, "%s: %u RX and %u TX elements (1 .. %u each)", who, nr, nt, HRT_BM_MAX_ELEMENTS);
    if (br < 1 || br > HRT_BM_MAX_BEAMS || bt < 1 || bt > HRT_BM_MAX_BEAMS)
        return hrt_fail(HRT_E_INVALID, "%s: %u RX and %u TX beams (1 .. %u each)", who, br, bt, HRT_BM_MAX_BEAMS);
    const uint64_t pts = (uint64_t)br * bt * sp->num_times * sp->num_freqs;
    if (pts > HRT_BM_MAX_POINTS)
        return hrt_fail(HRT_E_INVALID, "%s: Br * Bt * num_times * num_freqs = %llu > 2^24", who,
                        (unsigned long long)pts);
    if (!isfinite(fa_hz) || !(fa_hz > 0.0))
        return hrt_fail(HRT_E_INVALID, "%s: the array frequency must be finite and > 0", who);
    return HRT_OK;
}

uint64_t hrt_sparse_beam_out_bytes(const hrt_sparse_spec *spec, uint32_t br, uint32_t bt)
{
    if (sparse_check(spec, "hrt_sparse_beam_out_bytes")) return 0;
    return (uint64_t)spec->num_rx * spec->num_tx * br * bt * 2u * spec->num_times * spec->num_freqs * 8u;
}

int hrt_sparse_beam_channel(int device, const hrt_sparse_spec *spec, const float *d_rx_el, uint32_t nr,
                            const float *d_tx_el, uint32_t nt, double fa_hz, const float *d_rx_w, uint32_t br,
                            const float *d_tx_w, uint32_t bt, const void *d_paths, float *d_out, int accumulate,
                            void *stream)
{
    const char *who = "hrt_sparse_beam_channel";
    int rc = sparse_check(spec, who);
    if (rc) return rc;
    if (!d_rx_el || !d_tx_el || !d_rx_w || !d_tx_w || !d_paths || !d_out)
        return hrt_fail(HRT_E_INVALID, "%s: NULL device pointer", who);
    if ((rc = sparse_beam_check(spec, nr, nt, br, bt, fa_hz, who))) return rc;
    if ((uintptr_t)d_paths % 8u) return hrt_fail(HRT_E_INVALID, "%s: d_paths is not 8-byte aligned", who);
    if (accumulate != 0 && accumulate != 1) return hrt_fail(HRT_E_INVALID, "%s: accumulate must be 0 or 1", who);
    hrt_ksparse_beam K;
    memset(&K, 0, sizeof K);
    K.links = spec->num_rx * spec->num_tx;
    K.max_paths = spec->max_paths;
    K.nr = nr; K.nt = nt; K.br = br; K.bt = bt; K.npairs = br * bt;
    if ((uint64_t)K.links * 2u * K.npairs * spec->num_times * spec->num_freqs >= (1ull << 39))
        return hrt_fail(HRT_E_INVALID, "%s: more than 2^39 outputs", who);
    K.g.K = spec->num_freqs; K.g.T = spec->num_times;
    K.g.K1 = (spec->num_freqs + HRT_CH_K2 - 1) / HRT_CH_K2;
    K.g.rows = K.g.K1 * K.g.T;
    K.g.pblocks = (K.npairs + HRT_AC_PAIRS - 1) / HRT_AC_PAIRS;
    K.g.cblocks = (K.g.rows + HRT_AC_GROWS - 1) / HRT_AC_GROWS;
    K.g.f0 = spec->f0_hz; K.g.df = spec->df_hz; K.g.t0 = spec->t0_s; K.g.dt = spec->dt_s;
    K.g.fa_c = fa_hz / HRT_SPEED_OF_LIGHT;
    K.accumulate = (uint32_t)accumulate;
    K.rx_el = d_rx_el; K.tx_el = d_tx_el;
    K.rx_w = d_rx_w; K.tx_w = d_tx_w;
    K.paths = (const uint8_t *)d_paths;
    K.out = d_out;
    HRT_HIP(hrt_hip_set_device(device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_sparse_beam(&K, stream), "sparse beam kernel");
    return HRT_OK;
}

/* after the last batch: the merged lists stay at d_paths; the beam channel is evaluated once, and only it (and the
 * lists, if asked for) comes down.  The offsets and the weights are ch_compute's upload (ac_job_arrays,
 * beam_job_beams); the aux is hrt_compute_sparse_array_channel's sp_job. */
static int sb_job_deliver(const ch_job *j, int device, const void *d_paths, void *out)
{
    const sp_job *sj = (const sp_job *)j->aux;
    const hrt_array_spec a = ac_job_arrays(j);
    const hrt_beam_spec b = beam_job_beams(j);
    const uint64_t bytes = hrt_sparse_beam_out_bytes(&sj->sp, j->nbr, j->nbt);
    void *d_B = NULL;
    int rc = hrt_device_malloc(device, &d_B, bytes);
    if (!rc)
        rc = hrt_sparse_beam_channel(device, &sj->sp, a.rx_elements, j->nr, a.tx_elements, j->nt, j->fa, b.rx_weights,
                                     j->nbr, b.tx_weights, j->nbt, d_paths, (float *)d_B, 0, NULL);
    if (!rc) rc = hrt_device_sync(device, NULL);
    if (!rc) rc = hrt_device_download(device, out, d_B, bytes);
    if (!rc && sj->paths_out) rc = hrt_device_download(device, sj->paths_out, d_paths, j->out_bytes);
    if (d_B) hrt_device_free(device, d_B);
    return rc;
}

int hrt_compute_sparse_beam_channel(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                    const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                                    const hrt_dominant_spec *dspec, const hrt_channel_spec *grid, const Vec3 *rx_el,
                                    size_t nr, const Vec3 *tx_el, size_t nt, double f_a, const float *rx_weights,
                                    size_t n_rx_beams, const float *tx_weights, size_t n_tx_beams, float *out,
                                    void *paths_out, hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    const char *dev = "hrt_sparse_beam_channel";
    int rc = dominant_check(dspec);
    if (rc) return rc;
    if ((rc = dominant_links_check(nrx, ntx, dspec))) return rc;
    if (!grid) return hrt_fail(HRT_E_INVALID, "hrt_compute_sparse_beam_channel: NULL grid");
    if ((rc = beam_counts_check(nr, nt, n_rx_beams, n_tx_beams, dev))) return rc;
    sp_job sj;
    memset(&sj, 0, sizeof sj);
    sj.sp.f0_hz = grid->f0_hz; sj.sp.df_hz = grid->df_hz; sj.sp.num_freqs = grid->num_freqs;
    sj.sp.t0_s = grid->t0_s; sj.sp.dt_s = grid->dt_s; sj.sp.num_times = grid->num_times;
    sj.sp.num_rx = (uint32_t)nrx; sj.sp.num_tx = (uint32_t)ntx;
    sj.sp.max_paths = dspec->max_paths;
    sj.paths_out = paths_out;
    {   /* the grid (the parts are the dominant spec's), the counts, the points and f_a */
        const hrt_channel_spec g = {grid->f0_hz, grid->df_hz, grid->num_freqs, grid->t0_s, grid->dt_s,
                                    grid->num_times, dspec->parts};
        if ((rc = spec_check(&g))) return rc;
        if ((rc = sparse_beam_check(&sj.sp, (uint32_t)nr, (uint32_t)nt, (uint32_t)n_rx_beams, (uint32_t)n_tx_beams, f_a,
                                    dev)))
            return rc;
    }
    if (!rx_el || !tx_el) return hrt_fail(HRT_E_INVALID, "%s: NULL element offsets", dev);
    if (!rx_weights || !tx_weights) return hrt_fail(HRT_E_INVALID, "%s: NULL beam weights", dev);
    if ((rc = ac_offsets_check(rx_el, nr, tx_el, nt, dev))) return rc;
    if ((rc = beam_weights_check(rx_weights, n_rx_beams, nr, "RX", dev))) return rc;
    if ((rc = beam_weights_check(tx_weights, n_tx_beams, nt, "TX", dev))) return rc;
    if ((rc = ch_drop_in_check(scene, rx_pos, tx_pos, rx_vel, tx_vel, nrx, ntx, np, nb, out,
                               "hrt_compute_sparse_beam_channel")))
        return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = dspec;
    job.out_bytes = (uint64_t)nrx * ntx * (16u + (uint64_t)dspec->max_paths * sizeof(hrt_dominant_path));
    job.scratch_bytes = dm_job_scratch;
    job.run = dm_job_run;
    job.deliver = sb_job_deliver;
    job.finish = sp_job_finish;
    job.aux = &sj;
    return beam_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, rx_el, nr, tx_el, nt, f_a,
                        rx_weights, n_rx_beams, tx_weights, n_tx_beams, out, stats, t_begin);
}

/* ------------------------------------------------------------------ beam taps of path lists (hrt_sparse_beam_taps) */

/* the checks of a sparse beam taps call (`who`) behind sparse_taps_check that need no device: the counts, the points,
 * f_a.  There is no limit on Nr * Nt: the element-domain taps are never formed */
static int sparse_beam_taps_check(const hrt_sparse_taps_spec *sp, uint32_t nr, uint32_t nt, uint32_t br, uint32_t bt,
                                  double fa_hz, const char *who)
{
    if (nr < 1 || nr > HRT_BM_MAX_ELEMENTS || nt < 1 || nt > HRT_BM_MAX_ELEMENTS)
        return hrt_fail(HRT_E_INVALID, "%s: %u RX and %u TX elements (1 .. %u each)", who, nr, nt, HRT_BM_MAX_ELEMENTS);
    if (br < 1 || br > HRT_BM_MAX_BEAMS || bt < 1 || bt > HRT_BM_MAX_BEAMS)
        return hrt_fail(HRT_E_INVALID, "%s: %u RX and %u TX beams (1 .. %u each)", who, br, bt, HRT_BM_MAX_BEAMS);
    const uint64_t pts = (uint64_t)br * bt * sp->num_times * sp->num_taps;
    if (pts > HRT_BM_MAX_POINTS)
        return hrt_fail(HRT_E_INVALID, "%s: Br * Bt * num_times * num_taps = %llu > 2^24", who, (unsigned long long)pts);
    if (!isfinite(fa_hz) || !(fa_hz > 0.0))
        return hrt_fail(HRT_E_INVALID, "%s: the array frequency must be finite and > 0", who);
    return HRT_OK;
}

uint64_t hrt_sparse_beam_taps_out_bytes(const hrt_sparse_taps_spec *spec, uint32_t br, uint32_t bt)
{
    if (sparse_taps_check(spec, "hrt_sparse_beam_taps_out_bytes")) return 0;
    return (uint64_t)spec->num_rx * spec->num_tx * br * bt * 2u * spec->num_times * spec->num_taps * 8u;
}

int hrt_sparse_beam_taps(int device, const hrt_sparse_taps_spec *spec, const float *d_rx_el, uint32_t nr,
                         const float *d_tx_el, uint32_t nt, double fa_hz, const float *d_rx_w, uint32_t br,
                         const float *d_tx_w, uint32_t bt, const void *d_paths, float *d_out, int accumulate,
                         void *stream)
{
    const char *who = "hrt_sparse_beam_taps";
    int rc = sparse_taps_check(spec, who);
    if (rc) return rc;
    if (!d_rx_el || !d_tx_el || !d_rx_w || !d_tx_w || !d_paths || !d_out)
        return hrt_fail(HRT_E_INVALID, "%s: NULL device pointer", who);
    if ((rc = sparse_beam_taps_check(spec, nr, nt, br, bt, fa_hz, who))) return rc;
    if ((uintptr_t)d_paths % 8u) return hrt_fail(HRT_E_INVALID, "%s: d_paths is not 8-byte aligned", who);
    if (accumulate != 0 && accumulate != 1) return hrt_fail(HRT_E_INVALID, "%s: accumulate must be 0 or 1", who);
    hrt_ksparse_beam_taps K;
    memset(&K, 0, sizeof K);
    K.links = spec->num_rx * spec->num_tx;
    K.max_paths = spec->max_paths;
    K.nr = nr; K.nt = nt; K.br = br; K.bt = bt; K.npairs = br * bt;
    if ((uint64_t)K.links * 2u * K.npairs * spec->num_times * spec->num_taps >= (1ull << 39))
        return hrt_fail(HRT_E_INVALID, "%s: more than 2^39 outputs", who);
    K.fa_c = fa_hz / HRT_SPEED_OF_LIGHT;
    {   /* the grid of the beam taps (Br Bt pairs); a list has no records to chunk (nb = 0: nchunks stays 0) */
        const hrt_taps_spec t = sparse_taps_grid(spec);
        hrt_kview v;
        uint64_t per_chunk;
        memset(&v, 0, sizeof v);
        v.nrx = spec->num_rx; v.ntx = spec->num_tx;
        (void)taps_grid(&v, &t, K.npairs, 4u, &K.g, &per_chunk);
    }
    K.accumulate = (uint32_t)accumulate;
    K.rx_el = d_rx_el; K.tx_el = d_tx_el;
    K.rx_w = d_rx_w; K.tx_w = d_tx_w;
    K.paths = (const uint8_t *)d_paths;
    K.out = d_out;
    HRT_HIP(hrt_hip_set_device(device), "hipSetDevice");
    HRT_HIP(hrt_hip_launch_sparse_beam_taps(&K, stream), "sparse beam taps kernel");
    return HRT_OK;
}

/* after the last batch: the merged lists stay at d_paths; the beam taps are evaluated once, and only they (and the
 * lists, if asked for) come down.  The offsets and the weights are beam_compute's upload (ac_job_arrays,
 * beam_job_beams); the aux is hrt_compute_sparse_array_taps' spt_job. */
static int sbt_job_deliver(const ch_job *j, int device, const void *d_paths, void *out)
{
    const spt_job *sj = (const spt_job *)j->aux;
    const hrt_array_spec a = ac_job_arrays(j);
    const hrt_beam_spec b = beam_job_beams(j);
    const uint64_t bytes = hrt_sparse_beam_taps_out_bytes(&sj->sp, j->nbr, j->nbt);
    void *d_h = NULL;
    int rc = hrt_device_malloc(device, &d_h, bytes);
    if (!rc)
        rc = hrt_sparse_beam_taps(device, &sj->sp, a.rx_elements, j->nr, a.tx_elements, j->nt, j->fa, b.rx_weights,
                                  j->nbr, b.tx_weights, j->nbt, d_paths, (float *)d_h, 0, NULL);
    if (!rc) rc = hrt_device_sync(device, NULL);
    if (!rc) rc = hrt_device_download(device, out, d_h, bytes);
    if (!rc && sj->paths_out) rc = hrt_device_download(device, sj->paths_out, d_paths, j->out_bytes);
    if (d_h) hrt_device_free(device, d_h);
    return rc;
}

int hrt_compute_sparse_beam_taps(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                 const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                                 const hrt_dominant_spec *dspec, const hrt_taps_spec *grid, const Vec3 *rx_el,
                                 size_t nr, const Vec3 *tx_el, size_t nt, double f_a, const float *rx_weights,
                                 size_t n_rx_beams, const float *tx_weights, size_t n_tx_beams, float *out,
                                 void *paths_out, hrt_stats *stats)
{
    const double t_begin = hrt_now_s();
    const char *dev = "hrt_sparse_beam_taps";
    int rc = dominant_check(dspec);
    if (rc) return rc;
    if ((rc = dominant_links_check(nrx, ntx, dspec))) return rc;
    if (!grid) return hrt_fail(HRT_E_INVALID, "hrt_compute_sparse_beam_taps: NULL grid");
    if ((rc = beam_counts_check(nr, nt, n_rx_beams, n_tx_beams, dev))) return rc;
    spt_job sj;
    memset(&sj, 0, sizeof sj);
    sj.sp.fs_hz = grid->fs_hz; sj.sp.fc_hz = grid->fc_hz; sj.sp.t0_s = grid->t0_s; sj.sp.dt_s = grid->dt_s;
    sj.sp.l_min = grid->l_min; sj.sp.num_taps = grid->num_taps; sj.sp.num_times = grid->num_times;
    sj.sp.num_rx = (uint32_t)nrx; sj.sp.num_tx = (uint32_t)ntx;
    sj.sp.max_paths = dspec->max_paths;
    sj.paths_out = paths_out;
    {   /* the grid (the parts are the dominant spec's), the counts, the points and f_a */
        const hrt_taps_spec g = {grid->fs_hz, grid->fc_hz, grid->t0_s, grid->dt_s, grid->l_min, grid->num_taps,
                                 grid->num_times, dspec->parts};
        if ((rc = taps_spec_check(&g, dev))) return rc;
        if ((rc = sparse_beam_taps_check(&sj.sp, (uint32_t)nr, (uint32_t)nt, (uint32_t)n_rx_beams,
                                         (uint32_t)n_tx_beams, f_a, dev)))
            return rc;
    }
    if (!rx_el || !tx_el) return hrt_fail(HRT_E_INVALID, "%s: NULL element offsets", dev);
    if (!rx_weights || !tx_weights) return hrt_fail(HRT_E_INVALID, "%s: NULL beam weights", dev);
    if ((rc = ac_offsets_check(rx_el, nr, tx_el, nt, dev))) return rc;
    if ((rc = beam_weights_check(rx_weights, n_rx_beams, nr, "RX", dev))) return rc;
    if ((rc = beam_weights_check(tx_weights, n_tx_beams, nt, "TX", dev))) return rc;
    if ((rc = ch_drop_in_check(scene, rx_pos, tx_pos, rx_vel, tx_vel, nrx, ntx, np, nb, out,
                               "hrt_compute_sparse_beam_taps")))
        return rc;
    ch_job job;
    memset(&job, 0, sizeof job);
    job.spec = dspec;
    job.out_bytes = (uint64_t)nrx * ntx * (16u + (uint64_t)dspec->max_paths * sizeof(hrt_dominant_path));
    job.scratch_bytes = dm_job_scratch;
    job.run = dm_job_run;
    job.deliver = sbt_job_deliver;
    job.finish = spt_job_finish;
    job.aux = &sj;
    return beam_compute(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, &job, rx_el, nr, tx_el, nt, f_a,
                        rx_weights, n_rx_beams, tx_weights, n_tx_beams, out, stats, t_begin);
}
