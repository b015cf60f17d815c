/* hrt_pathsum.h -- what the path-sum families (hrt_channel, hrt_array_channel, hrt_taps, hrt_array_taps,
 * hrt_power_profiles, hrt_dominant_paths, hrt_beam_channel, hrt_beam_taps, hrt_array_covariance) share: the view of the
 * workspace of a finished hrt_trace that their kernels read (plain C, the first member of hrt_kchannel, hrt_karray,
 * hrt_ktaps, hrt_karray_taps, hrt_kpower, hrt_kdominant, hrt_kbeam, hrt_kbeam_taps and hrt_kcov; filled by
 * csrc/host/channel.c; also of hrt_kpatterns, csrc/hrt_patterns.h, whose kernels WRITE the amplitudes this view reads,
 * before any family runs), the grid of the two pair families (hrt_kgrid) and of the three taps families (hrt_ktgrid), and,
 * for the .hip files, the device helpers that read them: the field accessors, the chunk ranges and the batch fill, the
 * staged record with its departure direction (hrt_kshard), the element offsets and the steering products of the array
 * families, the LoS entry, the two halves the complex reduce kernels share, and the reduce walk and the launch of the
 * pair families and of the taps families.
 *
 * Every family sums, per link (rx, tx), the LoS entry (shard rank 0 only) and the scatter records of the link's TX
 * segment in every hit block.  The records of a segment are cut into nchunks chunks; a partial kernel writes one
 * chunk's sums to the scratch and a reduce kernel adds the chunks in a fixed order (no atomics: bit-reproducible).
 * The scratch starts with seg, the TX segments found by hrt_channel_segments_kernel (csrc/hrt_channel.hip). */
#ifndef HRT_PATHSUM_H
#define HRT_PATHSUM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    const uint8_t *ws;              /* workspace of a finished hrt_trace */
    uint64_t cap, off_counts, off_los, off_hits, hit_block_bytes, off_recs, rec_block_bytes, off_masks;
    uint32_t nb, nrx, ntx, num_local;
    uint32_t nchunks;               /* record chunks per (link, block); 0: no scatter part */
    uint32_t los, accumulate;       /* add the LoS term (shard rank 0 only) / add into out */
    uint32_t *seg;                  /* scratch: [nb][ntx + 1] first hit of every TX segment */
} hrt_kview;

/* The shard of the trace, for the families that need a record's departure direction: the member right after v in
 * hrt_karray, hrt_karray_taps, hrt_kpower, hrt_kdominant, hrt_kbeam, hrt_kbeam_taps and hrt_kcov.  20 bytes, 4-aligned (not padded to 24): the fields that follow it
 * in those structs keep the kernel-argument offsets they had when these four were written out there (new offsets
 * alone moved hrt_array_partial_kernel's SGPR spills and its time: profiles/HISTORY.md). */
typedef struct {
    uint64_t num_paths;             /* the shard's N: departure directions from the global path */
    uint32_t rank, count, chunk;
} __attribute__((packed, aligned(4))) hrt_kshard;

/* The grid of the pair families (hrt_array_channel: element pairs, hrt_beam_channel: beam pairs), a member of hrt_karray
 * and hrt_kbeam at the offsets these fields had when they were written out there (8-aligned in both; asserted in the
 * two headers).  csrc/hrt_pair_gemm.inc and pair_output read it as P.g. */
typedef struct {
    uint32_t K, T, K1, rows;        /* rows = T * K1 */
    uint32_t pblocks, cblocks;      /* ceil(npairs / HRT_AC_PAIRS), ceil(rows / HRT_AC_GROWS) */
    double f0, df, t0, dt;
    double fa_c;                    /* f_a / c: revolutions per metre of path difference */
} hrt_kgrid;

/* The grid of the taps families (hrt_taps: rows = T; hrt_array_taps, hrt_beam_taps: rows = pairs * T), filled by
 * taps_grid() of csrc/host/channel.c.  A member of hrt_karray_taps and hrt_kbeam_taps at the offsets these fields had
 * when they were written out there (8-aligned in both; asserted in the two headers).  hrt_ktaps keeps these fields
 * (without rows, which is its T) written out where they always were: taps_plan() copies them from one of these, and
 * the device code below takes either as its grid G (profiles/HISTORY.md: the struct's layout in hrt_ktaps alone
 * regrouped the kernel-argument loads of hrt_taps_partial_kernel).  csrc/hrt_taps_gemm.inc, taps_output and
 * launch_taps_family read it as G.  A row tile is 16 rows g = 4 row + q (4 rows), a column tile 16 taps; a workgroup
 * holds 16 x 4 tiles (rt = 4: 4 x 4 a wave, the 4 waves along the rows; hrt_taps: 4 x 4 tiles, 4 x 1 a wave, the waves
 * along the columns) or 1 x 16 tiles (rt = 1: 1 x 4 a wave, the waves along the columns). */
typedef struct {
    uint32_t L, T;                  /* taps, time samples */
    int32_t l_min;
    uint32_t rows;                  /* (pair, time) rows */
    uint32_t rtiles, ctiles;        /* ceil(4 rows / 16), ceil(L / 16) */
    uint32_t rt;                    /* the form: row tiles per wave, 4 (rtiles >= 4) or 1 */
    uint32_t rblocks, cblocks;      /* workgroups along the rows and the columns */
    double fs, fc, t0, dt;
} hrt_ktgrid;

/* hrt_channel_segments_kernel: V->seg[b][t] for every bounce b and t <= ntx */
int hrt_hip_launch_segments(const hrt_kview *V, void *stream);

#ifdef __cplusplus
}
#endif

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "hrt_device.h"
#include "hrt_launch_dir.h"
#include "hrt_sinc.h"

static_assert(sizeof(hrt_kshard) == 20 && sizeof(hrt_kview) % 8 == 0, "hrt_kshard: the offsets after it");

// floats of a staged record (stage_record): te re, te im, tm re, tm im, tau, nu, u_rx (3), u_tx (3)
#define HRT_PS_REC_FLOATS 12u

namespace {

// the fraction of a phase in revolutions, as the argument of sincospi (half revolutions, in [-1, 1])
__device__ __forceinline__ float half_revs(double ph)
{
    return (float)(2.0 * (ph - rint(ph)));
}

__device__ __forceinline__ const float *rec_field(const hrt_kview &V, uint32_t b, uint32_t rx, uint32_t f)
{
    return reinterpret_cast<const float *>(V.ws + V.off_recs + (uint64_t)b * V.rec_block_bytes +
                                           ((uint64_t)rx * HRT_REC_FIELDS + f) * V.cap * 4u);
}

__device__ __forceinline__ const uint32_t *hit_field(const hrt_kview &V, uint32_t b, uint32_t f)
{
    return reinterpret_cast<const uint32_t *>(V.ws + V.off_hits + (uint64_t)b * V.hit_block_bytes +
                                              (uint64_t)f * V.cap * 4u);
}

// the unblocked bits of the records of hit block b at receiver rx: hit i is bit i & 63 of word i >> 6
__device__ __forceinline__ const uint64_t *mask_row(const hrt_kview &V, uint32_t b, uint32_t rx)
{
    return reinterpret_cast<const uint64_t *>(V.ws + V.off_masks) + ((uint64_t)b * V.nrx + rx) * (V.cap / 64u);
}

// the records [start, end) of chunk c of the TX segment of hit block b
__device__ __forceinline__ void chunk_range(const hrt_kview &V, uint32_t b, uint32_t tx, uint32_t c, uint32_t &start,
                                            uint32_t &end)
{
    const uint32_t s0 = V.seg[b * (V.ntx + 1u) + tx], s1 = V.seg[b * (V.ntx + 1u) + tx + 1u];
    const uint64_t n = s1 - s0;
    start = s0 + (uint32_t)(n * c / V.nchunks);
    end = s0 + (uint32_t)(n * (c + 1u) / V.nchunks);
}

// u_tx of hit i of block b, a ray of TX tx: the launch direction of the ray's global path (csrc/hrt_launch_dir.h)
__device__ __forceinline__ hrt_launch_dir_t hit_launch_dir(const hrt_kview &V, const hrt_kshard &S, uint32_t b,
                                                           uint32_t tx, uint32_t i)
{
    const uint32_t local = hit_field(V, b, HRT_HIT_RAY)[i] - tx * V.num_local;
    return hrt_launch_dir(hrt_shard_path(local, S.chunk, S.count, S.rank), S.num_paths);
}

// The HRT_PS_REC_FLOATS floats of record i of hit block b at receiver rx into R (a caller that sums in FP64 widens
// them itself): nu is the float difference FS0 - DFS, u_rx the record's HRT_REC_DIR.  The two MFMA kernels that stage
// into LDS (hrt_array_partial_kernel, hrt_array_taps_partial_kernel) write these lines out: see there.
__device__ __forceinline__ void stage_record(const hrt_kview &V, const hrt_kshard &S, uint32_t b, uint32_t rx,
                                             uint32_t tx, uint32_t i, float *R)
{
    R[0] = rec_field(V, b, rx, HRT_REC_A_TE_RE)[i];
    R[1] = rec_field(V, b, rx, HRT_REC_A_TE_IM)[i];
    R[2] = rec_field(V, b, rx, HRT_REC_A_TM_RE)[i];
    R[3] = rec_field(V, b, rx, HRT_REC_A_TM_IM)[i];
    R[4] = rec_field(V, b, rx, HRT_REC_TAU)[i];
    R[5] = __uint_as_float(hit_field(V, b, HRT_HIT_FS0)[i]) - rec_field(V, b, rx, HRT_REC_DFS)[i];
    R[6] = rec_field(V, b, rx, HRT_REC_DIRX)[i];
    R[7] = rec_field(V, b, rx, HRT_REC_DIRY)[i];
    R[8] = rec_field(V, b, rx, HRT_REC_DIRZ)[i];
    const hrt_launch_dir_t d = hit_launch_dir(V, S, b, tx, i);
    R[9] = d.fx;
    R[10] = d.fy;
    R[11] = d.fz;
}

// e[0..2] = r_i, e[3..5] = q_j of element pair a = i nt + j (the sEl rows of the array kernels)
__device__ __forceinline__ void load_pair(const float *rx_el, const float *tx_el, uint32_t nt, uint32_t a, float *e)
{
    const uint32_t i = a / nt, j = a - i * nt;
    for (int q = 0; q < 3; ++q) {
        e[q] = rx_el[3u * i + q];
        e[3 + q] = tx_el[3u * j + q];
    }
}

// r . u in FP64 from float operands.  The steering path difference of an element pair (metres) is
// dot3(r_i, u_rx) + dot3(q_j, u_tx); the LoS term has u_rx = -u_tx.
__device__ __forceinline__ double dot3(const float *r, const float *u)
{
    return (double)r[0] * u[0] + (double)r[1] * u[1] + (double)r[2] * u[2];
}

// The two halves the complex reduce kernels share (one float2 per thread; hrt_channel_reduce_kernel carries both
// polarisations in a float4 and stores them T * K apart: it keeps its own).  The partial sums of one output, chunk
// 0's at src and the chunks `stride` apart, added in index order ...
__device__ __forceinline__ float2 sum_chunks(const float2 *src, uint32_t nchunks, uint64_t stride)
{
    float2 s = make_float2(0.f, 0.f);
    for (uint32_t c = 0; c < nchunks; ++c) {
        const float2 v = src[(uint64_t)c * stride];
        s.x += v.x;
        s.y += v.y;
    }
    return s;
}

// ... and the store: s, added to what is there if accumulate
__device__ __forceinline__ void store_out(float2 *o, float2 s, uint32_t accumulate)
{
    if (accumulate) {
        const float2 v = o[0];
        s.x += v.x;
        s.y += v.y;
    }
    o[0] = s;
}

// What the reduce kernels of the pair families share (one thread per output gid = ((link * npairs + pair) * 2 + pol)
// * T K + col; partial sums [link][chunk][pol][pair][T K]): the output's link, pair and column and the sum s of its
// chunks (false past the last output), and the W phase of a LoS entry (tau, nu) at a column, in revolutions.
struct hrt_pair_output {
    uint32_t link, pair;
    uint64_t col;
    float2 s;
};

__device__ __forceinline__ bool pair_output(const hrt_kview &V, const hrt_kgrid &G, uint32_t npairs, const float *partial,
                                            uint64_t gid, hrt_pair_output &o)
{
    const uint64_t tk = (uint64_t)G.T * G.K;
    const uint64_t per_link = (uint64_t)npairs * 2u * tk;
    if (gid >= per_link * V.nrx * V.ntx) return false;
    o.link = (uint32_t)(gid / per_link);
    const uint64_t e = gid - (uint64_t)o.link * per_link;   // = (pair * 2 + pol) * tk + col
    const uint32_t pol = (uint32_t)(e / tk) & 1u;
    o.pair = (uint32_t)(e / (2u * tk));
    o.col = e % tk;
    const float2 *src = reinterpret_cast<const float2 *>(partial) + (uint64_t)o.link * V.nchunks * per_link +
                        ((uint64_t)pol * npairs + o.pair) * tk + o.col;
    o.s = sum_chunks(src, V.nchunks, per_link);
    return true;
}

__device__ __forceinline__ double pair_los_phase(const hrt_kgrid &G, uint64_t col, float tau, float nu)
{
    const uint32_t m = (uint32_t)(col / G.K), k = (uint32_t)(col % G.K);
    const double t = G.t0 + (double)m * G.dt, f = G.f0 + (double)k * G.df;
    return (double)nu * t - f * (double)tau;
}

// The LoS entry of a link: a (real, TE = TM), tau, nu (the path list's freq_shift) and u = directions_tx
// (directions_rx = -u).  False where the LoS is blocked.  Coincident: a = 1, tau = nu = 0, directions_rx = (1, 0, 0),
// directions_tx = (-1, 0, 0) (src/compute_paths.c:533-534).
struct hrt_los_entry {
    float a, tau, nu, ux, uy, uz;
};

__device__ __forceinline__ bool los_entry(const hrt_kview &V, uint32_t link, hrt_los_entry &e)
{
    const float *L = reinterpret_cast<const float *>(V.ws + V.off_los) + (uint64_t)link * HRT_LOS_FLOATS;
    const uint32_t status = __float_as_uint(L[HRT_LOS_STATUS]);
    e = hrt_los_entry{1.f, 0.f, 0.f, -1.f, 0.f, 0.f};
    if (status == 2u) {   // clear
        e.a = L[HRT_LOS_A]; e.tau = L[HRT_LOS_TAU]; e.nu = L[HRT_LOS_FS];
        e.ux = L[HRT_LOS_DIRX]; e.uy = L[HRT_LOS_DIRY]; e.uz = L[HRT_LOS_DIRZ];
    }
    return status == 0u || status == 2u;
}

// What the reduce kernels of the taps families share (one thread per output gid = ((link * npairs + pair) * 2 + pol)
// * T L + m L + tap; partial sums in the same order per chunk; hrt_taps: npairs = 1; G: the hrt_ktgrid, or the
// hrt_ktaps, which has its fields): the output's link, pair, time sample and tap and the sum s of its chunks (false
// past the last output); of a LoS entry at an output, the phase nu t_m - f_c tau in revolutions (the array family adds
// its steering) and the weight a sinc(l - f_s tau).
struct hrt_taps_output {
    uint32_t link, pair, m, tap;
    float2 s;
};

template <typename TG>
__device__ __forceinline__ bool taps_output(const hrt_kview &V, const TG &G, uint32_t npairs, const float *partial,
                                            uint64_t gid, hrt_taps_output &o)
{
    const uint64_t tl = (uint64_t)G.T * G.L;
    const uint64_t per_link = (uint64_t)npairs * 2u * tl;
    if (gid >= per_link * V.nrx * V.ntx) return false;
    o.link = (uint32_t)(gid / per_link);
    const uint64_t e = gid - (uint64_t)o.link * per_link;   // = (pair * 2 + pol) * tl + m * L + tap
    o.pair = (uint32_t)(e / (2u * tl));
    const uint64_t mi = e % tl;
    o.m = (uint32_t)(mi / G.L);
    o.tap = (uint32_t)(mi % G.L);
    const float2 *src = reinterpret_cast<const float2 *>(partial) + (uint64_t)o.link * V.nchunks * per_link + e;
    o.s = sum_chunks(src, V.nchunks, per_link);
    return true;
}

template <typename TG>
__device__ __forceinline__ double taps_los_phase(const TG &G, uint32_t m, const hrt_los_entry &L)
{
    const double t = G.t0 + (double)m * G.dt;
    return (double)L.nu * t - G.fc * (double)L.tau;
}

template <typename TG>
__device__ __forceinline__ float taps_los_weight(const TG &G, uint32_t tap, const hrt_los_entry &L)
{
    return L.a * sinc_tap(G.l_min + (int32_t)tap, sinc_prep(G.fs, L.tau));
}

// Fill sB / sI (bounce, hit) with the next at most BATCH unblocked records of chunk c of link (rx, tx), compacted by
// mask ballots; (b, cur, end) is where the walk stands (start it with b = 0 and chunk_range of block 0).  Every wave
// takes the same decisions; wave 0 writes the list.  Returns the number of records staged: 0 once the chunk is done.
// (hrt_array_partial_kernel writes the same loop out: see there.)
template <uint32_t BATCH>
__device__ __forceinline__ uint32_t fill_batch(const hrt_kview &V, uint32_t rx, uint32_t tx, uint32_t c, uint32_t lane,
                                               uint32_t w, uint32_t &b, uint32_t &cur, uint32_t &end, uint32_t *sB,
                                               uint32_t *sI)
{
    uint32_t n = 0;
    while (n < BATCH && b < V.nb) {
        if (cur >= end) {
            if (++b < V.nb) chunk_range(V, b, tx, c, cur, end);
            continue;
        }
        const uint32_t i = cur + lane;
        const uint64_t *mask = mask_row(V, b, rx);
        const bool live = i < end && ((mask[i >> 6] >> (i & 63u)) & 1u);
        const uint64_t bal = __ballot(live);
        const uint32_t cnt = __popcll(bal), take = min(cnt, BATCH - n);
        const uint32_t rank = __popcll(bal & ((1ull << lane) - 1ull));
        if (w == 0 && live && rank < take) {
            sB[n + rank] = b;
            sI[n + rank] = i;
        }
        if (take < cnt) {   // resume at the first live record not taken
            uint64_t rest = bal;
            for (uint32_t t = 0; t < take; ++t) rest &= rest - 1ull;
            cur += (uint32_t)__builtin_ctzll(rest);
        } else {
            cur += 64u;
        }
        n += take;
    }
    return n;
}

// The launch of a pair family (P: hrt_karray or hrt_kbeam): the TX segments and the partial kernel where the call has
// a scatter part, the family's LoS pre-pass where it has one (`los`, one thread per (link, pair); may be NULL) and
// the call a LoS part, then the reduce kernel, one thread per output.
template <typename KP>
int launch_pair_family(const KP *P, uint32_t threads, void (*partial)(const KP), void (*los)(const KP),
                       void (*reduce)(const KP), void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint32_t links = P->v.nrx * P->v.ntx;
    if (P->v.nchunks) {
        const int e = hrt_hip_launch_segments(&P->v, stream);
        if (e) return e;
        hipLaunchKernelGGL(partial, dim3(P->g.pblocks * P->g.cblocks, P->v.nchunks, links), dim3(threads), 0, st, *P);
    }
    if (los && P->v.los) {
        const uint64_t g = (uint64_t)links * P->npairs;
        hipLaunchKernelGGL(los, dim3((unsigned)((g + 255u) / 256u)), dim3(256), 0, st, *P);
    }
    const uint64_t n = (uint64_t)links * P->npairs * 2u * P->g.T * P->g.K;
    hipLaunchKernelGGL(reduce, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, st, *P);
    return (int)hipGetLastError();
}

// The launch of a taps family (P: hrt_ktaps, hrt_karray_taps or hrt_kbeam_taps, G its grid; npairs 1 for hrt_ktaps): as
// launch_pair_family, with the partial kernel in the form of G.rt (`partial4`: rt = 4, `partial1`: rt = 1).
template <typename KP, typename TG>
int launch_taps_family(const KP *P, const TG &G, uint32_t npairs, uint32_t threads, void (*partial4)(const KP),
                       void (*partial1)(const KP), void (*los)(const KP), void (*reduce)(const KP), void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint32_t links = P->v.nrx * P->v.ntx;
    if (P->v.nchunks) {
        const int e = hrt_hip_launch_segments(&P->v, stream);
        if (e) return e;
        hipLaunchKernelGGL(G.rt == 4u ? partial4 : partial1, dim3(G.rblocks * G.cblocks, P->v.nchunks, links),
                           dim3(threads), 0, st, *P);
    }
    if (los && P->v.los) {
        const uint64_t g = (uint64_t)links * npairs;
        hipLaunchKernelGGL(los, dim3((unsigned)((g + 255u) / 256u)), dim3(256), 0, st, *P);
    }
    const uint64_t n = (uint64_t)links * npairs * 2u * G.T * G.L;
    hipLaunchKernelGGL(reduce, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, st, *P);
    return (int)hipGetLastError();
}

}  // namespace
#endif /* __HIPCC__ */

#endif /* HRT_PATHSUM_H */
