/* compute_paths.c -- the drop-in entry point: host arrays in, the reference's dense layout out.
 *
 * Replaces src/compute_paths.c:419-757 of the reference behind the same C symbol
 * (inc/compute_paths.h:59-74).  The tracing itself happens on the GPU (hrt_trace); this file
 * only moves data and lays the compact device result out the way the reference's callers
 * expect, INCLUDING the reference's observable layout quirks:
 *   Q1  scatter directions_tx is never written
 *   Q2  slots of dead rays, and directions/freq_shift of blocked records, are not touched
 *   Q3  a blocked LoS pair leaves its directions/freq_shift untouched
 *   Q9  scatter freq_shift launch term + memcpy replication (src/compute_paths.c:494-508)
 *   Q10 the "+= 0" on freq_shift[tx*np+path] (:663-664): replayed in the reference's (bounce, tx)
 *       order -- it can turn a -0 into +0, or a slot into NaN for a non-finite mesh velocity
 *   Q11/Q12/Q14 RaysInfo snapshot offsets use stride num_bounces, the active-mask snapshot is
 *       always taken from byte 0, dead rays keep their last origin/direction
 *
 * Rays are processed in batches (round-robin shards of the path index, hrt_device.h) sized to
 * a device-memory budget, so the dense ABI works for any num_rays the HOST arrays can hold
 * (with raysInfo_scat != NULL the launch set must fit one batch).
 *
 * There is no CPU tracing path here: any HIP failure is an error.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hrt_internal.h"

#include <pthread.h>
#include <unistd.h>
#include <math.h>

/* (the parallel-for of the host writers, hrt_parallel_ranges, and hrt_host_threads: parallel.c) */

/* ---- launch-table cache -------------------------------------------------------------------
 * The launch directions depend on num_rays only, and the coherent launch order of an unbatched
 * call on them only: callers that sample a channel again and again (moving endpoints, same ray
 * count) would otherwise spend a third of every call recomputing 3*np double-precision libm
 * results.  One entry (the last num_rays), owned by the library until hrt_cache_clear() or the
 * next different num_rays; HRT_NO_CACHE=1 disables it; tables beyond 1 GiB are not kept. */
static pthread_mutex_t g_cache_lock = PTHREAD_MUTEX_INITIALIZER;
static struct { uint64_t np; float *dirs; uint32_t *order; } g_cache;

void hrt_cache_clear(void)
{
    pthread_mutex_lock(&g_cache_lock);
    free(g_cache.dirs); free(g_cache.order);
    g_cache.np = 0; g_cache.dirs = NULL; g_cache.order = NULL;
    pthread_mutex_unlock(&g_cache_lock);
    hrt_pool_release_all();   /* (batch.c) */
    hrt_list_cache_clear();   /* (path_list.c) */
    hrt_parallel_release();   /* ... and the calling thread's parked helper threads */
}

int hrt_launch_cache_enabled(uint64_t np) { return !hrt_env_int("HRT_NO_CACHE", 0) && np * 16 <= (1ull << 30); }

/* copies of the cached tables for `np` into dirs / order (either may be NULL); 1 if served */
int hrt_launch_cache_get(uint64_t np, float *dirs, uint32_t *order)
{
    int hit = 0;
    pthread_mutex_lock(&g_cache_lock);
    if (g_cache.np == np && g_cache.dirs && (!order || g_cache.order)) {
        if (dirs) memcpy(dirs, g_cache.dirs, np * 12);
        if (order) memcpy(order, g_cache.order, np * 4);
        hit = 1;
    }
    pthread_mutex_unlock(&g_cache_lock);
    return hit;
}

void hrt_launch_cache_put(uint64_t np, const float *dirs, const uint32_t *order)
{
    if (!hrt_launch_cache_enabled(np)) return;
    pthread_mutex_lock(&g_cache_lock);
    if (g_cache.np != np) {
        free(g_cache.dirs); free(g_cache.order);
        g_cache.dirs = NULL; g_cache.order = NULL; g_cache.np = np;
    }
    if (dirs && !g_cache.dirs && (g_cache.dirs = (float *)malloc(np * 12))) memcpy(g_cache.dirs, dirs, np * 12);
    if (order && !g_cache.order && (g_cache.order = (uint32_t *)malloc(np * 4))) memcpy(g_cache.order, order, np * 4);
    if (!g_cache.dirs) { free(g_cache.order); g_cache.order = NULL; g_cache.np = 0; }
    pthread_mutex_unlock(&g_cache_lock);
}

#ifndef HRT_SCATTER_AHEAD
#define HRT_SCATTER_AHEAD 64u
#endif
typedef struct {
    const hrt_shard *s;
    const uint32_t *ray;
    float *const *rec;
    const uint64_t *mask;
    ChannelInfo *scat;
    uint64_t n_loc, i_base;   /* the range handed to scatter_range is relative to i_base */
    size_t rx, b, ntx, nb, np, amp_stride;
    /* slim records: directions_rx and tau are not copied from the device (16 of a record's 36 bytes)
     * but formed here from the hit's origin and delay (16 bytes per HIT) with the reference's own
     * float sequence (src/compute_paths.c:676-678, :709): sub, mul, add, sqrtf, div -- IEEE
     * operations, contraction off: the same bits as the device's */
    const float *hs[4];       /* NULL: the records carry them */
    float rxp[3];
    uint64_t unblocked[HRT_MAX_SCATTER_THREADS];
} scatter_ctx;

/* The slim path forms tau and directions_rx HERE with the reference's float sequence: the bits only match the
 * device's if nothing in this file is contracted into an FMA.  The Makefile says -ffp-contract=off; so does the source */
#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif
#if defined(__FAST_MATH__)
#error "compute_paths.c must not be built with -ffast-math: the slim records are formed on the host bit-exactly"
#endif

/* records of (bounce b, rx) -> dense slots ((rx*ntx+tx)*nb+b)*np+p   (src/compute_paths.c:674).
 * The index arithmetic is the hot part of the host side (27 M records on C3): the 64-bit
 * divisions of the general shard mapping cost more than the nine stores, so the two common cases
 * -- one TX, and one batch or the default power-of-two granule -- are done with shifts. */
static void scatter_range(void *vctx, uint64_t i0, uint64_t i1, int tid)
{
    scatter_ctx *c = (scatter_ctx *)vctx;
    ChannelInfo *scat = c->scat;
    uint64_t unb = 0;
    const hrt_shard *s = c->s;
    const uint32_t ch = s->chunk ? s->chunk : 4096u;
    const int ch_pow2 = (ch & (ch - 1u)) == 0u;
    int sh = 0;
    while ((1u << sh) < ch) ++sh;
    const uint64_t count = s->count, rank = s->rank, n_loc = c->n_loc;
    float *const a0 = scat->a_te_re, *const a1 = scat->a_te_im, *const a2 = scat->a_tm_re, *const a3 = scat->a_tm_im;
    const size_t as = c->amp_stride;
    float *const tau = scat->tau, *const fs = scat->freq_shift;
    Vec3 *const drx = scat->directions_rx;
    const float *r0 = c->rec[HRT_REC_A_TE_RE], *r1 = c->rec[HRT_REC_A_TE_IM], *r2 = c->rec[HRT_REC_A_TM_RE],
                *r3 = c->rec[HRT_REC_A_TM_IM], *r4 = c->rec[HRT_REC_TAU], *r5 = c->rec[HRT_REC_DIRX],
                *r6 = c->rec[HRT_REC_DIRY], *r7 = c->rec[HRT_REC_DIRZ], *r8 = c->rec[HRT_REC_DFS];
    const float *const hox = c->hs[0], *const hoy = c->hs[1], *const hoz = c->hs[2], *const htau = c->hs[3];
    const float rxx = c->rxp[0], rxy = c->rxp[1], rxz = c->rxp[2];
    /* The slots of consecutive records are scattered over a window of the dense arrays (the launch
     * order walks a z-band of 32 768 paths by azimuth, not by path index: 128 KB per array, seven
     * arrays): most stores miss the near caches, so the lines of the record HRT_SCATTER_AHEAD entries
     * on are requested for ownership now (its slot arithmetic is repeated: cheaper than the misses it
     * hides; warm C3 readback 39-42 -> 33 ms; 16 ... 128 entries ahead measure the same within noise, 4
     * and 8 gain nothing).  Ordering each window of 8 192 records by slot first -- sequential stores,
     * random loads from the staging -- was slower than either (48 ms). */
#define SLOT_OF(I, OFF)                                                                          \
    do {                                                                                         \
        uint64_t ql_ = c->ray[(I)];                                                              \
        size_t tx_ = 0;                                                                          \
        if (c->ntx > 1) { tx_ = ql_ / n_loc; ql_ -= tx_ * n_loc; }                               \
        uint64_t p_;                                                                             \
        if (count == 1) p_ = ql_;                                                                \
        else if (ch_pow2) p_ = (((ql_ >> sh) * count + rank) << sh) + (ql_ & (ch - 1u));         \
        else p_ = ((ql_ / ch) * count + rank) * ch + ql_ % ch;                                   \
        (OFF) = ((c->rx * c->ntx + tx_) * c->nb + c->b) * c->np + p_;                            \
    } while (0)
    const uint64_t i_end = c->i_base + i1;
    for (uint64_t i = c->i_base + i0; i < i_end; ++i) {
        if (i + HRT_SCATTER_AHEAD < i_end) {
            size_t offp;
            SLOT_OF(i + HRT_SCATTER_AHEAD, offp);
            __builtin_prefetch(&a0[offp * as], 1, 1); __builtin_prefetch(&a1[offp * as], 1, 1);
            __builtin_prefetch(&a2[offp * as], 1, 1); __builtin_prefetch(&a3[offp * as], 1, 1);
            __builtin_prefetch(&tau[offp], 1, 1); __builtin_prefetch(&drx[offp], 1, 1);
            __builtin_prefetch(&fs[offp], 1, 1);
        }
        size_t off;
        SLOT_OF(i, off);
        a0[off * as] = r0[i];
        a1[off * as] = r1[i];
        a2[off * as] = r2[i];
        a3[off * as] = r3[i];
        const int unblocked = (int)((c->mask[i >> 6] >> (i & 63)) & 1u);
        if (hox) {
            if (unblocked) {   /* :676-678 shadow direction and distance, :709 delay, :707 direction */
                const float wx = rxx - hox[i], wy = rxy - hoy[i], wz = rxz - hoz[i];
                const float d2rx = sqrtf((wx * wx + wy * wy) + wz * wz);
                const float ux = wx / d2rx, uy = wy / d2rx, uz = wz / d2rx;
                tau[off] = htau[i] + d2rx / HRT_C_F;
                drx[off] = (Vec3){-ux, -uy, -uz};
                fs[off] -= r8[i];       /* :722 */
                ++unb;
            } else {
                tau[off] = 0.f;         /* :688 */
            }
            continue;
        }
        tau[off] = r4[i];
        if (unblocked) {
            drx[off] = (Vec3){r5[i], r6[i], r7[i]};
            fs[off] -= r8[i];       /* :722 */
            ++unb;
        }
    }
#undef SLOT_OF
    c->unblocked[tid] += unb;
}

/* a memcpy cut into ranges */
typedef struct { float *dst; const float *src; } copy_ctx;
static void copy_range(void *vctx, uint64_t i0, uint64_t i1, int tid)
{
    (void)tid;
    const copy_ctx *c = (const copy_ctx *)vctx;
    memcpy(c->dst + i0, c->src + i0, (i1 - i0) * sizeof(float));
}

/* RaysInfo, this batch's part, on the helper threads (a snapshot is 24 B per launched ray and bounce: 0.5 GB on
 * C3 -- one thread took 0.15 s of the 0.19 s call for it):
 * rays_init_range    the launch block: state of local ray il of every TX = {tx_pos, direction}
 * rays_update_range  after a bounce: the rays that hit take their new state, and their bit in the bounce's
 *                    active string (atomic OR: neighbouring entries share bytes)
 * rays_copy_range    the batch's states -> the dense snapshot, granule by granule (item = tx * n_gran + granule) */
typedef struct {
    const hrt_shard *s;
    Ray *cur;                 /* [ntx][n_loc] */
    const float *dirs;        /* [n_loc][3] */
    const Vec3 *tx_pos;
    const uint32_t *ray;
    float *const *st;         /* o.xyz, d.xyz of the hits */
    uint8_t *act;
    Ray *dst;                 /* snapshot base of this bounce: dst + tx * dst_tx_stride + p */
    uint64_t dst_tx_stride, n_loc, np, n_gran;
    size_t ntx;
    uint32_t ch;
} rays_ctx;
static void rays_init_range(void *vctx, uint64_t i0, uint64_t i1, int tid)
{
    (void)tid;
    const rays_ctx *c = (const rays_ctx *)vctx;
    for (size_t tx = 0; tx < c->ntx; ++tx)
        for (uint64_t il = i0; il < i1; ++il) {
            Ray *r = &c->cur[tx * c->n_loc + il];
            r->o = c->tx_pos[tx];
            memcpy(&r->d, c->dirs + 3 * il, sizeof(Vec3));
        }
}
static void rays_update_range(void *vctx, uint64_t i0, uint64_t i1, int tid)
{
    (void)tid;
    const rays_ctx *c = (const rays_ctx *)vctx;
    for (uint64_t i = i0; i < i1; ++i) {
        const uint32_t ql = c->ray[i];           /* tx * n_loc + local path */
        const uint64_t tx = ql / c->n_loc, il = ql - tx * c->n_loc;
        const uint64_t q = tx * c->np + hrt_shard_global_path(c->s, il);
        __atomic_fetch_or(&c->act[q / 8], (uint8_t)(1u << (q % 8)), __ATOMIC_RELAXED);
        Ray *r = &c->cur[ql];
        r->o = (Vec3){c->st[0][i], c->st[1][i], c->st[2][i]};
        r->d = (Vec3){c->st[3][i], c->st[4][i], c->st[5][i]};
    }
}
static void rays_copy_range(void *vctx, uint64_t i0, uint64_t i1, int tid)
{
    (void)tid;
    const rays_ctx *c = (const rays_ctx *)vctx;
    for (uint64_t it = i0; it < i1; ++it) {
        const uint64_t tx = it / c->n_gran, il = (it - tx * c->n_gran) * c->ch;
        const uint64_t len = c->n_loc - il < c->ch ? c->n_loc - il : c->ch;
        memcpy(c->dst + tx * c->dst_tx_stride + hrt_shard_global_path(c->s, il), c->cur + tx * c->n_loc + il, len * sizeof(Ray));
    }
}

/* Q10 adds of one TX run (distinct slots: one per ray), see run_batch */
typedef struct {
    const hrt_shard *s;
    const uint32_t *ray, *tri;
    const float *h_mesh;
    const uint32_t *tri_mesh;
    float *fs_tx;            /* freq_shift + tx * np */
    float dop_mult;
    uint64_t ray_base, i_base;
} q10_ctx;
static void q10_range(void *vctx, uint64_t i0, uint64_t i1, int tid)
{
    (void)tid;
    q10_ctx *c = (q10_ctx *)vctx;
    const hrt_shard *s = c->s;
    const uint32_t ch = s->chunk ? s->chunk : 4096u;
    const uint64_t count = s->count, rank = s->rank;
    const uint64_t i_end = c->i_base + i1;
    for (uint64_t i = c->i_base + i0; i < i_end; ++i) {
        if (i + HRT_SCATTER_AHEAD < i_end) {   /* as in scatter_range */
            const uint64_t qa = c->ray[i + HRT_SCATTER_AHEAD] - c->ray_base;
            __builtin_prefetch(&c->fs_tx[(count == 1) ? qa : ((qa / ch) * count + rank) * ch + qa % ch], 1, 1);
        }
        const uint64_t ql = c->ray[i] - c->ray_base;
        const uint64_t p = (count == 1) ? ql : ((ql / ch) * count + rank) * ch + ql % ch;
        const float *mv = c->h_mesh + (size_t)c->tri_mesh[c->tri[i]] * HRT_MESH_FLOATS;
        const float zero = 0.f;   /* d - d with finite d */
        float z = (zero * mv[0] + zero * mv[1]) + zero * mv[2];
        c->fs_tx[p] += z * c->dop_mult;
    }
}

/* ---- devices --------------------------------------------------------------------------------
 * HRT_DEVICES="0,1,2,3" (HIP device ids; an id may repeat: logical devices on one GPU, which is how
 * the multi-device path is tested on a one-GPU box) or HRT_DEVICE=n (one device, default 0).
 * compute_paths() is one blocking call (inc/compute_paths.h:59-74); with D devices the round-robin
 * batches of the launch set (hrt_shard) are dealt to D host threads, one per device, each with its
 * own problem copy, workspace, streams and page-locked staging; every device copies its records
 * over its own PCIe link straight into the caller's dense arrays (the slots of different batches are
 * disjoint: no exchange step, no RCCL). */
static int parse_devices(int *dev)
{
    const char *v = getenv("HRT_DEVICES");
    int n = 0;
    if (v && *v) {
        const char *q = v;
        while (*q && n < HRT_MAX_DEVICES) {
            char *end = NULL;
            long d = strtol(q, &end, 10);
            if (end == q) break;
            dev[n++] = (int)d;
            q = end;
            while (*q == ',' || *q == ' ') ++q;
        }
    }
    if (n == 0) { dev[0] = hrt_env_int("HRT_DEVICE", 0); n = 1; }
    return n;
}

#define DL(dst, off, bytes)                                                              \
    do {                                                                                 \
        rc = hrt_device_download(w->device, (dst), (const uint8_t *)w->d_ws + (off), (bytes)); \
        if (rc) goto done;                                                               \
    } while (0)

/* one batch (shard g of G) on this worker's device: tables, trace, readback into the dense arrays */
static int run_batch(dev_ctx *c, uint32_t g)
{
    work_t *w = &c->w;
    hrt_problem *prob = c->prob;
    const size_t nb = c->nb, nrx = c->nrx, ntx = c->ntx, np = c->np, nq = c->nq;
    const uint32_t G = c->G;
    ChannelInfo *los = c->los, *scat = c->scat;
    RaysInfo *los_rays = c->los_rays, *scat_rays = c->scat_rays;
    const Vec3 *rx_pos = c->rx_pos, *tx_pos = c->tx_pos;
    hrt_stats *st = &c->st;
    int rc = HRT_OK;
    hrt_layout L;
    double t0;

    hrt_shard s = {np, g, G, 0, (uint32_t)nb};
    const uint64_t n_loc = hrt_shard_num_local(&s);
    if (n_loc == 0) return HRT_OK;
    rc = hrt_layout_query(prob, &s, &L);
    if (rc) goto done;
    if (c->host_launch) {
        /* this batch's launch directions: gather from the whole-sphere table */
        const float *src = w->h_dirs;
        if (G > 1) {
            if (!w->dirs_batch) w->dirs_batch = (float *)malloc(hrt_shard_num_local(&(hrt_shard){np, 0, G, 0, (uint32_t)nb}) * 12);
            if (!w->dirs_batch) { rc = hrt_fail(HRT_E_NOMEM, "out of host memory"); goto done; }
            for (uint64_t i = 0; i < n_loc; ++i)
                memcpy(w->dirs_batch + 3 * i, w->h_dirs + 3 * hrt_shard_global_path(&s, i), 12);
            src = w->dirs_batch;
        }
        t0 = hrt_now_s();
        if (!(G == 1 && hrt_launch_cache_enabled(np) && hrt_launch_cache_get(np, NULL, w->h_order))) {
            if ((rc = hrt_launch_order_host(&s, src, w->h_order))) goto done;
            if (G == 1) hrt_launch_cache_put(np, w->h_dirs, w->h_order);
        }
        c->t_launch += hrt_now_s() - t0;   /* host-side launch preparation */
        t0 = hrt_now_s();
        if ((rc = hrt_device_upload(w->device, w->d_dirs, src, n_loc * 12))) goto done;
        if ((rc = hrt_device_upload(w->device, w->d_order, w->h_order, n_loc * 4))) goto done;
    } else {
        t0 = hrt_now_s();
        if (G > 1 && (rc = hrt_launch_dirs_device(&s, (float *)w->d_dirs, w->device, NULL, NULL))) goto done;
        if ((rc = hrt_launch_order_device(&s, (uint32_t *)w->d_order, w->device, NULL))) goto done;
        c->t_launch += hrt_now_s() - t0;
        t0 = hrt_now_s();
    }
    if ((rc = hrt_trace_batch(prob, &s, &L, w, st))) goto done;   /* (batch.c) */
    c->t_dev += hrt_now_s() - t0;

    t0 = hrt_now_s();

    /* ---- LoS block (identical in every batch; written once, by the owner of batch 0) :515-577 ---- */
    if (g == 0) {
        DL(w->h_los, L.off_los, nrx * ntx * HRT_LOS_FLOATS * sizeof(float));
        const size_t as = c->amp_stride;
        for (size_t off = 0; off < nrx * ntx; ++off) los->a_te_im[off * as] = los->a_tm_im[off * as] = 0.f;
        for (size_t rx = 0, off = 0; rx < nrx; ++rx)
            for (size_t tx = 0; tx < ntx; ++tx, ++off) {
                const float *q = w->h_los + HRT_LOS_FLOATS * off;
                uint32_t status;
                memcpy(&status, &q[HRT_LOS_STATUS], 4);
                const uint8_t bit = (uint8_t)(1u << (off % 8));
                if (los_rays) {
                    Ray *r = &los_rays->rays[off];
                    r->o = tx_pos[tx];
                    r->d.x = rx_pos[rx].x - tx_pos[tx].x;
                    r->d.y = rx_pos[rx].y - tx_pos[tx].y;
                    r->d.z = rx_pos[rx].z - tx_pos[tx].z;
                }
                if (status == 0u) {          /* coincident */
                    los->directions_rx[off] = (Vec3){1.f, 0.f, 0.f};
                    los->directions_tx[off] = (Vec3){-1.f, 0.f, 0.f};
                    los->a_te_re[off * as] = los->a_tm_re[off * as] = 1.f;
                    los->tau[off] = 0.f;
                    los->freq_shift[off] = 0.f;
                    if (los_rays) los_rays->rays_active[off / 8] |= bit;
                } else if (status == 1u) {   /* blocked: Q3 */
                    los->a_te_re[off * as] = los->a_tm_re[off * as] = los->tau[off] = 0.f;
                    if (los_rays) los_rays->rays_active[off / 8] &= (uint8_t)~bit;
                } else {
                    Vec3 u = {q[HRT_LOS_DIRX], q[HRT_LOS_DIRY], q[HRT_LOS_DIRZ]};
                    los->directions_tx[off] = u;
                    los->directions_rx[off] = (Vec3){-u.x, -u.y, -u.z};
                    los->a_te_re[off * as] = los->a_tm_re[off * as] = q[HRT_LOS_A];
                    los->tau[off] = q[HRT_LOS_TAU];
                    los->freq_shift[off] = q[HRT_LOS_FS];
                    if (los_rays) los_rays->rays_active[off / 8] |= bit;
                }
            }
    }

    /* ---- bounces: scatter the compact blocks into the dense arrays ----
     * With one TX (one run per bounce) the NEXT bounce is started while the last block of this one is
     * written: its rays and triangles and its first record block are requested then (`pre`), so no
     * copy is waited for with the writer idle except the very first. */
    if (scat_rays) {
        /* :589 -- the launch block [tx][p] = {tx_pos, direction}, this batch's paths; and the batch's ray
         * states (the directions of a device-generated launch set are fetched from d_dirs) */
        const float *dsrc;
        if (c->host_launch) dsrc = (G > 1) ? w->dirs_batch : w->h_dirs;
        else {
            if (!w->dirs_batch) w->dirs_batch = (float *)malloc(hrt_shard_num_local(&(hrt_shard){np, 0, G, 0, (uint32_t)nb}) * 12);
            if (!w->dirs_batch) { rc = hrt_fail(HRT_E_NOMEM, "out of host memory"); goto done; }
            if ((rc = hrt_device_download(w->device, w->dirs_batch, w->d_dirs, n_loc * 12))) goto done;
            dsrc = w->dirs_batch;
        }
        if (!w->cur_rays) w->cur_rays = (Ray *)malloc(ntx * hrt_shard_num_local(&(hrt_shard){np, 0, G, 0, (uint32_t)nb}) * sizeof(Ray));
        if (!w->cur_rays) { rc = hrt_fail(HRT_E_NOMEM, "out of host memory"); goto done; }
        const uint32_t ch = s.chunk ? s.chunk : 4096u;
        rays_ctx rc0;
        memset(&rc0, 0, sizeof rc0);
        rc0.s = &s; rc0.cur = w->cur_rays; rc0.dirs = dsrc; rc0.tx_pos = tx_pos; rc0.n_loc = n_loc; rc0.np = np;
        rc0.ntx = ntx; rc0.ch = ch; rc0.n_gran = (n_loc + ch - 1) / ch;
        rc0.dst = scat_rays->rays; rc0.dst_tx_stride = np;   /* :589: the launch block is [tx][p] */
        hrt_parallel_ranges(rays_init_range, &rc0, n_loc, c->scatter_threads);
        hrt_parallel_ranges(rays_copy_range, &rc0, ntx * rc0.n_gran, c->scatter_threads);
    }
    const int can_pre = !prob->tune.no_bounce_prefetch;
    /* slim records (default; HRT_FULL_RECORDS=1 copies all nine fields): see scatter_ctx */
    const int slim = !hrt_env_int("HRT_FULL_RECORDS", 0);
    static const int hs_field[4] = {HRT_HIT_OX, HRT_HIT_OY, HRT_HIT_OZ, HRT_HIT_TAU};
    int pre = 0, pre_block_next = 0, flip = 0;   /* staging set of a block: (slot + flip) & 1 */
    for (size_t b = 0; b < nb; ++b) {
        const uint64_t H = w->h_counts[b + 1];
        const uint64_t hb = L.off_hits + b * L.hit_block_bytes;
        const int prefetched = pre, pre_block = pre_block_next;   /* this bounce's hit arrays / first block are on their way */
        pre = 0; pre_block_next = 0;
        if (H && prefetched) {   /* requested during the previous bounce, into the second pair of arrays */
            uint32_t *t_ = w->ray; w->ray = w->ray2; w->ray2 = t_;
            t_ = w->tri; w->tri = w->tri2; w->tri2 = t_;
            for (int k = 0; k < 4; ++k) { float *f_ = w->hs[k]; w->hs[k] = w->hs2[k]; w->hs2[k] = f_; }
            int e = hrt_hip_stream_sync(w->copy_stream);
            if (!e) e = hrt_hip_stream_sync(w->copy_stream2);
            if (e) { rc = hrt_fail(HRT_E_HIP, "hipStreamSynchronize failed (%d)", e); goto done; }
        } else if (H) {
            DL(w->ray, hb + (uint64_t)HRT_HIT_RAY * L.cap * 4, H * 4);
            DL(w->tri, hb + (uint64_t)HRT_HIT_TRI * L.cap * 4, H * 4);
            for (int k = 0; k < 4 && slim; ++k) DL(w->hs[k], hb + (uint64_t)hs_field[k] * L.cap * 4, H * 4);
        }
        /* Q10: the reference adds dot(d - d, mesh_velocity) * f/c -- a signed zero, or NaN for a
         * non-finite velocity -- to freq_shift[tx*np + path] of every ray that hit (:663-664),
         * in its loop order (bounce, tx, path), interleaved with the records' "-=" on the same
         * array.  The two can meet in one slot (the slot tx*np + path is the dense slot of rx 0,
         * TX (tx*np+path) / (nb*np), ...), and x + (+0) turns a -0 into +0, so the order is
         * replayed: the hit list is grouped by TX in ascending order (the launch set is, and the
         * compaction is stable), and per TX the adds go first, then that TX's records. */
        /* records of (b, rx): D2H into one of two page-locked staging sets on a copy stream,
         * so that the copy of block rx+1 runs while the host threads scatter block rx */
#define FETCH_RX(B, RX, SET_REC, SET_MASK, I0, I1)                                                   \
    do {                                                                                             \
        const uint64_t rb_ = L.off_recs + (uint64_t)(B) * L.rec_block_bytes + (uint64_t)(RX) * HRT_REC_FIELDS * L.cap * 4; \
        const uint64_t i0_ = (I0), n_ = (I1) - (I0), w0_ = (I0) / 64, w1_ = ((I1) + 63) / 64;         \
        int e_ = 0;                                                                                  \
        for (int k = 0; k < HRT_REC_FIELDS && !e_; ++k)                                              \
            if (!(slim && k >= HRT_REC_TAU && k <= HRT_REC_DIRZ))   /* formed on the host from the hits */ \
            e_ = hrt_hip_d2h_async((SET_REC)[k] + i0_, (const uint8_t *)w->d_ws + rb_ + ((uint64_t)k * L.cap + i0_) * 4, n_ * 4, \
                                   (k & 1) ? w->copy_stream2 : w->copy_stream);                      \
        if (!e_)                                                                                     \
            e_ = hrt_hip_d2h_async((SET_MASK) + w0_, (const uint8_t *)w->d_ws + L.off_masks + (((uint64_t)(B) * nrx + (RX)) * (L.cap / 64) + w0_) * 8, \
                                   (w1_ - w0_) * 8, w->copy_stream2);                                \
        if (e_) { rc = hrt_fail(HRT_E_HIP, "hipMemcpyAsync D2H failed (%d)", e_); goto done; }       \
    } while (0)
        /* runs of equal TX in the hit list (at most ntx) */
        uint64_t nruns = 0;
        if (H) {
            uint32_t cur = (uint32_t)(w->ray[0] / n_loc);
            w->run_start[0] = 0; w->run_tx[0] = cur; nruns = 1;
            for (;;) {   /* run boundaries by bisection on the (ascending) TX of the entries */
                uint64_t lo_i = w->run_start[nruns - 1], hi_i = H;
                const uint32_t t_cur = w->run_tx[nruns - 1];
                while (lo_i < hi_i) {   /* first entry with tx > t_cur */
                    const uint64_t mid = (lo_i + hi_i) / 2;
                    if ((uint32_t)(w->ray[mid] / n_loc) > t_cur) hi_i = mid; else lo_i = mid + 1;
                }
                if (lo_i >= H) break;
                if (nruns >= ntx) { rc = hrt_fail(HRT_E_HIP, "hit list is not grouped by TX"); goto done; }
                w->run_start[nruns] = lo_i;
                w->run_tx[nruns] = (uint32_t)(w->ray[lo_i] / n_loc);
                ++nruns;
            }
            w->run_start[nruns] = H;
        }
        /* The blocks of this bounce in the order they are scattered.  rx 0 goes run by run, each run behind its own
         * Q10 adds: the reference's order (tx, path, rx) on the only slots where two operations meet -- the adds touch
         * the dense slots [0, ntx*np), which are record slots of rx 0.  (A +-0 add and a subtraction commute bit for
         * bit, tests/test_scatter_order_model.py, so even there the order could not be seen; it is kept literal: it
         * costs ntx blocks per bounce, not ntx * nrx.)  Every record of rx >= 1 lives at
         * ((rx*ntx+tx)*nb+b)*np+p >= ntx*nb*np, beyond anything an add touches, and a record touches its own slot
         * only: rx >= 1 is scattered over the WHOLE hit list at once, nrx - 1 blocks instead of nruns * (nrx - 1)
         * (C5, 8 TX x 8 RX: 15 blocks per bounce instead of 64 -- a block costs ~0.1 ms of copies, syncs and
         * fork/join whatever its size).  The copy of block k+1 overlaps the scatter of block k; behind the last
         * block the next bounce's hit arrays are requested (and, with one TX, its first block: the runs of several
         * TXs are only known once the rays are here). */
        const uint64_t nblk = nruns ? nruns + (nrx - 1) : 0;
#define BLK_RX(K) ((K) < nruns ? (size_t)0 : (size_t)((K) - nruns + 1))
#define BLK_I0(K) ((K) < nruns ? w->run_start[(K)] : (uint64_t)0)
#define BLK_I1(K) ((K) < nruns ? w->run_start[(K) + 1] : H)
        for (uint64_t k = 0; k < nblk; ++k) {
            const size_t rx = BLK_RX(k);
            const uint64_t r0 = BLK_I0(k), r1 = BLK_I1(k);
            if (k < nruns) {   /* the adds of this run's TX, in front of its records */
                const size_t txr = w->run_tx[k];
                q10_ctx qc = {&s, w->ray, w->tri, prob->h_mesh, prob->h_tri_mesh, scat->freq_shift + txr * np,
                              prob->dop_mult, txr * n_loc, r0};
                hrt_parallel_ranges(q10_range, &qc, r1 - r0, c->scatter_threads);
            }
            if (k == 0 && !pre_block) {
                if (flip & 1) FETCH_RX(b, rx, w->rec2, w->mask2, r0, r1);
                else FETCH_RX(b, rx, w->rec, w->mask, r0, r1);
            }
            /* RaysInfo: the hits' new origins and directions, wanted behind the last block.  Requested behind block
             * 0's sync, so that they travel while block 0 is scattered and block 1's sync waits for them -- with a
             * single block in front of its sync */
#define FETCH_ST()                                                                                   \
    do {                                                                                             \
        int e_ = 0;                                                                                  \
        for (int q = 0; q < 6 && !e_; ++q)                                                           \
            e_ = hrt_hip_d2h_async(w->st[q], (const uint8_t *)w->d_ws + hb + (uint64_t)(HRT_HIT_OX + q) * L.cap * 4, H * 4, \
                                   (q & 1) ? w->copy_stream2 : w->copy_stream);                      \
        if (e_) { rc = hrt_fail(HRT_E_HIP, "hipMemcpyAsync D2H failed (%d)", e_); goto done; }       \
    } while (0)
            if (k == 0 && scat_rays && nblk == 1) FETCH_ST();
            const size_t slot = (size_t)k + (size_t)flip;
            float *const *cur_rec = (slot & 1) ? w->rec2 : w->rec;
            const uint64_t *cur_mask = (slot & 1) ? w->mask2 : w->mask;
            {
                int e = hrt_hip_stream_sync(w->copy_stream);   /* block k has landed */
                if (!e) e = hrt_hip_stream_sync(w->copy_stream2);
                if (e) { rc = hrt_fail(HRT_E_HIP, "hipStreamSynchronize failed (%d)", e); goto done; }
            }
            if (k == 0 && scat_rays && nblk > 1) FETCH_ST();
            if (k + 1 < nblk) {
                if (slot & 1) FETCH_RX(b, BLK_RX(k + 1), w->rec, w->mask, BLK_I0(k + 1), BLK_I1(k + 1));
                else FETCH_RX(b, BLK_RX(k + 1), w->rec2, w->mask2, BLK_I0(k + 1), BLK_I1(k + 1));
            } else if (can_pre && b + 1 < nb && w->h_counts[b + 2] != 0) {
                /* the last block of this bounce: the next bounce's rays, triangles and (one TX) first block */
                const uint64_t Hn = w->h_counts[b + 2], hbn = L.off_hits + (b + 1) * L.hit_block_bytes;
                int e = hrt_hip_d2h_async(w->ray2, (const uint8_t *)w->d_ws + hbn + (uint64_t)HRT_HIT_RAY * L.cap * 4, Hn * 4, w->copy_stream);
                if (!e) e = hrt_hip_d2h_async(w->tri2, (const uint8_t *)w->d_ws + hbn + (uint64_t)HRT_HIT_TRI * L.cap * 4, Hn * 4, w->copy_stream2);
                for (int q = 0; q < 4 && slim && !e; ++q)
                    e = hrt_hip_d2h_async(w->hs2[q], (const uint8_t *)w->d_ws + hbn + (uint64_t)hs_field[q] * L.cap * 4, Hn * 4,
                                          (q & 1) ? w->copy_stream2 : w->copy_stream);
                if (e) { rc = hrt_fail(HRT_E_HIP, "hipMemcpyAsync D2H failed (%d)", e); goto done; }
                pre = 1;
                if (ntx == 1) {
                    if (slot & 1) FETCH_RX(b + 1, 0, w->rec, w->mask, 0, Hn);
                    else FETCH_RX(b + 1, 0, w->rec2, w->mask2, 0, Hn);
                    pre_block_next = 1;
                    flip = (int)((slot + 1) & 1);   /* slot 0 of the next bounce is the set just requested */
                }
            }
            {
                scatter_ctx sc;
                memset(&sc, 0, sizeof sc);
                sc.s = &s; sc.ray = w->ray; sc.rec = cur_rec; sc.mask = cur_mask; sc.scat = scat;
                sc.n_loc = n_loc; sc.rx = rx; sc.b = b; sc.ntx = ntx; sc.nb = nb; sc.np = np;
                sc.amp_stride = c->amp_stride;
                sc.i_base = r0;
                if (slim) {
                    for (int q = 0; q < 4; ++q) sc.hs[q] = w->hs[q];
                    sc.rxp[0] = rx_pos[rx].x; sc.rxp[1] = rx_pos[rx].y; sc.rxp[2] = rx_pos[rx].z;
                }
                if (!prob->tune.no_scatter)   /* (HRT_TUNE no_scatter: timing experiments, copies only) */
                    hrt_parallel_ranges(scatter_range, &sc, r1 - r0, c->scatter_threads);
                for (int t = 0; t < HRT_MAX_SCATTER_THREADS; ++t) st->records_unblocked += sc.unblocked[t];
            }
        }
#undef BLK_RX
#undef BLK_I0
#undef BLK_I1
#undef FETCH_ST
#undef FETCH_RX

        /* ---- RaysInfo snapshots (:732-743), this batch's paths.  The state of a ray after bounce b goes
         * to slot (tx * nb + b + 1) * np + p whether it hit or not (Q14: dead rays keep their last state), so
         * a snapshot depends on that ray's history alone: every batch writes the slots of its own paths
         * (granule by granule), on whatever device it ran.  The active bits go into the shared per-bounce
         * bit strings; the reference's copies of them (Q12) are made once all batches are done. ---- */
        if (scat_rays) {
            const uint32_t ch = s.chunk ? s.chunk : 4096u;
            rays_ctx rcb;
            memset(&rcb, 0, sizeof rcb);
            rcb.s = &s; rcb.cur = w->cur_rays; rcb.ray = w->ray; rcb.st = w->st; rcb.n_loc = n_loc; rcb.np = np;
            rcb.ntx = ntx; rcb.ch = ch; rcb.n_gran = (n_loc + ch - 1) / ch;
            rcb.act = c->act_all + (b + 1) * (nq / 8 + 1);
            rcb.dst = scat_rays->rays + (b + 1) * np; rcb.dst_tx_stride = nb * np;   /* slot (tx * nb + b + 1) * np + p */
            /* (the st arrays were requested with the first block and every later block's sync waited for them; the
             * next bounce's arrays may be on their way behind them: not waited for here) */
            hrt_parallel_ranges(rays_update_range, &rcb, H, c->scatter_threads);
            hrt_parallel_ranges(rays_copy_range, &rcb, ntx * rcb.n_gran, c->scatter_threads);
        }
    }
    c->t_rb += hrt_now_s() - t0;
done:
    return rc;
}

static void *worker_main(void *arg)
{
    dev_ctx *c = (dev_ctx *)arg;
    int rc = HRT_OK;
    for (uint32_t g = (uint32_t)c->index; g < c->G && !rc; g += (uint32_t)c->count) rc = run_batch(c, g);
    c->rc = rc;
    if (rc) snprintf(c->err, sizeof c->err, "%s", hrt_last_error());
    return NULL;
}

static int compute_paths_impl(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos,
                              const Vec3 *rx_vel, const Vec3 *tx_vel, float f_ghz, size_t nrx,
                              size_t ntx, size_t np, size_t nb, ChannelInfo *los, RaysInfo *los_rays,
                              ChannelInfo *scat, RaysInfo *scat_rays, hrt_stats *stats, size_t amp_stride);

int hrt_compute_paths_ex(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos,
                         const Vec3 *rx_vel, const Vec3 *tx_vel, float f_ghz, size_t nrx,
                         size_t ntx, size_t np, size_t nb, ChannelInfo *los, RaysInfo *los_rays,
                         ChannelInfo *scat, RaysInfo *scat_rays, hrt_stats *stats)
{
    return compute_paths_impl(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, los, los_rays, scat,
                              scat_rays, stats, 1);
}

/* The same call for callers whose amplitudes are COMPLEX arrays (numpy complex64, C99 float
 * _Complex): a_te_re / a_te_im (a_tm_*) point at the real and the imaginary part of element 0,
 * element i lives at [2 i] of each -- the dense writer then fills the caller's complex arrays in
 * place instead of four planes that somebody has to interleave afterwards (the pybind module did:
 * 2 GB of extra passes on C3).  Everything else as hrt_compute_paths_ex. */
int hrt_compute_paths_interleaved(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos,
                                  const Vec3 *rx_vel, const Vec3 *tx_vel, float f_ghz, size_t nrx,
                                  size_t ntx, size_t np, size_t nb, ChannelInfo *los, RaysInfo *los_rays,
                                  ChannelInfo *scat, RaysInfo *scat_rays, hrt_stats *stats)
{
    return compute_paths_impl(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb, los, los_rays, scat,
                              scat_rays, stats, 2);
}

static int compute_paths_impl(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos,
                              const Vec3 *rx_vel, const Vec3 *tx_vel, float f_ghz, size_t nrx,
                              size_t ntx, size_t np, size_t nb, ChannelInfo *los, RaysInfo *los_rays,
                              ChannelInfo *scat, RaysInfo *scat_rays, hrt_stats *stats, size_t amp_stride)
{
    const double t_begin = hrt_now_s();
    if (!scene || !los || !scat) return hrt_fail(HRT_E_INVALID, "compute_paths: NULL argument");
    if (np == 0 || nb == 0) return hrt_fail(HRT_E_INVALID, "num_rays and num_bounces must be > 0");
    if (nb > 65535) return hrt_fail(HRT_E_INVALID, "num_bounces > 65535 is not supported");

    hrt_stats st;
    memset(&st, 0, sizeof st);
    int devs[HRT_MAX_DEVICES];
    int D = parse_devices(devs);
    dev_ctx *ctx = (dev_ctx *)calloc((size_t)D, sizeof(dev_ctx));
    if (!ctx) return hrt_fail(HRT_E_NOMEM, "out of host memory");
    const int D_created = D;   /* a problem is made for each of these, however many end up with work */
    st.device = devs[0];
    const size_t nq = ntx * np;
    int rc = HRT_OK;
    int pool_taken = 0;
    double t0;

    for (int d = 0; d < D; ++d) {
        dev_ctx *c = &ctx[d];
        c->scene = scene; c->rx_pos = rx_pos; c->tx_pos = tx_pos; c->rx_vel = rx_vel; c->tx_vel = tx_vel;
        c->f_ghz = f_ghz; c->nrx = nrx; c->ntx = ntx; c->np = np; c->nb = nb; c->nq = nq;
        c->los = los; c->scat = scat; c->los_rays = los_rays; c->scat_rays = scat_rays;
        c->amp_stride = amp_stride;
        c->index = d; c->count = D; c->device = devs[d];
        c->host_launch = hrt_env_int("HRT_HOST_LAUNCH", 0);
        int thr = hrt_host_threads() / D;
        c->scatter_threads = thr > 0 ? thr : 1;
    }
    /* one problem per device (the scene is tiny; every device holds all of it) */
    for (int d = 0; d < D && !rc; ++d)
        rc = hrt_problem_create_for(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, ctx[d].device,
                                    (uint64_t)ntx * np / (uint64_t)D, &ctx[d].prob);
    if (rc) goto done;
    hrt_problem *prob = ctx[0].prob;

    /* normals: the reference leaves them in the scene for the caller (:208-224) */
    {
        uint32_t j = 0;
        for (uint32_t i = 0; i < scene->num_meshes; ++i) {
            Mesh *m = &scene->meshes[i];
            /* like the reference (:212) the old pointer is overwritten, NOT freed: a caller that
             * built the Mesh by hand may have left `ns` uninitialised or pointing at memory that is
             * not malloc'ed, which is legal against the reference ABI */
            m->ns = (Vec3 *)malloc((size_t)(m->num_triangles ? m->num_triangles : 1) * sizeof(Vec3));
            if (!m->ns) { rc = hrt_fail(HRT_E_NOMEM, "out of host memory"); goto done; }
            for (uint32_t f = 0; f < m->num_triangles; ++f, ++j)
                memcpy(&m->ns[f], prob->h_tri + (size_t)prob->accel.newidx[j] * HRT_TRI_FLOATS + 9, sizeof(Vec3));
        }
    }
    st.t_setup_s = hrt_now_s() - t_begin;

    /* ---- batches: how many round-robin shards so one workspace fits the budget (batch.c), a multiple of the
     * device count, at most one per granule ---- */
    uint32_t G = 1;
    {
        int same = 0;   /* logical devices on one GPU share its memory */
        for (int d = 0; d < D; ++d) same += ctx[d].device == ctx[0].device;
        if ((rc = hrt_plan_batches(prob, np, nb, D, same, 12, &G))) goto done;
        if (G > 1 && G % (uint32_t)D) G = (G / (uint32_t)D + 1) * (uint32_t)D;
        if ((uint64_t)G * 4096 > np + 4095) {   /* fewer granules than batches: fewer workers */
            G = (uint32_t)((np + 4095) / 4096);
            if (G < 1) G = 1;
        }
        if ((uint32_t)D > G) D = (int)G;
    }
    for (int d = 0; d < D; ++d) { ctx[d].G = G; ctx[d].count = D; }

    /* ---- buffers (pooled between calls) ---- */
    pool_taken = hrt_pool_begin();
    for (int d = 0; d < D && !rc; ++d) {
        ctx[d].use_pool = pool_taken;
        rc = hrt_worker_alloc(&ctx[d]);
    }
    if (rc) goto done;

    /* ---- launch tables + the dense pre-fills that do not depend on the trace.  Default: tables
     * generated ON THE DEVICE (directions bit-identical to the host libm's, hrt_launch_dirs_device;
     * coherent order by hrt_launch_order_device).  HRT_HOST_LAUNCH=1: the host generators + the
     * launch-table cache. ---- */
    {
        work_t *w = &ctx[0].w;
        const int host_launch = ctx[0].host_launch;
        t0 = hrt_now_s();
        hrt_shard whole = {np, 0, 1, 0, (uint32_t)nb};
        if (host_launch) {
            w->h_dirs = (float *)malloc(np * 3 * sizeof(float));
            if (!w->h_dirs) { rc = hrt_fail(HRT_E_NOMEM, "out of host memory"); goto done; }
            if (!(hrt_launch_cache_enabled(np) && hrt_launch_cache_get(np, w->h_dirs, NULL))) {
                rc = hrt_launch_dirs_host(&whole, w->h_dirs, hrt_env_int("HRT_HOST_THREADS", 0));
                if (rc) goto done;
                hrt_launch_cache_put(np, w->h_dirs, NULL);
            }
            /* Q9, literally: launch term at [tx*np*nb + p] (the memcpy replications follow below) */
            for (size_t tx = 0; tx < ntx; ++tx)
                for (size_t p = 0; p < np; ++p) {
                    const float *d = w->h_dirs + 3 * p;
                    float v = tx_vel[tx].x * d[0] + tx_vel[tx].y * d[1] + tx_vel[tx].z * d[2];
                    scat->freq_shift[tx * np * nb + p] = v * prob->dop_mult;
                }
            for (int d = 1; d < D; ++d) ctx[d].w.h_dirs = w->h_dirs;   /* shared, read-only; freed by worker 0 */
        } else {
            /* the launch Doppler term of every path (Q9) from directions generated on the device, in
             * pieces that fit the direction buffer: a "shard" with one granule per rank is a contiguous
             * range of the sphere.  With one batch the single piece is the whole launch set and its
             * directions stay in d_dirs for the trace. */
            const uint64_t n_buf = hrt_shard_num_local(&(hrt_shard){np, 0, G, 0, (uint32_t)nb});
            uint32_t pieces = (uint32_t)((np + n_buf - 1) / n_buf);
            uint64_t piece = ((np + pieces - 1) / pieces + 63) / 64 * 64;
            if (G == 1) { pieces = 1; piece = 0; }
            for (uint32_t k = 0; k < pieces; ++k) {
                hrt_shard ps = {np, k, pieces, (uint32_t)piece, (uint32_t)nb};
                const uint64_t n_p = hrt_shard_num_local(&ps);
                if (n_p == 0) continue;
                const uint64_t a = hrt_shard_global_path(&ps, 0);
                if ((rc = hrt_launch_dirs_device(&ps, (float *)w->d_dirs, w->device, NULL, NULL))) goto done;
                for (size_t tx = 0; tx < ntx; ++tx) {
                    const float tv[3] = {tx_vel[tx].x, tx_vel[tx].y, tx_vel[tx].z};
                    int e = hrt_hip_launch_fs0((const float *)w->d_dirs, n_p, tv, prob->dop_mult, (float *)w->d_ws, NULL);
                    if (e) { rc = hrt_fail_hip(e, "hrt_fs0_kernel"); goto done; }
                    if ((rc = hrt_device_download(w->device, scat->freq_shift + tx * np * nb + a, w->d_ws, n_p * 4))) goto done;
                }
            }
        }
        st.t_launch_dirs_s = hrt_now_s() - t0;
        /* Q9: the two memcpy replications of the launch term (source and destinations never overlap:
         * each is cut into ranges for the helper threads -- 240 MB on C3, 7 ms on one thread) */
        {
            const int thr = hrt_host_threads();
            for (size_t b = 1; b < nb; ++b) {
                copy_ctx cc = {scat->freq_shift + nq * b, scat->freq_shift};
                hrt_parallel_ranges(copy_range, &cc, nq, thr);
            }
            for (size_t rx = 1; rx < nrx; ++rx) {
                copy_ctx cc = {scat->freq_shift + nq * nb * rx, scat->freq_shift};
                hrt_parallel_ranges(copy_range, &cc, nq * nb, thr);
            }
        }

        if (scat_rays) {
            /* :469-471: all rays active before bounce 0; the bit strings after bounce 0 .. nb-1 start empty
             * (the bits beyond nq in the last byte are never cleared by the reference: they stay set) */
            const size_t nbq = nq / 8 + 1;
            uint8_t *act = (uint8_t *)calloc(nb + 1, nbq);
            if (!act) { rc = hrt_fail(HRT_E_NOMEM, "out of host memory"); goto done; }
            memset(act, 0xff, nbq);
            for (size_t b = 1; b <= nb; ++b)
                for (size_t q = nq; q < 8 * nbq; ++q) act[b * nbq + q / 8] |= (uint8_t)(1u << (q % 8));
            for (int d = 0; d < D; ++d) ctx[d].act_all = act;
        }
    }

    /* ---- the batches: one host thread per device ---- */
    {
        pthread_t th[HRT_MAX_DEVICES];
        int started[HRT_MAX_DEVICES] = {0};
        for (int d = 1; d < D; ++d) started[d] = pthread_create(&th[d], NULL, worker_main, &ctx[d]) == 0;
        worker_main(&ctx[0]);
        for (int d = 1; d < D; ++d) {
            if (started[d]) pthread_join(th[d], NULL);
            else worker_main(&ctx[d]);   /* a thread that would not start: run its batches here */
        }
        for (int d = 0; d < D; ++d) {
            if (ctx[d].rc && !rc) rc = hrt_fail(ctx[d].rc, "device %d: %s", ctx[d].device, ctx[d].err);
            for (size_t b = 0; b <= nb && b < 34; ++b) st.live[b] += ctx[d].st.live[b];
            st.records += ctx[d].st.records;
            st.records_unblocked += ctx[d].st.records_unblocked;
            st.tests += ctx[d].st.tests;
            /* phases: the slowest device */
            if (ctx[d].t_dev > st.t_device_s) st.t_device_s = ctx[d].t_dev;
            if (ctx[d].t_rb > st.t_readback_s) st.t_readback_s = ctx[d].t_rb;
            if (d < 16) {
                st.dev_id[d] = ctx[d].device;
                st.dev_batches[d] = (G - (uint32_t)d + (uint32_t)D - 1u) / (uint32_t)D;   /* batches d, d + D, ... */
                st.dev_t_device_s[d] = ctx[d].t_dev;
                st.dev_t_readback_s[d] = ctx[d].t_rb;
            }
            st.t_launch_dirs_s += ctx[d].t_launch / D;
        }
    }
    st.num_devices = D;
    st.num_batches = G;
    if (scat_rays && !rc) {
        /* :469-471, then per bounce and TX the reference's copy of its bit string FROM BYTE 0 (Q12: np / 8 + 1
         * bytes -- TX 0's bits and the first few of TX 1, which at the time of TX 0's copy are still the
         * previous bounce's), at stride nb */
        const size_t nbq = nq / 8 + 1, nbytes = np / 8 + 1;
        const uint8_t *act = ctx[0].act_all;
        memcpy(scat_rays->rays_active, act, nbq);
        for (size_t b = 0; b < nb; ++b)
            for (size_t tx = 0; tx < ntx; ++tx) {
                uint8_t *dst = scat_rays->rays_active + (tx * nb + (b + 1)) * nbytes;
                const uint8_t *cur = act + (b + 1) * nbq, *prev = act + b * nbq;
                memcpy(dst, cur, nbytes);
                if (tx == 0 && ntx > 1)
                    for (size_t bitp = np; bitp < 8 * nbytes; ++bitp) {
                        const uint8_t m = (uint8_t)(1u << (bitp % 8));
                        dst[bitp / 8] = (uint8_t)((dst[bitp / 8] & ~m) | (prev[bitp / 8] & m));
                    }
            }
    }

done:
    for (int d = 0; d < D; ++d) {
        if (d > 0 && ctx[d].w.h_dirs == ctx[0].w.h_dirs) ctx[d].w.h_dirs = NULL;   /* shared table */
        if (ctx[d].rc == HRT_OK && rc) ctx[d].rc = rc;
    }
    for (int d = D - 1; d >= 0; --d)
        if (ctx[d].w.d_ws || ctx[d].w.ray) hrt_worker_release(&ctx[d]);
    /* (every problem that was created: a launch set of fewer 4096-path granules than devices leaves
     * some devices without work, but their problems exist) */
    for (int d = (D_created > D ? D_created : D) - 1; d >= 0; --d) hrt_problem_destroy(ctx[d].prob);
    hrt_pool_end(pool_taken);
    free(ctx[0].act_all);
    free(ctx);
    st.t_total_s = hrt_now_s() - t_begin;
    if (!rc && stats) *stats = st;
    return rc;
}

void compute_paths(Scene *scene, Vec3 *rx_pos, Vec3 *tx_pos, Vec3 *rx_vel, Vec3 *tx_vel,
                   float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb,
                   ChannelInfo *los, RaysInfo *los_rays, ChannelInfo *scat, RaysInfo *scat_rays)
{
    int rc = hrt_compute_paths_ex(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, np, nb,
                                  los, los_rays, scat, scat_rays, NULL);
    if (rc != HRT_OK) {
        fprintf(stderr, "hermespy-rt_amd: compute_paths failed (%d): %s\n", rc, hrt_last_error());
        exit(70);
    }
}
