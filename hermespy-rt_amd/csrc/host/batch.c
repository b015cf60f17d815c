/* batch.c -- the batch loop the drop-in host entries share: hrt_compute_paths_ex (compute_paths.c),
 * hrt_compute_paths_list (path_list.c), hrt_compute_channel / hrt_compute_array_channel (channel.c).
 *
 * Each entry traces its launch set in batches (round-robin shards of the path index, hrt_device.h) sized to a
 * device-memory budget.  Here: the environment readers, the budget and batch search (hrt_plan_batches), one
 * batch's trace with the void-step retry and its statistics (hrt_trace_batch), the worker buffers pooled between
 * calls, and the setup of the single-device entries (hrt_solo_begin / hrt_solo_end).  What an entry does with a
 * finished trace is its own.
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "hrt_internal.h"

int hrt_env_int(const char *name, int dflt)
{
    const char *v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

uint64_t hrt_env_u64(const char *name, uint64_t dflt)
{
    const char *v = getenv(name);
    return (v && *v) ? strtoull(v, NULL, 10) : dflt;
}

/* ---- buffers kept between calls -------------------------------------------------------------
 * Device workspace and page-locked staging of the last call, one slot per worker, reused when the
 * next call fits (same device, capacity >= needed): a warm call saves ~25 ms of hipMalloc /
 * hipHostMalloc / hipFree on C3.  Released by hrt_cache_clear(); HRT_NO_CACHE=1 disables;
 * slots holding more than HRT_POOL_MAX_BYTES (default 5 GiB device + pinned: a warm C3 call holds 4.0 GB; a
 * reference-API caller never calls hrt_cache_clear(), so the default stays near what the headline configuration
 * needs.  C4 holds 14 GB -- its warm call is 0.04 s with them kept, 0.24 s without: such a caller raises it) are
 * not kept. */
static void work_free(work_t *w)
{
    if (w->copy_stream) {   /* no copy may be in flight into the staging buffers freed below */
        hrt_hip_stream_sync(w->copy_stream);
        hrt_hip_stream_destroy(w->copy_stream);
    }
    if (w->copy_stream2) {
        hrt_hip_stream_sync(w->copy_stream2);
        hrt_hip_stream_destroy(w->copy_stream2);
    }
    if (w->d_dirs) hrt_device_free(w->device, w->d_dirs);
    if (w->d_order) hrt_device_free(w->device, w->d_order);
    free(w->h_order);
    if (w->d_ws) hrt_device_free(w->device, w->d_ws);
    free(w->h_dirs); free(w->h_counts); free(w->h_los);
    /* D2H staging is page-locked (hipHostMalloc): 2-4x the pageable copy rate */
    hrt_hip_host_free(w->ray); hrt_hip_host_free(w->tri); hrt_hip_host_free(w->fs0);
    hrt_hip_host_free(w->ray2); hrt_hip_host_free(w->tri2); hrt_hip_host_free(w->fs02);
    for (int k = 0; k < 6; ++k) hrt_hip_host_free(w->st[k]);
    for (int k = 0; k < 4; ++k) { hrt_hip_host_free(w->hs[k]); hrt_hip_host_free(w->hs2[k]); }
    for (int k = 0; k < HRT_REC_FIELDS; ++k) hrt_hip_host_free(w->rec[k]);
    hrt_hip_host_free(w->mask);
    for (int k = 0; k < HRT_REC_FIELDS; ++k) hrt_hip_host_free(w->rec2[k]);
    hrt_hip_host_free(w->mask2);
    free(w->run_start); free(w->run_tx);
    free(w->dirs_batch); free(w->cur_rays);
}

typedef struct {
    int valid, device, with_rays, slim;
    uint64_t cap, ws_bytes, dirs_rows;
    work_t w;
} pool_slot;
static pthread_mutex_t g_pool_lock = PTHREAD_MUTEX_INITIALIZER;
static pool_slot g_pool[HRT_MAX_DEVICES];
static int g_pool_busy;

void hrt_pool_release_all(void)
{
    pthread_mutex_lock(&g_pool_lock);
    if (!g_pool_busy)
        for (int k = 0; k < HRT_MAX_DEVICES; ++k)
            if (g_pool[k].valid) { work_free(&g_pool[k].w); memset(&g_pool[k], 0, sizeof g_pool[k]); }
    pthread_mutex_unlock(&g_pool_lock);
}

/* device + page-locked bytes a worker holds for batches of `cap` entries (workspace, launch tables, staging) */
uint64_t hrt_worker_held_bytes(uint64_t ws_bytes, uint64_t dirs_rows, uint64_t cap)
{
    return ws_bytes + dirs_rows * 16 + cap * 4 * (5 + 2 * HRT_REC_FIELDS + 6 + 8);
}
/* may a batch of this size be chosen by default?  (the pool is on and the caller did not set the budget: then what
 * a worker holds must fit the pool, or every call allocates it again) */
int hrt_batch_fits_pool(uint64_t ws_bytes, uint64_t dirs_rows, uint64_t cap)
{
    if (hrt_env_u64("HRT_WORKSPACE_BYTES", 0) || hrt_env_int("HRT_NO_CACHE", 0)) return 1;
    return hrt_worker_held_bytes(ws_bytes, dirs_rows, cap) <= hrt_env_u64("HRT_POOL_MAX_BYTES", HRT_POOL_MAX_DEFAULT);
}

/* one call at a time owns the pool (compute_paths is not re-entrant; a concurrent call just
 * allocates its own buffers) */
int hrt_pool_begin(void)
{
    int taken = 0;
    if (hrt_env_int("HRT_NO_CACHE", 0)) return 0;
    pthread_mutex_lock(&g_pool_lock);
    if (!g_pool_busy) { g_pool_busy = 1; taken = 1; }
    pthread_mutex_unlock(&g_pool_lock);
    return taken;
}
void hrt_pool_end(int taken)
{
    if (!taken) return;
    pthread_mutex_lock(&g_pool_lock);
    g_pool_busy = 0;
    pthread_mutex_unlock(&g_pool_lock);
}

/* buffers of one worker, sized for its largest batch (from the pool when they fit) */
int hrt_worker_alloc(dev_ctx *c)
{
    work_t *w = &c->w;
    const size_t nb = c->nb, nrx = c->nrx, ntx = c->ntx, np = c->np;
    hrt_layout L;
    hrt_shard s0 = {np, (uint32_t)c->index, c->G, 0, (uint32_t)nb};
    int rc = hrt_layout_query(c->prob, &s0, &L);   /* a worker's first batch is never smaller than its others */
    if (rc) return rc;
    const uint64_t n_loc_max = hrt_shard_num_local(&(hrt_shard){np, 0, c->G, 0, (uint32_t)nb});
    const uint64_t cap = L.cap;
    const int with_rays = c->scat_rays != NULL;
    const int slim = !hrt_env_int("HRT_FULL_RECORDS", 0);   /* (the per-hit staging arrays hs / hs2 exist only then) */
    if (c->use_pool) {
        pool_slot *ps = &g_pool[c->index];
        if (ps->valid && ps->device == c->device && ps->cap >= cap && ps->ws_bytes >= L.total_bytes &&
            ps->dirs_rows >= n_loc_max + 64 && ps->with_rays >= with_rays && ps->slim >= slim) {
            *w = ps->w;
            c->cap_alloc = ps->cap; c->ws_alloc = ps->ws_bytes; c->dirs_rows_alloc = ps->dirs_rows;
            memset(ps, 0, sizeof *ps);
            w->device = c->device;
            /* per-call host arrays are not pooled; the small ones sized by nrx / ntx are re-made */
            w->h_dirs = NULL; w->cur_rays = NULL; w->dirs_batch = NULL;
            free(w->h_los); free(w->run_start); free(w->run_tx); free(w->h_counts);
            w->h_counts = (uint32_t *)calloc(nb + 4, 4);
            w->h_los = (float *)malloc(nrx * ntx * HRT_LOS_FLOATS * sizeof(float));
            w->run_start = (uint64_t *)malloc((ntx + 2) * sizeof(uint64_t));
            w->run_tx = (uint32_t *)malloc((ntx + 1) * sizeof(uint32_t));
            if (!w->h_los || !w->run_start || !w->run_tx || !w->h_counts) return hrt_fail(HRT_E_NOMEM, "out of host memory");
            return HRT_OK;
        }
        if (ps->valid) { work_free(&ps->w); memset(ps, 0, sizeof *ps); }
    }
    memset(w, 0, sizeof *w);
    w->device = c->device;
    if ((rc = hrt_device_malloc(w->device, &w->d_ws, L.total_bytes))) return rc;
    if ((rc = hrt_device_malloc(w->device, &w->d_dirs, (n_loc_max + 64) * 12))) return rc;   /* + rounding of a prefill piece */
    if ((rc = hrt_device_malloc(w->device, &w->d_order, (n_loc_max + 64) * 4))) return rc;
    w->h_order = (uint32_t *)malloc((n_loc_max + 64) * 4);
    w->h_counts = (uint32_t *)calloc(c->nb + 4, 4);
    w->h_los = (float *)malloc(nrx * ntx * HRT_LOS_FLOATS * sizeof(float));
    w->run_start = (uint64_t *)malloc((ntx + 2) * sizeof(uint64_t));
    w->run_tx = (uint32_t *)malloc((ntx + 1) * sizeof(uint32_t));
    int ok = w->h_order && w->h_counts && w->h_los && w->run_start && w->run_tx;
    ok &= hrt_hip_host_malloc((void **)&w->ray, cap * 4) == 0;
    ok &= hrt_hip_host_malloc((void **)&w->tri, cap * 4) == 0;
    ok &= hrt_hip_host_malloc((void **)&w->ray2, cap * 4) == 0;
    ok &= hrt_hip_host_malloc((void **)&w->tri2, cap * 4) == 0;
    ok &= hrt_hip_host_malloc((void **)&w->fs02, cap * 4) == 0;
    ok &= hrt_hip_host_malloc((void **)&w->fs0, cap * 4) == 0;
    ok &= hrt_hip_host_malloc((void **)&w->mask, cap / 64 * 8 + 8) == 0;
    for (int k = 0; k < 6 && with_rays; ++k) ok &= hrt_hip_host_malloc((void **)&w->st[k], cap * 4) == 0;
    for (int k = 0; k < 4 && slim; ++k) {
        ok &= hrt_hip_host_malloc((void **)&w->hs[k], cap * 4) == 0;
        ok &= hrt_hip_host_malloc((void **)&w->hs2[k], cap * 4) == 0;
    }
    for (int k = 0; k < HRT_REC_FIELDS; ++k) ok &= hrt_hip_host_malloc((void **)&w->rec[k], cap * 4) == 0;
    for (int k = 0; k < HRT_REC_FIELDS; ++k) ok &= hrt_hip_host_malloc((void **)&w->rec2[k], cap * 4) == 0;
    ok &= hrt_hip_host_malloc((void **)&w->mask2, cap / 64 * 8 + 8) == 0;
    ok &= hrt_hip_stream_create(&w->copy_stream) == 0;
    ok &= hrt_hip_stream_create(&w->copy_stream2) == 0;
    if (!ok) return hrt_fail(HRT_E_NOMEM, "out of host memory (page-locked staging)");
    c->cap_alloc = cap; c->ws_alloc = L.total_bytes; c->dirs_rows_alloc = n_loc_max + 64;
    return HRT_OK;
}

/* give the buffers back (pool) or free them */
void hrt_worker_release(dev_ctx *c)
{
    work_t *w = &c->w;
    free(w->h_dirs); w->h_dirs = NULL;
    free(w->cur_rays); w->cur_rays = NULL;
    free(w->dirs_batch); w->dirs_batch = NULL;
    const uint64_t held = hrt_worker_held_bytes(c->ws_alloc, c->dirs_rows_alloc, c->cap_alloc);
    if (c->use_pool && c->rc == HRT_OK && w->d_ws && held <= hrt_env_u64("HRT_POOL_MAX_BYTES", HRT_POOL_MAX_DEFAULT)) {
        if (w->copy_stream) hrt_hip_stream_sync(w->copy_stream);
        if (w->copy_stream2) hrt_hip_stream_sync(w->copy_stream2);
        pool_slot *ps = &g_pool[c->index];
        ps->valid = 1; ps->device = c->device; ps->with_rays = w->st[0] != NULL; ps->slim = w->hs[0] != NULL;
        ps->cap = c->cap_alloc; ps->ws_bytes = c->ws_alloc; ps->dirs_rows = c->dirs_rows_alloc;
        ps->w = *w;
        memset(w, 0, sizeof *w);
        return;
    }
    work_free(w);
    memset(w, 0, sizeof *w);
}

/* ---- the batch count ----
 * The first power of two G such that one batch's workspace plus its launch tables fits the budget, with at least
 * `devices` batches: HRT_WORKSPACE_BYTES, or min(free / 2, 16 GiB) of the problem's device shared by `sharers`
 * logical devices.  Unless the caller set the budget, also so that what a worker holds fits the buffer pool
 * (hrt_worker_release): buffers above HRT_POOL_MAX_BYTES are freed after the call and allocated again by the next
 * one -- C4's 14 GB in one batch: a warm call of 0.31 s, 0.17 of them hipMalloc / hipHostMalloc / hipFree; in four
 * batches 0.04 s (the batches' copies and host scatter overlap the next batch's kernels anyway). */
int hrt_plan_batches(const hrt_problem *prob, size_t np, size_t nb, int devices, int sharers,
                     uint64_t bytes_per_local_ray, uint32_t *G_out)
{
    uint64_t free_b = 0, total_b = 0;
    int rc = hrt_device_mem_info(prob->device, &free_b, &total_b);
    if (rc) return rc;
    uint64_t budget = hrt_env_u64("HRT_WORKSPACE_BYTES", 0);
    if (!budget) {
        budget = free_b / 2;
        if (budget > (16ull << 30)) budget = 16ull << 30;
        budget /= (uint64_t)(sharers > 0 ? sharers : 1);   /* logical devices on one GPU share its memory */
    }
    hrt_layout L;
    uint32_t G = 1, G_budget = 0;   /* G_budget: the first G that fits the memory budget */
    for (;;) {
        hrt_shard s = {np, 0, G, 0, (uint32_t)nb};
        rc = hrt_layout_query(prob, &s, &L);
        const uint64_t n_loc = hrt_shard_num_local(&s);
        const int fits = rc == HRT_OK && G >= (uint32_t)devices && L.total_bytes + n_loc * bytes_per_local_ray <= budget;
        if (fits && !G_budget) G_budget = G;
        /* (the pool rule only where it pays: a call of one or two budget-sized batches per device.  A call of
         * many batches amortises its allocations -- C5: 0.2 of 3.7 s -- and smaller batches cost it more than
         * that: 64 instead of 16 took 7.7 s) */
        if (fits && (G_budget > 2u * (uint32_t)devices || hrt_batch_fits_pool(L.total_bytes, n_loc + 64, L.cap))) break;
        if (rc != HRT_OK && rc != HRT_E_CAPACITY) return rc;
        if ((uint64_t)G * 4096 >= np) {   /* one granule per batch and still too big */
            if (rc == HRT_OK) break;      /* try anyway; hipMalloc decides */
            return rc;
        }
        G *= 2;
    }
    *G_out = G;
    return HRT_OK;
}

/* ---- one batch's trace ----
 * Trace shard s into the worker's workspace (launch tables in w->d_dirs / w->d_order), wait for it and read the
 * counts into w->h_counts; add the batch's work to *st (the LoS tests, the same in every batch, are counted by
 * rank 0 only).  A fused launch / the chain kernel that gave up waiting (the GPU is shared with other such
 * kernels: hrt_kernels.hip, lb_exclusive, hrt_chain_kernel) makes the step void: it is traced once more with that
 * switched off (chain -> a kernel per launch -> two kernels per launch), and so from now on. */
int hrt_trace_batch(const hrt_problem *prob, const hrt_shard *s, const hrt_layout *L, work_t *w, hrt_stats *st)
{
    const size_t nb = s->num_bounces;
    int rc;
    for (int attempt = 0;; ++attempt) {
        if ((rc = hrt_trace(prob, s, (const float *)w->d_dirs, (const uint32_t *)w->d_order, w->d_ws, L->total_bytes,
                            NULL, NULL))) return rc;
        if ((rc = hrt_device_sync(w->device, NULL))) return rc;
        if ((rc = hrt_device_download(w->device, w->h_counts, (const uint8_t *)w->d_ws + L->off_counts, (nb + 2) * 4)))
            return rc;
        if (!(w->h_counts[nb + 1] & HRT_ERR_VOID) || attempt >= 2 || !hrt_void_step_retry(w->h_counts[nb + 1])) break;
    }
    if (w->h_counts[nb + 1] != 0)
        return hrt_fail(HRT_E_HIP, "device reported internal error flags %u", w->h_counts[nb + 1]);
    hrt_stats bs;
    hrt_work_from_counts(prob, s, w->h_counts, &bs);
    for (size_t b = 0; b <= nb && b < 34; ++b) st->live[b] += bs.live[b];
    st->records += bs.records;
    st->tests += bs.tests - (s->rank ? (uint64_t)prob->num_rx * prob->num_tx * prob->num_tri : 0);
    return HRT_OK;
}

/* ---- the single-device entries (path_list.c, channel.c) ----
 * HRT_DEVICE (default 0), its problem, the batch count (16 bytes of launch tables per local ray) and the one
 * worker's buffers.  hrt_solo_end releases whatever was made, also after a failed hrt_solo_begin. */
int hrt_solo_begin(hrt_solo *so, Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                   const Vec3 *tx_vel, float f_ghz, size_t nrx, size_t ntx, size_t np, size_t nb, hrt_stats *st,
                   double t_begin)
{
    memset(so, 0, sizeof *so);
    const int device = hrt_env_int("HRT_DEVICE", 0);
    st->device = device;
    int rc = hrt_problem_create_for(scene, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, nrx, ntx, device,
                                    (uint64_t)ntx * np, &so->prob);
    if (rc) return rc;
    st->t_setup_s = hrt_now_s() - t_begin;
    dev_ctx *c = &so->wc;
    if ((rc = hrt_plan_batches(so->prob, np, nb, 1, 1, 16, &c->G))) return rc;
    c->prob = so->prob; c->nrx = nrx; c->ntx = ntx; c->np = np; c->nb = nb; c->index = 0; c->count = 1;
    c->device = device;
    so->pool_taken = hrt_pool_begin();
    c->use_pool = so->pool_taken;
    return hrt_worker_alloc(c);
}

void hrt_solo_end(hrt_solo *so, int rc)
{
    if (so->wc.w.d_ws || so->wc.w.ray) {
        so->wc.rc = rc;
        hrt_worker_release(&so->wc);
    }
    hrt_pool_end(so->pool_taken);
    hrt_problem_destroy(so->prob);
    so->prob = NULL;
}
