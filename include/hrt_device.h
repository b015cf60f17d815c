/* hrt_device.h -- device-resident form of the compute_paths hot path (C ABI).
 *
 * compute_paths() (hermespy_rt.h) takes and returns HOST arrays in the reference's dense
 * layout.  The functions here are the same path with everything resident in HBM and the
 * result in COMPACT form -- what a multi-GPU caller (one process per GPU, ray-sharded) and
 * bench.py drive.  compute_paths() itself is built on them.
 *
 * The caller owns the big buffers (launch directions, workspace): they are plain device
 * pointers, e.g. torch tensors' data_ptr(), and `stream` is a hipStream_t passed as void*
 * (NULL = the default stream).  No torch or HIP types appear in any signature.
 *
 * Reference lines each piece replaces (relative to the reference repository):
 *   hrt_problem_create   src/compute_paths.c:437-438 (precompute_materials/_normals, :171-224)
 *                        + the scene/endpoint arguments of compute_paths (:419-429)
 *   hrt_launch_dirs_host src/compute_paths.c:443-451 (Fibonacci sphere, double libm)
 *   hrt_trace            src/compute_paths.c:460-472 (state init), :515-577 (LoS),
 *                        :591-729 (bounce loop: moeller_trumbore :237-287, refl_coefs
 *                        :300-344, scat_coefs :359-415)
 */
#ifndef HRT_DEVICE_H
#define HRT_DEVICE_H

#include "hermespy_rt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Everything small and read-only, uploaded once: flattened triangle table (v1, e1, e2, unit
 * normal, mesh id; (mesh, face) order), per-mesh material/velocity, the eta table for the
 * carrier frequency, RX/TX positions and velocities. */
typedef struct hrt_problem hrt_problem;

int hrt_problem_create(const Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos,
                       const Vec3 *rx_vel, const Vec3 *tx_vel, float carrier_frequency_GHz,
                       size_t num_rx, size_t num_tx, int device, hrt_problem **out);
void hrt_problem_destroy(hrt_problem *p);
/* Fused launches and the chain kernel wait for each other's workgroups; when a wait runs out (the GPU is shared
 * with other such kernels) the step is void (HRT_ERR_FUSE_TIMEOUT / HRT_ERR_CHAIN_TIMEOUT in counts[nb + 1]), the
 * library switches that kernel off for the rest of the process and callers trace again (the drop-in calls do so
 * themselves).  hrt_fallback_state: bit 0 = fused launches are off, bit 1 = the chain kernel is off. */
int hrt_fallback_state(void);
#ifndef HRT_ERR_FUSE_TIMEOUT   /* (the same values in csrc/hrt_kparams.h, for the kernels) */
#define HRT_ERR_FUSE_TIMEOUT 0x100u
#define HRT_ERR_CHAIN_TIMEOUT 0x200u
#define HRT_ERR_VOID (HRT_ERR_FUSE_TIMEOUT | HRT_ERR_CHAIN_TIMEOUT)
#endif
uint32_t hrt_problem_num_triangles(const hrt_problem *p);
uint32_t hrt_problem_num_rx(const hrt_problem *p);
uint32_t hrt_problem_num_tx(const hrt_problem *p);
int hrt_problem_device(const hrt_problem *p);

/* Host copies of what was uploaded (for tests): eta table [17][12] in the reference's
 * MaterialPrecomputed field order (src/compute_paths.c:125-132); normals [T][3]; for row j of
 * the device table its (mesh, face) pair. */
int hrt_problem_eta_table(const hrt_problem *p, float *out17x12);
int hrt_problem_normals(const hrt_problem *p, float *outTx3);   /* in the reference's loop order */
int hrt_problem_tri_ids(const hrt_problem *p, uint32_t *mesh_out, uint32_t *face_out);
/* The device table is kept in a spatial (Morton) order for the acceleration structure
 * (csrc/host/accel.c); HRT_HIT_TRI values are rows of THAT table.  out[j] = position of row j in
 * the reference's (mesh, face) loop order (src/compute_paths.c:253-254), i.e. the flat index the
 * reference's scan would give the same triangle.  Environment: HRT_NO_REORDER=1 keeps the
 * reference's order (the identity here). */
int hrt_problem_tri_order(const hrt_problem *p, uint32_t *orig_of_row);

/* A shard of the launch set.  The N = num_paths launch directions of every TX are cut into
 * granules of `chunk` consecutive path indices dealt round-robin to `count` shards, so every
 * shard sees the whole sphere (a contiguous block would be a polar cap with a very different
 * hit rate).  Local ray i of shard r is global path
 *     p = ((i / chunk) * count + r) * chunk + i % chunk .
 * count = 1 is the unsharded problem. */
typedef struct {
    uint64_t num_paths;    /* global N per TX (the N in k/N of the Fibonacci sphere) */
    uint32_t rank, count;  /* shard r of G */
    uint32_t chunk;        /* granule; multiple of 64; 0 = 4096 */
    uint32_t num_bounces;
} hrt_shard;

uint64_t hrt_shard_num_local(const hrt_shard *s);
uint64_t hrt_shard_global_path(const hrt_shard *s, uint64_t local_i);

/* Launch directions of this shard's local rays, [num_local][3] floats, on the HOST with the
 * host libm (bit-identical to the reference's by construction).  num_threads <= 0: all
 * cores. */
int hrt_launch_dirs_host(const hrt_shard *s, float *out, int num_threads);

/* The same directions generated ON THE DEVICE into d_dirs (device [num_local][3] floats),
 * bit-identical to hrt_launch_dirs_host: the device evaluates the reference's formula with its
 * own double math library and flags every value whose rounding to float could depend on that
 * library's last bits (closer than 2^-44 relative to a float rounding boundary; about one ray
 * in a million); the flagged rays are recomputed with the host libm and patched in.  Blocks
 * until done; *num_patched (may be NULL) returns how many rays were patched. */
int hrt_launch_dirs_device(const hrt_shard *s, float *d_dirs, int device, void *stream,
                           uint64_t *num_patched);

/* Coherent launch order of this shard: a permutation of 0..num_local-1 (order[i] = local ray
 * launched by lane i) that walks the sphere in z-bands, serpentine in azimuth, so that 64
 * consecutive lanes -- one wavefront -- form a narrow ray packet (what the packet culling of
 * the trace kernel feeds on).  Pure function of `dirs` ([num_local][3], from
 * hrt_launch_dirs_host); dirs == NULL derives the keys from the path indices alone (for
 * directions generated on the device).  Results do not depend on the order (records carry ray ids); only
 * speed does. */
int hrt_launch_order_host(const hrt_shard *s, const float *dirs, uint32_t *order_out);

/* The same kind of order computed ON THE DEVICE into d_order (device [num_local] u32): bands are
 * ranges of the local index on a Fibonacci sphere, so one workgroup sorts one band segment by
 * azimuth in LDS.  Not the same permutation as hrt_launch_order_host (coarser azimuth keys), equally
 * coherent; what compute_paths() uses.  Blocks until done. */
int hrt_launch_order_device(const hrt_shard *s, uint32_t *d_order, int device, void *stream);

/* ---- workspace layout ----
 * cap = num_tx * num_local rounded up to 256 entries.  Every array below holds `cap`
 * elements of 4 bytes unless noted, so a field is a contiguous, coalesced run.
 *
 *   counts      u32[num_bounces + 2]   counts[b] (b >= 1) = rays that hit at bounce b-1
 *                                      = live rays entering bounce b; counts[0] unused;
 *                                      counts[num_bounces+1] = internal error flags (0)
 *   los         num_rx*num_tx entries of HRT_LOS_FLOATS floats
 *   hit block b (b = 0 .. num_bounces-1), fields HRT_HIT_*:
 *       the rays that hit something at bounce b, in the (stable) order of the live list they
 *       came from, with their state AFTER the bounce.  It is also the live list of bounce b+1.
 *   rec block b: for rx in 0..num_rx-1, fields HRT_REC_*: the scatter record of
 *       (hit i of block b, rx) at element i; plus one bit per (rx, i) "unblocked".
 *       A blocked record has a_* = tau = 0 and its dir/dfs elements are not written.
 */
enum {
    HRT_HIT_RAY = 0,   /* u32: tx * num_local + local_i */
    HRT_HIT_TRI,       /* u32: flat triangle index of the hit */
    HRT_HIT_THETA,     /* incidence angle */
    HRT_HIT_FS0,       /* launch Doppler term dot(tx_vel, d_launch) * f/c */
    HRT_HIT_OX, HRT_HIT_OY, HRT_HIT_OZ, HRT_HIT_DX, HRT_HIT_DY, HRT_HIT_DZ,
    HRT_HIT_A_TE_RE, HRT_HIT_A_TE_IM, HRT_HIT_A_TM_RE, HRT_HIT_A_TM_IM,
    HRT_HIT_TAU,
    HRT_HIT_FIELDS
};
enum {
    HRT_REC_A_TE_RE = 0, HRT_REC_A_TE_IM, HRT_REC_A_TM_RE, HRT_REC_A_TM_IM,
    HRT_REC_TAU,
    HRT_REC_DIRX, HRT_REC_DIRY, HRT_REC_DIRZ,   /* directions_rx */
    HRT_REC_DFS,       /* dot(d_to_rx - d_reflected, mesh_velocity) * f/c; the record's
                          freq_shift is FS0 - DFS */
    HRT_REC_FIELDS
};
enum {
    HRT_LOS_STATUS = 0,  /* as float bits of u32: 0 coincident, 1 blocked, 2 clear */
    HRT_LOS_A, HRT_LOS_TAU, HRT_LOS_DIRX, HRT_LOS_DIRY, HRT_LOS_DIRZ, HRT_LOS_FS,
    HRT_LOS_FLOATS = 8
};

typedef struct {
    uint64_t total_bytes;
    uint64_t cap;               /* elements per array */
    uint64_t off_counts;
    uint64_t off_los;
    uint64_t off_hits;          /* field f of block b at off_hits + b*hit_block_bytes + f*cap*4 */
    uint64_t hit_block_bytes;
    uint64_t off_recs;          /* field f of (b, rx) at off_recs + b*rec_block_bytes
                                                       + (rx*HRT_REC_FIELDS + f)*cap*4 */
    uint64_t rec_block_bytes;
    uint64_t off_masks;         /* u64 words of (b, rx) at off_masks + (b*num_rx + rx)*(cap/64)*8 */
    /* scratch of the stable compaction: survivor counts per WAVE of every 256-entry chunk (4 u32 per chunk), and per bounce the
     * sums over every 32 chunks (u32 [num_bounces][num_super]) */
    uint64_t off_chunk_cnt, off_super_cnt;
    /* trace results of one launch (internal scratch between the two kernels): for trace kind k
     * (0..num_rx-1 shadow to rx k, num_rx the bounce itself) a block of 2*cap words at
     * off_res + 2k*cap*4 -- the bounce: u32 triangle[cap] then f32 distance[cap]; a shadow trace:
     * one packed word per entry (triangle | blocked << 31), a half word on tables of fewer than
     * 32 767 triangles (triangle | blocked << 15) */
    uint64_t off_res;
    uint64_t num_super;
    /* re-sorting of the live list between bounces (only when the problem has it on, HRT_SORT_RAYS):
     * a hit-block-sized scratch, 4 x cap u32 of keys / indices, the sort's temporary storage */
    uint64_t off_sort_scratch, off_sort_keys, off_sort_tmp, sort_tmp_bytes;
    /* status words of the fused kernels (stable compaction inside ONE kernel: per-chunk, per-group
     * and per-supergroup survivor counts): u32 [num_bounces + 1][lb_stride], zeroed with the counts
     * at the start of every trace */
    uint64_t off_lb, lb_stride;
    /* queue of the packets too wide to cull (tables of more than 1 024 triangles): wide_cap entries of
     * 8 bytes, then 64 keys of 8 bytes per entry; wide_cap = 0: none */
    uint64_t off_wide_q, off_wide_key, wide_cap;
} hrt_layout;

/* HRT_E_CAPACITY when num_tx * (local rays) exceeds 2^32 / (HRT_HIT_FIELDS * 4) - 512
 * (~71.5 M): the kernels address the field arrays of a block by 32-bit offsets from the block's
 * buffer descriptor.  Use more shards (the drop-in compute_paths does so by itself). */
int hrt_layout_query(const hrt_problem *p, const hrt_shard *s, hrt_layout *out);

/* Per-launch device times of one hrt_trace call, filled only when requested. */
typedef struct {
    float los_ms;
    float trace_ms[33];         /* trace kernel of launch b = 0..num_bounces (patch tables: the primary rays only;
                                 * a fused launch: its one kernel) */
    float shade_ms[33];         /* shade kernel (Fresnel, reflect, compaction; records unless records_ms) of launch b */
    float records_ms[33];       /* hrt_records_kernel of launch b (patch tables: shadow traces + scatter records);
                                 * 0 where the trace and shade kernels do that work */
    uint32_t num_bounce_launches;
} hrt_kernel_times;

/* Enqueue the whole path on `stream`: zero the counters, LoS kernel, then num_bounces + 1
 * launches; launch b = trace kernel (the num_rx shadow rays of every hit of bounce b-1 and the
 * rays of bounce b: intersection only) + a one-workgroup scan (stable compaction offsets) +
 * shade kernel (scatter records of bounce b-1; Fresnel, delay, reflection of bounce b;
 * survivors written in order into the next live list).
 * Asynchronous unless `times` != NULL, in which case HIP events are recorded around every
 * launch on `stream` and the call returns after the stream drained.
 * d_dirs:  device [num_local][3] floats (this shard's launch directions).
 * d_order: device [num_local] u32 coherent launch order (hrt_launch_order_host), or NULL for
 *          index order (same results, less coherent packets). */
int hrt_trace(const hrt_problem *p, const hrt_shard *s, const float *d_dirs,
              const uint32_t *d_order, void *d_workspace, uint64_t workspace_bytes, void *stream,
              hrt_kernel_times *times);

/* Per-kernel timing WITHOUT a synchronisation per call: a timer owns the HIP events of one
 * hrt_trace; hrt_trace_timed records them on `stream` and returns at once (asynchronous, like
 * hrt_trace with times == NULL); hrt_timer_read waits for the timer's last event and converts.
 * Use one timer per call in flight (bench.py: one per timed step, read after the timed region). */
typedef struct hrt_timer hrt_timer;
int hrt_timer_create(uint32_t num_bounces, hrt_timer **out);
void hrt_timer_destroy(hrt_timer *t);
int hrt_trace_timed(const hrt_problem *p, const hrt_shard *s, const float *d_dirs,
                    const uint32_t *d_order, void *d_workspace, uint64_t workspace_bytes,
                    void *stream, hrt_timer *timer);

/* hrt_trace / hrt_trace_timed (timer may be NULL) with options.  HRT_DIRS_IN_LAUNCH_ORDER: d_dirs
 * is already permuted into launch order, d_dirs[i] = direction of ray d_order[i] (a caller that
 * traces the same launch set repeatedly permutes once; the launch kernels then read contiguous
 * runs instead of gathering 12-byte rows).  Results are identical. */
#define HRT_DIRS_IN_LAUNCH_ORDER 1u
int hrt_trace_flags(const hrt_problem *p, const hrt_shard *s, const float *d_dirs,
                    const uint32_t *d_order, void *d_workspace, uint64_t workspace_bytes,
                    void *stream, hrt_timer *timer, uint32_t flags);
int hrt_timer_read(hrt_timer *t, hrt_kernel_times *out);

/* Algorithmic work of a finished trace from its (host copy of) counts: see hrt_stats. */
void hrt_work_from_counts(const hrt_problem *p, const hrt_shard *s, const uint32_t *counts,
                          hrt_stats *out);

/* ---- packed export and gather: the exchange step of the sharded path (one process per GPU) ----
 * Every rank packs its compact result into ONE run of 32-bit words in HBM (floats bit-cast); the runs are
 * gathered to one rank.  A rank's META block (hrt_export_meta_words(nb, nrx) u32) holds what sizes the run:
 *     meta[0 .. nb + 1]                 the counts block of the trace (meta[b + 1] = H_b, the hits of bounce b)
 *     meta[nb + 2 + b * nrx + rx]       U_(b, rx): the unblocked records of (bounce b, rx)
 * Layout of the run, bounce after bounce (H = H_b):
 *     hit rows   [4][H]                 HRT_HIT_RAY, _TRI, _THETA, _FS0
 *     then per rx -- HRT_EXPORT_FULL:        records [HRT_REC_FIELDS][H], mask [2 * ceil(H / 64)] ("unblocked" bits)
 *                 -- HRT_EXPORT_UNBLOCKED:   index [U] (hit i of each kept record), records [HRT_REC_FIELDS][U]
 *                    (blocked records are all zero: 14 % of C3's; they need not travel)
 * hermespy-rt_amd/sharding.py is the torch.distributed binding of the same layout. */
#define HRT_EXPORT_FULL 0u
#define HRT_EXPORT_UNBLOCKED 1u
typedef struct {
    uint64_t hits, unblocked, records;      /* H_b, U_(b, rx), records in the run (H or U) */
    uint64_t off_hit;                       /* word offsets into the run: hit rows [4][hits] */
    uint64_t off_index;                     /* HRT_EXPORT_UNBLOCKED: [records] hit indices */
    uint64_t off_rec;                       /* [HRT_REC_FIELDS][records] */
    uint64_t off_mask;                      /* HRT_EXPORT_FULL: [2 * ceil(hits / 64)] */
} hrt_export_part;
uint32_t hrt_export_meta_words(uint32_t num_bounces, uint32_t num_rx);
uint64_t hrt_export_words(const uint32_t *meta, uint32_t num_bounces, uint32_t num_rx, uint32_t flags);
int hrt_export_locate(const uint32_t *meta, uint32_t num_bounces, uint32_t num_rx, uint32_t flags, uint32_t bounce,
                      uint32_t rx, hrt_export_part *out);

/* The gather of one shard's rank (s->rank of s->count) to `root`; buffers are kept between steps.
 * With a transport of the caller's own (sharding.py: torch.distributed):
 *     hrt_gather_prepare      meta block of the finished trace in d_workspace, on the device (hrt_gather_meta_device)
 *     (exchange the meta blocks)   hrt_gather_set_meta for every rank whose block is known here
 *     hrt_gather_pack         this rank's run;   hrt_gather_recv_buffer: where the root receives rank r's
 * or, over RCCL (librccl is bound at run time; `comm` is the caller's ncclComm_t, e.g. from
 * hrt_rccl_comm_create): hrt_gather_rccl does all of it -- ncclAllGather of the meta blocks, one group of
 * ncclSend / ncclRecv -- and returns when the root holds every run (hrt_gather_export; the other ranks hold the
 * meta blocks). */
typedef struct hrt_gather hrt_gather;
int hrt_gather_create(const hrt_problem *p, const hrt_shard *s, int root, uint32_t flags, hrt_gather **out);
void hrt_gather_destroy(hrt_gather *g);
uint32_t hrt_gather_meta_words(const hrt_gather *g);
const uint32_t *hrt_gather_meta_device(const hrt_gather *g);
int hrt_gather_prepare(hrt_gather *g, const void *d_workspace, void *stream);
int hrt_gather_set_meta(hrt_gather *g, uint32_t rank, const uint32_t *host_meta);
const uint32_t *hrt_gather_meta(const hrt_gather *g, uint32_t rank);   /* host; NULL if not known */
int hrt_gather_pack(hrt_gather *g, const void *d_workspace, void *stream, const void **d_run, uint64_t *words);
int hrt_gather_recv_buffer(hrt_gather *g, uint32_t rank, void **d_buf, uint64_t *words);
int hrt_gather_export(const hrt_gather *g, uint32_t rank, const void **d_run, uint64_t *words);
const void *hrt_gather_received(const hrt_gather *g, uint32_t rank);
typedef struct { char internal[128]; } hrt_rccl_id;   /* ncclUniqueId */
int hrt_rccl_unique_id(hrt_rccl_id *out);
int hrt_rccl_comm_create(const hrt_rccl_id *id, int world, int rank, int device, void **comm);
int hrt_rccl_comm_destroy(void *comm);
int hrt_gather_rccl(hrt_gather *g, void *comm, const void *d_workspace, void *stream, int self_loop);

/* ---- channel frequency responses from the traced paths (csrc/host/channel.c, csrc/hrt_channel.hip) ----
 * H[rx][tx][pol][m][k] as hermespy_rt.h defines it (hrt_channel_spec, hrt_compute_channel), formed from the
 * workspace of a finished hrt_trace (its counts too, on the device: no host synchronisation), asynchronous on
 * `stream`.  accumulate = 0 overwrites d_out, 1 adds to it.  Only shard rank 0 adds the LoS term, so the
 * outputs of the shards of one launch set sum to the whole channel.  If the trace's error word
 * (counts[num_bounces + 1]) is nonzero the output is undefined: check it first, as before reading records.
 * Deterministic: partial sums go to the caller's scratch (hrt_channel_scratch_bytes) and are reduced in a fixed
 * order, no floating-point atomics; two calls with the same inputs give the same bits.
 * HRT_E_INVALID, before the device is touched: num_freqs or num_times 0, num_freqs * num_times > 2^20, parts 0
 * or with unknown bits, f0 / df / t0 / dt not finite, scratch too small. */
int hrt_channel_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_channel_spec *spec,
                              uint64_t *out);
int hrt_channel(const hrt_problem *p, const hrt_shard *s, const void *d_workspace,
                const hrt_channel_spec *spec, void *d_scratch, uint64_t scratch_bytes,
                float *d_out, int accumulate, void *stream);

/* ---- antenna-array channel responses from the traced paths (csrc/host/channel.c, csrc/hrt_array_channel.hip) ----
 * H[rx][tx][i][j][pol][m][k] as hermespy_rt.h defines it (hrt_compute_array_channel), formed from the workspace of
 * a finished hrt_trace, asynchronous on `stream`, with the guarantees of hrt_channel: accumulate = 0 overwrites
 * d_out, 1 adds to it; only shard rank 0 adds the LoS term; partial sums go to the caller's scratch
 * (hrt_array_channel_scratch_bytes) and are reduced in a fixed order, no floating-point atomics, so two calls with
 * the same inputs give the same bits.  The element offsets are DEVICE pointers here ([Nr][3] and [Nt][3] floats,
 * e.g. torch tensors) and are not read on the host: their finiteness is the caller's to ensure (the host entries
 * check it).  HRT_E_INVALID, before the device is touched: every hrt_channel check; NULL arrays or element
 * pointers; Nr or Nt outside 1..1024; Nr * Nt * num_times * num_freqs > 2^24; f_a not finite or <= 0. */
typedef struct {
    uint32_t num_rx_elements, num_tx_elements;   /* Nr, Nt: 1 .. 1024 */
    const float *rx_elements;                    /* device [Nr][3]: r_i (m) */
    const float *tx_elements;                    /* device [Nt][3]: q_j (m) */
    double array_frequency_hz;                   /* f_a: the frequency of the steering phases */
} hrt_array_spec;
int hrt_array_channel_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_channel_spec *spec,
                                    const hrt_array_spec *arrays, uint64_t *out);
int hrt_array_channel(const hrt_problem *p, const hrt_shard *s, const void *d_workspace,
                      const hrt_channel_spec *spec, const hrt_array_spec *arrays, void *d_scratch,
                      uint64_t scratch_bytes, float *d_out, int accumulate, void *stream);

/* ---- beamformed (codebook) channel responses from the traced paths (csrc/host/channel.c, csrc/hrt_beam_channel.hip) ----
 * B[rx][tx][a][b][pol][m][k] as hermespy_rt.h defines it (hrt_compute_beam_channel): hrt_array_channel's H contracted
 * with the combiner conj(W_rx[a]) and the precoder W_tx[b], with the weights folded into every path's steering term on
 * the device, so H is never formed and Nr * Nt is not limited.  Formed from the workspace of a finished hrt_trace,
 * asynchronous on `stream`, with the guarantees of hrt_channel: accumulate = 0 overwrites d_out, 1 adds to it; only
 * shard rank 0 adds the LoS term; partial sums and the LoS gains go to the caller's scratch
 * (hrt_beam_channel_scratch_bytes) and are reduced in a fixed order, no floating-point atomics, so two calls with the
 * same inputs give the same bits.  The element offsets (hrt_array_spec) and the weights are DEVICE pointers and are not
 * read on the host: their finiteness is the caller's to ensure (the host entries check it).  One codebook is shared by
 * all RX and one by all TX; the weights are not normalised.  HRT_E_INVALID, before the device is touched: every
 * hrt_channel check; NULL arrays, beams, element or weight pointers; Nr or Nt outside 1..256; Br or Bt outside
 * 1..256; Br * Bt * num_times * num_freqs > 2^24; f_a not finite or <= 0; 2^39 outputs or more; scratch too small. */
typedef struct {
    uint32_t num_rx_beams, num_tx_beams;         /* Br, Bt: 1 .. 256 */
    const float *rx_weights;                     /* device [Br][Nr][2] (re, im): W_rx, applied conjugated (w^H) */
    const float *tx_weights;                     /* device [Bt][Nt][2] (re, im): W_tx, applied as it is (f) */
} hrt_beam_spec;
int hrt_beam_channel_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_channel_spec *spec,
                                   const hrt_array_spec *arrays, const hrt_beam_spec *beams, uint64_t *out);
int hrt_beam_channel(const hrt_problem *p, const hrt_shard *s, const void *d_workspace,
                     const hrt_channel_spec *spec, const hrt_array_spec *arrays, const hrt_beam_spec *beams,
                     void *d_scratch, uint64_t scratch_bytes, float *d_out, int accumulate, void *stream);

/* ---- sampled channel impulse responses from the traced paths (csrc/host/channel.c, csrc/hrt_taps.hip) ----
 * h[rx][tx][pol][m][i] as hermespy_rt.h defines it (hrt_taps_spec, hrt_compute_taps), formed from the workspace of
 * a finished hrt_trace (its counts read on the device: no host synchronisation), asynchronous on `stream`, with the
 * guarantees of hrt_channel: accumulate = 0 overwrites d_out, 1 adds to it; only shard rank 0 adds the LoS term, so
 * the outputs of the shards of one launch set sum to the whole result; partial sums go to the caller's scratch
 * (hrt_taps_scratch_bytes) and are reduced in a fixed order, no floating-point atomics, so two calls with the same
 * inputs give the same bits; the output is undefined if the trace's error word is set.
 * HRT_E_INVALID, before the device is touched: every hrt_compute_taps spec check, num_rx * num_tx > 65535,
 * scratch too small. */
int hrt_taps_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_taps_spec *spec, uint64_t *out);
int hrt_taps(const hrt_problem *p, const hrt_shard *s, const void *d_workspace, const hrt_taps_spec *spec,
             void *d_scratch, uint64_t scratch_bytes, float *d_out, int accumulate, void *stream);

/* ---- antenna-array impulse responses from the traced paths (csrc/host/channel.c, csrc/hrt_array_taps.hip) ----
 * h[rx][tx][i][j][pol][m][l] as hermespy_rt.h defines it (hrt_compute_array_taps), formed from the workspace of a
 * finished hrt_trace (its counts read on the device: no host synchronisation), asynchronous on `stream`, with the
 * guarantees of hrt_taps: accumulate = 0 overwrites d_out, 1 adds to it; only shard rank 0 adds the LoS term, so the
 * outputs of the shards of one launch set sum to the whole result; partial sums go to the caller's scratch
 * (hrt_array_taps_scratch_bytes) and are reduced in a fixed order, no floating-point atomics, so two calls with the
 * same inputs give the same bits; the output is undefined if the trace's error word is set.  The element offsets are
 * DEVICE pointers, as in hrt_array_channel (their finiteness is the caller's to ensure; the host entries check it).
 * HRT_E_INVALID, before the device is touched: every hrt_taps check; NULL arrays or element pointers; Nr or Nt
 * outside 1..1024; Nr * Nt * num_times * num_taps > 2^24; f_a not finite or <= 0; num_rx * num_tx > 65535; 2^39
 * outputs or more; scratch too small. */
int hrt_array_taps_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_taps_spec *spec,
                                 const hrt_array_spec *arrays, uint64_t *out);
int hrt_array_taps(const hrt_problem *p, const hrt_shard *s, const void *d_workspace, const hrt_taps_spec *spec,
                   const hrt_array_spec *arrays, void *d_scratch, uint64_t scratch_bytes, float *d_out, int accumulate,
                   void *stream);

/* ---- beamformed (codebook) impulse responses from the traced paths (csrc/host/channel.c, csrc/hrt_beam_taps.hip) ----
 * h[rx][tx][a][b][pol][m][l] as hermespy_rt.h defines it (hrt_compute_beam_taps): hrt_array_taps' h contracted with
 * the combiner conj(W_rx[a]) and the precoder W_tx[b], with the weights folded into every path's steering term on the
 * device, so the element-domain taps are never formed and Nr * Nt is not limited.  Formed from the workspace of a
 * finished hrt_trace, asynchronous on `stream`, with the guarantees of hrt_taps: accumulate = 0 overwrites d_out, 1
 * adds to it; only shard rank 0 adds the LoS term; partial sums and the LoS gains go to the caller's scratch
 * (hrt_beam_taps_scratch_bytes) and are reduced in a fixed order, no floating-point atomics, so two calls with the
 * same inputs give the same bits.  The element offsets (hrt_array_spec) and the weights (hrt_beam_spec) are DEVICE
 * pointers and are not read on the host, as in hrt_beam_channel.  HRT_E_INVALID, before the device is touched: every
 * hrt_taps check; NULL arrays, beams, element or weight pointers; Nr or Nt outside 1..256; Br or Bt outside 1..256;
 * Br * Bt * num_times * num_taps > 2^24; f_a not finite or <= 0; 2^39 outputs or more; scratch too small. */
int hrt_beam_taps_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_taps_spec *spec,
                                const hrt_array_spec *arrays, const hrt_beam_spec *beams, uint64_t *out);
int hrt_beam_taps(const hrt_problem *p, const hrt_shard *s, const void *d_workspace, const hrt_taps_spec *spec,
                  const hrt_array_spec *arrays, const hrt_beam_spec *beams, void *d_scratch, uint64_t scratch_bytes,
                  float *d_out, int accumulate, void *stream);

/* ---- received signals: taps applied to waveforms (csrc/host/channel.c, csrc/hrt_propagate.hip) ----
 * y as hermespy_rt.h defines it (hrt_propagate_spec, hrt_compute_received_signal), hrt_propagate_out_floats floats at
 * d_out, from d_taps (complex [num_rx][num_tx][nr][nt][2][num_times][num_taps]: the output of hrt_array_taps, of
 * hrt_taps with nr = nt = 1, or of hrt_beam_taps with its beam counts) and d_signal (complex [num_tx][nt]
 * [num_samples]), all DEVICE pointers, asynchronous on `stream` of `device`.  It needs no problem: it reads only the
 * two tensors.  accumulate = 0 overwrites d_out, 1 adds to it; every element of d_out is written exactly once, also
 * where the sum is empty; no scratch, no partial sums and no floating-point atomics, so two calls with the same inputs
 * give the same bits.  HRT_E_INVALID, before the device is touched: a NULL pointer; any of num_rx, num_tx, nr, nt,
 * num_times, num_taps, samples_per_block, num_samples, num_out equal to 0; nr or nt > 1024; nr * nt * num_times *
 * num_taps > 2^24; |l_min| or |l_min + num_taps| > 2^24; num_samples or num_out > 2^31; accumulate not 0 or 1. */
int hrt_propagate(int device, const hrt_propagate_spec *spec, const void *d_taps, const void *d_signal, void *d_out,
                  int accumulate, void *stream);

/* ---- per-point MIMO SVD of an array channel (csrc/host/channel.c, csrc/hrt_svd.hip) ----
 * sigma, u, v and sweeps as hermespy_rt.h defines them (hrt_svd_spec, hrt_compute_channel_svd), hrt_svd_out_bytes
 * bytes at d_out, from d_H (complex [num_rx][num_tx][nr][nt][2][num_times][num_freqs]: the output of
 * hrt_array_channel, or any tensor of that layout), both DEVICE pointers, asynchronous on `stream` of `device`.  It
 * needs no problem: it reads only the tensor, and does not write it.  Every byte of d_out is written exactly once; no
 * scratch and no atomics, so two calls with the same input give the same bytes.  The SVD of one shard's partial H is
 * not the channel's SVD: a sharded caller sums H first.  HRT_E_INVALID, before the device is touched: a NULL pointer;
 * num_rx, num_tx, num_times or num_freqs equal to 0; min(nr, nt) outside 1..16; max(nr, nt) outside 1..64;
 * nr * nt * num_times * num_freqs > 2^24; `want` with bits other than HRT_SVD_U | HRT_SVD_V; 2^31 points or more. */
int hrt_channel_svd(int device, const hrt_svd_spec *spec, const void *d_H, void *d_out, void *stream);

/* ---- per-point linear MIMO equalizers of an array channel (csrc/host/channel.c, csrc/hrt_equalizer.hip) ----
 * W, sinr and status as hermespy_rt.h defines them (hrt_equalizer_spec, hrt_compute_channel_equalizer),
 * hrt_equalizer_out_bytes bytes at d_out, from d_H (complex [num_rx][num_tx][nr][nt][2][num_times][num_freqs]: the
 * output of hrt_array_channel, or any tensor of that layout), both DEVICE pointers, asynchronous on `stream` of
 * `device`.  It needs no problem: it reads only the tensor, and does not write it.  Every byte of d_out is written
 * exactly once; no scratch and no atomics, so two calls with the same input give the same bytes.  The equalizer of one
 * shard's partial H is not the channel's: a sharded caller sums H first.  HRT_E_INVALID, before the device is touched:
 * a NULL pointer; num_rx, num_tx, num_times or num_freqs equal to 0; nt outside 1..16; nr outside 1..64; a kind other
 * than HRT_EQ_ZF and HRT_EQ_LMMSE; HRT_EQ_ZF with nr < nt; `flags` with bits other than HRT_EQ_W; a noise that is not
 * finite and > 0; nr * nt * num_times * num_freqs > 2^24; 2^31 points or more. */
int hrt_channel_equalizer(int device, const hrt_equalizer_spec *spec, const void *d_H, void *d_out, void *stream);

/* ---- per-point linear MIMO precoders of an array channel (csrc/host/channel.c, csrc/hrt_precoder.hip) ----
 * P, sinr and status as hermespy_rt.h defines them (hrt_precoder_spec, hrt_compute_channel_precoder),
 * hrt_precoder_out_bytes bytes at d_out, from d_H (complex [num_rx][num_tx][nr][nt][2][num_times][num_freqs]: the
 * output of hrt_array_channel, or any tensor of that layout), both DEVICE pointers, asynchronous on `stream` of
 * `device`.  It needs no problem: it reads only the tensor, and does not write it.  Every byte of d_out is written
 * exactly once; no scratch and no atomics, so two calls with the same input give the same bytes.  The precoder of one
 * shard's partial H is not the channel's: a sharded caller sums H first.  HRT_E_INVALID, before the device is touched:
 * a NULL pointer; num_rx, num_tx, num_times or num_freqs equal to 0; nr outside 1..16; nt outside 1..64; a kind other
 * than HRT_PC_MRT, HRT_PC_ZF and HRT_PC_RZF; a norm other than HRT_PC_TOTAL and HRT_PC_STREAM; HRT_PC_ZF with nr > nt;
 * `flags` with bits other than HRT_PC_P; a noise, a power or (HRT_PC_RZF) a regularization that is not finite and > 0;
 * nr * nt * num_times * num_freqs > 2^24; 2^31 points or more. */
int hrt_channel_precoder(int device, const hrt_precoder_spec *spec, const void *d_H, void *d_out, void *stream);

/* ---- per-subband precoder codebook selection on an array channel (csrc/host/channel.c, csrc/hrt_codebook.hip) ----
 * index, metric, status, table and effective as hermespy_rt.h defines them (hrt_codebook_spec,
 * hrt_compute_codebook_select), hrt_codebook_out_bytes bytes at d_out, from d_H (complex
 * [num_rx][num_tx][nr][nt][2][num_times][num_freqs]: the output of hrt_array_channel, or any tensor of that layout) and
 * d_codebook (complex [entries][nt][layers]), all DEVICE pointers, asynchronous on `stream` of `device`.  It needs no
 * problem: it reads only the two tensors, and writes neither.  Every byte of d_out is written exactly once; no scratch
 * and no atomics, so two calls with the same input give the same bytes.  The selection of one shard's partial H is not
 * the channel's: a sharded caller sums H first.  HRT_E_INVALID, before the device is touched: a NULL pointer; num_rx,
 * num_tx, num_times or num_freqs equal to 0; nr outside 1..16; nt outside 1..64; layers outside 1..min(4, nt); entries
 * outside 1..4096; subband outside 1..num_freqs; a metric other than HRT_CS_POWER and HRT_CS_CAPACITY; `flags` with
 * bits other than HRT_CS_TABLE and HRT_CS_EFFECTIVE; under HRT_CS_CAPACITY a noise that is not finite and > 0; 2^31
 * points or more; 2^31 table entries (num_rx num_tx entries 2 num_times B) or more. */
int hrt_codebook_select(int device, const hrt_codebook_spec *spec, const void *d_H, const void *d_codebook, void *d_out,
                        void *stream);

/* ---- per-point maximum-likelihood detection on an array channel (csrc/host/channel.c, csrc/hrt_detect.hip) ----
 * index, metric, status and llr as hermespy_rt.h defines them (hrt_detect_spec, hrt_compute_channel_detect),
 * hrt_detect_out_bytes bytes at d_out, from d_H (complex [num_rx][num_tx][nr][nt][2][num_times][num_freqs]: the output
 * of hrt_array_channel, or any tensor of that layout), d_Y (complex [num_rx][num_tx][nr][2][num_times][num_freqs]) and
 * d_constellation (complex [2^bits]), all DEVICE pointers, asynchronous on `stream` of `device`.  It needs no
 * problem: it reads only the three tensors, and writes none of them.  Every byte of d_out is written exactly once; no
 * scratch and no atomics, so two calls with the same input give the same bytes.  Detection on one shard's partial H
 * is not the channel's: a sharded caller sums H first.  HRT_E_INVALID, before the device is touched: a NULL pointer;
 * num_rx, num_tx, num_times or num_freqs equal to 0; nr outside 1..64; bits outside 1..8; nt < 1 or nt * bits > 12;
 * `flags` with bits other than HRT_DT_LLR; a noise that is not finite and > 0; nr * nt * num_times * num_freqs > 2^24;
 * 2^31 points or more. */
int hrt_channel_detect(int device, const hrt_detect_spec *spec, const void *d_H, const void *d_Y,
                       const void *d_constellation, void *d_out, void *stream);

/* ---- per-point K-best tree-search detection on an array channel (csrc/host/channel.c, csrc/hrt_kbest.hip) ----
 * index, metric, status and llr as hermespy_rt.h defines them (hrt_kbest_spec, hrt_compute_channel_kbest),
 * hrt_kbest_out_bytes bytes at d_out, from d_H, d_Y and d_constellation as hrt_channel_detect takes them, all DEVICE
 * pointers, asynchronous on `stream` of `device`.  It needs no problem, reads only the three tensors and writes none
 * of them.  Every byte of d_out is written exactly once; no scratch and no atomics, so two calls with the same input
 * give the same bytes.  HRT_E_INVALID, before the device is touched: a NULL pointer; num_rx, num_tx, num_times or
 * num_freqs equal to 0; nr outside 1..64; nt outside 1..16; bits outside 1..8; nt * bits > 32; k not one of 1, 2, 4,
 * 8, 16, 32, 64; `flags` with bits other than HRT_KB_LLR | HRT_KB_SORTED; a noise or a clip that is not finite and
 * > 0; nr * nt * num_times * num_freqs > 2^24; 2^31 points or more. */
int hrt_channel_kbest(int device, const hrt_kbest_spec *spec, const void *d_H, const void *d_Y,
                      const void *d_constellation, void *d_out, void *stream);

/* ---- per-link power statistics from the traced paths (csrc/host/channel.c, csrc/hrt_power.hip) ----
 * moments, pdp, arrival and departure as hermespy_rt.h defines them (hrt_power_spec, hrt_compute_power_profiles),
 * hrt_power_out_doubles doubles at d_out, formed from the workspace of a finished hrt_trace (its counts read on the
 * device: no host synchronisation), asynchronous on `stream`, with the guarantees of hrt_taps: accumulate = 0
 * overwrites d_out, 1 adds to it; only shard rank 0 adds the LoS term, so the outputs of the shards of one launch
 * set sum to the whole result; the moments' partial sums go to the caller's scratch (hrt_power_profiles_scratch_bytes)
 * and are reduced in a fixed order, the histograms are u64 fixed-point sums scaled by this call's own total power
 * (never by what d_out holds); no floating-point atomics, so two calls with the same inputs give the same bits; the
 * output is undefined if the trace's error word is set.
 * HRT_E_INVALID, before the device is touched: every hrt_compute_power_profiles check, scratch too small. */
int hrt_power_profiles_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_power_spec *spec,
                                     uint64_t *out);
int hrt_power_profiles(const hrt_problem *p, const hrt_shard *s, const void *d_workspace, const hrt_power_spec *spec,
                       void *d_scratch, uint64_t scratch_bytes, double *d_out, int accumulate, void *stream);

/* ---- spatial covariance matrices of an antenna array (csrc/host/channel.c, csrc/hrt_covariance.hip) ----
 * R_rx and R_tx as hermespy_rt.h defines them (hrt_covariance_spec, hrt_compute_array_covariance),
 * hrt_covariance_out_floats floats at d_out (0 for a NULL argument; the element counts of the sides asked for are
 * read from `arrays`), formed from the workspace of a finished hrt_trace (its counts read on the device: no host
 * synchronisation), asynchronous on `stream`, with the guarantees of hrt_power_profiles: accumulate = 0 overwrites
 * d_out, 1 adds to it; only shard rank 0 adds the LoS term, so the outputs of the shards of one launch set sum to the
 * whole result; partial sums go to the caller's scratch (hrt_array_covariance_scratch_bytes) and are reduced in a
 * fixed order, no floating-point atomics, so two calls with the same inputs give the same bits; the output is
 * undefined if the trace's error word is set.  The element offsets are DEVICE pointers, as in hrt_array_channel (their
 * finiteness is the caller's to ensure; the host entries check it); those of a side that is not asked for are not read
 * and may be NULL.  HRT_E_INVALID, before the device is touched: NULL spec or arrays; parts or sides 0 or with unknown
 * bits; a requested side with 0 or more than 256 elements or a NULL element pointer; f_a not finite or <= 0;
 * num_rx * num_tx > 65535; num_rx * num_tx * 2 * (Nr^2 + Nt^2) > 2^26; scratch too small. */
uint64_t hrt_covariance_out_floats(size_t num_rx, size_t num_tx, const hrt_array_spec *arrays,
                                   const hrt_covariance_spec *spec);
int hrt_array_covariance_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_covariance_spec *spec,
                                       const hrt_array_spec *arrays, uint64_t *out);
int hrt_array_covariance(const hrt_problem *p, const hrt_shard *s, const void *d_workspace,
                         const hrt_covariance_spec *spec, const hrt_array_spec *arrays, void *d_scratch,
                         uint64_t scratch_bytes, float *d_out, int accumulate, void *stream);

/* ---- antenna radiation patterns and orientations (csrc/host/channel.c, csrc/hrt_patterns.hip) ----
 * The weights hermespy_rt.h defines (hrt_pattern), applied IN PLACE to the workspace of a finished hrt_trace (its
 * counts read on the device: no host synchronisation), asynchronous on `stream`: afterwards every path-sum family
 * above sums the weighted paths.  It applies whenever it is called: applying twice weights twice (a trace writes the
 * amplitudes anew).  Tables and rotations are DEVICE pointers (d_rx_rot [num_rx][9], d_tx_rot [num_tx][9]; NULL:
 * identity); their contents are the caller's to ensure (the host entries check them).  No atomics: two runs on equal
 * inputs give equal bits.  HRT_E_INVALID, before the device is touched: a NULL problem, shard, workspace or spec;
 * kind > 3; a table with a NULL pointer, num_zenith outside 2 .. 181 or num_azimuth outside 1 .. 360; gain_db not
 * finite or |gain_db| > 200; a workspace smaller than the layout. */
typedef struct {
    hrt_pattern rx, tx;
    const float *d_rx_rot, *d_tx_rot;
} hrt_pattern_spec;
int hrt_apply_patterns(const hrt_problem *p, const hrt_shard *s, void *d_workspace, uint64_t workspace_bytes,
                       const hrt_pattern_spec *spec, void *stream);

/* ---- the K strongest paths per link from the traced paths (csrc/host/channel.c, csrc/hrt_dominant.hip) ----
 * header and records as hermespy_rt.h defines them (hrt_dominant_spec, hrt_dominant_path,
 * hrt_compute_dominant_paths), hrt_dominant_out_bytes bytes at d_out, selected from the workspace of a finished
 * hrt_trace (its counts read on the device: no host synchronisation), asynchronous on `stream`.  Here `tri` is the
 * ROW of the device table (HRT_HIT_TRI; hrt_problem_tri_order translates it to the reference's flat index).
 * accumulate = 0 overwrites d_out; accumulate = 1 MERGES: the new list of a link is the first K of (the records
 * d_out already holds, united with this call's eligible terms) and `eligible` is added to what d_out holds.  A term
 * in the first K of a union is in the first K of its part, and only shard rank 0 contributes the LoS entry, so the
 * shards and batches of one launch set, merged in any order, give byte for byte the unsharded result.  The candidate
 * lists go to the caller's scratch (hrt_dominant_paths_scratch_bytes); no floating-point atomics, and the result is
 * a function of the set of terms only, so two calls with the same inputs give the same bits; the output is
 * undefined if the trace's error word is set.
 * HRT_E_INVALID, before the device is touched: every hrt_compute_dominant_paths check; num_paths of the shard
 * >= 2^48; scratch too small. */
int hrt_dominant_paths_scratch_bytes(const hrt_problem *p, const hrt_shard *s, const hrt_dominant_spec *spec,
                                     uint64_t *out);
int hrt_dominant_paths(const hrt_problem *p, const hrt_shard *s, const void *d_workspace,
                       const hrt_dominant_spec *spec, void *d_scratch, uint64_t scratch_bytes, void *d_out,
                       int accumulate, void *stream);

/* ---- the array channel of dominant-path lists (csrc/host/channel.c, csrc/hrt_sparse_channel.hip) ----
 * H as hermespy_rt.h defines it (hrt_sparse_spec, hrt_compute_sparse_array_channel), hrt_sparse_out_bytes bytes at
 * d_out, from the lists at d_paths (hrt_sparse_paths_bytes bytes in hrt_dominant_paths' layout: its output, a merged or
 * a synthetic list; 8-byte aligned), the element offsets d_rx_el [nr][3] and d_tx_el [nt][3] -- all DEVICE pointers --
 * asynchronous on `stream` of `device`.  It takes no problem handle and reads only the buffer, and does not write it.
 * accumulate = 0 overwrites d_out, 1 adds to it.  One workgroup sums all live slots of a link in index order: every
 * byte of d_out is written exactly once (added to once), no atomics and no scratch, so two calls with the same input
 * give the same bytes; a link's bytes depend only on its own slots; slots at or beyond min(kept, max_paths) are never
 * read.  The finiteness of the offsets is the caller's to ensure (the host entries check it).  The two size functions
 * return 0 for a NULL or refused spec.  HRT_E_INVALID, before the device is touched: a NULL pointer; num_rx * num_tx
 * of 0 or above 65 535; max_paths of 0 or above 1 024; num_rx * num_tx * max_paths above 2^22; num_freqs or num_times
 * 0; num_freqs * num_times above 2^20; f0, df, t0 or dt not finite; nr or nt outside 1..1024; nr * nt * num_times *
 * num_freqs above 2^24; f_a not finite or <= 0; d_paths not 8-byte aligned; accumulate not 0 or 1. */
uint64_t hrt_sparse_paths_bytes(const hrt_sparse_spec *spec);
uint64_t hrt_sparse_out_bytes(const hrt_sparse_spec *spec, uint32_t nr, uint32_t nt);
int hrt_sparse_array_channel(int device, const hrt_sparse_spec *spec, const float *d_rx_el, uint32_t nr,
                             const float *d_tx_el, uint32_t nt, double fa_hz, const void *d_paths, float *d_out,
                             int accumulate, void *stream);

/* ---- the array taps of dominant-path lists (csrc/host/channel.c, csrc/hrt_sparse_taps.hip) ----
 * h as hermespy_rt.h defines it (hrt_sparse_taps_spec, hrt_compute_sparse_array_taps), hrt_sparse_taps_out_bytes bytes
 * at d_out, from the lists at d_paths (num_rx * num_tx * (16 + 72 max_paths) bytes in hrt_dominant_paths' layout: its
 * output, a merged or a synthetic list; 8-byte aligned), the element offsets d_rx_el [nr][3] and d_tx_el [nt][3] -- all
 * DEVICE pointers -- asynchronous on `stream` of `device`.  As hrt_sparse_array_channel: no problem handle, reads only
 * the buffer and does not write it; accumulate = 0 overwrites d_out, 1 adds to it; one workgroup sums all live slots of
 * a link in index order, so every byte of d_out is written exactly once (added to once), without atomics or scratch,
 * and two calls with the same input give the same bytes; a link's bytes depend only on its own slots; slots at or
 * beyond min(kept, max_paths) are never read.  The finiteness of the offsets is the caller's to ensure.  The size
 * function returns 0 for a NULL or refused spec.  HRT_E_INVALID, before the device is touched: a NULL pointer; num_rx *
 * num_tx of 0 or above 65 535; max_paths of 0 or above 1 024; num_rx * num_tx * max_paths above 2^22; num_taps or
 * num_times 0; num_taps * num_times above 2^20; f_s not finite or <= 0; f_c, t0 or dt not finite; |l_min| or |l_min +
 * num_taps| above 2^24; nr or nt outside 1..1024; nr * nt * num_times * num_taps above 2^24; f_a not finite or <= 0;
 * d_paths not 8-byte aligned; accumulate not 0 or 1. */
uint64_t hrt_sparse_taps_out_bytes(const hrt_sparse_taps_spec *spec, uint32_t nr, uint32_t nt);
int hrt_sparse_array_taps(int device, const hrt_sparse_taps_spec *spec, const float *d_rx_el, uint32_t nr,
                          const float *d_tx_el, uint32_t nt, double fa_hz, const void *d_paths, float *d_out,
                          int accumulate, void *stream);

/* ---- the beam channel of dominant-path lists (csrc/host/channel.c, csrc/hrt_sparse_beam.hip) ----
 * B as hermespy_rt.h defines it (hrt_compute_sparse_beam_channel), hrt_sparse_beam_out_bytes bytes at d_out, from the
 * lists at d_paths (hrt_sparse_paths_bytes bytes in hrt_dominant_paths' layout: its output, a merged or a synthetic
 * list; 8-byte aligned), the element offsets d_rx_el [nr][3] and d_tx_el [nt][3] and the codebooks d_rx_w [br][nr][2]
 * and d_tx_w [bt][nt][2] (hrt_beam_spec's layout and conventions) -- all DEVICE pointers -- asynchronous on `stream` of
 * `device`.  As hrt_sparse_array_channel: no problem handle, reads only the buffer and does not write it; accumulate =
 * 0 overwrites d_out, 1 adds to it; one workgroup sums all live slots of a link in index order, so every byte of d_out
 * is written exactly once (added to once), without atomics or scratch, and two calls with the same input give the same
 * bytes; a link's bytes depend only on its own slots below min(kept, max_paths), the grid, the elements and the
 * weights; slots at or beyond that are never read.  The element-domain matrix is never formed: there is no limit on
 * nr * nt.  The finiteness of the offsets and of the weights is the caller's to ensure (the host entries check it).
 * The size function returns 0 for a NULL or refused spec.  HRT_E_INVALID, before the device is touched: every refusal
 * of hrt_sparse_array_channel's spec (num_rx * num_tx, max_paths, their product, the grid); a NULL pointer; nr or nt
 * outside 1..256; br or bt outside 1..256; br * bt * num_times * num_freqs above 2^24; f_a not finite or <= 0; d_paths
 * not 8-byte aligned; accumulate not 0 or 1. */
uint64_t hrt_sparse_beam_out_bytes(const hrt_sparse_spec *spec, uint32_t br, uint32_t bt);
int hrt_sparse_beam_channel(int device, const hrt_sparse_spec *spec, const float *d_rx_el, uint32_t nr,
                            const float *d_tx_el, uint32_t nt, double fa_hz, const float *d_rx_w, uint32_t br,
                            const float *d_tx_w, uint32_t bt, const void *d_paths, float *d_out, int accumulate,
                            void *stream);

/* ---- the beam taps of dominant-path lists (csrc/host/channel.c, csrc/hrt_sparse_beam_taps.hip) ----
 * h as hermespy_rt.h defines it (hrt_compute_sparse_beam_taps), hrt_sparse_beam_taps_out_bytes bytes at d_out, from the
 * lists at d_paths (num_rx * num_tx * (16 + 72 max_paths) bytes in hrt_dominant_paths' layout: its output, a merged or
 * a synthetic list; 8-byte aligned), the element offsets d_rx_el [nr][3] and d_tx_el [nt][3] and the codebooks d_rx_w
 * [br][nr][2] and d_tx_w [bt][nt][2] (hrt_beam_spec's layout and conventions) -- all DEVICE pointers -- asynchronous
 * on `stream` of `device`.  The spec is hrt_sparse_array_taps'.  As hrt_sparse_array_taps: no problem handle, reads
 * only the buffer and does not write it; accumulate = 0 overwrites d_out, 1 adds to it; one workgroup sums all live
 * slots of a link in index order, so every byte of d_out is written exactly once (added to once), without atomics or
 * scratch, and two calls with the same input give the same bytes; a link's bytes depend only on its own header word,
 * its slots below min(kept, max_paths), the grid, the elements and the weights; slots at or beyond that are never
 * read.  The element-domain taps are never formed: there is no limit on nr * nt.  The finiteness of the offsets and of
 * the weights is the caller's to ensure (the host entries check it).  The size function returns 0 for a NULL or
 * refused spec.  HRT_E_INVALID, before the device is touched: every refusal hrt_sparse_array_taps makes on the spec
 * (num_rx * num_tx, max_paths, their product, the taps grid); a NULL pointer; nr or nt outside 1..256; br or bt outside
 * 1..256; br * bt * num_times * num_taps above 2^24; f_a not finite or <= 0; d_paths not 8-byte aligned; accumulate
 * not 0 or 1. */
uint64_t hrt_sparse_beam_taps_out_bytes(const hrt_sparse_taps_spec *spec, uint32_t br, uint32_t bt);
int hrt_sparse_beam_taps(int device, const hrt_sparse_taps_spec *spec, const float *d_rx_el, uint32_t nr,
                         const float *d_tx_el, uint32_t nt, double fa_hz, const float *d_rx_w, uint32_t br,
                         const float *d_tx_w, uint32_t bt, const void *d_paths, float *d_out, int accumulate,
                         void *stream);

/* sizes of the structs this build writes in full (a binding compares them with its own mirror) */
uint64_t hrt_stats_size(void);
uint64_t hrt_layout_size(void);

/* ---- thin helpers over the HIP runtime for C callers without one ---- */
int hrt_device_count(int *out);
int hrt_device_malloc(int device, void **out, uint64_t bytes);
int hrt_device_free(int device, void *ptr);
int hrt_device_upload(int device, void *dst, const void *src, uint64_t bytes);
int hrt_device_download(int device, void *dst, const void *src, uint64_t bytes);
int hrt_device_sync(int device, void *stream);
/* total/free HBM bytes */
int hrt_device_mem_info(int device, uint64_t *free_bytes, uint64_t *total_bytes);

/* Sionna / Mitsuba scene (scene.xml, the PLY files it names, optional scene.csv) -> Scene, the job of
 * the reference's importer tool (src/scene_fromSionna.c:103-488) as a library call.  `out` is
 * filled with malloc()ed meshes (release with free_scene); the file names box.xml and
 * simple_reflector.xml select the two built-in scenes.  See csrc/host/sionna_import.c for the
 * accepted formats.  CLI: lib/hrt_import_sionna. */
int hrt_scene_import_sionna(const char *xml_path, Scene *out);

/* Device self test: evaluates on the GPU, over n host floats, one of the float libm
 * restatements the shading code uses -- fn 0 sinf, 1 cosf, 2 expf, 3 acosf (csrc/hrt_libm.h)
 * -- or, fn 4, the incidence angle of src/compute_paths.c:281-283 for dot(n, d) = in[i]
 * ((float)acos((double)x) folded to [0, pi/2]); fn 5 / 6 the sine / cosine of the fused
 * hrt_sincosf and fn 7 hrt_cosf_nb (the branch-free forms the shade kernel calls).  Tests compare
 * the result with the host libm.
 * fn 8 .. 10 evaluate primitives of the patch-mask and record kernels on items of K floats, n / K items,
 * floats [K i, K i + K) of `in` and of `out` belonging to item i (64 consecutive items share a wave):
 * fn 8, K = 8: the bitwise OR over the wave of the item's eight 32-bit words (carried as float bits);
 * fn 9, K = 1: in / c, c the float speed of light; fn 10, K = 4: (s, alpha, theta_s, theta_i) -> the
 * four scattering pattern terms of src/compute_paths.c:359-415.
 * fn 11, K = 168: the triangle walk of the trace and record kernels over rows given inline.  Item = o[3], d[3],
 * kind (u32 bits: 0 primary, 2 shadow, other: a lane without a ray), T <= 8 (u32 bits), eight rows of 20 floats
 * (v1, e1, e2 in the first nine words, the row's original index as the bits of the last; rows past T all zero).
 * out[K i] = bits of the closest row (0xffffffff: none), out[K i + 1] = the bits of its distance (kind 0) or
 * 1 / 0 for "distance <= 1" (kind 2); the rest of the item's output is zero. */
int hrt_selftest_math(int device, int fn, const float *in, float *out, uint64_t n);

/* Diagnostic counters of the trace kernel; all zero unless the library was built with
 * `make STATS=1`.  out48 = [3 kinds][16]: kind 0 primary traces of launch 0, 1 primary traces
 * of later launches, 2 shadow traces; columns: 0 wave-traces, 1 packets usable as a whole,
 * 2 candidate triangles after packet culling, 3 / 4 / 5 staged bodies reaching stage 2, stage 3,
 * the exact divisions, 6 (sub-)packets walked [flat: heavy packets], 7 packet-culling rounds of near
 * leaves [flat: candidates of heavy packets], 8 sphere-node rounds, 9 plane-node rounds, 10 plane
 * leaves judged, 11 of them with flagged triangles, 12 flagged triangles, 13 / 14 the longest and the total
 * duration of a wave-trace of hrt_trace_kernel in shader clocks, 15 of the staged bodies of column 5 those in
 * which every lane still in play held the certain-hit certificate (no u, v division). */
int hrt_debug_kernel_stats(int device, uint64_t *out48, int reset);

/* TEST ONLY -- a lane's own candidate lookup, for tests/test_gpu_candidates.py.  Every kernel that traces a ray on
 * tables of at most 256 triangles takes its candidates from bit masks built once per problem (csrc/hrt_kparams.h:
 * hrt_kpatch, hrt_krxt) and walks the UNION over its wave; this entry returns what ONE lane looks up, before any
 * union and without a walk, through the device functions the hot kernels call (patch_fetch, patch_locate, patch_load,
 * txcell_load, rxt_inside, rxt_cell_load).  One query per lane of one small kernel:
 *   in  [n][8]   origin xyz, direction xyz, table row (u32 bits), apex (u32 bits)
 *   out [n][10]  served (0 / 1), patch index, 8 mask words (bit j of word k = table row 32 k + j); all zero words
 *                and patch index 0 when not served
 *   mode 0  apex = RX k     the patch table of `row` for shadow rays to RX k (the direction is not used)
 *   mode 1  apex = TX t     the patch table of `row` for the image of TX t; the direction enters the line test
 *   mode 2  apex = TX t     the TX cell mask of launch 0 (origin and row are not used)
 *   mode 3  apex = RX k or num_rx + t: the per-cell mask on tables of at most 64 triangles (words 0, 1);
 *           served = the origin lies inside the region ball (a hot lane outside it asks for the whole table)
 * An apex past the tables is not served.  HRT_E_INVALID, nothing launched: the problem has no table for the mode;
 * mode outside 0 .. 3; NULL pointers; n > 2^26.  Host arrays; blocks until done. */
int hrt_debug_candidates(const hrt_problem *p, int mode, uint64_t n, const float *in, uint32_t *out);
/* TEST ONLY -- what the candidate tables were built with: nuv [T][2] the grid of every table row as the kernels
 * read it (0 0 = not served), {hmax, ro_rx, ro_img}, the number of patches (patch indices of row j:
 * [base_j, base_j + nu nv), base_j = the sum over the rows before it), kinds = bit 0 patch tables, bit 1 their
 * image-apex part, bit 2 TX cell masks, bit 3 per-cell masks (tables of at most 64 triangles). */
int hrt_debug_table_info(const hrt_problem *p, uint32_t *nuv, float *hmax_ro_rx_ro_img, uint64_t *num_patch,
                         uint32_t *kinds);

/* TEST ONLY -- the last launch of a trace alone, for tests/test_gpu_records_planted.py.  With nb = s->num_bounces,
 * launch nb traces the shadow rays of the entries of hit block nb - 1 and writes their scatter records (record block
 * and mask block nb - 1); it has no primary rays.  The caller plants hit block nb - 1 and counts[nb] (the number of its
 * entries) in the workspace; this entry runs launch nb on them with hrt_trace's own kernel parameters and launch shims:
 * hrt_records_kernel where the launch plan gives it the records (patch tables), else hrt_trace_kernel (shadow units)
 * followed by hrt_shade_kernel<.., true>.  It never runs the fused kernel or the chain kernel: where hrt_trace would
 * fuse launch nb, the trace + shade pair runs instead.  Before the launch it zeroes what hrt_trace has zeroed or
 * produced by then and launch nb reads -- the error word counts[nb + 1] and every control word between it and the LoS
 * entries (unit counters, survivor counts, status words); counts[0 .. nb], the LoS entries and the hit, record and mask
 * blocks are left alone (the trace + shade pair also writes the shadow result scratch behind the mask blocks).
 * HRT_E_INVALID, nothing launched: NULL arguments, a bad shard (num_bounces = 0 included), a workspace that is too
 * small or not 256-byte aligned, counts[nb] > cap.  Default stream; blocks until done. */
int hrt_debug_last_launch(const hrt_problem *p, const hrt_shard *s, void *d_workspace, uint64_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* HRT_DEVICE_H */
