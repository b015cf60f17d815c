// hrt_dominant.hip -- the K strongest paths per link (hrt_dominant_paths) from the workspace of a finished hrt_trace,
// for gfx950.  The order, the candidates and the scratch are csrc/hrt_dominant.h; the workspace view and its readers
// csrc/hrt_pathsum.h; the TX segments of the hit blocks come from hrt_channel_segments_kernel (csrc/hrt_channel.hip).
//   hrt_dominant_partial_kernel  one workgroup per (record chunk, link): every lane tests its records' mask bits,
//                                reads the four amplitude fields (16 B per record) and forms the FP64 power; a
//                                record that beats the K-th key so far goes to the pending slots in LDS.
//   hrt_dominant_merge_kernel    one workgroup per (HRT_DM_FANIN chunk lists, link): the first K of their union.
//   hrt_dominant_final_kernel    one workgroup per link, one thread per output slot: the first K of the remaining
//                                lists, the LoS entry (shard rank 0) and, when accumulating, the records the output
//                                holds; then the 72-byte records of the winners (tau, nu, directions and the FP64
//                                launch direction for K records, not for every record), the zero tail, the header.
// All three keep HRT_DM_SLOTS candidates in LDS: the K kept so far, sorted, then the pending ones.  When the pending
// slots could overflow in the next step the workgroup sorts the used slots (bitonic, 128-bit keys) and keeps the first K.
// The keys of distinct terms are distinct, so what is kept is a function of the set of terms offered, not of the
// order the (integer, LDS) atomic counter hands the pending slots out in: two calls give the same bits, and shards
// or batches merged in any order give the unsharded bytes.  No floating-point atomics, no waits but barriers.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_dominant.h"
#include "hrt_pathsum.h"

static_assert(sizeof(hrt_dominant_path) == 72 && sizeof(hrt_dm_cand) == 24, "hrt_dominant_path / hrt_dm_cand");
static_assert(HRT_DM_MAX_PATHS + HRT_DM_FINAL_THREADS <= HRT_DM_SLOTS, "one step of pending candidates must fit");

namespace {

constexpr uint32_t N = HRT_DM_SLOTS;
constexpr uint64_t PATH_MASK = (1ull << HRT_DM_PATH_BITS) - 1ull;

// the LDS of a workgroup: N candidates (hi 0: empty), the pending count and the K-th key so far
struct dm_lds {
    uint64_t *hi, *lo;
    uint32_t *ix, *cnt;
    uint64_t *thr;
};

#define DM_LDS(S)                                                                                                      \
    __shared__ uint64_t sHi[N], sLo[N], sThr[2];                                                                       \
    __shared__ uint32_t sIx[N], sCnt;                                                                                  \
    const dm_lds S = {sHi, sLo, sIx, &sCnt, sThr}

__device__ __forceinline__ bool key_gt(uint64_t ah, uint64_t al, uint64_t bh, uint64_t bl)
{
    return ah > bh || (ah == bh && al > bl);
}

__device__ __forceinline__ uint64_t key_lo(int32_t bounce, uint64_t path)
{
    return ~(((uint64_t)(uint32_t)(bounce + 1) << HRT_DM_PATH_BITS) | (path & PATH_MASK));
}

// every product of two floats is exact in FP64: the value does not depend on contraction
__device__ __forceinline__ double term_power(float ter, float tei, float tmr, float tmi)
{
#pragma clang fp contract(off)
    return ((double)ter * ter + (double)tei * tei) + ((double)tmr * tmr + (double)tmi * tmi);
}

__device__ __forceinline__ uint64_t key_hi(double power)
{
    return (uint64_t)__double_as_longlong(power) + 1ull;
}

template <uint32_t NT>
__device__ __forceinline__ void dm_init(const dm_lds &S, uint32_t tid)
{
    for (uint32_t t = tid; t < N; t += NT) S.hi[t] = 0ull;
    if (tid == 0) {
        *S.cnt = 0u;
        S.thr[0] = S.thr[1] = 0ull;
    }
    __syncthreads();
}

// a candidate into the next pending slot (dm_room has made sure there is one)
__device__ __forceinline__ void dm_push(const dm_lds &S, uint32_t K, uint64_t hi, uint64_t lo, uint32_t ix)
{
    const uint32_t q = K + atomicAdd(S.cnt, 1u);
    S.hi[q] = hi;
    S.lo[q] = lo;
    S.ix[q] = ix;
}

// the K kept and the pending candidates sorted, largest key first (empty slots last); the first K stay.  The
// network spans the least power of two that holds them (the slots behind the pending ones are empty).
template <uint32_t NT>
__device__ void dm_flush(const dm_lds &S, uint32_t K, uint32_t tid)
{
    __syncthreads();
    const uint32_t used = K + *S.cnt;   // (the counter is reset behind the barriers of the network)
    uint32_t n = 2u;
    while (n < used) n <<= 1;
    for (uint32_t k = 2u; k <= n; k <<= 1)
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            for (uint32_t t = tid; t < n / 2u; t += NT) {
                const uint32_t a = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), b = a | j;
                const uint64_t ah = S.hi[a], al = S.lo[a], bh = S.hi[b], bl = S.lo[b];
                const bool swap = (a & k) ? key_gt(ah, al, bh, bl) : key_gt(bh, bl, ah, al);
                if (swap) {
                    const uint32_t ai = S.ix[a], bi = S.ix[b];
                    S.hi[a] = bh; S.lo[a] = bl; S.ix[a] = bi;
                    S.hi[b] = ah; S.lo[b] = al; S.ix[b] = ai;
                }
            }
            __syncthreads();
        }
    for (uint32_t t = K + tid; t < n; t += NT) S.hi[t] = 0ull;
    if (tid == 0) {
        *S.cnt = 0u;
        S.thr[0] = S.hi[K - 1u];
        S.thr[1] = S.lo[K - 1u];
    }
    __syncthreads();
}

// room for `need` more pending candidates (need <= N - K); every thread takes the same decision
template <uint32_t NT>
__device__ __forceinline__ void dm_room(const dm_lds &S, uint32_t K, uint32_t need, uint32_t tid)
{
    __syncthreads();
    const uint32_t c = *S.cnt;
    __syncthreads();
    if (c + need > N - K) dm_flush<NT>(S, K, tid);
}

// offer the n candidates at src (empty ones are skipped)
template <uint32_t NT>
__device__ void dm_stream(const dm_lds &S, const hrt_dm_cand *src, uint32_t n, uint32_t K, uint32_t tid)
{
    for (uint32_t base = 0; base < n; base += NT) {
        dm_room<NT>(S, K, NT, tid);
        const uint32_t q = base + tid;
        if (q < n) {
            const hrt_dm_cand c = src[q];
            if (c.hi && key_gt(c.hi, c.lo, S.thr[0], S.thr[1])) dm_push(S, K, c.hi, c.lo, c.ix);
        }
    }
}

template <uint32_t NT>
__device__ __forceinline__ void dm_store(const dm_lds &S, hrt_dm_cand *dst, uint32_t K, uint32_t tid)
{
    for (uint32_t t = tid; t < K; t += NT) dst[t] = hrt_dm_cand{S.hi[t], S.lo[t], S.ix[t], 0u};
}

}  // namespace

__global__ void __launch_bounds__(HRT_DM_THREADS) hrt_dominant_partial_kernel(const hrt_kdominant D)
{
    constexpr uint32_t NT = HRT_DM_THREADS;
    const hrt_kview &V = D.v;
    const uint32_t c = blockIdx.x, link = blockIdx.y, K = D.K;
    const uint32_t rx = link / V.ntx, tx = link % V.ntx;
    const uint32_t tid = threadIdx.x;
    DM_LDS(S);
    __shared__ uint32_t sTotal;
    if (tid == 0) sTotal = 0u;
    dm_init<NT>(S, tid);

    uint32_t count = 0;
    for (uint32_t b = 0; b < V.nb; ++b) {
        uint32_t start, end;
        chunk_range(V, b, tx, c, start, end);
        const uint64_t *mask = mask_row(V, b, rx);
        const float *ter = rec_field(V, b, rx, HRT_REC_A_TE_RE), *tei = rec_field(V, b, rx, HRT_REC_A_TE_IM);
        const float *tmr = rec_field(V, b, rx, HRT_REC_A_TM_RE), *tmi = rec_field(V, b, rx, HRT_REC_A_TM_IM);
        const uint32_t *ray = hit_field(V, b, HRT_HIT_RAY);
        for (uint32_t base = start; base < end; base += 2u * NT) {
            dm_room<NT>(S, K, 2u * NT, tid);
            const uint64_t th = S.thr[0], tl = S.thr[1];
#pragma unroll
            for (uint32_t r = 0; r < 2u; ++r) {
                const uint32_t i = base + r * NT + tid;
                if (i >= end || !((mask[i >> 6] >> (i & 63u)) & 1u)) continue;
                ++count;
                const uint64_t hi = key_hi(term_power(ter[i], tei[i], tmr[i], tmi[i]));
                if (hi < th) continue;
                const uint64_t path = hrt_shard_path(ray[i] - tx * V.num_local, D.sh.chunk, D.sh.count, D.sh.rank);
                const uint64_t lo = key_lo((int32_t)b, path);
                if (key_gt(hi, lo, th, tl)) dm_push(S, K, hi, lo, i);
            }
        }
    }
    dm_flush<NT>(S, K, tid);
    dm_store<NT>(S, D.la + ((uint64_t)link * V.nchunks + c) * K, K, tid);
    if (count) atomicAdd(&sTotal, count);
    __syncthreads();
    if (tid == 0) D.ca[(uint64_t)link * V.nchunks + c] = sTotal;
}

__global__ void __launch_bounds__(HRT_DM_THREADS) hrt_dominant_merge_kernel(const hrt_kdominant D)
{
    constexpr uint32_t NT = HRT_DM_THREADS;
    const hrt_kview &V = D.v;
    const uint32_t m = blockIdx.x, link = blockIdx.y, K = D.K, tid = threadIdx.x;
    const uint32_t l0 = m * HRT_DM_FANIN, l1 = min(l0 + HRT_DM_FANIN, V.nchunks);
    DM_LDS(S);
    dm_init<NT>(S, tid);
    dm_stream<NT>(S, D.la + ((uint64_t)link * V.nchunks + l0) * K, (l1 - l0) * K, K, tid);
    dm_flush<NT>(S, K, tid);
    dm_store<NT>(S, D.lb + ((uint64_t)link * D.nmid + m) * K, K, tid);
    if (tid == 0) {
        uint64_t n = 0;
        for (uint32_t l = l0; l < l1; ++l) n += D.ca[(uint64_t)link * V.nchunks + l];
        D.cb[(uint64_t)link * D.nmid + m] = n;
    }
}

__global__ void __launch_bounds__(HRT_DM_FINAL_THREADS) hrt_dominant_final_kernel(const hrt_kdominant D)
{
    constexpr uint32_t NT = HRT_DM_FINAL_THREADS;
    const hrt_kview &V = D.v;
    const uint32_t link = blockIdx.x, K = D.K, tid = threadIdx.x;
    const uint32_t rx = link / V.ntx, tx = link % V.ntx;
    const uint64_t links = (uint64_t)V.nrx * V.ntx;
    uint64_t *hdr = reinterpret_cast<uint64_t *>(D.out) + 2u * (uint64_t)link;
    hrt_dominant_path *recs = reinterpret_cast<hrt_dominant_path *>(D.out + 16u * links) + (uint64_t)link * K;
    DM_LDS(S);
    __shared__ uint32_t sKept;
    if (tid == 0) sKept = 0u;

    // what the output holds (read before anything of it is written: the barriers of dm_init and below)
    uint32_t kept_old = 0;
    uint64_t eligible = 0;
    if (V.accumulate) {
        const uint64_t k0 = hdr[0];
        kept_old = k0 < K ? (uint32_t)k0 : K;
        eligible = hdr[1];
    }
    dm_init<NT>(S, tid);
    if (V.accumulate) {
        if (tid < kept_old) {
            const hrt_dominant_path &o = recs[tid];
            dm_push(S, K, key_hi(o.power), key_lo(o.bounce, o.path), HRT_DM_IX_OLD | tid);
        }
        dm_flush<NT>(S, K, tid);
    }
    hrt_los_entry le;
    const bool los = V.los && los_entry(V, link, le);
    if (los) {
        ++eligible;
        if (tid == 0) dm_push(S, K, key_hi(term_power(le.a, 0.f, le.a, 0.f)), key_lo(-1, ~0ull), HRT_DM_IX_LOS);
    }
    const uint32_t nlists = D.nmid ? D.nmid : V.nchunks;
    const hrt_dm_cand *lists = (D.nmid ? D.lb : D.la) + (uint64_t)link * nlists * K;
    const uint64_t *cnts = (D.nmid ? D.cb : D.ca) + (uint64_t)link * nlists;
    dm_stream<NT>(S, lists, nlists * K, K, tid);
    dm_flush<NT>(S, K, tid);
    for (uint32_t l = 0; l < nlists; ++l) eligible += cnts[l];

    // the record of this thread's slot, in registers: a winner may be a record another slot of the output holds
    union {
        hrt_dominant_path p;
        uint64_t w[9];
    } R;
#pragma unroll
    for (int q = 0; q < 9; ++q) R.w[q] = 0ull;
    const bool valid = tid < K && S.hi[tid] != 0ull;
    if (valid) {
        const uint64_t hi = S.hi[tid], tie = ~S.lo[tid];
        const uint32_t ix = S.ix[tid];
        if (tid + 1u == K || S.hi[tid + 1u] == 0ull) sKept = tid + 1u;
        if (ix == HRT_DM_IX_LOS) {
            R.p.power = __longlong_as_double((long long)(hi - 1ull));
            R.p.path = UINT64_MAX;
            R.p.bounce = -1;
            R.p.tri = UINT32_MAX;
            R.p.a_te_re = le.a; R.p.a_te_im = 0.f; R.p.a_tm_re = le.a; R.p.a_tm_im = 0.f;
            R.p.tau = le.tau;
            R.p.freq_shift = le.nu;
            R.p.u_tx[0] = le.ux; R.p.u_tx[1] = le.uy; R.p.u_tx[2] = le.uz;
            R.p.u_rx[0] = -le.ux; R.p.u_rx[1] = -le.uy; R.p.u_rx[2] = -le.uz;
        } else if (ix & HRT_DM_IX_OLD) {
            const uint64_t *src = reinterpret_cast<const uint64_t *>(recs + (ix & ~HRT_DM_IX_OLD));
#pragma unroll
            for (int q = 0; q < 9; ++q) R.w[q] = src[q];
        } else {
            const uint32_t b = (uint32_t)(tie >> HRT_DM_PATH_BITS) - 1u;
            float F[HRT_PS_REC_FLOATS];
            stage_record(V, D.sh, b, rx, tx, ix, F);
            R.p.power = __longlong_as_double((long long)(hi - 1ull));
            R.p.path = tie & PATH_MASK;
            R.p.bounce = (int32_t)b;
            R.p.tri = hit_field(V, b, HRT_HIT_TRI)[ix];
            R.p.a_te_re = F[0]; R.p.a_te_im = F[1]; R.p.a_tm_re = F[2]; R.p.a_tm_im = F[3];
            R.p.tau = F[4];
            R.p.freq_shift = F[5];
            for (int q = 0; q < 3; ++q) {
                R.p.u_rx[q] = F[6 + q];
                R.p.u_tx[q] = F[9 + q];
            }
        }
    }
    __syncthreads();
    if (tid < K) {
        uint64_t *dst = reinterpret_cast<uint64_t *>(recs + tid);
#pragma unroll
        for (int q = 0; q < 9; ++q) dst[q] = R.w[q];
    }
    if (tid == 0) {
        hdr[0] = sKept;
        hdr[1] = eligible;
    }
}

extern "C" int hrt_hip_launch_dominant(const hrt_kdominant *D, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint32_t links = D->v.nrx * D->v.ntx;
    if (D->v.nchunks) {
        const int e = hrt_hip_launch_segments(&D->v, stream);
        if (e) return e;
        hipLaunchKernelGGL(hrt_dominant_partial_kernel, dim3(D->v.nchunks, links), dim3(HRT_DM_THREADS), 0, st, *D);
        if (D->nmid)
            hipLaunchKernelGGL(hrt_dominant_merge_kernel, dim3(D->nmid, links), dim3(HRT_DM_THREADS), 0, st, *D);
    }
    hipLaunchKernelGGL(hrt_dominant_final_kernel, dim3(links), dim3(HRT_DM_FINAL_THREADS), 0, st, *D);
    return (int)hipGetLastError();
}
