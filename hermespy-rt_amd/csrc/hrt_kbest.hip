// hrt_kbest.hip -- per-point K-best tree-search MIMO detection with list max-log bit LLRs on an array channel, for
// gfx950: near-ML detection where the Q = M^Nt hypotheses of hrt_detect.hip are too many to score.
//
//     [H | y] = Q [R | z] (modified Gram-Schmidt, optionally sorted), rho = |y - Q z|^2
//     level i = Nt - 1 .. 0:  PED' = PED + |z_i - sum_{t > i} R_it s_t - R_ii s|^2, the K smallest survive
//     llr[j][b] = clamp((min over the list's leaves with bit 0 - min over those with bit 1) / N0)
//
// The lane groups, the LDS image, the order of every sum and the selection network are csrc/hrt_kbest.h's; the
// arithmetic is hermespy_rt.h's (hrt_kbest_spec).  One kernel, instantiated per group size G:
//   stage in   every thread clears its matrix words; after a barrier the workgroup loads [H | y] of its
//              HRT_KB_THREADS / G points with the point index fastest and writes each entry to its owner's word.
//   factor     the column norms (largest of H's: the null threshold; a sum that is not finite flags the point), then
//              per position the pick (sorted: the smallest recomputed residual norm, the lowest stream on a tie), the
//              scale and the projections of every stream not yet picked, ascending, and of y.  A null column leaves a
//              zero row.  Lane 0 of the group writes R and z; the order is a nibble per position in a register pair.
//   tree       a lane is a survivor (PED, key).  Per level: b once, then M children; a batch (one symbol across the
//              group) is bitonic-sorted descending and merged into the running best K; a batch that cannot enter the
//              list is skipped on a wave-uniform ballot.
//   end        the list is sorted: lane 0 holds the decision.  Per bit position the two minima are butterflies over the
//              group; a first pass finds whether any quotient is not finite, a second forms, clamps and stores.
// Every thread runs every step (a group beyond the last point works on zeros and stores nothing), so the barriers and
// ballots are uniform.  Shuffles stay inside a group and a word of LDS belongs to one point, so a point's bytes depend
// on its own H and y only.  No atomics, no scratch, vector stores only.
#include <hip/hip_runtime.h>

#include <float.h>
#include <stdint.h>

#include "hermespy_rt.h"
#include "hrt_kbest.h"

#define EQ_T HRT_KB_THREADS

// reduce, from-lane, norm^2, dot, scale and project on a lane's rows: shared with the equalizer and the precoder
#include "hrt_mgs.inc"

// (PED, key) order: the smaller PED, the lower key on a tie
__device__ __forceinline__ bool kb_less(float ap, uint32_t ak, float bp, uint32_t bk)
{
    return ap < bp || (ap == bp && ak < bk);
}

// compare-exchange with lane ^ j: keep the smaller of the two (min) or the larger
template <uint32_t G>
__device__ __forceinline__ void kb_cx(float &p, uint32_t &k, uint32_t j, bool min)
{
    const float op = __shfl_xor(p, (int)j, 64);
    const uint32_t ok = (uint32_t)__shfl_xor((int)k, (int)j, 64);
    const bool take = min ? kb_less(op, ok, p, k) : kb_less(p, k, op, ok);
    p = take ? op : p;
    k = take ? ok : k;
}

__device__ __forceinline__ float kb_min(float a, float b) { return b < a ? b : a; }

template <uint32_t G>
__device__ __forceinline__ float kb_group_min(float v)
{
#pragma unroll
    for (uint32_t off = 1u; off < G; off *= 2u) v = kb_min(v, __shfl_xor(v, (int)off, 64));
    return v;
}

template <uint32_t G>
__global__ void __launch_bounds__(HRT_KB_THREADS)
hrt_kbest_kernel(const hrt_kkbest P, const float2 *__restrict__ H, const float2 *__restrict__ Y,
                 const float2 *__restrict__ S)
{
    __shared__ float sM[HRT_KB_WORDS * EQ_T];
    __shared__ float2 sS[HRT_KB_MAX_M];
    constexpr uint32_t PPB = EQ_T / G;

    const uint32_t tid = threadIdx.x, l = tid % G, sp_own = tid / G;
    const uint32_t nr = P.nr, nt = P.nt, n = nt + 1u, mk = P.mk, B = P.b, M = 1u << B, nb = nt * B, K = P.k;
    const uint64_t pt0 = (uint64_t)blockIdx.x * PPB, pt_own = pt0 + sp_own;
    float *const wA = sM + tid;                                         // this lane's matrix words
    float *const pw = sM + mk * n * 2u * EQ_T + sp_own * G;             // the point's words: word w at pw[(w / G) EQ_T + w % G]
#define KB_PW(w) pw[((w) / G) * EQ_T + (w) % G]

    // ---- stage in
    for (uint32_t x = tid; x < M; x += EQ_T) sS[x] = S[x];
    for (uint32_t e = 0; e < mk * n * 2u; ++e) wA[e * EQ_T] = 0.f;
    __syncthreads();
    for (uint32_t w = tid; w < nr * n * PPB; w += EQ_T) {
        const uint32_t sp = w % PPB, e = w / PPB, i = e / n, j = e % n;
        const uint64_t pt = pt0 + sp;
        if (pt >= P.points) continue;
        const uint64_t link = pt / P.pts, q = pt % P.pts;
        const float2 h = j < nt ? H[((link * nr + i) * nt + j) * P.pts + q] : Y[(link * nr + i) * P.pts + q];
        float *x = sM + (((i / G) * n + j) * 2u) * EQ_T + sp * G + i % G;
        x[0] = h.x;
        x[EQ_T] = h.y;
    }
    __syncthreads();

    // ---- factor: the column norms first
    float nmax = 0.f, nsum = 0.f;
    for (uint32_t c = 0; c < n; ++c) {
        const float a = eq_reduce<G>(eq_lane_norm2(wA, c, mk, n));
        if (c < nt) nmax = a > nmax ? a : nmax;
        nsum = nsum + a;
    }
    bool bad = !(nsum <= FLT_MAX);
    const float thr = ((float)(nr + nt) * 0x1p-23f) * sqrtf(nmax);
    bool deficient = false;
    uint64_t order = 0u;                    // nibble t: the stream at position t
    uint32_t chosen = 0u;
    for (uint32_t t = 0; t < nt; ++t) {
        uint32_t c = t;
        float a = 0.f;
        if (P.sorted) {
            bool first = true;
            for (uint32_t u = 0; u < nt; ++u) {
                if ((chosen >> u) & 1u) continue;
                const float au = eq_reduce<G>(eq_lane_norm2(wA, u, mk, n));
                if (first || au < a) {
                    a = au;
                    c = u;
                }
                first = false;
            }
        } else {
            a = eq_reduce<G>(eq_lane_norm2(wA, c, mk, n));
        }
        chosen |= 1u << c;
        order |= (uint64_t)c << (4u * t);
        const float r = sqrtf(a);
        const bool null = !(r > thr);
        deficient = deficient || null;
        if (!null) eq_scale(wA, c, mk, n, r);
        for (uint32_t u = 0; u < n; ++u) {
            if (u < nt && ((chosen >> u) & 1u)) continue;
            float rr = 0.f, ri = 0.f;
            if (!null) {
                eq_lane_dot(wA, c, u, mk, n, rr, ri);
                rr = eq_reduce<G>(rr);
                ri = eq_reduce<G>(ri);
                eq_project(wA, c, u, mk, n, rr, ri);
            }
            if (l == 0u) {
                const uint32_t w = (u < nt ? t * nt + u : nt * nt + t) * 2u;
                KB_PW(w) = rr;
                KB_PW(w + 1u) = ri;
            }
        }
        if (l == 0u) {
            const uint32_t w = (t * nt + c) * 2u;
            KB_PW(w) = null ? 0.f : r;
            KB_PW(w + 1u) = 0.f;
        }
    }
    const float rho = eq_reduce<G>(eq_lane_norm2(wA, nt, mk, n));
    bad = bad || !(rho <= FLT_MAX);
    __syncthreads();

    // ---- tree: a lane is a survivor
    const bool live = pt_own < P.points;
    float ped = l == 0u ? rho : INFINITY;
    uint32_t key = l == 0u ? 0u : 0xffffffffu;
    for (uint32_t i = nt; i-- > 0u;) {
        const uint32_t c = (uint32_t)(order >> (4u * i)) & 15u;
        const float rii = KB_PW((i * nt + c) * 2u);
        float br = 0.f, bi = 0.f;
        for (uint32_t t = i + 1u; t < nt; ++t) {
            const uint32_t u = (uint32_t)(order >> (4u * t)) & 15u;
            const float xr = KB_PW((i * nt + u) * 2u), xi = KB_PW((i * nt + u) * 2u + 1u);
            const float2 s = sS[(key >> (u * B)) & (M - 1u)];
            const float pr = xr * s.x - xi * s.y, pi = xr * s.y + xi * s.x;
            br = t == i + 1u ? pr : br + pr;
            bi = t == i + 1u ? pi : bi + pi;
        }
        const float zr = KB_PW((nt * nt + i) * 2u), zi = KB_PW((nt * nt + i) * 2u + 1u);
        if (i + 1u < nt) {
            br = zr - br;
            bi = zi - bi;
        } else {
            br = zr;
            bi = zi;
        }
        const bool valid = ped <= FLT_MAX;
        float bp = INFINITY;                // the running best of this level, ascending over the group
        uint32_t bk = 0xffffffffu;
        for (uint32_t x = 0; x < M; ++x) {
            const float2 s = sS[x];
            const float er = br - rii * s.x, ei = bi - rii * s.y;
            float cp = valid ? ped + (er * er + ei * ei) : INFINITY;
            uint32_t ck = valid ? key | (x << (c * B)) : 0xffffffffu;
            bad = bad || (valid && !(cp <= FLT_MAX));
            if (P.skip) {
                const float kth = eq_from<G>(bp, K - 1u);
                if (__ballot(live && valid && !(cp > kth)) == 0ull) continue;
            }
            // the batch, descending
#pragma unroll
            for (uint32_t k = 2u; k <= G; k <<= 1) {
#pragma unroll
                for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
                    const bool down = (l & k) == 0u || k == G, lower = (l & j) == 0u;
                    kb_cx<G>(cp, ck, j, lower != down);
                }
            }
            if (kb_less(cp, ck, bp, bk)) {
                bp = cp;
                bk = ck;
            }
#pragma unroll
            for (uint32_t j = G >> 1; j > 0u; j >>= 1) kb_cx<G>(bp, bk, j, (l & j) == 0u);
            if (l >= K) {
                bp = INFINITY;
                bk = 0xffffffffu;
            }
        }
        ped = bp;
        key = bk;
    }

    // ---- end: the list is sorted, lane 0 holds the decision
    const float dm = eq_from<G>(ped, 0u);
    const uint32_t dq = (uint32_t)__shfl((int)key, 0, (int)G);
    const bool llr = P.llr != 0u;
    const bool leaf = ped <= FLT_MAX;
    if (llr) {
        for (uint32_t p = 0; p < nb; ++p) {
            const bool one = (key >> p) & 1u;
            const float m0 = kb_group_min<G>(leaf && !one ? ped : INFINITY);
            const float m1 = kb_group_min<G>(leaf && one ? ped : INFINITY);
            if (m0 <= FLT_MAX && m1 <= FLT_MAX) bad = bad || !(fabsf((m0 - m1) / P.n0) <= FLT_MAX);
        }
    }
    // (bad is group-uniform but for the children's test, which a lane makes on its own children)
    if constexpr (G == 64u) bad = __ballot(bad) != 0ull;
    else bad = ((__ballot(bad) >> ((tid % 64u) / G * G)) & ((1ull << G) - 1ull)) != 0ull;

    const uint32_t pt = (uint32_t)pt_own;
    const uint32_t status = bad ? HRT_KB_NONFINITE : deficient ? HRT_KB_DEFICIENT : 0u;
    uint32_t *const o = reinterpret_cast<uint32_t *>(P.out);
    if (live && l == 0u) {
        o[pt] = bad ? 0xffffffffu : dq;
        reinterpret_cast<float *>(o)[(uint64_t)P.points + pt] = bad ? 0.f : dm;
        o[2ull * P.points + pt] = status;
    }
    if (llr) {
        const uint32_t link = pt / P.pts, rem = pt % P.pts;
        float *const L = reinterpret_cast<float *>(o) + 3ull * P.points;
        for (uint32_t p = 0; p < nb; ++p) {
            const bool one = (key >> p) & 1u;
            const float m0 = kb_group_min<G>(leaf && !one ? ped : INFINITY);
            const float m1 = kb_group_min<G>(leaf && one ? ped : INFINITY);
            float v;
            if (!(m0 <= FLT_MAX)) v = P.clip;           // no leaf with bit 0: the decision's bit is 1
            else if (!(m1 <= FLT_MAX)) v = -P.clip;
            else {
                v = (m0 - m1) / P.n0;
                v = v > P.clip ? P.clip : v;
                v = v < -P.clip ? -P.clip : v;
            }
            // position p = j B + (B - 1 - b) is written at llr[link][j][b][rem]
            const uint32_t j = p / B, b = B - 1u - p % B;
            if (live && l == p % G) L[(((uint64_t)link * nt + j) * B + b) * P.pts + rem] = bad ? 0.f : v;
        }
    }
#undef KB_PW
}

extern "C" int hrt_hip_launch_kbest(const hrt_kkbest *P, const void *H, const void *Y, const void *S, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const float2 *h = (const float2 *)H, *y = (const float2 *)Y, *s = (const float2 *)S;
    const uint32_t g = P->g;
    if (g == 0u || g != hrt_kbest_form(P->nr, P->nt, P->k) || P->mk != (P->nr + g - 1u) / g || P->b < 1u
        || P->b > HRT_KB_MAX_B || P->nt * P->b > HRT_KB_MAX_BITS || P->points == 0u || P->pts == 0u)
        return (int)hipErrorInvalidValue;
    const uint32_t ppb = HRT_KB_THREADS / g;
    const dim3 grid((P->points + ppb - 1u) / ppb), block(HRT_KB_THREADS);
    switch (g) {
    case 1u: hipLaunchKernelGGL(hrt_kbest_kernel<1u>, grid, block, 0, st, *P, h, y, s); break;
    case 2u: hipLaunchKernelGGL(hrt_kbest_kernel<2u>, grid, block, 0, st, *P, h, y, s); break;
    case 4u: hipLaunchKernelGGL(hrt_kbest_kernel<4u>, grid, block, 0, st, *P, h, y, s); break;
    case 8u: hipLaunchKernelGGL(hrt_kbest_kernel<8u>, grid, block, 0, st, *P, h, y, s); break;
    case 16u: hipLaunchKernelGGL(hrt_kbest_kernel<16u>, grid, block, 0, st, *P, h, y, s); break;
    case 32u: hipLaunchKernelGGL(hrt_kbest_kernel<32u>, grid, block, 0, st, *P, h, y, s); break;
    case 64u: hipLaunchKernelGGL(hrt_kbest_kernel<64u>, grid, block, 0, st, *P, h, y, s); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
