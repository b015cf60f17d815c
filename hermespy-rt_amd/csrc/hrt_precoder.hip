// hrt_precoder.hip -- per-point linear MIMO precoders (MRT, ZF, RZF) of the array channel and the downlink SINR of every
// stream behind them, for gfx950: many small independent problems, direct (a triangular factorisation, no iteration).
//
//     P0 = H^H | H^H (H H^H)^-1 | H^H (H H^H + alpha I)^-1,   P = P0 scaled to the power,
//     E = H P,   sinr_i = |E_ii|^2 / (sum_{j != i} |E_ij|^2 + N0)
//
// Modified Gram-Schmidt in float on A = [H^H; sqrt(alpha) I] = Q R: the equalizer's factorisation with the sides swapped
// (csrc/hrt_precoder.h; the loops are csrc/hrt_mgs.inc, shared with csrc/hrt_equalizer.hip).  One kernel, instantiated
// per group size G:
//   stage in   every thread clears its own words and sets its rows of T = I; after a barrier the workgroup loads the
//              entries of its HRT_PC_THREADS / G points with the point index fastest and writes conj(H[i][t]) to the
//              owner of row t, column i.
//   start      the squared column norms of A, |row i of H|^2 + alpha: their largest sets the singular threshold
//              thr = (Nr + Nt) 2^-23 sqrt(largest); a sum that is not finite flags the point HRT_PC_NONFINITE.
//   factor     (ZF, RZF) the equalizer's column operations, on the top block and on T alike.
//   weights    (ZF, RZF) P0 = Q1 T^H in place, columns ascending.  For MRT the top block already is P0.
//   normalise  the squared column norms of P0 (per-lane sums, butterfly); the top block is scaled by
//              sqrt(Ptot / sum of them) (TOTAL) or column i by sqrt((Ptot / Nr) / its own) (STREAM).  A norm that is
//              not > 0 flags the point HRT_PC_SINGULAR.
//   sinr       for every row i of H the lane reads H[i][t] of its own rows t again from global memory (just loaded by
//              the workgroup: L2), accumulates its part of E[i][j] = sum_t H[i][t] P[t][j] for all j in its first 2 Nr
//              words of T's region (dead by now), and the butterfly leaves E[i][:] in every lane; lane 0 stores sinr_i.
//   stage out  a flagged point has cleared its words (before sinr); after a barrier the workgroup stores P with the
//              point index fastest; lane 0 of a group stores status.
// A word of LDS belongs to one lane between the barriers and the butterflies and shuffles stay inside a group, so a
// point's bits depend on its own matrix only.  No atomics, no scratch; every output byte is written once.
#include <hip/hip_runtime.h>

#include <float.h>
#include <stdint.h>

#include "hermespy_rt.h"
#include "hrt_precoder.h"

#define EQ_T HRT_PC_THREADS

#include "hrt_mgs.inc"

// x[:, c] *= s on `rows` rows of this lane
__device__ __forceinline__ void pc_times(float *w, uint32_t c, uint32_t rows, uint32_t n, float s)
{
    for (uint32_t k = 0; k < rows; ++k) {
        float *x = w + ((k * n + c) * 2u) * EQ_T;
        x[0] = x[0] * s;
        x[EQ_T] = x[EQ_T] * s;
    }
}

template <uint32_t G>
__global__ void __launch_bounds__(HRT_PC_THREADS) hrt_precoder_kernel(const hrt_kprecoder P)
{
    __shared__ float sM[HRT_PC_WORDS * EQ_T];
    constexpr uint32_t PPB = EQ_T / G;

    const uint32_t tid = threadIdx.x, l = tid % G, sp_own = tid / G;
    const uint32_t nt = P.nt, n = P.nr, mk = P.mk, nk = P.nk;
    const uint64_t pt0 = (uint64_t)blockIdx.x * PPB, pt_own = pt0 + sp_own;
    float *const wA = sM + tid;                     // this lane's words of the top block (rows: transmit elements) ...
    float *const wT = wA + mk * n * 2u * EQ_T;      // ... and of T
    const bool aug = P.kind == HRT_PC_RZF;
    const float lam = aug ? P.alpha : 0.f;
    const float2 *const H = reinterpret_cast<const float2 *>(P.H);

    // ---- stage in
    for (uint32_t e = 0; e < (mk + nk) * n * 2u; ++e) wA[e * EQ_T] = 0.f;
    for (uint32_t k = 0; k < nk; ++k) {
        const uint32_t r = k * G + l;
        if (r < n) wT[((k * n + r) * 2u) * EQ_T] = 1.f;
    }
    __syncthreads();
    for (uint32_t w = tid; w < n * nt * PPB; w += EQ_T) {
        const uint32_t sp = w % PPB, e = w / PPB, i = e / nt, t = e % nt;
        const uint64_t pt = pt0 + sp;
        if (pt >= P.points) continue;
        const uint64_t link = pt / P.pts, q = pt % P.pts;
        const float2 h = H[((link * n + i) * nt + t) * P.pts + q];
        float *x = sM + (((t / G) * n + i) * 2u) * EQ_T + sp * G + t % G;
        x[0] = h.x;
        x[EQ_T] = -h.y;
    }
    __syncthreads();

    // ---- start: the column norms of A
    float nmax, nsum;
    eq_start<G>(wA, wT, mk, nk, n, aug, lam, nmax, nsum);
    const bool bad = !(nsum <= FLT_MAX);
    const float thr = ((float)(n + nt) * 0x1p-23f) * sqrtf(nmax);

    // ---- factor and weights: A = Q R, T = R^-1, P0 = Q1 T^H
    bool sing = false;
    if (P.kind != HRT_PC_MRT) {
        sing = eq_factor<G>(wA, wT, mk, nk, n, aug, lam, thr);
        eq_weights<G>(wA, wT, mk, n);
    }

    // ---- normalise
    float tot = 0.f;
    bool zero = false;
    for (uint32_t i = 0; i < n; ++i) {
        const float c = eq_reduce<G>(eq_lane_norm2(wA, i, mk, n));
        tot = tot + c;
        if (P.stream) {
            zero = zero || !(c > 0.f);
            pc_times(wA, i, mk, n, sqrtf(P.power / c));
        }
    }
    if (!P.stream) {
        zero = !(tot > 0.f);
        const float s = sqrtf(P.power / tot);
        for (uint32_t i = 0; i < n; ++i) pc_times(wA, i, mk, n, s);
    }
    const uint32_t status = bad ? HRT_PC_NONFINITE : (sing || zero) ? HRT_PC_SINGULAR
                                : !(tot <= FLT_MAX) ? HRT_PC_NONFINITE : 0u;
    if (status)
        for (uint32_t e = 0; e < mk * n * 2u; ++e) wA[e * EQ_T] = 0.f;

    // ---- effective channel and sinr: E = H P of the H in memory and the P in LDS, one row of H at a time
    const bool live = pt_own < P.points;
    const uint64_t link_own = live ? pt_own / P.pts : 0u, q_own = live ? pt_own % P.pts : 0u;
    const float2 *const Hp = H + link_own * n * nt * P.pts + q_own;      // H[i][t] of this point: Hp[(i Nt + t) pts]
    for (uint32_t i = 0; i < n; ++i) {
        for (uint32_t j = 0; j < 2u * n; ++j) wT[j * EQ_T] = 0.f;
        for (uint32_t k = 0; k < mk; ++k) {
            const uint32_t t = k * G + l;
            float2 h = make_float2(0.f, 0.f);
            if (live && t < nt) h = Hp[((uint64_t)i * nt + t) * P.pts];
            for (uint32_t j = 0; j < n; ++j) {
                const float pr = wA[((k * n + j) * 2u) * EQ_T], pi = wA[((k * n + j) * 2u + 1u) * EQ_T];
                float *a = wT + (j * 2u) * EQ_T;
                a[0] = a[0] + (h.x * pr - h.y * pi);
                a[EQ_T] = a[EQ_T] + (h.x * pi + h.y * pr);
            }
        }
        float sig = 0.f, itf = 0.f;
        for (uint32_t j = 0; j < n; ++j) {
            const float er = eq_reduce<G>(wT[(j * 2u) * EQ_T]), ei = eq_reduce<G>(wT[(j * 2u + 1u) * EQ_T]);
            const float m = er * er + ei * ei;
            if (j == i) sig = m;
            else itf = itf + m;
        }
        if (l == 0u && live) P.sinr[(link_own * n + i) * P.pts + q_own] = status ? 0.f : sig / (itf + P.n0);
    }

    // ---- stage out
    if (l == 0u && live) P.status[pt_own] = status;
    if (P.P) {
        __syncthreads();
        float2 *const o = reinterpret_cast<float2 *>(P.P);
        for (uint32_t w = tid; w < nt * n * PPB; w += EQ_T) {
            const uint32_t sp = w % PPB, e = w / PPB, t = e / n, i = e % n;
            const uint64_t pt = pt0 + sp;
            if (pt >= P.points) continue;
            const uint64_t link = pt / P.pts, q = pt % P.pts;
            const float *x = sM + (((t / G) * n + i) * 2u) * EQ_T + sp * G + t % G;
            o[((link * nt + t) * n + i) * P.pts + q] = make_float2(x[0], x[EQ_T]);
        }
    }
}

extern "C" int hrt_hip_launch_precoder(const hrt_kprecoder *P, uint32_t g, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint64_t ppb = HRT_PC_THREADS / g;
    const dim3 grid((uint32_t)((P->points + ppb - 1u) / ppb)), block(HRT_PC_THREADS);
    switch (g) {
    case 1u: hipLaunchKernelGGL(hrt_precoder_kernel<1u>, grid, block, 0, st, *P); break;
    case 2u: hipLaunchKernelGGL(hrt_precoder_kernel<2u>, grid, block, 0, st, *P); break;
    case 4u: hipLaunchKernelGGL(hrt_precoder_kernel<4u>, grid, block, 0, st, *P); break;
    case 8u: hipLaunchKernelGGL(hrt_precoder_kernel<8u>, grid, block, 0, st, *P); break;
    case 16u: hipLaunchKernelGGL(hrt_precoder_kernel<16u>, grid, block, 0, st, *P); break;
    case 32u: hipLaunchKernelGGL(hrt_precoder_kernel<32u>, grid, block, 0, st, *P); break;
    case 64u: hipLaunchKernelGGL(hrt_precoder_kernel<64u>, grid, block, 0, st, *P); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
