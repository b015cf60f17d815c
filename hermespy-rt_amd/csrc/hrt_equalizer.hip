// hrt_equalizer.hip -- per-point linear MIMO equalizers (ZF, LMMSE) of the array channel and their SINR, for gfx950:
// many small independent problems, direct (a triangular factorisation, no iteration).
//
//     W = (H^H H + lambda I)^-1 H^H,   sinr_i = 1 / (N0 G_ii) - [LMMSE],   G = (H^H H + lambda I)^-1
//
// Modified Gram-Schmidt in float on A = [H; sqrt(lambda) I] = Q R; csrc/hrt_equalizer.h has the lane groups, the LDS
// layout and why the bottom block is carried as T = R^-1 alone.  One kernel, instantiated per group size G:
//   stage in   every thread clears its own words and sets its rows of T = I; after a barrier the workgroup loads the
//              entries of its HRT_EQ_THREADS / G points with the point index fastest (the points of a workgroup are
//              contiguous for every (i, j)) and writes each to its owner's word.
//   start      the squared column norms of A, |h_c|^2 + lambda: their largest sets the singular threshold
//              thr = (Nr + Nt) 2^-23 sqrt(largest); a sum that is not finite flags the point HRT_EQ_NONFINITE.
//   factor     for column j: r_jj = |a_j| (singular where r_jj <= thr), a_j /= r_jj; for every later column i,
//              r = q_j^H a_i and a_i -= r q_j.  Every operation acts on the rows of the top block and of T alike.
//   weights    W^H = Q1 T^H in place, columns ascending: column i becomes sum_{c >= i} conj(T[i, c]) q_c (T is upper
//              triangular, so the columns it reads are not yet overwritten); T[i, c] comes from its owner by a shuffle.
//   sinr       the owner of row i of T sums |T[i, c]|^2 over c and leaves 1 / (N0 G_ii) - [LMMSE] in the row's first word.
//   stage out  a flagged point clears its words; after a barrier the workgroup stores sinr and W (conjugated and
//              transposed on the way) with the point index fastest.
// A word of LDS belongs to one lane between the barriers and the butterflies and shuffles stay inside a group, so a
// point's bits depend on its own matrix only.  No atomics, no scratch, no global memory but the one load and the stores.
#include <hip/hip_runtime.h>

#include <float.h>
#include <stdint.h>

#include "hermespy_rt.h"
#include "hrt_equalizer.h"

#define EQ_T HRT_EQ_THREADS

// reduce, from-lane, norm^2, dot, scale, project and the start, factor and weights loops: shared with the precoder
#include "hrt_mgs.inc"

template <uint32_t G>
__global__ void __launch_bounds__(HRT_EQ_THREADS) hrt_equalizer_kernel(const hrt_kequalizer P)
{
    __shared__ float sM[HRT_EQ_WORDS * EQ_T];
    constexpr uint32_t PPB = EQ_T / G;

    const uint32_t tid = threadIdx.x, l = tid % G, sp_own = tid / G;
    const uint32_t nr = P.nr, n = P.nt, mk = P.mk, nk = P.nk;
    const uint64_t pt0 = (uint64_t)blockIdx.x * PPB, pt_own = pt0 + sp_own;
    float *const wA = sM + tid;                     // this lane's words of the top block ...
    float *const wT = wA + mk * n * 2u * EQ_T;      // ... and of T
    const bool aug = P.lmmse != 0u;
    const float lam = aug ? P.n0 : 0.f;

    // ---- stage in
    for (uint32_t e = 0; e < (mk + nk) * n * 2u; ++e) wA[e * EQ_T] = 0.f;
    for (uint32_t k = 0; k < nk; ++k) {
        const uint32_t r = k * G + l;
        if (r < n) wT[((k * n + r) * 2u) * EQ_T] = 1.f;
    }
    __syncthreads();
    {
        const float2 *const H = reinterpret_cast<const float2 *>(P.H);
        for (uint32_t w = tid; w < nr * n * PPB; w += EQ_T) {
            const uint32_t sp = w % PPB, e = w / PPB, i = e / n, j = e % n;
            const uint64_t pt = pt0 + sp;
            if (pt >= P.points) continue;
            const uint64_t link = pt / P.pts, q = pt % P.pts;
            const float2 h = H[((link * nr + i) * n + j) * P.pts + q];
            float *x = sM + (((i / G) * n + j) * 2u) * EQ_T + sp * G + i % G;
            x[0] = h.x;
            x[EQ_T] = h.y;
        }
    }
    __syncthreads();

    // ---- start: the column norms of A
    float nmax, nsum;
    eq_start<G>(wA, wT, mk, nk, n, aug, lam, nmax, nsum);
    const bool bad = !(nsum <= FLT_MAX);
    const float thr = ((float)(nr + n) * 0x1p-23f) * sqrtf(nmax);

    // ---- factor: A = Q R, T = R^-1
    const bool sing = eq_factor<G>(wA, wT, mk, nk, n, aug, lam, thr);
    const uint32_t status = bad ? HRT_EQ_NONFINITE : sing ? HRT_EQ_SINGULAR : 0u;

    // ---- weights: W^H = Q1 T^H, column i <- sum_{c >= i} conj(T[i, c]) q_c
    if (P.W) eq_weights<G>(wA, wT, mk, n);

    // ---- sinr: G_ii = |row i of T|^2, left in the row's first word
    const float one = aug ? 1.f : 0.f;
    for (uint32_t k = 0; k < nk; ++k) {
        float *t = wT + (k * n * 2u) * EQ_T;
        float gii = 0.f;
        for (uint32_t c = 0; c < n; ++c) {
            const float xr = t[(c * 2u) * EQ_T], xi = t[(c * 2u + 1u) * EQ_T];
            gii = gii + (xr * xr + xi * xi);
        }
        t[0] = status ? 0.f : 1.f / (P.n0 * gii) - one;
    }

    // ---- stage out
    if (status)
        for (uint32_t e = 0; e < mk * n * 2u; ++e) wA[e * EQ_T] = 0.f;
    if (l == 0u && pt_own < P.points) P.status[pt_own] = status;
    __syncthreads();
    const float *const rT = sM + mk * n * 2u * EQ_T;
    for (uint32_t w = tid; w < n * PPB; w += EQ_T) {
        const uint32_t sp = w % PPB, i = w / PPB;
        const uint64_t pt = pt0 + sp;
        if (pt >= P.points) continue;
        const uint64_t link = pt / P.pts, q = pt % P.pts;
        P.sinr[(link * n + i) * P.pts + q] = rT[((i / G) * n * 2u) * EQ_T + sp * G + i % G];
    }
    if (P.W) {
        float2 *const o = reinterpret_cast<float2 *>(P.W);
        for (uint32_t w = tid; w < n * nr * PPB; w += EQ_T) {
            const uint32_t sp = w % PPB, e = w / PPB, i = e / nr, r = e % nr;
            const uint64_t pt = pt0 + sp;
            if (pt >= P.points) continue;
            const uint64_t link = pt / P.pts, q = pt % P.pts;
            const float *x = sM + (((r / G) * n + i) * 2u) * EQ_T + sp * G + r % G;
            o[((link * n + i) * nr + r) * P.pts + q] = make_float2(x[0], -x[EQ_T]);
        }
    }
}

extern "C" int hrt_hip_launch_equalizer(const hrt_kequalizer *P, uint32_t g, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint64_t ppb = HRT_EQ_THREADS / g;
    const dim3 grid((uint32_t)((P->points + ppb - 1u) / ppb)), block(HRT_EQ_THREADS);
    switch (g) {
    case 1u: hipLaunchKernelGGL(hrt_equalizer_kernel<1u>, grid, block, 0, st, *P); break;
    case 2u: hipLaunchKernelGGL(hrt_equalizer_kernel<2u>, grid, block, 0, st, *P); break;
    case 4u: hipLaunchKernelGGL(hrt_equalizer_kernel<4u>, grid, block, 0, st, *P); break;
    case 8u: hipLaunchKernelGGL(hrt_equalizer_kernel<8u>, grid, block, 0, st, *P); break;
    case 16u: hipLaunchKernelGGL(hrt_equalizer_kernel<16u>, grid, block, 0, st, *P); break;
    case 32u: hipLaunchKernelGGL(hrt_equalizer_kernel<32u>, grid, block, 0, st, *P); break;
    case 64u: hipLaunchKernelGGL(hrt_equalizer_kernel<64u>, grid, block, 0, st, *P); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
