// hrt_svd.hip -- per-point SVD of the array channel, for gfx950: many small independent problems with iteration.
//
//     H[rx, tx, :, :, pol, t, k] = u diag(sigma) v^H,   sigma descending, >= 0
//
// One-sided (Hestenes) complex Jacobi in float on A = H (Nr >= Nt) or H^H, m x n; csrc/hrt_svd.h has the lane groups
// and the LDS layout.  One kernel, instantiated per group size G:
//   stage in   every thread clears its own words and sets its rows of V = I; after a barrier the workgroup loads the
//              entries of its HRT_SVD_THREADS / G points with the point index fastest (the points of a workgroup are
//              contiguous for every (i, j)) and writes each to its owner's word.
//   sweeps     at most HRT_SVD_MAX_SWEEPS; nothing else in the loop depends on the data.  A pair (p, q) is skipped where
//              |a_p^H a_q| <= tol |a_p| |a_q| or where a column's squared norm is at or below floor^2 times the largest
//              of this sweep (tol = max(m, n) 2^-24, floor = max(m, n) 2^-23): noise is not rotated against noise, and
//              0 / 0 is not formed.  A point whose sweep rotated nothing is done and rotates nothing from then on; a
//              wave leaves the loop when all its points are done.  Column norms that are not finite end the point at
//              once, as HRT_SVD_NOT_CONVERGED.
//   order      sigma_c = |a_c|; rank by (sigma descending, column ascending), NaN first; every lane permutes the
//              columns of its own rows in place (cycle by cycle, at most n - 1 swaps).
//   stage out  per sorted column: sigma again (the same bits: same data, same order), the long side's column divided
//              by it, or exact zeros where sigma_d <= floor sigma_0; after a barrier the workgroup stores u and v with
//              the point index fastest.
// A word of LDS belongs to one lane between the two barriers and the butterflies stay inside a group, so a point's
// bits depend on its own matrix only.  No atomics, no scratch, no global memory but the one load and the stores.
#include <hip/hip_runtime.h>

#include <float.h>
#include <stdint.h>

#include "hermespy_rt.h"
#include "hrt_svd.h"

#define SVD_T HRT_SVD_THREADS

// sum over the G lanes of a group; every lane ends with the same bits (a + b = b + a at each level)
template <uint32_t G>
__device__ __forceinline__ float svd_reduce(float v)
{
#pragma unroll
    for (uint32_t off = 1u; off < G; off *= 2u) v = v + __shfl_xor(v, (int)off);
    return v;
}

// |a_c|^2 over the group
template <uint32_t G>
__device__ __forceinline__ float svd_norm2(const float *w, uint32_t c, uint32_t mk, uint32_t n)
{
    float a = 0.f;
    for (uint32_t k = 0; k < mk; ++k) {
        const float xr = w[((k * n + c) * 2u) * SVD_T], xi = w[((k * n + c) * 2u + 1u) * SVD_T];
        a = a + (xr * xr + xi * xi);
    }
    return svd_reduce<G>(a);
}

// [x y] <- [x y] J,  J = [[cs, sr + j si], [-(sr - j si), cs]], on `rows` rows of this lane
__device__ __forceinline__ void svd_rotate(float *w, uint32_t rows, uint32_t n, uint32_t p, uint32_t q, float cs, float sr,
                                           float si)
{
    for (uint32_t k = 0; k < rows; ++k) {
        float *x = w + ((k * n + p) * 2u) * SVD_T, *y = w + ((k * n + q) * 2u) * SVD_T;
        const float xr = x[0], xi = x[SVD_T], yr = y[0], yi = y[SVD_T];
        x[0] = cs * xr - (sr * yr + si * yi);
        x[SVD_T] = cs * xi - (sr * yi - si * yr);
        y[0] = (sr * xr - si * xi) + cs * yr;
        y[SVD_T] = (sr * xi + si * xr) + cs * yi;
    }
}

__device__ __forceinline__ void svd_swap(float *w, uint32_t rows, uint32_t n, uint32_t a, uint32_t b)
{
    for (uint32_t k = 0; k < rows; ++k)
        for (uint32_t part = 0; part < 2u; ++part) {
            float *x = w + ((k * n + a) * 2u + part) * SVD_T, *y = w + ((k * n + b) * 2u + part) * SVD_T;
            const float t = *x;
            *x = *y;
            *y = t;
        }
}

// the workgroup's store of one side: rows x n complex entries per point from the region `w0` (thread 0's words)
template <uint32_t G>
__device__ __forceinline__ void svd_store(const hrt_ksvd &P, const float *w0, uint32_t rows, float *dst, uint64_t pt0)
{
    constexpr uint32_t PPB = SVD_T / G;
    float2 *const o = reinterpret_cast<float2 *>(dst);
    for (uint32_t w = threadIdx.x; w < rows * P.n * PPB; w += SVD_T) {
        const uint32_t sp = w % PPB, e = w / PPB, r = e / P.n, d = e % P.n;
        const uint64_t pt = pt0 + sp;
        if (pt >= P.points) continue;
        const uint64_t link = pt / P.pts, q = pt % P.pts;
        const float *x = w0 + (((r / G) * P.n + d) * 2u) * SVD_T + sp * G + r % G;
        o[((link * rows + r) * P.n + d) * P.pts + q] = make_float2(x[0], x[SVD_T]);
    }
}

template <uint32_t G>
__global__ void __launch_bounds__(HRT_SVD_THREADS) hrt_svd_kernel(const hrt_ksvd P)
{
    __shared__ float sM[HRT_SVD_WORDS * SVD_T];
    constexpr uint32_t PPB = SVD_T / G;

    const uint32_t tid = threadIdx.x, l = tid % G, sp_own = tid / G;
    const uint32_t m = P.m, n = P.n, mk = P.mk, nk = P.nk;
    const uint64_t pt0 = (uint64_t)blockIdx.x * PPB, pt_own = pt0 + sp_own;
    float *const wA = sM + tid;                     // this lane's words of A ...
    float *const wV = wA + mk * n * 2u * SVD_T;     // ... and of V

    // ---- stage in
    for (uint32_t e = 0; e < (mk + nk) * n * 2u; ++e) wA[e * SVD_T] = 0.f;
    for (uint32_t k = 0; k < nk; ++k) {
        const uint32_t r = k * G + l;
        if (r < n) wV[((k * n + r) * 2u) * SVD_T] = 1.f;
    }
    __syncthreads();
    {
        const float2 *const H = reinterpret_cast<const float2 *>(P.H);
        for (uint32_t w = tid; w < P.nr * P.nt * PPB; w += SVD_T) {
            const uint32_t sp = w % PPB, e = w / PPB, i = e / P.nt, j = e % P.nt;
            const uint64_t pt = pt0 + sp;
            if (pt >= P.points) continue;
            const uint64_t link = pt / P.pts, q = pt % P.pts;
            const float2 h = H[((link * P.nr + i) * P.nt + j) * P.pts + q];
            const uint32_t r = P.tall ? i : j, c = P.tall ? j : i;
            float *x = sM + (((r / G) * n + c) * 2u) * SVD_T + sp * G + r % G;
            x[0] = h.x;
            x[SVD_T] = P.tall ? h.y : -h.y;
        }
    }
    __syncthreads();

    // ---- sweeps
    const float tol = (float)m * 0x1p-24f, flo = (float)m * 0x1p-23f;
    uint32_t sweeps = 0u;
    bool done = pt_own >= P.points;
    for (uint32_t sw = 0; sw < HRT_SVD_MAX_SWEEPS; ++sw) {
        if (__all(done)) break;
        float nmax = 0.f, nsum = 0.f;
        for (uint32_t c = 0; c < n; ++c) {
            const float a = svd_norm2<G>(wA, c, mk, n);
            nmax = a > nmax ? a : nmax;
            nsum = nsum + a;
        }
        if (!done && !(nsum <= FLT_MAX)) {
            done = true;
            sweeps = HRT_SVD_NOT_CONVERGED;
        }
        const float cfloor = (flo * flo) * nmax;
        uint32_t rot = 0u;
        for (uint32_t p = 0; p + 1u < n; ++p)
            for (uint32_t q = p + 1u; q < n; ++q) {
                float al = 0.f, be = 0.f, gr = 0.f, gi = 0.f;
                for (uint32_t k = 0; k < mk; ++k) {
                    const float *x = wA + ((k * n + p) * 2u) * SVD_T, *y = wA + ((k * n + q) * 2u) * SVD_T;
                    const float xr = x[0], xi = x[SVD_T], yr = y[0], yi = y[SVD_T];
                    al = al + (xr * xr + xi * xi);
                    be = be + (yr * yr + yi * yi);
                    gr = gr + (xr * yr + xi * yi);
                    gi = gi + (xr * yi - xi * yr);
                }
                al = svd_reduce<G>(al);
                be = svd_reduce<G>(be);
                gr = svd_reduce<G>(gr);
                gi = svd_reduce<G>(gi);
                const float ag = sqrtf(gr * gr + gi * gi);
                const bool skip = ag <= tol * (sqrtf(al) * sqrtf(be)) || al <= cfloor || be <= cfloor;
                if (!done && !skip) {
                    ++rot;
                    const float zeta = (be - al) / (2.f * ag);
                    const float t = (zeta >= 0.f ? 1.f : -1.f) / (fabsf(zeta) + sqrtf(1.f + zeta * zeta));
                    const float cs = 1.f / sqrtf(1.f + t * t), sn = cs * t;
                    const float sr = sn * (gr / ag), si = sn * (gi / ag);
                    svd_rotate(wA, mk, n, p, q, cs, sr, si);
                    svd_rotate(wV, nk, n, p, q, cs, sr, si);
                }
            }
        if (!done) {
            if (rot == 0u) done = true;
            else ++sweeps;
        }
    }
    if (!done) sweeps = HRT_SVD_NOT_CONVERGED;

    // ---- order: rank of column c = columns before it, in 4 bits at 4 c
    uint64_t rk = 0u;
    {
        float sig[HRT_SVD_MAX_SHORT];
#pragma unroll
        for (uint32_t j = 0; j < HRT_SVD_MAX_SHORT; ++j) sig[j] = -1.f;   // (an unused column ranks after every used one)
        for (uint32_t c = 0; c < n; ++c) {
            const float sg = sqrtf(svd_norm2<G>(wA, c, mk, n));
            const float key = sg != sg ? INFINITY : sg;   // NaN first
#pragma unroll
            for (uint32_t j = 0; j < HRT_SVD_MAX_SHORT; ++j) sig[j] = j == c ? key : sig[j];   // (registers: no runtime index)
        }
        uint32_t before[HRT_SVD_MAX_SHORT];
#pragma unroll
        for (uint32_t j = 0; j < HRT_SVD_MAX_SHORT; ++j) before[j] = 0u;
#pragma unroll
        for (uint32_t c = 0; c + 1u < HRT_SVD_MAX_SHORT; ++c)
#pragma unroll
            for (uint32_t d = c + 1u; d < HRT_SVD_MAX_SHORT; ++d) {
                const uint32_t later = sig[d] > sig[c] ? 1u : 0u;   // the later column goes first only where larger
                before[c] += later;
                before[d] += 1u - later;
            }
#pragma unroll
        for (uint32_t j = 0; j < HRT_SVD_MAX_SHORT; ++j) rk |= (uint64_t)(before[j] & 15u) << (4u * j);
    }
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t t = 0; t < n; ++t) {
            const uint32_t d = (uint32_t)(rk >> (4u * i)) & 15u;
            if (d == i) break;
            svd_swap(wA, mk, n, i, d);
            svd_swap(wV, nk, n, i, d);
            const uint64_t rd = (rk >> (4u * d)) & 15u;
            rk &= ~((15ull << (4u * i)) | (15ull << (4u * d)));
            rk |= (rd << (4u * i)) | ((uint64_t)d << (4u * d));
        }

    // ---- stage out
    const uint64_t link_own = pt_own < P.points ? pt_own / P.pts : 0u, q_own = pt_own < P.points ? pt_own % P.pts : 0u;
    const bool writer = l == 0u && pt_own < P.points;
    float s0 = 0.f;
    for (uint32_t d = 0; d < n; ++d) {
        const float sg = sqrtf(svd_norm2<G>(wA, d, mk, n));
        if (d == 0u) s0 = sg;
        const bool null = sg <= flo * s0;
        for (uint32_t k = 0; k < mk; ++k) {
            float *x = wA + ((k * n + d) * 2u) * SVD_T;
            x[0] = null ? 0.f : x[0] / sg;
            x[SVD_T] = null ? 0.f : x[SVD_T] / sg;
        }
        if (writer) P.sigma[(link_own * n + d) * P.pts + q_own] = sg;
    }
    if (writer) P.sweeps[pt_own] = sweeps;
    __syncthreads();
    const float *const rA = sM, *const rV = sM + mk * n * 2u * SVD_T;
    if (P.u) svd_store<G>(P, P.tall ? rA : rV, P.nr, P.u, pt0);
    if (P.v) svd_store<G>(P, P.tall ? rV : rA, P.nt, P.v, pt0);
}

extern "C" int hrt_hip_launch_svd(const hrt_ksvd *P, uint32_t g, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint64_t ppb = HRT_SVD_THREADS / g;
    const dim3 grid((uint32_t)((P->points + ppb - 1u) / ppb)), block(HRT_SVD_THREADS);
    switch (g) {
    case 1u: hipLaunchKernelGGL(hrt_svd_kernel<1u>, grid, block, 0, st, *P); break;
    case 2u: hipLaunchKernelGGL(hrt_svd_kernel<2u>, grid, block, 0, st, *P); break;
    case 4u: hipLaunchKernelGGL(hrt_svd_kernel<4u>, grid, block, 0, st, *P); break;
    case 8u: hipLaunchKernelGGL(hrt_svd_kernel<8u>, grid, block, 0, st, *P); break;
    case 16u: hipLaunchKernelGGL(hrt_svd_kernel<16u>, grid, block, 0, st, *P); break;
    case 32u: hipLaunchKernelGGL(hrt_svd_kernel<32u>, grid, block, 0, st, *P); break;
    case 64u: hipLaunchKernelGGL(hrt_svd_kernel<64u>, grid, block, 0, st, *P); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
