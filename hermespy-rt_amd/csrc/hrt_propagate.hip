// hrt_propagate.hip -- received signals: sampled impulse responses (the output of the taps families) applied to
// baseband waveforms, for gfx950.
//
//     y[rx, i, pol, n] = sum_tx sum_j sum_{l < L} h[rx, tx, i, j, pol, m(n), l] x[tx, j, n - l_min - l]
//     m(n) = min(n / S, M - 1),   x[.., k] = 0 outside 0 <= k < N
//
// Two kernels, chosen by hrt_propagate_form (csrc/hrt_propagate.h, which has the tiling):
//   hrt_propagate_mfma_kernel     one workgroup (4 waves) per (16 complex rows, HRT_PG_COLS samples): the real GEMM
//                                 against the Toeplitz operand of x on v_mfma_f32_16x16x4_f32.  The window of x that
//                                 HRT_PG_LC taps of one TX port need lies in LDS, re/im interleaved: a B read
//                                 (ds_read_b32) takes dword 2 (e + col) + c in lanes 16 kq + col with c = kq & 1 and
//                                 e one less in the upper half wave, 32 different banks in each half wave.  A comes
//                                 from h directly, one float2 per lane and k step, requested one step ahead; a column
//                                 tile in the same block m as the tile before it reuses that tile's A.
//   hrt_propagate_general_kernel  one lane per (row, sample): an fmaf chain over (tx, j, l); only the taps that meet
//                                 a sample of x are walked.
// The whole reduction of an output happens in one lane or one wave, in a fixed order: no partial sums, no scratch, no
// atomics; two calls give the same bits.  Rows past R, taps past L and samples past N_out are zeros in the operands
// (selects on A and B), never a branch round an MFMA.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_propagate.h"

typedef float hrt_f32x4 __attribute__((ext_vector_type(4)));

// h[r][p][0][0] of row r = (rx, i, pol) and port p = (tx, j), in complex elements
__device__ __forceinline__ uint64_t pg_h_offset(const hrt_kpropagate &P, uint32_t r, uint32_t p)
{
    const uint32_t rx = r / (2u * P.nr), i = (r >> 1) % P.nr, pol = r & 1u;
    const uint32_t tx = p / P.nt, j = p % P.nt;
    return (((((uint64_t)rx * P.ntx + tx) * P.nr + i) * P.nt + j) * 2u + pol) * P.M * P.L;
}

__device__ __forceinline__ void pg_store(const hrt_kpropagate &P, uint32_t r, uint64_t n, float re, float im)
{
    float2 *d = reinterpret_cast<float2 *>(P.out) + (uint64_t)r * P.N_out + n;
    if (P.accumulate) {
        const float2 o = *d;
        re += o.x;
        im += o.y;
    }
    *d = make_float2(re, im);
}

__global__ void __launch_bounds__(HRT_PG_THREADS) hrt_propagate_mfma_kernel(const hrt_kpropagate P)
{
    __shared__ float sX[2u * HRT_PG_WINDOW];   // complex window of x: entry e at dwords 2 e, 2 e + 1

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t kq = lane >> 4, col = lane & 15u;   // A: row col, k = kq; B: k = kq, sample col
    const uint32_t dl = kq >> 1, c = kq & 1u;          // k = (tap l + dl, part c: 0 re, 1 im)
    const uint64_t n_wg = (uint64_t)blockIdx.x * HRT_PG_COLS;
    const uint32_t rtiles = (P.R + 15u) / 16u;
    const float2 *const h = reinterpret_cast<const float2 *>(P.h);
    const float2 *const x = reinterpret_cast<const float2 *>(P.x);

    uint32_t mt[HRT_PG_WTILES];    // the block of each column tile (a tile lies in one block: S % 16 == 0 or M == 1)
    uint32_t nl[HRT_PG_WTILES];    // this lane's sample of each column tile, within the workgroup
    bool nlive[HRT_PG_WTILES];
#pragma unroll
    for (uint32_t t = 0; t < HRT_PG_WTILES; ++t) {
        const uint32_t c0 = (w * HRT_PG_WTILES + t) * 16u;
        const uint64_t n0 = n_wg + c0 < P.N_out ? n_wg + c0 : P.N_out - 1u;   // (a tile past N_out reads a block in use)
        const uint64_t mq = n0 / P.S;
        mt[t] = mq < P.M - 1u ? (uint32_t)mq : P.M - 1u;
        nl[t] = c0 + col;
        nlive[t] = n_wg + nl[t] < P.N_out;
    }

    for (uint32_t rt = blockIdx.y; rt < rtiles; rt += gridDim.y) {
        const uint32_t r = rt * 16u + col;
        const bool rlive = r < P.R;
        const uint32_t ra = rlive ? r : P.R - 1u;   // (a row to read; its values are replaced by zeros)
        hrt_f32x4 yre[HRT_PG_WTILES], yim[HRT_PG_WTILES];
#pragma unroll
        for (uint32_t t = 0; t < HRT_PG_WTILES; ++t) {
            yre[t] = hrt_f32x4{0.f, 0.f, 0.f, 0.f};
            yim[t] = hrt_f32x4{0.f, 0.f, 0.f, 0.f};
        }

        for (uint32_t p = 0; p < P.P; ++p) {
            const float2 *hp = h + pg_h_offset(P, ra, p);
            const float2 *xp = x + (uint64_t)p * P.N;
            for (uint32_t l0 = 0; l0 < P.L; l0 += HRT_PG_LC) {
                const uint32_t lc = P.L - l0 < HRT_PG_LC ? P.L - l0 : HRT_PG_LC;
                // window entry e is x[kb + e]; sample n_wg + nl under tap l0 + d is entry nl + lc - d (0 <= d <= lc)
                const int64_t kb = (int64_t)n_wg - (int64_t)P.l_min - (int64_t)(l0 + lc);
                __syncthreads();
                for (uint32_t e = tid; e < HRT_PG_COLS + lc; e += HRT_PG_THREADS) {
                    const int64_t k = kb + (int64_t)e;
                    float2 v = make_float2(0.f, 0.f);
                    if (k >= 0 && k < (int64_t)P.N) v = xp[k];
                    sX[2u * e] = v.x;
                    sX[2u * e + 1u] = v.y;
                }
                __syncthreads();

                // A of one k step: (re, -im) for Re y, (im, re) for Im y; zeros past the rows and the taps
                auto load_a = [&](uint32_t d0, float (&are)[HRT_PG_WTILES], float (&aim)[HRT_PG_WTILES]) {
                    const uint32_t d = d0 + dl;
                    const bool live = rlive && d < lc;
                    const uint32_t la = l0 + (d < lc ? d : 0u);
#pragma unroll
                    for (uint32_t t = 0; t < HRT_PG_WTILES; ++t) {
                        if (t == 0u || mt[t] != mt[t - 1u]) {
                            const float2 hv = hp[(uint64_t)mt[t] * P.L + la];
                            are[t] = live ? (c ? -hv.y : hv.x) : 0.f;
                            aim[t] = live ? (c ? hv.x : hv.y) : 0.f;
                        } else {
                            are[t] = are[t - 1u];
                            aim[t] = aim[t - 1u];
                        }
                    }
                };

                float are[HRT_PG_WTILES], aim[HRT_PG_WTILES];
                load_a(0u, are, aim);
                for (uint32_t d0 = 0; d0 < lc; d0 += 2u) {
                    float nre[HRT_PG_WTILES], nim[HRT_PG_WTILES];
                    if (d0 + 2u < lc) {
                        load_a(d0 + 2u, nre, nim);
                    } else {
#pragma unroll
                        for (uint32_t t = 0; t < HRT_PG_WTILES; ++t) nre[t] = nim[t] = 0.f;
                    }
                    const uint32_t d = d0 + dl;
                    const bool klive = d < lc;
#pragma unroll
                    for (uint32_t t = 0; t < HRT_PG_WTILES; ++t) {
                        const float xv = sX[2u * (nl[t] + lc - d) + c];
                        const float b = klive && nlive[t] ? xv : 0.f;
                        yre[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(are[t], b, yre[t], 0, 0, 0);
                        yim[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(aim[t], b, yim[t], 0, 0, 0);
                    }
#pragma unroll
                    for (uint32_t t = 0; t < HRT_PG_WTILES; ++t) {
                        are[t] = nre[t];
                        aim[t] = nim[t];
                    }
                }
            }
        }

        // D: lane (kq, col), register q: row 16 rt + 4 kq + q, sample nl
#pragma unroll
        for (uint32_t t = 0; t < HRT_PG_WTILES; ++t) {
            if (!nlive[t]) continue;
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) {
                const uint32_t row = rt * 16u + 4u * kq + q;
                if (row < P.R) pg_store(P, row, n_wg + nl[t], yre[t][q], yim[t][q]);
            }
        }
    }
}

__global__ void __launch_bounds__(HRT_PG_THREADS) hrt_propagate_general_kernel(const hrt_kpropagate P)
{
    const uint64_t n = (uint64_t)blockIdx.x * HRT_PG_THREADS + threadIdx.x;
    if (n >= P.N_out) return;
    const uint64_t mq = n / P.S;
    const uint32_t m = mq < P.M - 1u ? (uint32_t)mq : P.M - 1u;
    // tap l meets x[k0 - l]: the taps with 0 <= k0 - l < N, l_lo <= l <= l_hi (none where l_hi < l_lo)
    const int64_t k0 = (int64_t)n - (int64_t)P.l_min;
    const int64_t lo = k0 - ((int64_t)P.N - 1), hi = k0 < (int64_t)P.L - 1 ? k0 : (int64_t)P.L - 1;
    const int64_t l_lo = lo > 0 ? lo : 0;
    const float2 *const h = reinterpret_cast<const float2 *>(P.h);
    const float2 *const x = reinterpret_cast<const float2 *>(P.x);
    for (uint32_t r = blockIdx.y; r < P.R; r += gridDim.y) {
        float re = 0.f, im = 0.f;
        for (uint32_t p = 0; p < P.P; ++p) {
            const float2 *hp = h + pg_h_offset(P, r, p) + (uint64_t)m * P.L;
            const float2 *xp = x + (uint64_t)p * P.N;
            for (int64_t l = l_lo; l <= hi; ++l) {
                const float2 hv = hp[l], xv = xp[k0 - l];
                re = fmaf(hv.x, xv.x, re);
                re = fmaf(-hv.y, xv.y, re);
                im = fmaf(hv.x, xv.y, im);
                im = fmaf(hv.y, xv.x, im);
            }
        }
        pg_store(P, r, n, re, im);
    }
}

extern "C" int hrt_hip_launch_propagate(const hrt_kpropagate *P, uint32_t form, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint32_t cblocks = (uint32_t)((P->N_out + HRT_PG_COLS - 1u) / HRT_PG_COLS);
    if (form == HRT_PG_MFMA) {
        const uint32_t rtiles = (P->R + 15u) / 16u;
        hipLaunchKernelGGL(hrt_propagate_mfma_kernel, dim3(cblocks, rtiles < 65535u ? rtiles : 65535u),
                           dim3(HRT_PG_THREADS), 0, st, *P);
    } else {
        hipLaunchKernelGGL(hrt_propagate_general_kernel, dim3(cblocks, P->R < 65535u ? P->R : 65535u),
                           dim3(HRT_PG_THREADS), 0, st, *P);
    }
    return (int)hipGetLastError();
}
