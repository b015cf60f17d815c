// hrt_detect.hip -- per-point maximum-likelihood MIMO detection with max-log bit LLRs on an array channel, for gfx950:
// every hypothesis q of the Q = M^Nt symbol vectors is scored against the received vector of a point.
//
//     d_q = |y - H s(q)|^2,   q* = argmin_q d_q (lowest q on a tie),
//     llr[j][b] = (min over q with bit 0 of d_q - min over q with bit 1 of d_q) / N0
//
// The form, the LDS image and the bit positions are csrc/hrt_detect.h's; the order of every sum is hermespy_rt.h's
// (hrt_detect_spec).  VALU form: a lane owns one hypothesis, so its distance never leaves the lane and the epilogue is
// compare-and-move only.  One launch on the caller's stream, instantiated per Nt (the lane's Nt symbols stay in
// registers) and per width:
//   narrow  Q < 64: 64 / Q points per wave, one hypothesis per lane, H and y read per group (vector loads, the lanes of
//           a group at one address);
//   wide    Q >= 64: one point per wave, Q / 64 tiles; H and y are wave-uniform (scalar loads).  Per tile a lane forms
//           its d, keeps its running best (d, q) with a strict <, whether any d was not finite and, with LLRs, the two
//           minima per tile bit.
// Epilogue: the (d, q) butterfly over the group, the per-bit minima as hrt_detect.h describes, one subtraction and one
// division per bit, then lane 0 of the group stores index, metric and status and lane p the LLR of bit position p.
// A point's bytes depend on its own H, y, the constellation and N0 only.  No atomics, no scratch, vector stores only.
#include <hip/hip_runtime.h>

#include <float.h>
#include <stdint.h>

#include "hermespy_rt.h"
#include "hrt_detect.h"

#define DT_T HRT_DT_THREADS
#define DT_LB HRT_DT_LANE_BITS

__device__ __forceinline__ float dt_min(float a, float b) { return b < a ? b : a; }

template <uint32_t NT, bool WIDE>
__global__ void __launch_bounds__(HRT_DT_THREADS)
hrt_detect_kernel(const hrt_kdetect P, const float2 *__restrict__ H, const float2 *__restrict__ Y,
                  const float2 *__restrict__ S)
{
    __shared__ float2 sS[HRT_DT_MAX_M];

    const uint32_t tid = threadIdx.x, lane = tid % 64u;
    const uint32_t nr = P.nr, B = P.b, M = 1u << B, nb = NT * B, g = WIDE ? 64u : P.g;
    for (uint32_t x = tid; x < M; x += DT_T) sS[x] = S[x];
    __syncthreads();

    // the wave's points: 64 / g of them from `first` on
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid / 64u));
    const uint64_t first = ((uint64_t)blockIdx.x * HRT_DT_WAVES + wave) * (64u / g);
    if (first >= P.points) return;
    uint32_t pt = (uint32_t)first;
    bool live = true;
    if (!WIDE) {
        pt += lane / g;
        live = pt < P.points;
        if (!live) pt = P.points - 1u;      // (a group beyond the end repeats the last point and stores nothing)
    }
    const uint32_t ql = WIDE ? lane : lane % g;
    const uint32_t link = pt / P.pts, rem = pt % P.pts;
    const uint64_t pts = P.pts;
    const float2 *const Hp = H + (uint64_t)link * nr * NT * pts + rem;    // H[i][j]: Hp[(i NT + j) pts]
    const float2 *const Yp = Y + (uint64_t)link * nr * pts + rem;         // y[i]: Yp[i pts]
    const bool llr = P.llr != 0u;

    float bd = INFINITY;
    uint32_t bq = 0xffffffffu;
    uint32_t bad = 0u;
    float t0[DT_LB], t1[DT_LB];             // the minima per tile bit (positions 6 ..)
#pragma unroll
    for (uint32_t t = 0; t < DT_LB; ++t) t0[t] = t1[t] = INFINITY;

    const uint32_t tiles = WIDE ? P.tiles : 1u;
    for (uint32_t tile = 0; tile < tiles; ++tile) {
        const uint32_t q = tile * 64u + ql;
        float2 s[NT];
#pragma unroll
        for (uint32_t j = 0; j < NT; ++j) s[j] = sS[(q >> (j * B)) & (M - 1u)];
        float d = 0.f;
        for (uint32_t i = 0; i < nr; ++i) {
            const float2 *const h = Hp + (uint64_t)i * NT * pts;
            float er = 0.f, ei = 0.f;
#pragma unroll
            for (uint32_t j = 0; j < NT; ++j) {
                const float2 x = h[(uint64_t)j * pts];
                const float pr = x.x * s[j].x - x.y * s[j].y, pi = x.x * s[j].y + x.y * s[j].x;
                er = j == 0u ? pr : er + pr;
                ei = j == 0u ? pi : ei + pi;
            }
            const float2 y = Yp[(uint64_t)i * pts];
            const float rr = y.x - er, ri = y.y - ei;
            d = d + (rr * rr + ri * ri);
        }
        bad |= !(d <= FLT_MAX);
        if (d < bd) {
            bd = d;
            bq = q;
        }
        if (WIDE && llr) {
#pragma unroll
            for (uint32_t t = 0; t < DT_LB; ++t) {
                if (DT_LB + t >= nb) break;
                if ((tile >> t) & 1u) t1[t] = dt_min(t1[t], d);
                else t0[t] = dt_min(t0[t], d);
            }
        }
    }

    // ---- the hard decision: the smaller d, the lower q on a tie
    const float dm = bd;                    // the lane's own minimum
#pragma unroll
    for (uint32_t off = 32u; off > 0u; off >>= 1) {
        if (off >= g) continue;
        const float od = __shfl_xor(bd, (int)off, 64);
        const uint32_t oq = (uint32_t)__shfl_xor((int)bq, (int)off, 64);
        bad |= (uint32_t)__shfl_xor((int)bad, (int)off, 64);
        if (od < bd || (od == bd && oq < bq)) {
            bd = od;
            bq = oq;
        }
    }

    // ---- the bit minima and the LLRs: every lane of the group ends with every (m0, m1); lane p keeps position p's
    float mine = 0.f;
    if (llr) {
#pragma unroll
        for (uint32_t p = 0; p < HRT_DT_MAX_BITS; ++p) {
            if (p >= nb) continue;
            float m0, m1;
            if (p < DT_LB) {                // a lane bit
                float a = dm;
#pragma unroll
                for (uint32_t off = 1u; off < 64u; off <<= 1)
                    if (off < g && off != (1u << p)) a = dt_min(a, __shfl_xor(a, (int)off, 64));
                const float o = __shfl_xor(a, (int)(1u << p), 64);
                const bool one = (lane >> p) & 1u;
                m0 = one ? o : a;
                m1 = one ? a : o;
            } else {                        // a tile bit
                m0 = t0[p < DT_LB ? 0u : p - DT_LB];
                m1 = t1[p < DT_LB ? 0u : p - DT_LB];
#pragma unroll
                for (uint32_t off = 1u; off < 64u; off <<= 1) {
                    m0 = dt_min(m0, __shfl_xor(m0, (int)off, 64));
                    m1 = dt_min(m1, __shfl_xor(m1, (int)off, 64));
                }
            }
            const float v = (m0 - m1) / P.n0;
            bad |= !(fabsf(v) <= FLT_MAX);
            if (ql == p) mine = v;
        }
    }

    if (!live) return;
    uint32_t *const o = reinterpret_cast<uint32_t *>(P.out);
    const uint32_t status = bad ? HRT_DT_NONFINITE : 0u;
    if (ql == 0u) {
        o[pt] = status ? 0xffffffffu : bq;
        reinterpret_cast<float *>(o)[(uint64_t)P.points + pt] = status ? 0.f : bd;
        o[2ull * P.points + pt] = status;
    }
    if (llr && ql < nb) {
        // position p = j B + (B - 1 - b) is written at llr[link][j][b][rem]
        const uint32_t j = ql / B, b = B - 1u - ql % B;
        float *const L = reinterpret_cast<float *>(o) + 3ull * P.points;
        L[(((uint64_t)link * NT + j) * B + b) * pts + rem] = status ? 0.f : mine;
    }
}

template <uint32_t NT>
static void dt_launch(const hrt_kdetect &P, const float2 *h, const float2 *y, const float2 *s, hipStream_t st)
{
    const uint64_t waves = ((uint64_t)P.points + 64u / P.g - 1u) / (64u / P.g);
    const dim3 grid((uint32_t)((waves + HRT_DT_WAVES - 1u) / HRT_DT_WAVES)), block(HRT_DT_THREADS);
    if (P.g == 64u) hipLaunchKernelGGL((hrt_detect_kernel<NT, true>), grid, block, 0, st, P, h, y, s);
    else if constexpr (NT < HRT_DT_LANE_BITS) hipLaunchKernelGGL((hrt_detect_kernel<NT, false>), grid, block, 0, st, P, h, y, s);
}

extern "C" int hrt_hip_launch_detect(const hrt_kdetect *P, const void *H, const void *Y, const void *S, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const float2 *h = (const float2 *)H, *y = (const float2 *)Y, *s = (const float2 *)S;
    if (P->g == 0u || P->g != hrt_detect_form(P->nt, P->b) || P->tiles != hrt_detect_tiles(P->nt, P->b) || P->nr < 1u
        || P->nr > HRT_DT_MAX_NR || P->points == 0u || P->pts == 0u)
        return (int)hipErrorInvalidValue;
    switch (P->nt) {
    case 1u: dt_launch<1u>(*P, h, y, s, st); break;
    case 2u: dt_launch<2u>(*P, h, y, s, st); break;
    case 3u: dt_launch<3u>(*P, h, y, s, st); break;
    case 4u: dt_launch<4u>(*P, h, y, s, st); break;
    case 5u: dt_launch<5u>(*P, h, y, s, st); break;
    case 6u: dt_launch<6u>(*P, h, y, s, st); break;
    case 7u: dt_launch<7u>(*P, h, y, s, st); break;
    case 8u: dt_launch<8u>(*P, h, y, s, st); break;
    case 9u: dt_launch<9u>(*P, h, y, s, st); break;
    case 10u: dt_launch<10u>(*P, h, y, s, st); break;
    case 11u: dt_launch<11u>(*P, h, y, s, st); break;
    case 12u: dt_launch<12u>(*P, h, y, s, st); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
