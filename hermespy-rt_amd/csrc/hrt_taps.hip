// hrt_taps.hip -- sampled channel impulse responses (taps) from the workspace of a finished hrt_trace, for gfx950.
//
//     h[rx, tx, pol, m, i] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)) sinc(l_i - f_s tau_p)
//     t_m = t0 + m dt,  l_i = l_min + i
//
// over the LoS entry (hrt_taps_reduce_kernel) and every unblocked scatter record (hrt_taps_partial_kernel) of the
// link.  The TX segments of the hit blocks come from hrt_channel_segments_kernel (csrc/hrt_channel.hip); the workspace
// view, its readers, the batch fill, the reduce walk and the launch are csrc/hrt_pathsum.h; the sinc weights
// csrc/hrt_sinc.h; the tile setup and the MFMA loop csrc/hrt_taps_gemm.inc.
//   hrt_taps_partial_kernel  one workgroup (4 waves) per (row block x column block, record chunk, link): the real
//                            GEMM of csrc/hrt_taps.h on v_mfma_f32_16x16x4_f32, partial sums to the scratch.  The
//                            unblocked records of the chunk are compacted by mask ballots and staged HRT_TP_BATCH at a
//                            time: their sinc parameters, then U over the block's rows in LDS; every lane forms its
//                            own B operand V (one record, one tap) in registers.
//   hrt_taps_reduce_kernel   per output: the chunks in a fixed order, plus the LoS term, into out.
// No floating-point atomics anywhere: two calls with the same inputs give the same bits.
//
// Precision: every phase is reduced in FP64 to a fraction of a revolution -- nu t_m, f_c tau
// and x = f_s tau.  With n = rint(x), f = x - n, sinc(l - x) = -(-1)^(l - n) sin(pi f) / (pi (l - n - f)): one f32
// sinpi per record and, per tap, an exact integer difference, one v_rcp_f32 and a sign.  Where |l - x| < 1e-4 the
// weight is 1 (the f32 rounding of sinc there; exactly 1 where l - x is exactly 0).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_pathsum.h"
#include "hrt_taps.h"

// RT row tiles x (HRT_TP_WTILES / RT) column tiles per wave, the 4 waves along the columns (csrc/hrt_taps.h)
template <uint32_t RT>
__global__ void __launch_bounds__(HRT_TP_THREADS) hrt_taps_partial_kernel(const hrt_ktaps P)
{
    constexpr uint32_t CT = HRT_TP_WTILES / RT, WT = HRT_TP_WTILES, WR = 1u, WC = 4u;
    constexpr uint32_t BT = RT * 4u;   // time samples of the block
    const hrt_kview &V = P.v;
    const hrt_ktaps &G = P;   // the grid of csrc/hrt_taps_gemm.inc: its fields, written out (csrc/hrt_taps.h)
    const uint32_t blk = blockIdx.x, c = blockIdx.y, link = blockIdx.z;
    const uint32_t rb = blk % P.rblocks, cb = blk / P.rblocks;
    const uint32_t rx = link / V.ntx, tx = link % V.ntx;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t wr = 0, wc = w;                     // the wave's place in the block
    const uint32_t kq = lane >> 4, col = lane & 15u;   // A / B operand: record 4 g + kq; row / tap `col` of a tile

    __shared__ float sU[HRT_TP_BATCH][BT * 4u];   // U of the block's rows g = 4 mm + q
    __shared__ float sRec[HRT_TP_BATCH][6];        // te re, te im, tm re, tm im, tau, nu
    __shared__ sinc_rec sS[HRT_TP_BATCH];
    __shared__ uint32_t sB[HRT_TP_BATCH], sI[HRT_TP_BATCH];   // (bounce, hit) of the staged records

#define HRT_TG_U(j, x) sU[j][x]
#define HRT_TG_PART 1
#include "hrt_taps_gemm.inc"

    uint32_t b = 0, cur = 0, end = 0;
    chunk_range(V, 0, tx, c, cur, end);
    for (;;) {
        const uint32_t n = fill_batch<HRT_TP_BATCH>(V, rx, tx, c, lane, w, b, cur, end, sB, sI);
        if (n == 0) break;
        __syncthreads();
        if (tid < HRT_TP_BATCH) {   // the record's fields and sinc parameters (zeros past n: U = 0 there)
            float *R = sRec[tid];
            sinc_rec q = {0, 0.f, 0.f};
            if (tid < n) {
                const uint32_t rb2 = sB[tid], i = sI[tid];
                R[0] = rec_field(V, rb2, rx, HRT_REC_A_TE_RE)[i];
                R[1] = rec_field(V, rb2, rx, HRT_REC_A_TE_IM)[i];
                R[2] = rec_field(V, rb2, rx, HRT_REC_A_TM_RE)[i];
                R[3] = rec_field(V, rb2, rx, HRT_REC_A_TM_IM)[i];
                R[4] = rec_field(V, rb2, rx, HRT_REC_TAU)[i];
                R[5] = __uint_as_float(hit_field(V, rb2, HRT_HIT_FS0)[i]) - rec_field(V, rb2, rx, HRT_REC_DFS)[i];
                q = sinc_prep(P.fs, R[4]);
            } else {
                for (int f = 0; f < 6; ++f) R[f] = 0.f;
            }
            sS[tid] = q;
        }
        __syncthreads();
#pragma unroll 1
        for (uint32_t e = tid; e < HRT_TP_BATCH * BT; e += HRT_TP_THREADS) {   // U
            const uint32_t j = e / BT, mm = e % BT, m = rb * BT + mm;
            const float *R = sRec[j];
            float u0 = 0.f, u1 = 0.f, u2 = 0.f, u3 = 0.f;
            if (j < n && m < P.T) {
                const double t = P.t0 + (double)m * P.dt;
                float sn, cs;
                sincospif(half_revs((double)R[5] * t - P.fc * (double)R[4]), &sn, &cs);
                u0 = R[0] * cs - R[1] * sn;
                u1 = R[0] * sn + R[1] * cs;
                u2 = R[2] * cs - R[3] * sn;
                u3 = R[2] * sn + R[3] * cs;
            }
            float *U = &sU[j][4u * mm];
            U[0] = u0; U[1] = u1; U[2] = u2; U[3] = u3;
        }
        __syncthreads();
#define HRT_TG_PART 2
#include "hrt_taps_gemm.inc"
        __syncthreads();
    }
#undef HRT_TG_U

    // D: lane = (row group kq, column col), register q: row 4 kq + q of the tile = (time 4 R + kq, part q).  Part 3 of
    // the shared text splits a row into (pair, time); here a row is a time sample
    const uint64_t tl = (uint64_t)P.T * P.L;
    float2 *dst = reinterpret_cast<float2 *>(P.partial) + ((uint64_t)link * V.nchunks + c) * 2u * tl;
#pragma unroll
    for (uint32_t t = 0; t < WT; ++t) {
        const uint32_t m = (r0 + t / CT) * 4u + kq, i = (c0 + t % CT) * 16u + col;
        if (live[t] && m < P.T && i < P.L) {
            float2 *d = dst + (uint64_t)m * P.L + i;
            d[0] = make_float2(acc[t][0], acc[t][1]);
            d[tl] = make_float2(acc[t][2], acc[t][3]);
        }
    }
}

// one thread per output (link, pol, m, i): the chunks in order, + LoS, -> out
__global__ void hrt_taps_reduce_kernel(const hrt_ktaps P)
{
    const hrt_kview &V = P.v;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    hrt_taps_output o;
    if (!taps_output(V, P, 1u, P.partial, gid, o)) return;
    float2 s = o.s;
    hrt_los_entry L;
    if (V.los && los_entry(V, o.link, L)) {   // a real: TE = TM
        float sn, cs;
        sincospif(half_revs(taps_los_phase(P, o.m, L)), &sn, &cs);
        const float v = taps_los_weight(P, o.tap, L);
        s.x += v * cs;
        s.y += v * sn;
    }
    store_out(reinterpret_cast<float2 *>(P.out) + gid, s, V.accumulate);
}

extern "C" int hrt_hip_launch_taps(const hrt_ktaps *P, void *stream)
{
    return launch_taps_family<hrt_ktaps>(P, *P, 1u, HRT_TP_THREADS, hrt_taps_partial_kernel<4u>,
                                         hrt_taps_partial_kernel<1u>, NULL, hrt_taps_reduce_kernel, stream);
}
