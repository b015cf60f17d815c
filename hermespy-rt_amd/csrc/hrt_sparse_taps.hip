// hrt_sparse_taps.hip -- antenna-array (MIMO) sampled impulse responses from dominant-path lists, for gfx950.  The
// input is a buffer of hrt_dominant_paths' layout (header {kept, eligible} per link, then max_paths 72-byte slots per
// link); for every link, element pair (i, j), polarisation, time sample m and tap l_k = l_min + k, with
// n = min(kept[link], max_paths):
//
//     h[link, i, j, pol, m, k] = sum_{p < n} a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p))
//                                        * exp(j 2 pi f_a (r_i . u_rx_p + q_j . u_tx_p) / c) sinc(l_k - f_s tau_p)
//
//   hrt_sparse_taps_kernel  one workgroup (4 waves) per (row block x column block, link): the real GEMM of
//                           csrc/hrt_array_taps.h on v_mfma_f32_16x16x4_f32 (parts 1 and 2 of csrc/hrt_taps_gemm.inc,
//                           as hrt_array_taps_partial_kernel runs them, in its two forms) over ALL of the link's slots,
//                           walked in index order HRT_TP_BATCH at a time, the accumulators written straight to out.
//                           A slot's twelve floats from a_te_re on are staged into LDS in stage_record's order
//                           (csrc/hrt_pathsum.h) as six 8-byte loads per slot, as in csrc/hrt_sparse_channel.hip; the
//                           sinc parameters and U over the block's (pair, time) rows are formed from them as in
//                           csrc/hrt_array_taps.hip.
// One workgroup owns its outputs and sums a link's slots in one fixed order: every byte of out is written exactly once
// (or added to once), no atomics, no scratch, and two calls with the same input give the same bytes.  A workgroup reads
// only its own link's header entry and slots < n: what the other slots or links hold cannot reach its outputs.  The
// LoS entry is an ordinary slot; power, path, bounce and tri are not read.  The whole phase is formed in FP64 and
// reduced once to a fraction of a revolution: one f32 sincospi per (slot, pair, time) row of the block.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_pathsum.h"
#include "hrt_sparse_taps.h"

static_assert(HRT_PS_REC_FLOATS * 4u + HRT_SP_SLOT_FIRST == HRT_SP_SLOT_BYTES && HRT_SP_SLOT_BYTES % 8u == 0 &&
                  HRT_SP_SLOT_FIRST % 8u == 0,
              "a slot's staged floats: its last 48 bytes, 8-byte aligned");
static_assert(HRT_TP_BATCH * (HRT_PS_REC_FLOATS / 2u) <= HRT_TP_THREADS, "one 8-byte load per thread stages a batch");

// RT row tiles x CT column tiles per wave, WR waves along the rows: the two forms of csrc/hrt_array_taps.h
template <uint32_t RT, uint32_t CT, uint32_t WR>
__global__ void __launch_bounds__(HRT_TP_THREADS) hrt_sparse_taps_kernel(const hrt_ksparse_taps P)
{
    constexpr uint32_t WC = 4u / WR, WT = RT * CT;
    constexpr uint32_t BR = WR * RT * 4u;   // (pair, time) rows of the block
    const hrt_ktgrid &G = P.g;              // the grid, also of csrc/hrt_taps_gemm.inc
    const uint32_t blk = blockIdx.x, link = blockIdx.z;
    const uint32_t rb = blk % G.rblocks, cb = blk / G.rblocks;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t wr = w / WC, wc = w % WC;           // the wave's place in the block
    const uint32_t kq = lane >> 4, col = lane & 15u;   // A / B operand: slot 4 g + kq; row / tap `col` of a tile

    __shared__ float sU[HRT_TP_BATCH][BR * 4u];   // U of the block's rows g = 4 mm + q
    __shared__ float sRec[HRT_TP_BATCH][HRT_PS_REC_FLOATS];
    __shared__ sinc_rec sS[HRT_TP_BATCH];
    __shared__ float sEl[BR][6];                  // r_i, q_j of the block's rows
    __shared__ double sT[BR];                     // t_m of the block's rows

    // the link's live slots: the header's kept, never more than the list holds (the same for every thread)
    const uint64_t kept = reinterpret_cast<const uint64_t *>(P.paths)[2u * link];
    const uint32_t nlive = kept < P.max_paths ? (uint32_t)kept : P.max_paths;
    if (nlive == 0 && P.accumulate) return;   // nothing to add: out stays as it is

    if (tid < BR) {   // row mm = (pair a, time m): a = i Nt + j
        const uint32_t row = rb * BR + tid;
        float e[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        double t = 0.0;
        if (row < G.rows) {
            const uint32_t a = row / G.T, m = row - a * G.T;
            load_pair(P.rx_el, P.tx_el, P.nt, a, e);
            t = G.t0 + (double)m * G.dt;
        }
        for (int q = 0; q < 6; ++q) sEl[tid][q] = e[q];
        sT[tid] = t;
    }

#define HRT_TG_U(j, x) sU[j][x]
#define HRT_TG_PART 1
#include "hrt_taps_gemm.inc"

    const uint8_t *slots = P.paths + 16ull * P.links + (uint64_t)link * P.max_paths * HRT_SP_SLOT_BYTES;
    for (uint32_t s0 = 0; s0 < nlive; s0 += HRT_TP_BATCH) {
        const uint32_t n = min(nlive - s0, HRT_TP_BATCH);
        if (tid < n * (HRT_PS_REC_FLOATS / 2u)) {   // slot s0 + j, floats 2 q and 2 q + 1 of its twelve
            const uint32_t j = tid / (HRT_PS_REC_FLOATS / 2u), q = tid % (HRT_PS_REC_FLOATS / 2u);
            const float2 v = *reinterpret_cast<const float2 *>(slots + (uint64_t)(s0 + j) * HRT_SP_SLOT_BYTES +
                                                               HRT_SP_SLOT_FIRST + 8u * q);
            *reinterpret_cast<float2 *>(&sRec[j][2u * q]) = v;
        }
        // sRec is not read by the MFMA loop, so a fast wave may stage the next batch while the others are still in the
        // loop of this one; sS and sU are written only behind this barrier (the first pass: sEl and sT too)
        __syncthreads();
        if (tid < HRT_TP_BATCH) {   // the slot's sinc parameters (zeros past n)
            sinc_rec q = {0, 0.f, 0.f};
            if (tid < n) q = sinc_prep(G.fs, sRec[tid][4]);
            sS[tid] = q;
        }
#pragma unroll 1
        for (uint32_t e = tid; e < HRT_TP_BATCH * BR; e += HRT_TP_THREADS) {   // U
            const uint32_t j = e / BR, mm = e % BR;
            const float *R = sRec[j], *E = sEl[mm];
            float u0 = 0.f, u1 = 0.f, u2 = 0.f, u3 = 0.f;
            if (j < n && rb * BR + mm < G.rows) {
                const double pr = dot3(E, R + 6), pt = dot3(E + 3, R + 9);   // r_i . u_rx, q_j . u_tx
                float sn, cs;
                sincospif(half_revs((double)R[5] * sT[mm] - G.fc * (double)R[4] + P.fa_c * (pr + pt)), &sn, &cs);
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
    }
#undef HRT_TG_U

    // D: lane = (row group kq, column col), register q: row 4 kq + q of the tile = ((pair, time) row 4 R + kq, part q),
    // the lane mapping of part 3 of csrc/hrt_taps_gemm.inc, to out[link][pair][pol][m][l]: the 16 lanes of a col run
    // store 16 consecutive float2.  A link without live slots writes its zeros
    const uint64_t tl = (uint64_t)G.T * G.L;
    float2 *dst = reinterpret_cast<float2 *>(P.out) + (uint64_t)link * 2u * P.npairs * tl;
#pragma unroll
    for (uint32_t t = 0; t < WT; ++t) {
        const uint32_t row = (r0 + t / CT) * 4u + kq, i = (c0 + t % CT) * 16u + col;
        if (live[t] && row < G.rows && i < G.L) {
            const uint32_t pair = row / G.T, m = row - pair * G.T;
            float2 *d = dst + ((uint64_t)pair * 2u * G.T + m) * G.L + i;
            store_out(d, make_float2(acc[t][0], acc[t][1]), P.accumulate);
            store_out(d + tl, make_float2(acc[t][2], acc[t][3]), P.accumulate);
        }
    }
}

extern "C" int hrt_hip_launch_sparse_taps(const hrt_ksparse_taps *P, void *stream)
{
    const dim3 grid(P->g.rblocks * P->g.cblocks, 1u, P->links);
    if (P->g.rt == 4u)
        hipLaunchKernelGGL((hrt_sparse_taps_kernel<4u, 4u, 4u>), grid, dim3(HRT_TP_THREADS), 0, (hipStream_t)stream, *P);
    else
        hipLaunchKernelGGL((hrt_sparse_taps_kernel<1u, 4u, 1u>), grid, dim3(HRT_TP_THREADS), 0, (hipStream_t)stream, *P);
    return (int)hipGetLastError();
}
