// hrt_array_taps.hip -- antenna-array (MIMO) sampled impulse responses from the workspace of a finished hrt_trace,
// for gfx950.  For every link (rx, tx), element pair (i, j), polarisation, time sample m and tap l_k = l_min + k:
//
//     h[rx, tx, i, j, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p))
//                                        * exp(j 2 pi f_a (r_i . u_rx + q_j . u_tx) / c) sinc(l_k - f_s tau_p)
//
// over the LoS entry (hrt_array_taps_reduce_kernel) and every unblocked scatter record (hrt_array_taps_partial_kernel)
// of the link.  The TX segments of the hit blocks come from hrt_channel_segments_kernel (csrc/hrt_channel.hip); the
// workspace view, its readers, the batch fill, the reduce walk and the launch are csrc/hrt_pathsum.h; the sinc weights
// csrc/hrt_sinc.h; the tile setup, the MFMA loop and the write-back csrc/hrt_taps_gemm.inc.
//   hrt_array_taps_partial_kernel  one workgroup (4 waves) per (row block x column block, record chunk, link): the
//                                  real GEMM of csrc/hrt_array_taps.h on v_mfma_f32_16x16x4_f32, partial sums to the
//                                  scratch.  The unblocked records of the chunk are compacted by mask ballots and
//                                  staged HRT_TP_BATCH at a time: their fields, departure direction and sinc
//                                  parameters, then U over the block's (pair, time) rows in LDS (steering and phase
//                                  in one sincospi); every lane forms its own B operand V (one record, one tap) in
//                                  registers.
//   hrt_array_taps_reduce_kernel   per output: the chunks in a fixed order, plus the LoS term, into out.
// No floating-point atomics anywhere: two calls with the same inputs give the same bits.
//
// u_rx is the record's HRT_REC_DIR (directions_rx); u_tx the launch direction of the record's ray (csrc/
// hrt_launch_dir.h), as in csrc/hrt_array_channel.hip.  The whole phase nu t_m - f_c tau + f_a (r . u_rx + q . u_tx)
// / c is formed in FP64 and reduced once to a fraction of a revolution: one f32 sincospi per (record, pair, time)
// row of the block.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_array_taps.h"
#include "hrt_pathsum.h"

// RT row tiles x CT column tiles per wave; the 4 waves of the block stand WR along the rows and 4 / WR along the
// columns (the two forms of csrc/hrt_array_taps.h: <4, 4, 4> and <1, 4, 1>)
template <uint32_t RT, uint32_t CT, uint32_t WR>
__global__ void __launch_bounds__(HRT_TP_THREADS) hrt_array_taps_partial_kernel(const hrt_karray_taps P)
{
    constexpr uint32_t WC = 4u / WR, WT = RT * CT;
    constexpr uint32_t BR = WR * RT * 4u;   // (pair, time) rows of the block
    const hrt_kview &V = P.v;
    const hrt_ktgrid &G = P.g;   // the grid, also of csrc/hrt_taps_gemm.inc
    const uint32_t blk = blockIdx.x, c = blockIdx.y, link = blockIdx.z;
    const uint32_t rb = blk % G.rblocks, cb = blk / G.rblocks;
    const uint32_t rx = link / V.ntx, tx = link % V.ntx;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t wr = w / WC, wc = w % WC;           // the wave's place in the block
    const uint32_t kq = lane >> 4, col = lane & 15u;   // A / B operand: record 4 g + kq; row / tap `col` of a tile

    __shared__ float sU[HRT_TP_BATCH][BR * 4u];   // U of the block's rows g = 4 mm + q
    __shared__ float sRec[HRT_TP_BATCH][HRT_PS_REC_FLOATS];
    __shared__ sinc_rec sS[HRT_TP_BATCH];
    __shared__ uint32_t sB[HRT_TP_BATCH], sI[HRT_TP_BATCH];   // (bounce, hit) of the staged records
    __shared__ float sEl[BR][6];                               // r_i, q_j of the block's rows
    __shared__ double sT[BR];                                  // t_m of the block's rows

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

    uint32_t b = 0, cur = 0, end = 0;
    chunk_range(V, 0, tx, c, cur, end);
    for (;;) {
        const uint32_t n = fill_batch<HRT_TP_BATCH>(V, rx, tx, c, lane, w, b, cur, end, sB, sI);
        if (n == 0) break;
        __syncthreads();
        if (tid < HRT_TP_BATCH) {   // the record's fields, departure direction and sinc parameters (zeros past n)
            float *R = sRec[tid];
            sinc_rec q = {0, 0.f, 0.f};
            if (tid < n) {
                // stage_record (csrc/hrt_pathsum.h), written out as in hrt_array_partial_kernel: through the helper
                // the <1, 4, 1> form ran 1.4 % slower on C3 (8.30 against 8.19 ms, run-to-run spread 0.1 %) and whole
                // calls of the <4, 4, 4> form 0.2 % (T = 64, L = 64: 1 034.9 against 1 032.6 ms, spread 0.06 %); this
                // form compiles to the instructions the kernel had before
                const uint32_t bb = sB[tid], i = sI[tid];
                R[0] = rec_field(V, bb, rx, HRT_REC_A_TE_RE)[i];
                R[1] = rec_field(V, bb, rx, HRT_REC_A_TE_IM)[i];
                R[2] = rec_field(V, bb, rx, HRT_REC_A_TM_RE)[i];
                R[3] = rec_field(V, bb, rx, HRT_REC_A_TM_IM)[i];
                R[4] = rec_field(V, bb, rx, HRT_REC_TAU)[i];
                R[5] = __uint_as_float(hit_field(V, bb, HRT_HIT_FS0)[i]) - rec_field(V, bb, rx, HRT_REC_DFS)[i];
                R[6] = rec_field(V, bb, rx, HRT_REC_DIRX)[i];
                R[7] = rec_field(V, bb, rx, HRT_REC_DIRY)[i];
                R[8] = rec_field(V, bb, rx, HRT_REC_DIRZ)[i];
                const hrt_launch_dir_t d = hit_launch_dir(V, P.sh, bb, tx, i);
                R[9] = d.fx;
                R[10] = d.fy;
                R[11] = d.fz;
                q = sinc_prep(G.fs, R[4]);
            } else {
                for (uint32_t f = 0; f < HRT_PS_REC_FLOATS; ++f) R[f] = 0.f;
            }
            sS[tid] = q;
        }
        __syncthreads();
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
        __syncthreads();
    }

#undef HRT_TG_U
#define HRT_TG_PART 3
#include "hrt_taps_gemm.inc"
}

// one thread per output (link, pair, pol, m, i): the chunks in order, + LoS, -> out
__global__ void hrt_array_taps_reduce_kernel(const hrt_karray_taps P)
{
    const hrt_kview &V = P.v;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    hrt_taps_output o;
    if (!taps_output(V, P.g, P.npairs, P.partial, gid, o)) return;
    float2 s = o.s;
    hrt_los_entry L;
    if (V.los && los_entry(V, o.link, L)) {   // a real: TE = TM
        const uint32_t i = o.pair / P.nt, j = o.pair - i * P.nt;
        const float u_tx[3] = {L.ux, L.uy, L.uz}, u_rx[3] = {-L.ux, -L.uy, -L.uz};
        const double pr = dot3(P.rx_el + 3u * i, u_rx), pt = dot3(P.tx_el + 3u * j, u_tx);
        float sn, cs;
        sincospif(half_revs(taps_los_phase(P.g, o.m, L) + P.fa_c * (pr + pt)), &sn, &cs);
        const float v = taps_los_weight(P.g, o.tap, L);
        s.x += v * cs;
        s.y += v * sn;
    }
    store_out(reinterpret_cast<float2 *>(P.out) + gid, s, V.accumulate);
}

extern "C" int hrt_hip_launch_array_taps(const hrt_karray_taps *P, void *stream)
{
    return launch_taps_family<hrt_karray_taps>(P, P->g, P->npairs, HRT_TP_THREADS,
                                               hrt_array_taps_partial_kernel<4u, 4u, 4u>,
                                               hrt_array_taps_partial_kernel<1u, 4u, 1u>, NULL,
                                               hrt_array_taps_reduce_kernel, stream);
}
