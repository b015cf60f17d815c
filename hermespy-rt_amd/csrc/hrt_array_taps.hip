// hrt_array_taps.hip -- antenna-array (MIMO) sampled impulse responses from the workspace of a finished hrt_trace,
// for gfx950.  For every link (rx, tx), element pair (i, j), polarisation, time sample m and tap l_k = l_min + k:
//
//     h[rx, tx, i, j, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p))
//                                        * exp(j 2 pi f_a (r_i . u_rx + q_j . u_tx) / c) sinc(l_k - f_s tau_p)
//
// over the LoS entry (hrt_array_taps_reduce_kernel) and every unblocked scatter record (hrt_array_taps_partial_kernel)
// of the link.  The TX segments of the hit blocks come from hrt_channel_segments_kernel (csrc/hrt_channel.hip); the
// workspace view, its readers and the batch fill are csrc/hrt_pathsum.h; the sinc weights csrc/hrt_sinc.h.
//   hrt_array_taps_partial_kernel  one workgroup (4 waves) per (row block x column block, record chunk, link): the
//                                  real GEMM of csrc/hrt_array_taps.h on v_mfma_f32_16x16x4_f32, partial sums to the
//                                  scratch.  The unblocked records of the chunk are compacted by mask ballots and
//                                  staged HRT_TP_BATCH at a time: their fields, departure direction and sinc
//                                  parameters, then U over the block's (pair, time) rows in LDS (steering and phase
//                                  in one sincospi); every lane forms its own B operand V (one record, one tap) in
//                                  registers, as hrt_taps_partial_kernel does.
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
#include "hrt_sinc.h"

typedef float hrt_f32x4 __attribute__((ext_vector_type(4)));

// RT row tiles x CT column tiles per wave; the 4 waves of the block stand WR along the rows and 4 / WR along the
// columns (the two forms of csrc/hrt_array_taps.h: <4, 4, 4> and <1, 4, 1>)
template <uint32_t RT, uint32_t CT, uint32_t WR>
__global__ void __launch_bounds__(HRT_TP_THREADS) hrt_array_taps_partial_kernel(const hrt_karray_taps P)
{
    constexpr uint32_t WC = 4u / WR, WT = RT * CT;
    constexpr uint32_t BR = WR * RT * 4u;   // (pair, time) rows of the block
    const hrt_kview &V = P.v;
    const uint32_t blk = blockIdx.x, c = blockIdx.y, link = blockIdx.z;
    const uint32_t rb = blk % P.rblocks, cb = blk / P.rblocks;
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
        if (row < P.rows) {
            const uint32_t a = row / P.T, m = row - a * P.T;
            load_pair(P.rx_el, P.tx_el, P.nt, a, e);
            t = P.t0 + (double)m * P.dt;
        }
        for (int q = 0; q < 6; ++q) sEl[tid][q] = e[q];
        sT[tid] = t;
    }

    // this wave's first row tile and column tile
    const uint32_t r0 = (rb * WR + wr) * RT, c0 = (cb * WC + wc) * CT;
    bool live[WT];
    int32_t tap[CT];
#pragma unroll
    for (uint32_t t = 0; t < WT; ++t) live[t] = r0 + t / CT < P.rtiles && c0 + t % CT < P.ctiles;
#pragma unroll
    for (uint32_t t = 0; t < CT; ++t) tap[t] = P.l_min + (int32_t)((c0 + t) * 16u + col);
    hrt_f32x4 acc[WT];
#pragma unroll
    for (uint32_t t = 0; t < WT; ++t) acc[t] = hrt_f32x4{0.f, 0.f, 0.f, 0.f};

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
                q = sinc_prep(P.fs, R[4]);
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
            if (j < n && rb * BR + mm < P.rows) {
                const double pr = dot3(E, R + 6), pt = dot3(E + 3, R + 9);   // r_i . u_rx, q_j . u_tx
                float sn, cs;
                sincospif(half_revs((double)R[5] * sT[mm] - P.fc * (double)R[4] + P.fa_c * (pr + pt)), &sn, &cs);
                u0 = R[0] * cs - R[1] * sn;
                u1 = R[0] * sn + R[1] * cs;
                u2 = R[2] * cs - R[3] * sn;
                u3 = R[2] * sn + R[3] * cs;
            }
            float *U = &sU[j][4u * mm];
            U[0] = u0; U[1] = u1; U[2] = u2; U[3] = u3;
        }
        __syncthreads();
        for (uint32_t g = 0; 4u * g < n; ++g) {
            const uint32_t j = 4u * g + kq;
            const sinc_rec q = sS[j];
            float v[CT];
#pragma unroll
            for (uint32_t t = 0; t < CT; ++t) v[t] = sinc_tap(tap[t], q);
#pragma unroll
            for (uint32_t rt = 0; rt < RT; ++rt) {
                const float a = sU[j][(wr * RT + rt) * 16u + col];
#pragma unroll
                for (uint32_t t = 0; t < CT; ++t)
                    if (live[rt * CT + t])
                        acc[rt * CT + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, v[t], acc[rt * CT + t], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // D: lane = (row group kq, column col), register q: row 4 kq + q of the tile = ((pair, time) row 4 R + kq, part q)
    const uint64_t tl = (uint64_t)P.T * P.L;
    float2 *dst = reinterpret_cast<float2 *>(P.partial) + ((uint64_t)link * V.nchunks + c) * 2u * P.npairs * tl;
#pragma unroll
    for (uint32_t t = 0; t < WT; ++t) {
        const uint32_t row = (r0 + t / CT) * 4u + kq, i = (c0 + t % CT) * 16u + col;
        if (live[t] && row < P.rows && i < P.L) {
            const uint32_t a = row / P.T, m = row - a * P.T;
            float2 *d = dst + ((uint64_t)a * 2u * P.T + m) * P.L + i;
            d[0] = make_float2(acc[t][0], acc[t][1]);
            d[tl] = make_float2(acc[t][2], acc[t][3]);
        }
    }
}

// one thread per output (link, pair, pol, m, i): the chunks in order, + LoS, -> out
__global__ void hrt_array_taps_reduce_kernel(const hrt_karray_taps P)
{
    const hrt_kview &V = P.v;
    const uint64_t tl = (uint64_t)P.T * P.L;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t per_link = (uint64_t)P.npairs * 2u * tl;
    if (gid >= per_link * V.nrx * V.ntx) return;
    const uint32_t link = (uint32_t)(gid / per_link);
    const uint64_t e = gid - (uint64_t)link * per_link;   // = (pair * 2 + pol) * tl + m * L + i

    const float2 *src = reinterpret_cast<const float2 *>(P.partial) + (uint64_t)link * V.nchunks * per_link + e;
    float2 s = sum_chunks(src, V.nchunks, per_link);
    hrt_los_entry L;
    if (V.los && los_entry(V, link, L)) {   // a real: TE = TM
        const uint32_t pair = (uint32_t)(e / (2u * tl));
        const uint32_t i = pair / P.nt, j = pair - i * P.nt;
        const float u_tx[3] = {L.ux, L.uy, L.uz}, u_rx[3] = {-L.ux, -L.uy, -L.uz};
        const double pr = dot3(P.rx_el + 3u * i, u_rx), pt = dot3(P.tx_el + 3u * j, u_tx);
        const uint64_t mi = e % tl;
        const uint32_t m = (uint32_t)(mi / P.L), k = (uint32_t)(mi % P.L);
        const double t = P.t0 + (double)m * P.dt;
        float sn, cs;
        sincospif(half_revs((double)L.nu * t - P.fc * (double)L.tau + P.fa_c * (pr + pt)), &sn, &cs);
        const float v = L.a * sinc_tap(P.l_min + (int32_t)k, sinc_prep(P.fs, L.tau));
        s.x += v * cs;
        s.y += v * sn;
    }
    store_out(reinterpret_cast<float2 *>(P.out) + gid, s, V.accumulate);
}

extern "C" int hrt_hip_launch_array_taps(const hrt_karray_taps *P, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint32_t links = P->v.nrx * P->v.ntx;
    if (P->v.nchunks) {
        const int e = hrt_hip_launch_segments(&P->v, stream);
        if (e) return e;
        const dim3 grid(P->rblocks * P->cblocks, P->v.nchunks, links);
        if (P->rt == 4u)
            hipLaunchKernelGGL((hrt_array_taps_partial_kernel<4u, 4u, 4u>), grid, dim3(HRT_TP_THREADS), 0, st, *P);
        else
            hipLaunchKernelGGL((hrt_array_taps_partial_kernel<1u, 4u, 1u>), grid, dim3(HRT_TP_THREADS), 0, st, *P);
    }
    const uint64_t n = (uint64_t)links * P->npairs * 2u * P->T * P->L;
    hipLaunchKernelGGL(hrt_array_taps_reduce_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, st, *P);
    return (int)hipGetLastError();
}
