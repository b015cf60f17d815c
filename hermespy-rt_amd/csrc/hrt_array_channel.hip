// hrt_array_channel.hip -- antenna-array (MIMO) channel responses from the workspace of a finished hrt_trace,
// for gfx950.  For every link (rx, tx), element pair (i, j) and polarisation:
//
//     H[rx, tx, i, j, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p)) exp(j 2 pi f_a (r_i . u_rx + q_j . u_tx) / c)
//
// over the LoS entry (hrt_array_reduce_kernel) and every unblocked scatter record (hrt_array_partial_kernel) of
// the link.  The TX segments of the hit blocks come from hrt_channel_segments_kernel (csrc/hrt_channel.hip); the
// workspace view and its readers are csrc/hrt_pathsum.h.
//   hrt_array_partial_kernel  one workgroup (4 waves) per (pair block x column block, record chunk, link): the
//                             complex GEMM of csrc/hrt_array_channel.h on v_mfma_f32_32x32x2_f32, partial sums to
//                             the scratch.  The unblocked records of the chunk are compacted by mask ballots and
//                             staged HRT_AC_BATCH at a time: their fields, then S (one sincos per element pair),
//                             U over the block's rows (m, k1) and V over k2 in LDS, then one MFMA per record, pair
//                             tile, column tile and polarisation.
//   hrt_array_reduce_kernel   per output: the chunks in a fixed order, plus the LoS term, into out.
// No floating-point atomics anywhere: two calls with the same inputs give the same bits.
//
// u_rx is the record's HRT_REC_DIR (directions_rx); u_tx the launch direction of the record's ray (RaysInfo
// bounce 0), evaluated here from the global path with the float/double sequence of hrt_launch_dirs_kernel
// (csrc/hrt_launch_dir.h) -- independent of the trace's direction table and its order.  Every phase is reduced
// in FP64 to a fraction of a revolution (f tau and f_a r . u / c reach hundreds of revolutions) and evaluated with
// an f32 sincospi.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_array_channel.h"
#include "hrt_channel.h"
#include "hrt_pathsum.h"

typedef float hrt_f32x16 __attribute__((ext_vector_type(16)));

__global__ void __launch_bounds__(HRT_AC_THREADS) hrt_array_partial_kernel(const hrt_karray P)
{
    const hrt_kview &V = P.v;
    const uint32_t blk = blockIdx.x, c = blockIdx.y, link = blockIdx.z;
    const uint32_t pb = blk % P.pblocks, cb = blk / P.pblocks;
    const uint32_t rx = link / V.ntx, tx = link % V.ntx;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t h = lane >> 5, k2 = lane & 15u, rsub = (lane >> 4) & 1u;

    __shared__ float sRec[HRT_AC_BATCH][HRT_PS_REC_FLOATS];
    __shared__ float4 sU[HRT_AC_BATCH][HRT_AC_GROWS];        // a_te U, a_tm U (complex) of the block's rows g
    __shared__ float4 sV[HRT_AC_BATCH][HRT_CH_K2];           // (Re V, -Im V, Im V, Re V): B = u . half h
    __shared__ float sA[HRT_AC_BATCH][2][64];                // the A operand of every lane, per pair tile
    __shared__ float sEl[HRT_AC_PAIRS][6];                   // r_i, q_j of the block's pairs
    __shared__ uint32_t sB[HRT_AC_BATCH], sI[HRT_AC_BATCH];  // (bounce, hit) of the staged records

    if (tid < HRT_AC_PAIRS) {
        const uint32_t a = pb * HRT_AC_PAIRS + tid;
        float e[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (a < P.npairs) load_pair(P.rx_el, P.tx_el, P.nt, a, e);
        for (int q = 0; q < 6; ++q) sEl[tid][q] = e[q];
    }

    // the MFMA tiles of this wave: pair tiles 0, 1 of the block; column tiles 2w, 2w + 1 (rows g 4w .. 4w + 3)
    const bool live_p1 = pb * HRT_AC_PAIRS + 16u < P.npairs;
    const bool live_c0 = cb * HRT_AC_GROWS + 4u * w < P.rows;
    const bool live_c1 = cb * HRT_AC_GROWS + 4u * w + 2u < P.rows;
    hrt_f32x16 acc[2][2][2];   // [pair tile][column tile][pol]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][t][q][r] = 0.f;

    uint32_t b = 0, cur = 0, end = 0;
    chunk_range(V, 0, tx, c, cur, end);
    for (;;) {
        // the batch fill of fill_batch (csrc/hrt_pathsum.h), written out: through the helper the compiler schedules
        // this kernel's staging differently (376 VGPRs instead of 384) and the kernel ran about 1 % slower on C3
        uint32_t n = 0;
        while (n < HRT_AC_BATCH && b < V.nb) {
            if (cur >= end) {
                if (++b < V.nb) chunk_range(V, b, tx, c, cur, end);
                continue;
            }
            const uint32_t i = cur + lane;
            const uint64_t *mask = mask_row(V, b, rx);
            const bool live = i < end && ((mask[i >> 6] >> (i & 63u)) & 1u);
            const uint64_t bal = __ballot(live);
            const uint32_t cnt = __popcll(bal), take = min(cnt, HRT_AC_BATCH - n);
            const uint32_t rank = __popcll(bal & ((1ull << lane) - 1ull));
            if (w == 0 && live && rank < take) {
                sB[n + rank] = b;
                sI[n + rank] = i;
            }
            if (take < cnt) {   // resume at the first live record not taken
                uint64_t rest = bal;
                for (uint32_t t = 0; t < take; ++t) rest &= rest - 1ull;
                cur += (uint32_t)__builtin_ctzll(rest);
            } else {
                cur += 64u;
            }
            n += take;
        }
        if (n == 0) break;
        __syncthreads();
        if (tid < n) {
            // stage_record (csrc/hrt_pathsum.h), written out like the batch fill: through the helper the compiler
            // hoists the field addresses differently and this kernel ran 2.0 % slower on C3 (1 866.7 against
            // 1 830.6 ms, run-to-run spread 0.01 %); this form compiles to the instructions it had before
            const uint32_t rb = sB[tid], i = sI[tid];
            float *R = sRec[tid];
            R[0] = rec_field(V, rb, rx, HRT_REC_A_TE_RE)[i];
            R[1] = rec_field(V, rb, rx, HRT_REC_A_TE_IM)[i];
            R[2] = rec_field(V, rb, rx, HRT_REC_A_TM_RE)[i];
            R[3] = rec_field(V, rb, rx, HRT_REC_A_TM_IM)[i];
            R[4] = rec_field(V, rb, rx, HRT_REC_TAU)[i];
            R[5] = __uint_as_float(hit_field(V, rb, HRT_HIT_FS0)[i]) - rec_field(V, rb, rx, HRT_REC_DFS)[i];
            R[6] = rec_field(V, rb, rx, HRT_REC_DIRX)[i];
            R[7] = rec_field(V, rb, rx, HRT_REC_DIRY)[i];
            R[8] = rec_field(V, rb, rx, HRT_REC_DIRZ)[i];
            const hrt_launch_dir_t d = hit_launch_dir(V, P.sh, rb, tx, i);
            R[9] = d.fx;
            R[10] = d.fy;
            R[11] = d.fz;
        }
        __syncthreads();
#pragma unroll 1
        for (uint32_t e = tid; e < n * HRT_AC_GROWS; e += HRT_AC_THREADS) {   // U
            const uint32_t j = e / HRT_AC_GROWS, r = e % HRT_AC_GROWS, g = cb * HRT_AC_GROWS + r;
            const float *R = sRec[j];
            float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
            if (g < P.rows) {
                const uint32_t m = g / P.K1, k1 = g - m * P.K1;
                const double t = P.t0 + (double)m * P.dt;
                const double f = P.f0 + (double)(k1 * HRT_CH_K2) * P.df;
                float sn, cs;
                sincospif(half_revs((double)R[5] * t - f * (double)R[4]), &sn, &cs);
                u = make_float4(R[0] * cs - R[1] * sn, R[0] * sn + R[1] * cs, R[2] * cs - R[3] * sn, R[2] * sn + R[3] * cs);
            }
            sU[j][r] = u;
        }
#pragma unroll 1
        for (uint32_t e = tid; e < n * HRT_CH_K2; e += HRT_AC_THREADS) {   // V
            const uint32_t j = e / HRT_CH_K2, q = e % HRT_CH_K2;
            float sn, cs;
            sincospif(half_revs(-(double)q * P.df * (double)sRec[j][4]), &sn, &cs);
            sV[j][q] = make_float4(cs, -sn, sn, cs);
        }
#pragma unroll 1
        for (uint32_t e = tid; e < n * HRT_AC_PAIRS; e += HRT_AC_THREADS) {   // S, as the A operand of each lane
            const uint32_t j = e / HRT_AC_PAIRS, q = e % HRT_AC_PAIRS;
            const float *R = sRec[j], *E = sEl[q];
            float sn = 0.f, cs = 0.f;
            if (pb * HRT_AC_PAIRS + q < P.npairs) {
                const double pr = dot3(E, R + 6), pt = dot3(E + 3, R + 9);   // r_i . u_rx, q_j . u_tx
                sincospif(half_revs(P.fa_c * (pr + pt)), &sn, &cs);
            }
            float *A = sA[j][q >> 4];
            const uint32_t row = q & 15u;
            A[row] = cs;        // Re H row, k = 0: Re S
            A[row + 32u] = -sn; // Re H row, k = 1: -Im S
            A[row + 16u] = sn;  // Im H row, k = 0: Im S
            A[row + 48u] = cs;  // Im H row, k = 1: Re S
        }
        __syncthreads();
        const float2 *sV2 = reinterpret_cast<const float2 *>(&sV[0][0]);
        for (uint32_t j = 0; j < n; ++j) {
            const float2 v = sV2[(j * HRT_CH_K2 + k2) * 2u + h];
            const float4 u0 = sU[j][4u * w + rsub], u1 = sU[j][4u * w + 2u + rsub];
            // lane (k = h, column): h = 0 Re(U V), h = 1 Im(U V)
            const float b00 = fmaf(u0.x, v.x, u0.y * v.y), b01 = fmaf(u0.z, v.x, u0.w * v.y);
            const float b10 = fmaf(u1.x, v.x, u1.y * v.y), b11 = fmaf(u1.z, v.x, u1.w * v.y);
            const float a0 = sA[j][0][lane], a1 = sA[j][1][lane];
            if (live_c0) {
                acc[0][0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b00, acc[0][0][0], 0, 0, 0);
                acc[0][0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b01, acc[0][0][1], 0, 0, 0);
                if (live_p1) {
                    acc[1][0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b00, acc[1][0][0], 0, 0, 0);
                    acc[1][0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b01, acc[1][0][1], 0, 0, 0);
                }
            }
            if (live_c1) {
                acc[0][1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b10, acc[0][1][0], 0, 0, 0);
                acc[0][1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b11, acc[0][1][1], 0, 0, 0);
                if (live_p1) {
                    acc[1][1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b10, acc[1][1][0], 0, 0, 0);
                    acc[1][1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b11, acc[1][1][1], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // D: lane = column, register r = row (r & 3) + 8 (r >> 2) + 4 h; rows 0..15 Re H, 16..31 Im H of 16 pairs
    const uint64_t tk = (uint64_t)P.T * P.K;
    float2 *dst = reinterpret_cast<float2 *>(P.partial) + ((uint64_t)link * V.nchunks + c) * 2u * P.npairs * tk;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const uint32_t g = cb * HRT_AC_GROWS + 4u * w + 2u * t + rsub;
        const uint32_t m = g / P.K1, k = (g - m * P.K1) * HRT_CH_K2 + k2;
        const bool col_ok = g < P.rows && k < P.K;
        float2 *d = dst + (uint64_t)m * P.K + k;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const uint32_t pair = pb * HRT_AC_PAIRS + 16u * a + (r & 3) + 8u * (r >> 2) + 4u * h;
                    if (col_ok && pair < P.npairs)
                        d[((uint64_t)q * P.npairs + pair) * tk] = make_float2(acc[a][t][q][r], acc[a][t][q][r + 8]);
                }
    }
}

// one thread per output (link, pair, pol, m, k): the chunks in order, + LoS, -> out
__global__ void hrt_array_reduce_kernel(const hrt_karray P)
{
    const hrt_kview &V = P.v;
    const uint64_t tk = (uint64_t)P.T * P.K;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t per_link = (uint64_t)P.npairs * 2u * tk;
    if (gid >= per_link * V.nrx * V.ntx) return;
    const uint32_t link = (uint32_t)(gid / per_link);
    const uint64_t e = gid - (uint64_t)link * per_link;   // = (pair * 2 + pol) * tk + col
    const uint32_t pair = (uint32_t)(e / (2u * tk)), pol = (uint32_t)(e / tk) & 1u;
    const uint64_t col = e % tk;

    const float2 *src = reinterpret_cast<const float2 *>(P.partial) + (uint64_t)link * V.nchunks * per_link +
                        ((uint64_t)pol * P.npairs + pair) * tk + col;
    float2 s = sum_chunks(src, V.nchunks, per_link);
    hrt_los_entry L;
    if (V.los && los_entry(V, link, L)) {
        const uint32_t i = pair / P.nt, j = pair - i * P.nt;
        const float u_tx[3] = {L.ux, L.uy, L.uz}, u_rx[3] = {-L.ux, -L.uy, -L.uz};
        const double pr = dot3(P.rx_el + 3u * i, u_rx), pt = dot3(P.tx_el + 3u * j, u_tx);
        const uint32_t m = (uint32_t)(col / P.K), k = (uint32_t)(col % P.K);
        const double t = P.t0 + (double)m * P.dt, f = P.f0 + (double)k * P.df;
        float sn, cs;
        sincospif(half_revs((double)L.nu * t - f * (double)L.tau + P.fa_c * (pr + pt)), &sn, &cs);
        s.x += L.a * cs;
        s.y += L.a * sn;
    }
    store_out(reinterpret_cast<float2 *>(P.out) + gid, s, V.accumulate);
}

extern "C" int hrt_hip_launch_array_channel(const hrt_karray *P, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint32_t links = P->v.nrx * P->v.ntx;
    if (P->v.nchunks) {
        const int e = hrt_hip_launch_segments(&P->v, stream);
        if (e) return e;
        hipLaunchKernelGGL(hrt_array_partial_kernel, dim3(P->pblocks * P->cblocks, P->v.nchunks, links),
                           dim3(HRT_AC_THREADS), 0, st, *P);
    }
    const uint64_t n = (uint64_t)links * P->npairs * 2u * P->T * P->K;
    hipLaunchKernelGGL(hrt_array_reduce_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, st, *P);
    return (int)hipGetLastError();
}
