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

__global__ void __launch_bounds__(HRT_AC_THREADS) hrt_array_partial_kernel(const hrt_karray P)
{
    const hrt_kview &V = P.v;
    const uint32_t blk = blockIdx.x, c = blockIdx.y, link = blockIdx.z;
    const uint32_t pb = blk % P.g.pblocks, cb = blk / P.g.pblocks;
    const uint32_t rx = link / V.ntx, tx = link % V.ntx;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t h = lane >> 5, k2 = lane & 15u, rsub = (lane >> 4) & 1u;

    __shared__ float sRec[HRT_AC_BATCH][HRT_PS_REC_FLOATS];
    __shared__ float4 sU[HRT_AC_BATCH][HRT_AC_GROWS];        // a_te U, a_tm U (complex) of the block's rows g
    __shared__ float4 sV[HRT_AC_BATCH][HRT_CH_K2];           // (Re V, -Im V, Im V, Re V): B = u . half h
    __shared__ float sA[HRT_AC_BATCH][2][64];                // the A operand of every lane, per pair tile
    __shared__ float sEl[HRT_AC_PAIRS][6];                   // r_i, q_j of the block's pairs
    __shared__ uint32_t sB[HRT_AC_BATCH], sI[HRT_AC_BATCH];  // (bounce, hit) of the staged records

    const uint32_t p0 = pb * HRT_AC_PAIRS;
    if (tid < HRT_AC_PAIRS) {
        const uint32_t a = p0 + tid;
        float e[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (a < P.npairs) load_pair(P.rx_el, P.tx_el, P.nt, a, e);
        for (int q = 0; q < 6; ++q) sEl[tid][q] = e[q];
    }

#define HRT_PG_PART 1
#include "hrt_pair_gemm.inc"

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
#define HRT_PG_PART 2
#include "hrt_pair_gemm.inc"
#pragma unroll 1
        for (uint32_t e = tid; e < n * HRT_AC_PAIRS; e += HRT_AC_THREADS) {   // S, as the A operand of each lane
            const uint32_t j = e / HRT_AC_PAIRS, q = e % HRT_AC_PAIRS;
            const float *R = sRec[j], *E = sEl[q];
            float sn = 0.f, cs = 0.f;
            if (p0 + q < P.npairs) {
                const double pr = dot3(E, R + 6), pt = dot3(E + 3, R + 9);   // r_i . u_rx, q_j . u_tx
                sincospif(half_revs(P.g.fa_c * (pr + pt)), &sn, &cs);
            }
            float *A = sA[j][q >> 4];
            const uint32_t row = q & 15u;
            A[row] = cs;        // Re H row, k = 0: Re S
            A[row + 32u] = -sn; // Re H row, k = 1: -Im S
            A[row + 16u] = sn;  // Im H row, k = 0: Im S
            A[row + 48u] = cs;  // Im H row, k = 1: Re S
        }
        __syncthreads();
#define HRT_PG_PART 3
#include "hrt_pair_gemm.inc"
        __syncthreads();
    }

#define HRT_PG_PART 4
#include "hrt_pair_gemm.inc"
}

// one thread per output (link, pair, pol, m, k): the chunks in order, + LoS, -> out
__global__ void hrt_array_reduce_kernel(const hrt_karray P)
{
    const hrt_kview &V = P.v;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    hrt_pair_output o;
    if (!pair_output(V, P.g, P.npairs, P.partial, gid, o)) return;
    float2 s = o.s;
    hrt_los_entry L;
    if (V.los && los_entry(V, o.link, L)) {
        const uint32_t i = o.pair / P.nt, j = o.pair - i * P.nt;
        const float u_tx[3] = {L.ux, L.uy, L.uz}, u_rx[3] = {-L.ux, -L.uy, -L.uz};
        const double pr = dot3(P.rx_el + 3u * i, u_rx), pt = dot3(P.tx_el + 3u * j, u_tx);
        float sn, cs;
        sincospif(half_revs(pair_los_phase(P.g, o.col, L.tau, L.nu) + P.g.fa_c * (pr + pt)), &sn, &cs);
        s.x += L.a * cs;
        s.y += L.a * sn;
    }
    store_out(reinterpret_cast<float2 *>(P.out) + gid, s, V.accumulate);
}

extern "C" int hrt_hip_launch_array_channel(const hrt_karray *P, void *stream)
{
    return launch_pair_family<hrt_karray>(P, HRT_AC_THREADS, hrt_array_partial_kernel, nullptr, hrt_array_reduce_kernel,
                                          stream);
}
