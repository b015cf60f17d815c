// hrt_sparse_channel.hip -- antenna-array (MIMO) channel responses from dominant-path lists, for gfx950.  The input
// is a buffer of hrt_dominant_paths' layout (header {kept, eligible} per link, then max_paths 72-byte slots per link);
// for every link, element pair (i, j) and polarisation, with n = min(kept[link], max_paths):
//
//     H[link, i, j, pol, m, k] = sum_{p < n} a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p)) exp(j 2 pi f_a (r_i . u_rx_p + q_j . u_tx_p) / c)
//
//   hrt_sparse_channel_kernel  one workgroup (4 waves) per (pair block x column block, link): the complex GEMM of
//                              csrc/hrt_array_channel.h on v_mfma_f32_32x32x2_f32 (parts 1 .. 3 of
//                              csrc/hrt_pair_gemm.inc, as hrt_array_partial_kernel runs them) over ALL of the link's
//                              slots, walked in index order HRT_AC_BATCH at a time, the accumulators written straight to
//                              out.  A slot's twelve floats from a_te_re on are staged into LDS in stage_record's order
//                              (csrc/hrt_pathsum.h) as six 8-byte loads per slot: a batch is one contiguous run of
//                              slots, so consecutive lanes read consecutive 8-byte words of 48 in every 72 bytes.
// One workgroup owns its outputs and sums a link's slots in one fixed order: every byte of out is written exactly once
// (or added to once), no atomics, no scratch, and two calls with the same input give the same bytes.  A workgroup reads
// only its own link's header entry and slots < n: what the other slots or links hold cannot reach its outputs.  The
// LoS entry is an ordinary slot; power, path, bounce and tri are not read.  Every phase is reduced in FP64 to a fraction
// of a revolution and evaluated with an f32 sincospi, as in the array kernel.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_channel.h"
#include "hrt_pathsum.h"
#include "hrt_sparse_channel.h"

static_assert(HRT_PS_REC_FLOATS * 4u + HRT_SP_SLOT_FIRST == HRT_SP_SLOT_BYTES && HRT_SP_SLOT_BYTES % 8u == 0 &&
                  HRT_SP_SLOT_FIRST % 8u == 0,
              "a slot's staged floats: its last 48 bytes, 8-byte aligned");
static_assert(HRT_AC_BATCH * (HRT_PS_REC_FLOATS / 2u) <= HRT_AC_THREADS, "one 8-byte load per thread stages a batch");

__global__ void __launch_bounds__(HRT_AC_THREADS) hrt_sparse_channel_kernel(const hrt_ksparse P)
{
    const uint32_t blk = blockIdx.x, link = blockIdx.y;
    const uint32_t pb = blk % P.g.pblocks, cb = blk / P.g.pblocks;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t h = lane >> 5, k2 = lane & 15u, rsub = (lane >> 4) & 1u;

    __shared__ float sRec[HRT_AC_BATCH][HRT_PS_REC_FLOATS];
    __shared__ float4 sU[HRT_AC_BATCH][HRT_AC_GROWS];        // a_te U, a_tm U (complex) of the block's rows g
    __shared__ float4 sV[HRT_AC_BATCH][HRT_CH_K2];           // (Re V, -Im V, Im V, Re V): B = u . half h
    __shared__ float sA[HRT_AC_BATCH][2][64];                // the A operand of every lane, per pair tile
    __shared__ float sEl[HRT_AC_PAIRS][6];                   // r_i, q_j of the block's pairs

    // the link's live slots: the header's kept, never more than the list holds (the same for every thread)
    const uint64_t kept = reinterpret_cast<const uint64_t *>(P.paths)[2u * link];
    const uint32_t nlive = kept < P.max_paths ? (uint32_t)kept : P.max_paths;
    if (nlive == 0 && P.accumulate) return;   // nothing to add: out stays as it is

    const uint32_t p0 = pb * HRT_AC_PAIRS;
    if (tid < HRT_AC_PAIRS) {
        const uint32_t a = p0 + tid;
        float e[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (a < P.npairs) load_pair(P.rx_el, P.tx_el, P.nt, a, e);
        for (int q = 0; q < 6; ++q) sEl[tid][q] = e[q];
    }

#define HRT_PG_PART 1
#include "hrt_pair_gemm.inc"

    const uint8_t *slots = P.paths + 16ull * P.links + (uint64_t)link * P.max_paths * HRT_SP_SLOT_BYTES;
    for (uint32_t s0 = 0; s0 < nlive; s0 += HRT_AC_BATCH) {
        const uint32_t n = min(nlive - s0, HRT_AC_BATCH);
        if (tid < n * (HRT_PS_REC_FLOATS / 2u)) {   // slot s0 + j, floats 2 q and 2 q + 1 of its twelve
            const uint32_t j = tid / (HRT_PS_REC_FLOATS / 2u), q = tid % (HRT_PS_REC_FLOATS / 2u);
            const float2 v = *reinterpret_cast<const float2 *>(slots + (uint64_t)(s0 + j) * HRT_SP_SLOT_BYTES +
                                                               HRT_SP_SLOT_FIRST + 8u * q);
            *reinterpret_cast<float2 *>(&sRec[j][2u * q]) = v;
        }
        __syncthreads();   // (the first pass: sEl too)
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

    // D: lane = column, register r = row (r & 3) + 8 (r >> 2) + 4 h; rows 0..15 Re, 16..31 Im of 16 pairs (part 4 of
    // csrc/hrt_pair_gemm.inc), to out[link][pair][pol][m][k]: the 16 lanes of a k2 run store 16 consecutive float2
    const uint64_t tk = (uint64_t)P.g.T * P.g.K;
    float2 *dst = reinterpret_cast<float2 *>(P.out) + (uint64_t)link * P.npairs * 2u * tk;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const uint32_t g = cb * HRT_AC_GROWS + 4u * w + 2u * t + rsub;
        const uint32_t m = g / P.g.K1, k = (g - m * P.g.K1) * HRT_CH_K2 + k2;
        const bool col_ok = g < P.g.rows && k < P.g.K;
        float2 *d = dst + (uint64_t)m * P.g.K + k;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const uint32_t pair = p0 + 16u * a + (r & 3) + 8u * (r >> 2) + 4u * h;
                    if (col_ok && pair < P.npairs)
                        store_out(d + ((uint64_t)pair * 2u + q) * tk, make_float2(acc[a][t][q][r], acc[a][t][q][r + 8]),
                                  P.accumulate);
                }
    }
}

extern "C" int hrt_hip_launch_sparse_channel(const hrt_ksparse *P, void *stream)
{
    hipLaunchKernelGGL(hrt_sparse_channel_kernel, dim3(P->g.pblocks * P->g.cblocks, P->links), dim3(HRT_AC_THREADS), 0,
                       (hipStream_t)stream, *P);
    return (int)hipGetLastError();
}
