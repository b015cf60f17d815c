// hrt_sparse_beam.hip -- beamformed (codebook) channel responses from dominant-path lists, for gfx950.  The input is a
// buffer of hrt_dominant_paths' layout (header {kept, eligible} per link, then max_paths 72-byte slots per link); for
// every link, RX beam a, TX beam b and polarisation, with n = min(kept[link], max_paths):
//
//     B[link, a, b, pol, m, k] = sum_{p < n} a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p)) g_rx[a](u_rx_p) g_tx[b](u_tx_p)
//     g_rx[a](u) = sum_i conj(W_rx[a, i]) exp(j 2 pi f_a r_i . u / c),  g_tx[b](u) = sum_j W_tx[b, j] exp(j 2 pi f_a q_j . u / c)
//
//   hrt_sparse_beam_kernel  one workgroup (4 waves) per (pair block x column block, link): the complex GEMM of
//                           csrc/hrt_beam_channel.h (parts 1 .. 3 of csrc/hrt_pair_gemm.inc, beam pairs for rows) over
//                           ALL of the link's slots, walked in index order HRT_AC_BATCH at a time and staged as
//                           hrt_sparse_channel_kernel stages them (six 8-byte loads per slot, stage_record's order).
//                           Its S stage is hrt_beam_partial_kernel's: per batch the gain stage of
//                           csrc/hrt_beam_gains.inc (part 1) and G = g_rx g_tx as the A operand of each lane.  The
//                           accumulators are written straight to out.
// One workgroup owns its outputs and sums a link's slots in one fixed order: every byte of out is written exactly once
// (or added to once), no atomics, no scratch, and two calls with the same input give the same bytes.  A workgroup reads
// only its own link's header entry and slots < n: what the other slots or links hold cannot reach its outputs.  The
// LoS entry is an ordinary slot; power, path, bounce and tri are not read.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_channel.h"
#include "hrt_pathsum.h"
#include "hrt_sparse_beam.h"

#define HRT_SB_SLOTS (HRT_AC_BATCH * HRT_AC_PAIRS / HRT_AC_THREADS)   // (record, beam) gains per thread and side

static_assert(HRT_AC_BATCH == 32u && HRT_AC_PAIRS == 32u && HRT_BM_ETILE == 32u, "the index arithmetic of the S stage");
static_assert(HRT_PS_REC_FLOATS * 4u + HRT_SP_SLOT_FIRST == HRT_SP_SLOT_BYTES && HRT_SP_SLOT_BYTES % 8u == 0 &&
                  HRT_SP_SLOT_FIRST % 8u == 0,
              "a slot's staged floats: its last 48 bytes, 8-byte aligned");
static_assert(HRT_AC_BATCH * (HRT_PS_REC_FLOATS / 2u) <= HRT_AC_THREADS, "one 8-byte load per thread stages a batch");

__global__ void __launch_bounds__(HRT_AC_THREADS) hrt_sparse_beam_kernel(const hrt_ksparse_beam P)
{
    const uint32_t blk = blockIdx.x, link = blockIdx.y;
    const uint32_t pb = blk % P.g.pblocks, cb = blk / P.g.pblocks;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t h = lane >> 5, k2 = lane & 15u, rsub = (lane >> 4) & 1u;

    __shared__ float sRec[HRT_AC_BATCH][HRT_PS_REC_FLOATS];
    __shared__ float4 sU[HRT_AC_BATCH][HRT_AC_GROWS];        // a_te U, a_tm U (complex) of the block's rows g
    __shared__ float4 sV[HRT_AC_BATCH][HRT_CH_K2];           // (Re V, -Im V, Im V, Re V): B = u . half h
    __shared__ float sA[HRT_AC_BATCH][2][64];                // the A operand of every lane, per pair tile
    __shared__ float2 sE[HRT_BM_ETILE][HRT_AC_BATCH];        // phase factors of one element tile: [element][slot]
    __shared__ float2 sW[HRT_AC_PAIRS][HRT_BM_ETILE + 1u];   // weights of the touched beams: [beam slot][element]
    __shared__ float2 sG[2][HRT_AC_PAIRS][HRT_AC_BATCH + 1u];   // gains: [side][beam slot][slot]

    // the link's live slots: the header's kept, never more than the list holds (the same for every thread)
    const uint64_t kept = reinterpret_cast<const uint64_t *>(P.paths)[2u * link];
    const uint32_t nlive = kept < P.max_paths ? (uint32_t)kept : P.max_paths;
    if (nlive == 0 && P.accumulate) return;   // nothing to add: out stays as it is

    // the beams of this block's pairs p0 .. p0 + 31: RX slot s is beam a0 + s; TX slot s is beam s where every TX
    // beam fits (Bt <= 32), else the beam of pair p0 + s
    const uint32_t p0 = pb * HRT_AC_PAIRS;
    const uint32_t a0 = p0 / P.bt;
    const uint32_t na = (min(p0 + HRT_AC_PAIRS, P.npairs) - 1u) / P.bt - a0 + 1u, nb = min(P.bt, HRT_AC_PAIRS);
    const bool tx_all = P.bt <= HRT_AC_PAIRS;

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
        __syncthreads();
#define HRT_PG_PART 2
#include "hrt_pair_gemm.inc"
        // S: the gains of the touched beams at every staged slot
#define HRT_BG_BATCH HRT_AC_BATCH
#define HRT_BG_THREADS HRT_AC_THREADS
#define HRT_BG_SLOTS HRT_SB_SLOTS
#define HRT_BG_E(e, j) sE[e][j]
#define HRT_BG_W(s, e) sW[s][e]
#define HRT_BG_P0 p0
#define HRT_BG_FA_C P.g.fa_c
#define HRT_BG_PART 1
#include "hrt_beam_gains.inc"
        __syncthreads();
#pragma unroll 1
        for (uint32_t e = tid; e < n * HRT_AC_PAIRS; e += HRT_AC_THREADS) {   // G, as the A operand of each lane
            const uint32_t j = e / HRT_AC_PAIRS, q = e % HRT_AC_PAIRS, pair = p0 + q;
            float gr = 0.f, gi = 0.f;   // padded pairs: A = 0
            if (pair < P.npairs) {
                const uint32_t a = pair / P.bt, bb = pair - a * P.bt;
                const float2 x = sG[0][a - a0][j], y = sG[1][tx_all ? bb : q][j];
                gr = fmaf(x.x, y.x, -(x.y * y.y));
                gi = fmaf(x.x, y.y, x.y * y.x);
            }
            float *A = sA[j][q >> 4];
            const uint32_t row = q & 15u;
            A[row] = gr;        // Re B row, k = 0: Re G
            A[row + 32u] = -gi; // Re B row, k = 1: -Im G
            A[row + 16u] = gi;  // Im B row, k = 0: Im G
            A[row + 48u] = gr;  // Im B row, k = 1: Re G
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

extern "C" int hrt_hip_launch_sparse_beam(const hrt_ksparse_beam *P, void *stream)
{
    hipLaunchKernelGGL(hrt_sparse_beam_kernel, dim3(P->g.pblocks * P->g.cblocks, P->links), dim3(HRT_AC_THREADS), 0,
                       (hipStream_t)stream, *P);
    return (int)hipGetLastError();
}
