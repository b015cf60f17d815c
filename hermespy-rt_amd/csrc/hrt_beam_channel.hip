// hrt_beam_channel.hip -- beamformed (codebook) channel responses from the workspace of a finished hrt_trace, for
// gfx950.  For every link (rx, tx), RX beam a, TX beam b and polarisation:
//
//     B[rx, tx, a, b, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p)) g_rx[a](u_p^rx) g_tx[b](u_p^tx)
//     g_rx[a](u) = sum_i conj(W_rx[a, i]) exp(j 2 pi f_a r_i . u / c),  g_tx[b](u) = sum_j W_tx[b, j] exp(j 2 pi f_a q_j . u / c)
//
// over the LoS entry and every unblocked scatter record of the link: hrt_array_channel's H contracted with the
// combiner w^H and the precoder f, without H ever being formed (csrc/hrt_beam_channel.h).  Paths, parts, u_rx and
// u_tx are those of csrc/hrt_array_channel.hip; the workspace view and its readers are csrc/hrt_pathsum.h.
//   hrt_beam_partial_kernel  one workgroup (4 waves) per (pair block x column block, record chunk, link): the GEMM of
//                            csrc/hrt_pair_gemm.inc with beam pairs for rows.  Its S stage: per batch of staged
//                            records, the gain stage of csrc/hrt_beam_gains.inc (the element phase factors tile by
//                            tile in LDS, the gains of the beams the block's pairs touch, FP32 within a tile, FP64
//                            across the tiles), and G = g_rx g_tx as the A operand of each lane.
//   hrt_beam_los_kernel      per (link, pair): G at the LoS directions (u_tx = HRT_LOS_DIR, u_rx = -u_tx), FP64 sums
//                            (part 2 of csrc/hrt_beam_gains.inc).
//   hrt_beam_reduce_kernel   per output: the chunks in a fixed order, plus the LoS term, into out.
// No floating-point atomics anywhere: two calls with the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_beam_channel.h"
#include "hrt_channel.h"
#include "hrt_pathsum.h"

#define HRT_BM_SLOTS (HRT_AC_BATCH * HRT_AC_PAIRS / HRT_AC_THREADS)   // (record, beam) gains per thread and side

static_assert(HRT_AC_BATCH == 32u && HRT_AC_PAIRS == 32u && HRT_BM_ETILE == 32u, "the index arithmetic of the S stage");

__global__ void __launch_bounds__(HRT_AC_THREADS) hrt_beam_partial_kernel(const hrt_kbeam P)
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
    __shared__ float2 sE[HRT_BM_ETILE][HRT_AC_BATCH];        // phase factors of one element tile: [element][record]
    __shared__ float2 sW[HRT_AC_PAIRS][HRT_BM_ETILE + 1u];   // weights of the touched beams: [beam slot][element]
    __shared__ float2 sG[2][HRT_AC_PAIRS][HRT_AC_BATCH + 1u];   // gains: [side][beam slot][record]
    __shared__ uint32_t sB[HRT_AC_BATCH], sI[HRT_AC_BATCH];  // (bounce, hit) of the staged records

    // the beams of this block's pairs p0 .. p0 + 31: RX slot s is beam a0 + s; TX slot s is beam s where every TX
    // beam fits (Bt <= 32), else the beam of pair p0 + s
    const uint32_t p0 = pb * HRT_AC_PAIRS;
    const uint32_t a0 = p0 / P.bt;
    const uint32_t na = (min(p0 + HRT_AC_PAIRS, P.npairs) - 1u) / P.bt - a0 + 1u, nb = min(P.bt, HRT_AC_PAIRS);
    const bool tx_all = P.bt <= HRT_AC_PAIRS;

#define HRT_PG_PART 1
#include "hrt_pair_gemm.inc"

    uint32_t b = 0, cur = 0, end = 0;
    chunk_range(V, 0, tx, c, cur, end);
    for (;;) {
        const uint32_t n = fill_batch<HRT_AC_BATCH>(V, rx, tx, c, lane, w, b, cur, end, sB, sI);
        if (n == 0) break;
        __syncthreads();
        if (tid < n) stage_record(V, P.sh, sB[tid], rx, tx, sI[tid], sRec[tid]);
        __syncthreads();
#define HRT_PG_PART 2
#include "hrt_pair_gemm.inc"
        // S: the gains of the touched beams at every staged record
#define HRT_BG_BATCH HRT_AC_BATCH
#define HRT_BG_THREADS HRT_AC_THREADS
#define HRT_BG_SLOTS HRT_BM_SLOTS
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

#define HRT_PG_PART 4
#include "hrt_pair_gemm.inc"
}

// one thread per (link, pair): G at the LoS directions (part 2 of csrc/hrt_beam_gains.inc)
__global__ void hrt_beam_los_kernel(const hrt_kbeam P)
{
#define HRT_BG_FA_C P.g.fa_c
#define HRT_BG_PART 2
#include "hrt_beam_gains.inc"
}

// one thread per output (link, pair, pol, m, k): the chunks in order, + LoS, -> out
__global__ void hrt_beam_reduce_kernel(const hrt_kbeam P)
{
    const hrt_kview &V = P.v;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    hrt_pair_output o;
    if (!pair_output(V, P.g, P.npairs, P.partial, gid, o)) return;
    float2 s = o.s;
    hrt_los_entry L;
    if (V.los && los_entry(V, o.link, L)) {
        const float2 G = reinterpret_cast<const float2 *>(P.los)[(uint64_t)o.link * P.npairs + o.pair];
        float sn, cs;
        sincospif(half_revs(pair_los_phase(P.g, o.col, L.tau, L.nu)), &sn, &cs);
        s.x += L.a * fmaf(cs, G.x, -(sn * G.y));
        s.y += L.a * fmaf(cs, G.y, sn * G.x);
    }
    store_out(reinterpret_cast<float2 *>(P.out) + gid, s, V.accumulate);
}

extern "C" int hrt_hip_launch_beam_channel(const hrt_kbeam *P, void *stream)
{
    return launch_pair_family<hrt_kbeam>(P, HRT_AC_THREADS, hrt_beam_partial_kernel, hrt_beam_los_kernel,
                                         hrt_beam_reduce_kernel, stream);
}
