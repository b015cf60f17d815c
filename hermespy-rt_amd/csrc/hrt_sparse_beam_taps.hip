// hrt_sparse_beam_taps.hip -- beamformed (codebook) sampled impulse responses from dominant-path lists, for gfx950.
// The input is a buffer of hrt_dominant_paths' layout (header {kept, eligible} per link, then max_paths 72-byte slots
// per link); for every link, RX beam a, TX beam b, polarisation, time sample m and tap l_k = l_min + k, with
// n = min(kept[link], max_paths):
//
//     h[link, a, b, pol, m, k] = sum_{p < n} a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)) g_rx[a](u_rx_p) g_tx[b](u_tx_p)
//                                        * sinc(l_k - f_s tau_p)
//     g_rx[a](u) = sum_i conj(W_rx[a, i]) exp(j 2 pi f_a r_i . u / c),  g_tx[b](u) = sum_j W_tx[b, j] exp(j 2 pi f_a q_j . u / c)
//
//   hrt_sparse_beam_taps_kernel  one workgroup (4 waves) per (row block x column block, link): the real GEMM of
//                                csrc/hrt_beam_taps.h on v_mfma_f32_16x16x4_f32 (parts 1 and 2 of
//                                csrc/hrt_taps_gemm.inc, (beam pair, time) rows, in the two forms of
//                                csrc/hrt_array_taps.h) over ALL of the link's slots, walked in index order
//                                HRT_TP_BATCH at a time and staged as hrt_sparse_taps_kernel stages them (six 8-byte
//                                loads per slot, stage_record's order).  Per batch the gain stage of
//                                csrc/hrt_beam_gains.inc (part 1) for the beams the block's rows touch, then
//                                U = a^pol e^{j phase} G as a complex product (|G| is not 1), as
//                                hrt_beam_taps_partial_kernel forms it.  The accumulators are written straight to out.
// One workgroup owns its outputs and sums a link's slots in one fixed order: every byte of out is written exactly once
// (or added to once), no atomics, no scratch, and two calls with the same input give the same bytes.  A workgroup reads
// only its own link's header entry and slots < n: what the other slots or links hold cannot reach its outputs.  The
// LoS entry is an ordinary slot; power, path, bounce and tri are not read.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_pathsum.h"
#include "hrt_sparse_beam_taps.h"

static_assert(HRT_TP_BATCH == 32u && HRT_BM_ETILE == 32u && HRT_TP_THREADS == 256u, "the index arithmetic of the gain stage");
static_assert(HRT_PS_REC_FLOATS * 4u + HRT_SP_SLOT_FIRST == HRT_SP_SLOT_BYTES && HRT_SP_SLOT_BYTES % 8u == 0 &&
                  HRT_SP_SLOT_FIRST % 8u == 0,
              "a slot's staged floats: its last 48 bytes, 8-byte aligned");
static_assert(HRT_TP_BATCH * (HRT_PS_REC_FLOATS / 2u) <= HRT_TP_THREADS, "one 8-byte load per thread stages a batch");

namespace {

constexpr uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

}  // namespace

// RT row tiles x CT column tiles per wave, WR waves along the rows: the two forms of csrc/hrt_array_taps.h
template <uint32_t RT, uint32_t CT, uint32_t WR>
__global__ void __launch_bounds__(HRT_TP_THREADS) hrt_sparse_beam_taps_kernel(const hrt_ksparse_beam_taps P)
{
    constexpr uint32_t WC = 4u / WR, WT = RT * CT;
    constexpr uint32_t BR = WR * RT * 4u;   // (pair, time) rows of the block = its capacity in pairs and beam slots
    constexpr uint32_t SLOTS = umax(1u, HRT_TP_BATCH * BR / HRT_TP_THREADS);   // (slot, beam) gains per thread and side
    constexpr uint32_t WS = HRT_BM_ETILE + 1u, GS = HRT_TP_BATCH + 1u;         // padded strides of sW and sG
    // U is formed after the gains and read until the batch's MFMA loop ends; the phase factors and the weights live
    // only while the gains are formed: they share one buffer
    constexpr uint32_t UF = HRT_TP_BATCH * BR * 4u, EF = 2u * HRT_BM_ETILE * HRT_TP_BATCH, WF = 2u * BR * WS;
    const hrt_ktgrid &G = P.g;              // the grid, also of csrc/hrt_taps_gemm.inc
    const uint32_t blk = blockIdx.x, link = blockIdx.z;
    const uint32_t rb = blk % G.rblocks, cb = blk / G.rblocks;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t wr = w / WC, wc = w % WC;           // the wave's place in the block
    const uint32_t kq = lane >> 4, col = lane & 15u;   // A / B operand: slot 4 g + kq; row / tap `col` of a tile

    __shared__ __attribute__((aligned(16))) float sMem[umax(UF, EF + WF)];
    __shared__ float2 sG[2][BR][GS];                           // gains: [side][beam slot][slot of the batch]
    __shared__ float sRec[HRT_TP_BATCH][HRT_PS_REC_FLOATS];
    __shared__ sinc_rec sS[HRT_TP_BATCH];
    __shared__ uint32_t sSlot[BR][2];                          // RX, TX beam slot of the block's rows
    __shared__ double sT[BR];                                  // t_m of the block's rows
    float *sU = sMem;                                          // [slot][4 BR]: U of the block's rows g = 4 mm + q
    float2 *sE = reinterpret_cast<float2 *>(sMem);             // [element][slot]: phase factors of one element tile
    float2 *sW = reinterpret_cast<float2 *>(sMem + EF);        // [beam slot][WS]: weights of the touched beams

    // the link's live slots: the header's kept, never more than the list holds (the same for every thread)
    const uint64_t kept = reinterpret_cast<const uint64_t *>(P.paths)[2u * link];
    const uint32_t nlive = kept < P.max_paths ? (uint32_t)kept : P.max_paths;
    if (nlive == 0 && P.accumulate) return;   // nothing to add: out stays as it is

    // the beams of this block's rows row0 .. row1: pairs pf .. pl (the block may begin and end inside a pair).  RX slot
    // s is beam a0 + s; TX slot s is beam s where every TX beam fits the block's capacity (Bt <= BR), else the beam of
    // pair pf + s
    const uint32_t row0 = rb * BR, row1 = min(row0 + BR, G.rows) - 1u;
    const uint32_t pf = row0 / G.T, pl = row1 / G.T;
    const uint32_t a0 = pf / P.bt;
    const bool tx_all = P.bt <= BR;
    const uint32_t na = pl / P.bt - a0 + 1u, nb = tx_all ? P.bt : pl - pf + 1u;

    if (tid < BR) {   // row mm = (pair, time m): pair = a Bt + b
        const uint32_t row = row0 + tid;
        uint32_t sa = 0, sb = 0;
        double t = 0.0;
        if (row <= row1) {
            const uint32_t pair = row / G.T, m = row - pair * G.T;
            const uint32_t a = pair / P.bt, b = pair - a * P.bt;
            sa = a - a0;
            sb = tx_all ? b : pair - pf;
            t = G.t0 + (double)m * G.dt;
        }
        sSlot[tid][0] = sa;
        sSlot[tid][1] = sb;
        sT[tid] = t;
    }

#define HRT_TG_U(j, x) sU[j * (BR * 4u) + x]
#define HRT_TG_PART 1
#include "hrt_taps_gemm.inc"

    const uint8_t *slots = P.paths + 16ull * P.links + (uint64_t)link * P.max_paths * HRT_SP_SLOT_BYTES;
    for (uint32_t s0 = 0; s0 < nlive; s0 += HRT_TP_BATCH) {
        const uint32_t n = min(nlive - s0, HRT_TP_BATCH);
        // No barrier before this write.  sRec is read by the gain stage and by the U stage only, and every wave left
        // the previous batch's U stage through the barrier in front of its MFMA loop; the MFMA loop reads sS and sU
        // and not sRec, so a fast wave may stage this batch while the others are still in the loop of the last one.
        // Rows at or beyond n are not written and keep stale floats: the gain stage, the sinc parameters and U all
        // guard with j < n
        if (tid < n * (HRT_PS_REC_FLOATS / 2u)) {   // slot s0 + j, floats 2 q and 2 q + 1 of its twelve
            const uint32_t j = tid / (HRT_PS_REC_FLOATS / 2u), q = tid % (HRT_PS_REC_FLOATS / 2u);
            const float2 v = *reinterpret_cast<const float2 *>(slots + (uint64_t)(s0 + j) * HRT_SP_SLOT_BYTES +
                                                               HRT_SP_SLOT_FIRST + 8u * q);
            *reinterpret_cast<float2 *>(&sRec[j][2u * q]) = v;
        }
        // The gains of the touched beams at every staged slot.  The stage begins with a barrier (Nr, Nt >= 1: it
        // always runs), and that one carries three things: sRec is whole before the phase factors read it; every
        // wave has left the previous batch's MFMA loop, so sE / sW may overwrite the sU they share LDS with and sS
        // may be rewritten below; on the first batch sSlot and sT are whole.  The stage's writes to sG are behind it
        // too, and sG's last readers (the previous U stage) are behind an earlier barrier still
#define HRT_BG_BATCH HRT_TP_BATCH
#define HRT_BG_THREADS HRT_TP_THREADS
#define HRT_BG_SLOTS SLOTS
#define HRT_BG_E(e, j) sE[e * HRT_TP_BATCH + j]
#define HRT_BG_W(s, e) sW[s * WS + e]
#define HRT_BG_P0 pf
#define HRT_BG_FA_C P.fa_c
#define HRT_BG_PART 1
#include "hrt_beam_gains.inc"
        // the gains are whole, and every read of the last element tile's phase factors and weights is done: U may
        // overwrite them
        __syncthreads();
        if (tid < HRT_TP_BATCH) {   // the slot's sinc parameters (zeros past n).  Written here and not with the staging:
            sinc_rec q = {0, 0.f, 0.f};   // sS is read by the MFMA loop, which the staging may overtake
            if (tid < n) q = sinc_prep(G.fs, sRec[tid][4]);
            sS[tid] = q;
        }
#pragma unroll 1
        for (uint32_t e = tid; e < HRT_TP_BATCH * BR; e += HRT_TP_THREADS) {   // U = a^pol e^{j phase} G
            const uint32_t j = e / BR, mm = e % BR;
            const float *R = sRec[j];
            float u0 = 0.f, u1 = 0.f, u2 = 0.f, u3 = 0.f;
            if (j < n && row0 + mm <= row1) {
                const float2 x = sG[0][sSlot[mm][0]][j], y = sG[1][sSlot[mm][1]][j];
                const float gr = fmaf(x.x, y.x, -(x.y * y.y)), gi = fmaf(x.x, y.y, x.y * y.x);
                float sn, cs;
                sincospif(half_revs((double)R[5] * sT[mm] - G.fc * (double)R[4]), &sn, &cs);
                const float er = cs * gr - sn * gi, ei = cs * gi + sn * gr;
                u0 = R[0] * er - R[1] * ei;
                u1 = R[0] * ei + R[1] * er;
                u2 = R[2] * er - R[3] * ei;
                u3 = R[2] * ei + R[3] * er;
            }
            float *U = &sU[j * (BR * 4u) + 4u * mm];
            U[0] = u0; U[1] = u1; U[2] = u2; U[3] = u3;
        }
        // U and the sinc parameters are whole before the MFMA loop reads them; behind this barrier nothing reads sRec
        // or sG until the next batch's gain stage
        __syncthreads();
#define HRT_TG_PART 2
#include "hrt_taps_gemm.inc"
        // No barrier here: what the next batch writes before its gain stage's first barrier is sRec alone (above)
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

extern "C" int hrt_hip_launch_sparse_beam_taps(const hrt_ksparse_beam_taps *P, void *stream)
{
    const dim3 grid(P->g.rblocks * P->g.cblocks, 1u, P->links);
    if (P->g.rt == 4u)
        hipLaunchKernelGGL((hrt_sparse_beam_taps_kernel<4u, 4u, 4u>), grid, dim3(HRT_TP_THREADS), 0, (hipStream_t)stream,
                           *P);
    else
        hipLaunchKernelGGL((hrt_sparse_beam_taps_kernel<1u, 4u, 1u>), grid, dim3(HRT_TP_THREADS), 0, (hipStream_t)stream,
                           *P);
    return (int)hipGetLastError();
}
