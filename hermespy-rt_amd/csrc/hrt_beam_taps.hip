// hrt_beam_taps.hip -- beamformed (codebook) sampled impulse responses from the workspace of a finished hrt_trace,
// for gfx950.  For every link (rx, tx), RX beam a, TX beam b, polarisation, time sample m and tap l_k = l_min + k:
//
//     h[rx, tx, a, b, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)) g_rx[a](u_p^rx) g_tx[b](u_p^tx)
//                                        * sinc(l_k - f_s tau_p)
//     g_rx[a](u) = sum_i conj(W_rx[a, i]) exp(j 2 pi f_a r_i . u / c),  g_tx[b](u) = sum_j W_tx[b, j] exp(j 2 pi f_a q_j . u / c)
//
// over the LoS entry and every unblocked scatter record of the link: hrt_array_taps' h contracted with the combiner
// w^H and the precoder f, without h ever being formed (csrc/hrt_beam_taps.h).  Paths, parts, u_rx and u_tx are those
// of csrc/hrt_array_taps.hip; the workspace view, its readers, the reduce walk and the launch are csrc/hrt_pathsum.h,
// the sinc weights csrc/hrt_sinc.h.
//   hrt_beam_taps_partial_kernel  one workgroup (4 waves) per (row block x column block, record chunk, link): the real
//                                 GEMM of csrc/hrt_taps_gemm.inc with (beam pair, time) rows.  Per batch of staged
//                                 records, the gain stage of csrc/hrt_beam_gains.inc for the beams the block's rows
//                                 touch (element phase factors tile by tile in LDS, FP32 within a tile, FP64 across
//                                 the tiles), then U = a^pol e^{j phase} G as a complex product; every lane forms
//                                 its own B operand V (one record, one tap) in registers.
//   hrt_beam_taps_los_kernel      per (link, pair): G at the LoS directions (u_tx = HRT_LOS_DIR, u_rx = -u_tx), FP64
//                                 (part 2 of csrc/hrt_beam_gains.inc).
//   hrt_beam_taps_reduce_kernel   per output: the chunks in a fixed order, plus the LoS term, into out.
// No floating-point atomics anywhere: two calls with the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_beam_taps.h"
#include "hrt_pathsum.h"

static_assert(HRT_TP_BATCH == 32u && HRT_BM_ETILE == 32u && HRT_TP_THREADS == 256u, "the index arithmetic of the gain stage");

namespace {

constexpr uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

}  // namespace

// RT row tiles x CT column tiles per wave; the 4 waves of the block stand WR along the rows and 4 / WR along the
// columns (the two forms of csrc/hrt_array_taps.h: <4, 4, 4> and <1, 4, 1>)
template <uint32_t RT, uint32_t CT, uint32_t WR>
__global__ void __launch_bounds__(HRT_TP_THREADS, 2) hrt_beam_taps_partial_kernel(const hrt_kbeam_taps P)
{
    constexpr uint32_t WC = 4u / WR, WT = RT * CT;
    constexpr uint32_t BR = WR * RT * 4u;   // (pair, time) rows of the block = its capacity in pairs and beam slots
    constexpr uint32_t SLOTS = umax(1u, HRT_TP_BATCH * BR / HRT_TP_THREADS);   // (record, beam) gains per thread and side
    constexpr uint32_t WS = HRT_BM_ETILE + 1u, GS = HRT_TP_BATCH + 1u;         // padded strides of sW and sG
    // U is formed after the gains and read until the batch ends; the phase factors and the weights live only while
    // the gains are formed: they share one buffer
    constexpr uint32_t UF = HRT_TP_BATCH * BR * 4u, EF = 2u * HRT_BM_ETILE * HRT_TP_BATCH, WF = 2u * BR * WS;
    const hrt_kview &V = P.v;
    const hrt_ktgrid &G = P.g;   // the grid, also of csrc/hrt_taps_gemm.inc
    const uint32_t blk = blockIdx.x, c = blockIdx.y, link = blockIdx.z;
    const uint32_t rb = blk % G.rblocks, cb = blk / G.rblocks;
    const uint32_t rx = link / V.ntx, tx = link % V.ntx;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t wr = w / WC, wc = w % WC;           // the wave's place in the block
    const uint32_t kq = lane >> 4, col = lane & 15u;   // A / B operand: record 4 g + kq; row / tap `col` of a tile

    __shared__ __attribute__((aligned(16))) float sMem[umax(UF, EF + WF)];
    __shared__ float2 sG[2][BR][GS];                           // gains: [side][beam slot][record]
    __shared__ float sRec[HRT_TP_BATCH][HRT_PS_REC_FLOATS];
    __shared__ sinc_rec sS[HRT_TP_BATCH];
    __shared__ uint32_t sB[HRT_TP_BATCH], sI[HRT_TP_BATCH];   // (bounce, hit) of the staged records
    __shared__ uint32_t sSlot[BR][2];                          // RX, TX beam slot of the block's rows
    __shared__ double sT[BR];                                  // t_m of the block's rows
    float *sU = sMem;                                          // [record][4 BR]: U of the block's rows g = 4 mm + q
    float2 *sE = reinterpret_cast<float2 *>(sMem);             // [element][record]: phase factors of one element tile
    float2 *sW = reinterpret_cast<float2 *>(sMem + EF);        // [beam slot][WS]: weights of the touched beams

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

    uint32_t b = 0, cur = 0, end = 0;
    chunk_range(V, 0, tx, c, cur, end);
    for (;;) {
        const uint32_t n = fill_batch<HRT_TP_BATCH>(V, rx, tx, c, lane, w, b, cur, end, sB, sI);
        if (n == 0) break;
        __syncthreads();
        if (tid < HRT_TP_BATCH) {   // the record's fields, both directions and sinc parameters (zeros past n)
            float *R = sRec[tid];
            sinc_rec q = {0, 0.f, 0.f};
            if (tid < n) {
                stage_record(V, P.sh, sB[tid], rx, tx, sI[tid], R);
                q = sinc_prep(G.fs, R[4]);
            } else {
                for (uint32_t f = 0; f < HRT_PS_REC_FLOATS; ++f) R[f] = 0.f;
            }
            sS[tid] = q;
        }
        // the gains of the touched beams at every staged record
#define HRT_BG_BATCH HRT_TP_BATCH
#define HRT_BG_THREADS HRT_TP_THREADS
#define HRT_BG_SLOTS SLOTS
#define HRT_BG_E(e, j) sE[e * HRT_TP_BATCH + j]
#define HRT_BG_W(s, e) sW[s * WS + e]
#define HRT_BG_P0 pf
#define HRT_BG_FA_C P.fa_c
#define HRT_BG_PART 1
#include "hrt_beam_gains.inc"
        __syncthreads();   // the gains are whole; the phase factors and the weights are read: U may overwrite them
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
        __syncthreads();
#define HRT_TG_PART 2
#include "hrt_taps_gemm.inc"
        __syncthreads();
    }

#undef HRT_TG_U
#define HRT_TG_PART 3
#include "hrt_taps_gemm.inc"
}

// one thread per (link, pair): G at the LoS directions (part 2 of csrc/hrt_beam_gains.inc)
__global__ void hrt_beam_taps_los_kernel(const hrt_kbeam_taps P)
{
#define HRT_BG_FA_C P.fa_c
#define HRT_BG_PART 2
#include "hrt_beam_gains.inc"
}

// one thread per output (link, pair, pol, m, i): the chunks in order, + LoS, -> out
__global__ void hrt_beam_taps_reduce_kernel(const hrt_kbeam_taps P)
{
    const hrt_kview &V = P.v;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    hrt_taps_output o;
    if (!taps_output(V, P.g, P.npairs, P.partial, gid, o)) return;
    float2 s = o.s;
    hrt_los_entry L;
    if (V.los && los_entry(V, o.link, L)) {   // a real: TE = TM
        const float2 G = reinterpret_cast<const float2 *>(P.los)[(uint64_t)o.link * P.npairs + o.pair];
        float sn, cs;
        sincospif(half_revs(taps_los_phase(P.g, o.m, L)), &sn, &cs);
        const float v = taps_los_weight(P.g, o.tap, L);
        s.x += v * fmaf(cs, G.x, -(sn * G.y));
        s.y += v * fmaf(cs, G.y, sn * G.x);
    }
    store_out(reinterpret_cast<float2 *>(P.out) + gid, s, V.accumulate);
}

extern "C" int hrt_hip_launch_beam_taps(const hrt_kbeam_taps *P, void *stream)
{
    return launch_taps_family<hrt_kbeam_taps>(P, P->g, P->npairs, HRT_TP_THREADS,
                                              hrt_beam_taps_partial_kernel<4u, 4u, 4u>,
                                              hrt_beam_taps_partial_kernel<1u, 4u, 1u>, hrt_beam_taps_los_kernel,
                                              hrt_beam_taps_reduce_kernel, stream);
}
