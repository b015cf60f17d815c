// hrt_beam_taps.hip -- beamformed (codebook) sampled impulse responses from the workspace of a finished hrt_trace,
// for gfx950.  For every link (rx, tx), RX beam a, TX beam b, polarisation, time sample m and tap l_k = l_min + k:
//
//     h[rx, tx, a, b, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)) g_rx[a](u_p^rx) g_tx[b](u_p^tx)
//                                        * sinc(l_k - f_s tau_p)
//     g_rx[a](u) = sum_i conj(W_rx[a, i]) exp(j 2 pi f_a r_i . u / c),  g_tx[b](u) = sum_j W_tx[b, j] exp(j 2 pi f_a q_j . u / c)
//
// over the LoS entry and every unblocked scatter record of the link: hrt_array_taps' h contracted with the combiner
// w^H and the precoder f, without h ever being formed (csrc/hrt_beam_taps.h).  Paths, parts, u_rx and u_tx are those
// of csrc/hrt_array_taps.hip; the workspace view and its readers are csrc/hrt_pathsum.h, the sinc weights
// csrc/hrt_sinc.h.
//   hrt_beam_taps_partial_kernel  one workgroup (4 waves) per (row block x column block, record chunk, link): the real
//                                 GEMM of hrt_array_taps_partial_kernel with (beam pair, time) rows.  Per batch of
//                                 staged records, the gain stage of hrt_beam_partial_kernel for the beams the block's
//                                 rows touch (element phase factors tile by tile in LDS, FP32 within a tile, FP64
//                                 across the tiles), then U = a^pol e^{j phase} G as a complex product; every lane
//                                 forms its own B operand V (one record, one tap) in registers.
//   hrt_beam_taps_los_kernel      per (link, pair): G at the LoS directions (u_tx = HRT_LOS_DIR, u_rx = -u_tx), FP64.
//   hrt_beam_taps_reduce_kernel   per output: the chunks in a fixed order, plus the LoS term, into out.
// No floating-point atomics anywhere: two calls with the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_beam_taps.h"
#include "hrt_pathsum.h"
#include "hrt_sinc.h"

typedef float hrt_f32x4 __attribute__((ext_vector_type(4)));

static_assert(HRT_TP_BATCH == 32u && HRT_BM_ETILE == 32u && HRT_TP_THREADS == 256u, "the index arithmetic of the gain stage");

namespace {

// weight e of beam `beam` of a codebook [beams][n][2]; the combiner (RX side) takes the conjugate
// (csrc/hrt_beam_channel.hip has the same helper)
__device__ __forceinline__ float2 beam_weight(const float *w, uint32_t n, uint32_t beam, uint32_t e, bool conj)
{
    const float *p = w + ((uint64_t)beam * n + e) * 2u;
    return make_float2(p[0], conj ? -p[1] : p[1]);
}

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
    const uint32_t blk = blockIdx.x, c = blockIdx.y, link = blockIdx.z;
    const uint32_t rb = blk % P.rblocks, cb = blk / P.rblocks;
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
    const uint32_t row0 = rb * BR, row1 = min(row0 + BR, P.rows) - 1u;
    const uint32_t pf = row0 / P.T, pl = row1 / P.T;
    const uint32_t a0 = pf / P.bt;
    const bool tx_all = P.bt <= BR;
    const uint32_t na = pl / P.bt - a0 + 1u, nb = tx_all ? P.bt : pl - pf + 1u;

    if (tid < BR) {   // row mm = (pair, time m): pair = a Bt + b
        const uint32_t row = row0 + tid;
        uint32_t sa = 0, sb = 0;
        double t = 0.0;
        if (row <= row1) {
            const uint32_t pair = row / P.T, m = row - pair * P.T;
            const uint32_t a = pair / P.bt, b = pair - a * P.bt;
            sa = a - a0;
            sb = tx_all ? b : pair - pf;
            t = P.t0 + (double)m * P.dt;
        }
        sSlot[tid][0] = sa;
        sSlot[tid][1] = sb;
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
        if (tid < HRT_TP_BATCH) {   // the record's fields, both directions and sinc parameters (zeros past n)
            float *R = sRec[tid];
            sinc_rec q = {0, 0.f, 0.f};
            if (tid < n) {
                stage_record(V, P.sh, sB[tid], rx, tx, sI[tid], R);
                q = sinc_prep(P.fs, R[4]);
            } else {
                for (uint32_t f = 0; f < HRT_PS_REC_FLOATS; ++f) R[f] = 0.f;
            }
            sS[tid] = q;
        }
        // the gains of the touched beams at every staged record, side 0 = RX (u_rx, conj W_rx), 1 = TX
#pragma unroll 1
        for (uint32_t side = 0; side < 2u; ++side) {
            const uint32_t N = side ? P.nt : P.nr, ns = side ? nb : na;
            const float *el = side ? P.tx_el : P.rx_el, *wt = side ? P.tx_w : P.rx_w;
            double gre[SLOTS], gim[SLOTS];
#pragma unroll
            for (uint32_t s = 0; s < SLOTS; ++s) gre[s] = gim[s] = 0.0;
#pragma unroll 1
            for (uint32_t e0 = 0; e0 < N; e0 += HRT_BM_ETILE) {
                const uint32_t ne = min(HRT_BM_ETILE, N - e0);
                __syncthreads();   // the records are staged; the readers of the tile (or of the U) before are done
#pragma unroll 1
                for (uint32_t x = tid; x < ne * HRT_TP_BATCH; x += HRT_TP_THREADS) {   // phase factors
                    const uint32_t j = x & 31u, e = x >> 5;
                    if (j < n) {
                        float sn, cs;
                        sincospif(half_revs(P.fa_c * dot3(el + 3u * (e0 + e), sRec[j] + 6u + 3u * side)), &sn, &cs);
                        sE[e * HRT_TP_BATCH + j] = make_float2(cs, sn);
                    }
                }
#pragma unroll 1
                for (uint32_t x = tid; x < ns * HRT_BM_ETILE; x += HRT_TP_THREADS) {   // weights
                    const uint32_t e = x & 31u, s = x >> 5;
                    const uint32_t beam = side == 0u ? a0 + s : (tx_all ? s : (pf + s) % P.bt);
                    if (e < ne) sW[s * WS + e] = beam_weight(wt, N, beam, e0 + e, side == 0u);
                }
                __syncthreads();
#pragma unroll
                for (uint32_t s = 0; s < SLOTS; ++s) {
                    const uint32_t x = tid + s * HRT_TP_THREADS, j = x & 31u, slot = x >> 5;
                    if (j < n && slot < ns) {
                        float re = 0.f, im = 0.f;
                        for (uint32_t e = 0; e < ne; ++e) {
                            const float2 wv = sW[slot * WS + e], ph = sE[e * HRT_TP_BATCH + j];
                            re = fmaf(wv.x, ph.x, re);
                            re = fmaf(-wv.y, ph.y, re);
                            im = fmaf(wv.x, ph.y, im);
                            im = fmaf(wv.y, ph.x, im);
                        }
                        gre[s] += (double)re;
                        gim[s] += (double)im;
                    }
                }
            }
#pragma unroll
            for (uint32_t s = 0; s < SLOTS; ++s) {
                const uint32_t x = tid + s * HRT_TP_THREADS, j = x & 31u, slot = x >> 5;
                if (j < n && slot < ns) sG[side][slot][j] = make_float2((float)gre[s], (float)gim[s]);
            }
        }
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
                sincospif(half_revs((double)R[5] * sT[mm] - P.fc * (double)R[4]), &sn, &cs);
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
        for (uint32_t g = 0; 4u * g < n; ++g) {
            const uint32_t j = 4u * g + kq;
            const sinc_rec q = sS[j];
            float v[CT];
#pragma unroll
            for (uint32_t t = 0; t < CT; ++t) v[t] = sinc_tap(tap[t], q);
#pragma unroll
            for (uint32_t rt = 0; rt < RT; ++rt) {
                const float a = sU[j * (BR * 4u) + (wr * RT + rt) * 16u + col];
#pragma unroll
                for (uint32_t t = 0; t < CT; ++t)
                    if (live[rt * CT + t])
                        acc[rt * CT + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, v[t], acc[rt * CT + t], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // D: lane = (row group kq, column col), register q: row 4 kq + q of the tile = ((pair, time) row 4 R + kq, part q).
    // A chunk that staged nothing writes its zeros: the scratch is not cleared between calls
    const uint64_t tl = (uint64_t)P.T * P.L;
    float2 *dst = reinterpret_cast<float2 *>(P.partial) + ((uint64_t)link * V.nchunks + c) * 2u * P.npairs * tl;
#pragma unroll
    for (uint32_t t = 0; t < WT; ++t) {
        const uint32_t row = (r0 + t / CT) * 4u + kq, i = (c0 + t % CT) * 16u + col;
        if (live[t] && row < P.rows && i < P.L) {
            const uint32_t pair = row / P.T, m = row - pair * P.T;
            float2 *d = dst + ((uint64_t)pair * 2u * P.T + m) * P.L + i;
            d[0] = make_float2(acc[t][0], acc[t][1]);
            d[tl] = make_float2(acc[t][2], acc[t][3]);
        }
    }
}

// one thread per (link, pair): G = g_rx[a](-u) g_tx[b](u) at the LoS entry's u = directions_tx (the coincident
// convention of los_entry; a blocked entry's gains are not read), as hrt_beam_los_kernel forms it
__global__ void hrt_beam_taps_los_kernel(const hrt_kbeam_taps P)
{
    const hrt_kview &V = P.v;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (uint64_t)P.npairs * V.nrx * V.ntx) return;
    const uint32_t link = (uint32_t)(gid / P.npairs), pair = (uint32_t)(gid - (uint64_t)link * P.npairs);
    const uint32_t a = pair / P.bt, b = pair - a * P.bt;
    hrt_los_entry L;
    (void)los_entry(V, link, L);
    const float u_tx[3] = {L.ux, L.uy, L.uz}, u_rx[3] = {-L.ux, -L.uy, -L.uz};
    double g[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (uint32_t side = 0; side < 2u; ++side) {
        const uint32_t N = side ? P.nt : P.nr, beam = side ? b : a;
        const float *el = side ? P.tx_el : P.rx_el, *wt = side ? P.tx_w : P.rx_w, *u = side ? u_tx : u_rx;
        for (uint32_t e = 0; e < N; ++e) {
            const float2 wv = beam_weight(wt, N, beam, e, side == 0u);
            float sn, cs;
            sincospif(half_revs(P.fa_c * dot3(el + 3u * e, u)), &sn, &cs);
            g[side][0] += (double)wv.x * cs - (double)wv.y * sn;
            g[side][1] += (double)wv.x * sn + (double)wv.y * cs;
        }
    }
    reinterpret_cast<float2 *>(P.los)[gid] = make_float2((float)(g[0][0] * g[1][0] - g[0][1] * g[1][1]),
                                                         (float)(g[0][0] * g[1][1] + g[0][1] * g[1][0]));
}

// one thread per output (link, pair, pol, m, i): the chunks in order, + LoS, -> out
__global__ void hrt_beam_taps_reduce_kernel(const hrt_kbeam_taps P)
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
        const float2 G = reinterpret_cast<const float2 *>(P.los)[(uint64_t)link * P.npairs + pair];
        const uint64_t mi = e % tl;
        const uint32_t m = (uint32_t)(mi / P.L), k = (uint32_t)(mi % P.L);
        const double t = P.t0 + (double)m * P.dt;
        float sn, cs;
        sincospif(half_revs((double)L.nu * t - P.fc * (double)L.tau), &sn, &cs);
        const float v = L.a * sinc_tap(P.l_min + (int32_t)k, sinc_prep(P.fs, L.tau));
        s.x += v * fmaf(cs, G.x, -(sn * G.y));
        s.y += v * fmaf(cs, G.y, sn * G.x);
    }
    store_out(reinterpret_cast<float2 *>(P.out) + gid, s, V.accumulate);
}

extern "C" int hrt_hip_launch_beam_taps(const hrt_kbeam_taps *P, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint32_t links = P->v.nrx * P->v.ntx;
    if (P->v.nchunks) {
        const int e = hrt_hip_launch_segments(&P->v, stream);
        if (e) return e;
        const dim3 grid(P->rblocks * P->cblocks, P->v.nchunks, links);
        if (P->rt == 4u)
            hipLaunchKernelGGL((hrt_beam_taps_partial_kernel<4u, 4u, 4u>), grid, dim3(HRT_TP_THREADS), 0, st, *P);
        else
            hipLaunchKernelGGL((hrt_beam_taps_partial_kernel<1u, 4u, 1u>), grid, dim3(HRT_TP_THREADS), 0, st, *P);
    }
    if (P->v.los) {
        const uint64_t g = (uint64_t)links * P->npairs;
        hipLaunchKernelGGL(hrt_beam_taps_los_kernel, dim3((unsigned)((g + 255u) / 256u)), dim3(256), 0, st, *P);
    }
    const uint64_t n = (uint64_t)links * P->npairs * 2u * P->T * P->L;
    hipLaunchKernelGGL(hrt_beam_taps_reduce_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, st, *P);
    return (int)hipGetLastError();
}
