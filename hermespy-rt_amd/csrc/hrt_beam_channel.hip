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
//                            hrt_array_partial_kernel with beam pairs for rows.  Only the S stage differs: per batch
//                            of staged records, the element phase factors (FP64 reduction, f32 sincospi) tile by tile
//                            in LDS, the gains of the beams the block's pairs touch (FP32 within a tile, FP64 across
//                            the tiles), and G = g_rx g_tx as the A operand of each lane.
//   hrt_beam_los_kernel      per (link, pair): G at the LoS directions (u_tx = HRT_LOS_DIR, u_rx = -u_tx), FP64 sums.
//   hrt_beam_reduce_kernel   per output: the chunks in a fixed order, plus the LoS term, into out.
// No floating-point atomics anywhere: two calls with the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_beam_channel.h"
#include "hrt_channel.h"
#include "hrt_pathsum.h"

#define HRT_BM_SLOTS (HRT_AC_BATCH * HRT_AC_PAIRS / HRT_AC_THREADS)   // (record, beam) gains per thread and side

static_assert(HRT_AC_BATCH == 32u && HRT_AC_PAIRS == 32u && HRT_BM_ETILE == 32u, "the index arithmetic of the S stage");

namespace {

// weight e of beam `beam` of a codebook [beams][n][2]; the combiner (RX side) takes the conjugate
__device__ __forceinline__ float2 beam_weight(const float *w, uint32_t n, uint32_t beam, uint32_t e, bool conj)
{
    const float *p = w + ((uint64_t)beam * n + e) * 2u;
    return make_float2(p[0], conj ? -p[1] : p[1]);
}

}  // namespace

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
        // S: the gains of the touched beams at every staged record, side 0 = RX (u_rx, conj W_rx), 1 = TX
#pragma unroll 1
        for (uint32_t side = 0; side < 2u; ++side) {
            const uint32_t N = side ? P.nt : P.nr, ns = side ? nb : na;
            const float *el = side ? P.tx_el : P.rx_el, *wt = side ? P.tx_w : P.rx_w;
            double gre[HRT_BM_SLOTS], gim[HRT_BM_SLOTS];
#pragma unroll
            for (uint32_t s = 0; s < HRT_BM_SLOTS; ++s) gre[s] = gim[s] = 0.0;
#pragma unroll 1
            for (uint32_t e0 = 0; e0 < N; e0 += HRT_BM_ETILE) {
                const uint32_t ne = min(HRT_BM_ETILE, N - e0);
                __syncthreads();   // the readers of the tile before are done
#pragma unroll 1
                for (uint32_t x = tid; x < ne * HRT_AC_BATCH; x += HRT_AC_THREADS) {   // phase factors
                    const uint32_t j = x & 31u, e = x >> 5;
                    if (j < n) {
                        float sn, cs;
                        sincospif(half_revs(P.g.fa_c * dot3(el + 3u * (e0 + e), sRec[j] + 6u + 3u * side)), &sn, &cs);
                        sE[e][j] = make_float2(cs, sn);
                    }
                }
#pragma unroll 1
                for (uint32_t x = tid; x < ns * HRT_BM_ETILE; x += HRT_AC_THREADS) {   // weights
                    const uint32_t e = x & 31u, s = x >> 5;
                    const uint32_t beam = side == 0u ? a0 + s : (tx_all ? s : (p0 + s) % P.bt);
                    if (e < ne) sW[s][e] = beam_weight(wt, N, beam, e0 + e, side == 0u);
                }
                __syncthreads();
#pragma unroll
                for (uint32_t s = 0; s < HRT_BM_SLOTS; ++s) {
                    const uint32_t x = tid + s * HRT_AC_THREADS, j = x & 31u, slot = x >> 5;
                    if (j < n && slot < ns) {
                        float re = 0.f, im = 0.f;
                        for (uint32_t e = 0; e < ne; ++e) {
                            const float2 wv = sW[slot][e], ph = sE[e][j];
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
            for (uint32_t s = 0; s < HRT_BM_SLOTS; ++s) {
                const uint32_t x = tid + s * HRT_AC_THREADS, j = x & 31u, slot = x >> 5;
                if (j < n && slot < ns) sG[side][slot][j] = make_float2((float)gre[s], (float)gim[s]);
            }
        }
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

// one thread per (link, pair): G = g_rx[a](-u) g_tx[b](u) at the LoS entry's u = directions_tx (the coincident
// convention of los_entry; a blocked entry's gains are not read)
__global__ void hrt_beam_los_kernel(const hrt_kbeam P)
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
            sincospif(half_revs(P.g.fa_c * dot3(el + 3u * e, u)), &sn, &cs);
            g[side][0] += (double)wv.x * cs - (double)wv.y * sn;
            g[side][1] += (double)wv.x * sn + (double)wv.y * cs;
        }
    }
    reinterpret_cast<float2 *>(P.los)[gid] = make_float2((float)(g[0][0] * g[1][0] - g[0][1] * g[1][1]),
                                                         (float)(g[0][0] * g[1][1] + g[0][1] * g[1][0]));
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
