// hrt_beam_gains.inc -- the beam gains the two beam families form the same way: kernel text hrt_beam_partial_kernel and
// hrt_beam_los_kernel (csrc/hrt_beam_channel.hip) share with hrt_beam_taps_partial_kernel and hrt_beam_taps_los_kernel
// (csrc/hrt_beam_taps.hip), pulled in part by part (#define HRT_BG_PART n, then #include) like csrc/hrt_pair_gemm.inc.
// g_rx[a](u) = sum_i conj(W_rx[a, i]) exp(j 2 pi f_a r_i . u / c), g_tx[b](u) = sum_j W_tx[b, j] exp(j 2 pi f_a q_j . u / c)
// (csrc/hrt_beam_channel.h; beam_weight is there).  In scope in both parts: P (nr, nt, bt, rx_el, tx_el, rx_w, tx_w) and
// HRT_BG_FA_C, f_a / c.
//
// Part 1, the gain stage of a partial kernel, inside its batch loop: for the n staged records, the gains of the beams
// the workgroup's pairs touch, into sG.  Element tiles of HRT_BM_ETILE phase factors (FP64 reduction, f32 sincospi) and
// the touched beams' weights in LDS; FP32 within a tile, FP64 across the tiles.  Each kernel keeps its __shared__
// declarations.  Both have 32 records a batch and 32 elements a tile (x & 31, x >> 5: asserted in the two files).  In
// scope: tid, n, sRec[n][HRT_PS_REC_FLOATS] (written before the stage's first barrier), and
//     a0, na               first RX beam of the workgroup's pairs and how many: RX slot s is beam a0 + s
//     nb, tx_all           TX slots: slot s is beam s where every TX beam fits (tx_all), else the beam of pair
//                          HRT_BG_P0 + s
//     HRT_BG_BATCH, HRT_BG_THREADS, HRT_BG_SLOTS   records a batch, threads, (record, beam) gains per thread and side
//     HRT_BG_E(e, j)       float2 phase factor of element e of the tile at record j
//     HRT_BG_W(s, e)       float2 weight of beam slot s at element e of the tile (index macros must not regroup their
//                          sums: csrc/hrt_taps_gemm.inc)
//     HRT_BG_P0            first pair of the workgroup
//     sG[2][slots][>= n]   float2 gains out: [side][beam slot][record], side 0 = RX (u_rx, conj W_rx), 1 = TX
// The caller's barrier after the stage makes sG whole.
//
// Part 2, the body of a LoS kernel, one thread per (link, pair): G = g_rx[a](-u) g_tx[b](u) at the LoS entry's u =
// directions_tx (the coincident convention of los_entry; a blocked entry's gains are not read), FP64 sums, into P.los
// [link][pair].  Kernel text and not a __device__ function: as a function (the whole body, the gains of a (link,
// pair), or one side's sum) the two kernels compiled to other instructions (profiles/HISTORY.md).
#if HRT_BG_PART == 1
#pragma unroll 1
        for (uint32_t side = 0; side < 2u; ++side) {
            const uint32_t N = side ? P.nt : P.nr, ns = side ? nb : na;
            const float *el = side ? P.tx_el : P.rx_el, *wt = side ? P.tx_w : P.rx_w;
            double gre[HRT_BG_SLOTS], gim[HRT_BG_SLOTS];
#pragma unroll
            for (uint32_t s = 0; s < HRT_BG_SLOTS; ++s) gre[s] = gim[s] = 0.0;
#pragma unroll 1
            for (uint32_t e0 = 0; e0 < N; e0 += HRT_BM_ETILE) {
                const uint32_t ne = min(HRT_BM_ETILE, N - e0);
                __syncthreads();   // the records are staged; the readers of the tile (or of what shares its LDS) are done
#pragma unroll 1
                for (uint32_t x = tid; x < ne * HRT_BG_BATCH; x += HRT_BG_THREADS) {   // phase factors
                    const uint32_t j = x & 31u, e = x >> 5;
                    if (j < n) {
                        float sn, cs;
                        sincospif(half_revs(HRT_BG_FA_C * dot3(el + 3u * (e0 + e), sRec[j] + 6u + 3u * side)), &sn, &cs);
                        HRT_BG_E(e, j) = make_float2(cs, sn);
                    }
                }
#pragma unroll 1
                for (uint32_t x = tid; x < ns * HRT_BM_ETILE; x += HRT_BG_THREADS) {   // weights
                    const uint32_t e = x & 31u, s = x >> 5;
                    const uint32_t beam = side == 0u ? a0 + s : (tx_all ? s : (HRT_BG_P0 + s) % P.bt);
                    if (e < ne) HRT_BG_W(s, e) = beam_weight(wt, N, beam, e0 + e, side == 0u);
                }
                __syncthreads();
#pragma unroll
                for (uint32_t s = 0; s < HRT_BG_SLOTS; ++s) {
                    const uint32_t x = tid + s * HRT_BG_THREADS, j = x & 31u, slot = x >> 5;
                    if (j < n && slot < ns) {
                        float re = 0.f, im = 0.f;
                        for (uint32_t e = 0; e < ne; ++e) {
                            const float2 wv = HRT_BG_W(slot, e), ph = HRT_BG_E(e, j);
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
            for (uint32_t s = 0; s < HRT_BG_SLOTS; ++s) {
                const uint32_t x = tid + s * HRT_BG_THREADS, j = x & 31u, slot = x >> 5;
                if (j < n && slot < ns) sG[side][slot][j] = make_float2((float)gre[s], (float)gim[s]);
            }
        }
#elif HRT_BG_PART == 2
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
            sincospif(half_revs(HRT_BG_FA_C * dot3(el + 3u * e, u)), &sn, &cs);
            g[side][0] += (double)wv.x * cs - (double)wv.y * sn;
            g[side][1] += (double)wv.x * sn + (double)wv.y * cs;
        }
    }
    reinterpret_cast<float2 *>(P.los)[gid] = make_float2((float)(g[0][0] * g[1][0] - g[0][1] * g[1][1]),
                                                         (float)(g[0][0] * g[1][1] + g[0][1] * g[1][0]));
#else
#error "HRT_BG_PART: 1 or 2"
#endif
#undef HRT_BG_PART
#undef HRT_BG_BATCH
#undef HRT_BG_THREADS
#undef HRT_BG_SLOTS
#undef HRT_BG_E
#undef HRT_BG_W
#undef HRT_BG_P0
#undef HRT_BG_FA_C
