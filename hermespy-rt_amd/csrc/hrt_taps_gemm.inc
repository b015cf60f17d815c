// hrt_taps_gemm.inc -- the body hrt_taps_partial_kernel (csrc/hrt_taps.hip), hrt_array_taps_partial_kernel
// (csrc/hrt_array_taps.hip) and hrt_beam_taps_partial_kernel (csrc/hrt_beam_taps.hip) share: the real GEMM of
// csrc/hrt_taps.h on v_mfma_f32_16x16x4_f32, (pair, time) rows x taps, with the sinc weights (csrc/hrt_sinc.h) as the B
// operand every lane forms in registers.  Kernel text, pulled in part by part inside the kernel body (#define
// HRT_TG_PART n, then #include) like csrc/hrt_pair_gemm.inc.  Each kernel keeps its __shared__ declarations, its record
// staging and its U stage.
//
// In scope everywhere: P (the kernel's parameters: P.partial), V = P.v, G (the grid: P.g, a hrt_ktgrid; in
// hrt_taps_partial_kernel P itself, csrc/hrt_taps.h), and
//     RT, CT, WR, WC, WT   row and column tiles per wave, waves along the rows and the columns, WT = RT * CT
//     rb, cb, link, c      row block, column block, link and record chunk of the workgroup
//     wr, wc               the wave's place in the block;  kq = lane >> 4, col = lane & 15
//     HRT_TG_U(j, x)       float x of staged record j of U.  The kernel's macro must not regroup the sum of its index
//                          (sU[j * (BR * 4u) + x], not ... + (x)): parenthesised, hrt_beam_taps_partial_kernel got
//                          other registers and another order
// Parts:
//   1  declares r0, c0 (the wave's first row tile and column tile), live, tap and the accumulators acc, zeroed
//   2  the MFMA loop over the n staged records: reads n, sS[n] (sinc_rec) and U
//   3  the D write-back of acc to the partial sums [link][chunk][pair][pol][T][L], rows = (pair, time); needs P.npairs.
//      hrt_taps_partial_kernel has no pairs (its rows are the time samples) and keeps its own write-back
#if HRT_TG_PART == 1
    const uint32_t r0 = (rb * WR + wr) * RT, c0 = (cb * WC + wc) * CT;
    bool live[WT];
    int32_t tap[CT];
#pragma unroll
    for (uint32_t t = 0; t < WT; ++t) live[t] = r0 + t / CT < G.rtiles && c0 + t % CT < G.ctiles;
#pragma unroll
    for (uint32_t t = 0; t < CT; ++t) tap[t] = G.l_min + (int32_t)((c0 + t) * 16u + col);
    typedef float hrt_f32x4 __attribute__((ext_vector_type(4)));
    hrt_f32x4 acc[WT];
#pragma unroll
    for (uint32_t t = 0; t < WT; ++t) acc[t] = hrt_f32x4{0.f, 0.f, 0.f, 0.f};
#elif HRT_TG_PART == 2
        for (uint32_t g = 0; 4u * g < n; ++g) {
            const uint32_t j = 4u * g + kq;
            const sinc_rec q = sS[j];
            float v[CT];
#pragma unroll
            for (uint32_t t = 0; t < CT; ++t) v[t] = sinc_tap(tap[t], q);
#pragma unroll
            for (uint32_t rt = 0; rt < RT; ++rt) {
                const float a = HRT_TG_U(j, (wr * RT + rt) * 16u + col);
#pragma unroll
                for (uint32_t t = 0; t < CT; ++t)
                    if (live[rt * CT + t])
                        acc[rt * CT + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, v[t], acc[rt * CT + t], 0, 0, 0);
            }
        }
#elif HRT_TG_PART == 3
    // D: lane = (row group kq, column col), register q: row 4 kq + q of the tile = ((pair, time) row 4 R + kq, part q).
    // A chunk that staged nothing writes its zeros: the scratch is not cleared between calls
    const uint64_t tl = (uint64_t)G.T * G.L;
    float2 *dst = reinterpret_cast<float2 *>(P.partial) + ((uint64_t)link * V.nchunks + c) * 2u * P.npairs * tl;
#pragma unroll
    for (uint32_t t = 0; t < WT; ++t) {
        const uint32_t row = (r0 + t / CT) * 4u + kq, i = (c0 + t % CT) * 16u + col;
        if (live[t] && row < G.rows && i < G.L) {
            const uint32_t pair = row / G.T, m = row - pair * G.T;
            float2 *d = dst + ((uint64_t)pair * 2u * G.T + m) * G.L + i;
            d[0] = make_float2(acc[t][0], acc[t][1]);
            d[tl] = make_float2(acc[t][2], acc[t][3]);
        }
    }
#else
#error "HRT_TG_PART: 1 .. 3"
#endif
#undef HRT_TG_PART
