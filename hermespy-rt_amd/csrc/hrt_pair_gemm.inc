// hrt_pair_gemm.inc -- the body hrt_array_partial_kernel (csrc/hrt_array_channel.hip) and hrt_beam_partial_kernel
// (csrc/hrt_beam_channel.hip) share: the complex GEMM of csrc/hrt_array_channel.h over HRT_AC_PAIRS rows (element or
// beam pairs) x HRT_AC_GROWS * 16 padded columns.  Kernel text, pulled in part by part inside the kernel body
// (#define HRT_PG_PART n, then #include) like csrc/hrt_fused_body.inc: as helper functions the same lines cost
// hrt_array_partial_kernel 16 AGPRs or another schedule (profiles/HISTORY.md).  Each kernel keeps its __shared__
// declarations, its batch fill and its S stage (the A operand of each lane, in sA).  hrt_sparse_channel_kernel
// (csrc/hrt_sparse_channel.hip) pulls in parts 1 .. 3 over the slots of a path list and writes acc out itself.
//
// In scope everywhere: P (the kernel's parameters: P.g the hrt_kgrid, P.npairs, P.partial), V = P.v, and
//     cb, link, c          column block, link and record chunk of the workgroup
//     p0                   first pair of the workgroup's pair block
//     tid, lane, w         thread, lane and wave;  h = lane >> 5, k2 = lane & 15, rsub = (lane >> 4) & 1
// Parts:
//   1  declares live_p1, live_c0, live_c1 and the accumulators acc, zeroed
//   2  the U and V stages of a batch: reads n, sRec[n][HRT_PS_REC_FLOATS]; writes sU[n][HRT_AC_GROWS], sV[n][HRT_CH_K2]
//   3  the MFMA loop over the n staged records: reads sU, sV, sA[n][2][64]
//   4  the D write-back of acc to the partial sums [link][chunk][pol][pair][T * K]
#if HRT_PG_PART == 1
    // the MFMA tiles of this wave: pair tiles 0, 1 of the block; column tiles 2w, 2w + 1 (rows g 4w .. 4w + 3)
    const bool live_p1 = p0 + 16u < P.npairs;
    const bool live_c0 = cb * HRT_AC_GROWS + 4u * w < P.g.rows;
    const bool live_c1 = cb * HRT_AC_GROWS + 4u * w + 2u < P.g.rows;
    typedef float hrt_f32x16 __attribute__((ext_vector_type(16)));
    hrt_f32x16 acc[2][2][2];   // [pair tile][column tile][pol]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][t][q][r] = 0.f;
#elif HRT_PG_PART == 2
#pragma unroll 1
        for (uint32_t e = tid; e < n * HRT_AC_GROWS; e += HRT_AC_THREADS) {   // U
            const uint32_t j = e / HRT_AC_GROWS, r = e % HRT_AC_GROWS, g = cb * HRT_AC_GROWS + r;
            const float *R = sRec[j];
            float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
            if (g < P.g.rows) {
                const uint32_t m = g / P.g.K1, k1 = g - m * P.g.K1;
                const double t = P.g.t0 + (double)m * P.g.dt;
                const double f = P.g.f0 + (double)(k1 * HRT_CH_K2) * P.g.df;
                float sn, cs;
                sincospif(half_revs((double)R[5] * t - f * (double)R[4]), &sn, &cs);
                u = make_float4(R[0] * cs - R[1] * sn, R[0] * sn + R[1] * cs, R[2] * cs - R[3] * sn, R[2] * sn + R[3] * cs);
            }
            sU[j][r] = u;
        }
#pragma unroll 1
        for (uint32_t e = tid; e < n * HRT_CH_K2; e += HRT_AC_THREADS) {   // V
            const uint32_t j = e / HRT_CH_K2, q = e % HRT_CH_K2;
            float sn, cs;
            sincospif(half_revs(-(double)q * P.g.df * (double)sRec[j][4]), &sn, &cs);
            sV[j][q] = make_float4(cs, -sn, sn, cs);
        }
#elif HRT_PG_PART == 3
        const float2 *sV2 = reinterpret_cast<const float2 *>(&sV[0][0]);
        for (uint32_t j = 0; j < n; ++j) {
            const float2 v = sV2[(j * HRT_CH_K2 + k2) * 2u + h];
            const float4 u0 = sU[j][4u * w + rsub], u1 = sU[j][4u * w + 2u + rsub];
            // lane (k = h, column): h = 0 Re(U V), h = 1 Im(U V)
            const float b00 = fmaf(u0.x, v.x, u0.y * v.y), b01 = fmaf(u0.z, v.x, u0.w * v.y);
            const float b10 = fmaf(u1.x, v.x, u1.y * v.y), b11 = fmaf(u1.z, v.x, u1.w * v.y);
            const float a0v = sA[j][0][lane], a1v = sA[j][1][lane];
            if (live_c0) {
                acc[0][0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0v, b00, acc[0][0][0], 0, 0, 0);
                acc[0][0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0v, b01, acc[0][0][1], 0, 0, 0);
                if (live_p1) {
                    acc[1][0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1v, b00, acc[1][0][0], 0, 0, 0);
                    acc[1][0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1v, b01, acc[1][0][1], 0, 0, 0);
                }
            }
            if (live_c1) {
                acc[0][1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0v, b10, acc[0][1][0], 0, 0, 0);
                acc[0][1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0v, b11, acc[0][1][1], 0, 0, 0);
                if (live_p1) {
                    acc[1][1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1v, b10, acc[1][1][0], 0, 0, 0);
                    acc[1][1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1v, b11, acc[1][1][1], 0, 0, 0);
                }
            }
        }
#elif HRT_PG_PART == 4
    // D: lane = column, register r = row (r & 3) + 8 (r >> 2) + 4 h; rows 0..15 Re, 16..31 Im of 16 pairs
    const uint64_t tk = (uint64_t)P.g.T * P.g.K;
    float2 *dst = reinterpret_cast<float2 *>(P.partial) + ((uint64_t)link * V.nchunks + c) * 2u * P.npairs * tk;
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
                        d[((uint64_t)q * P.npairs + pair) * tk] = make_float2(acc[a][t][q][r], acc[a][t][q][r + 8]);
                }
    }
#else
#error "HRT_PG_PART: 1 .. 4"
#endif
#undef HRT_PG_PART
