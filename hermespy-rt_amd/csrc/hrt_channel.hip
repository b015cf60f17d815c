// hrt_channel.hip -- channel frequency responses from the workspace of a finished hrt_trace, for gfx950.
//
//     H[rx, tx, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p)),  f_k = f0 + k df, t_m = t0 + m dt
//
// over the LoS entry (hrt_channel_reduce_kernel) and every scatter record (hrt_channel_partial_kernel) of
// the link.  Three kernels, all on the caller's stream, no host synchronisation:
//   hrt_channel_segments_kernel  the TX segments of every hit block: records of a block are TX-major (launch 0
//                                numbers lane i as TX i / num_local, compaction is stable, the re-sort key
//                                carries the TX in its top bits), so segment starts are a binary search on
//                                HRT_HIT_RAY;
//   hrt_channel_partial_kernel   one wave per (record chunk, row tile, link): the two-level DFT of
//                                csrc/hrt_channel.h as an FP32 complex GEMM on the VALU (explicit fmaf; the
//                                library builds with -ffp-contract=off), partial sums to the scratch;
//   hrt_channel_reduce_kernel    per output: the chunks in a fixed order, plus the LoS term, into out.
// No floating-point atomics anywhere: two calls with the same inputs give the same bits.  The workspace view and the
// helpers that read it are csrc/hrt_pathsum.h, shared with the array channel and the taps, which reuse the segments
// kernel.
//
// Phases are reduced in FP64 (fract of f * tau in revolutions; f tau reaches 10^4 revolutions at 70 GHz,
// more than an f32 product keeps) and then evaluated with an f32 sincospi.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_channel.h"
#include "hrt_pathsum.h"

// one thread per (bounce, t <= ntx): seg[b][t] = first entry of hit block b whose ray belongs to TX >= t
__global__ void hrt_channel_segments_kernel(const hrt_kview V)
{
    const uint32_t *counts = reinterpret_cast<const uint32_t *>(V.ws + V.off_counts);
    const uint32_t per = V.ntx + 1u;
    for (uint32_t i = threadIdx.x; i < V.nb * per; i += blockDim.x) {
        const uint32_t b = i / per, t = i % per;
        const uint32_t *ray = hit_field(V, b, HRT_HIT_RAY);
        uint32_t lo = 0, hi = counts[b + 1];
        if (hi > V.cap) hi = (uint32_t)V.cap;   // (a corrupt count must not walk out of the block)
        const uint64_t key = (uint64_t)t * V.num_local;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if ((uint64_t)ray[mid] < key) lo = mid + 1u;
            else hi = mid;
        }
        V.seg[i] = lo;
    }
}

__global__ void __launch_bounds__(HRT_CH_THREADS) hrt_channel_partial_kernel(const hrt_kchannel P)
{
    const hrt_kview &V = P.v;
    const uint32_t c = blockIdx.x, tile = blockIdx.y, link = blockIdx.z;
    const uint32_t rx = link / V.ntx, tx = link % V.ntx;
    const uint32_t l = threadIdx.x;
    const uint32_t tc = l & 3u, tr = l >> 2;        // this thread's outputs: rows 4 tr .. +3, cols 4 tc .. +3
    const uint32_t sj = l & (HRT_CH_BATCH - 1u);    // staging: record sj of the batch,
    const uint32_t sq = l / HRT_CH_BATCH;           // rows 16 sq .. +15 and cols 4 sq .. +3 of its U / V

    __shared__ float4 sU[HRT_CH_BATCH][HRT_CH_ROWS];   // a_te U, a_tm U (complex)
    __shared__ float2 sV[HRT_CH_BATCH][HRT_CH_K2];

    float acc[4][4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[i][j][q] = 0.f;

    for (uint32_t b = 0; b < V.nb; ++b) {
        uint32_t start, end;
        chunk_range(V, b, tx, c, start, end);
        if (start >= end) continue;
        const float *are = rec_field(V, b, rx, HRT_REC_A_TE_RE), *aim = rec_field(V, b, rx, HRT_REC_A_TE_IM);
        const float *bre = rec_field(V, b, rx, HRT_REC_A_TM_RE), *bim = rec_field(V, b, rx, HRT_REC_A_TM_IM);
        const float *tau_f = rec_field(V, b, rx, HRT_REC_TAU), *dfs_f = rec_field(V, b, rx, HRT_REC_DFS);
        const float *fs0_f = reinterpret_cast<const float *>(hit_field(V, b, HRT_HIT_FS0));
        const uint64_t *mask = mask_row(V, b, rx);
        for (uint32_t p0 = start; p0 < end; p0 += HRT_CH_BATCH) {
            {   // stage U and V of records p0 .. p0 + 15 (zeros past the chunk and for blocked records: their
                // amplitudes are exact zeros and their Doppler term is not written)
                const uint32_t i = p0 + sj;
                float te_re = 0.f, te_im = 0.f, tm_re = 0.f, tm_im = 0.f, tau = 0.f, nu = 0.f;
                if (i < end && ((mask[i >> 6] >> (i & 63u)) & 1u)) {
                    te_re = are[i]; te_im = aim[i]; tm_re = bre[i]; tm_im = bim[i];
                    tau = tau_f[i];
                    nu = fs0_f[i] - dfs_f[i];   // the path list's freq_shift
                }
                const bool live = te_re != 0.f || te_im != 0.f || tm_re != 0.f || tm_im != 0.f;
#pragma unroll 4
                for (uint32_t r = sq * 16u; r < sq * 16u + 16u; ++r) {
                    const uint32_t g = tile * HRT_CH_ROWS + r;
                    float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (live && g < P.rows) {
                        const uint32_t m = g / P.K1, k1 = g - m * P.K1;
                        const double t = P.t0 + (double)m * P.dt;
                        const double f = P.f0 + (double)(k1 * HRT_CH_K2) * P.df;
                        float sn, cs;
                        sincospif(half_revs((double)nu * t - f * (double)tau), &sn, &cs);
                        u = make_float4(te_re * cs - te_im * sn, te_re * sn + te_im * cs,
                                        tm_re * cs - tm_im * sn, tm_re * sn + tm_im * cs);
                    }
                    sU[sj][r] = u;
                }
#pragma unroll
                for (uint32_t k2 = sq * 4u; k2 < sq * 4u + 4u; ++k2) {
                    float sn = 0.f, cs = 1.f;
                    if (live) sincospif(half_revs(-(double)k2 * P.df * (double)tau), &sn, &cs);
                    sV[sj][k2] = make_float2(cs, sn);
                }
            }
            __syncthreads();
#pragma unroll 2
            for (uint32_t j = 0; j < HRT_CH_BATCH; ++j) {
                float4 u[4];
                float2 v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    u[q] = sU[j][tr * 4u + q];
                    v[q] = sV[j][tc * 4u + q];
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float *A = acc[a][e];
                        A[0] = fmaf(u[a].x, v[e].x, A[0]); A[0] = fmaf(-u[a].y, v[e].y, A[0]);
                        A[1] = fmaf(u[a].x, v[e].y, A[1]); A[1] = fmaf(u[a].y, v[e].x, A[1]);
                        A[2] = fmaf(u[a].z, v[e].x, A[2]); A[2] = fmaf(-u[a].w, v[e].y, A[2]);
                        A[3] = fmaf(u[a].z, v[e].y, A[3]); A[3] = fmaf(u[a].w, v[e].x, A[3]);
                    }
            }
            __syncthreads();
        }
    }
    float4 *dst = reinterpret_cast<float4 *>(P.partial) +
                  (((uint64_t)link * V.nchunks + c) * P.tiles + tile) * (HRT_CH_ROWS * HRT_CH_K2);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            dst[(tr * 4u + a) * HRT_CH_K2 + tc * 4u + e] = make_float4(acc[a][e][0], acc[a][e][1], acc[a][e][2], acc[a][e][3]);
}

// one thread per (link, row, column) of the padded grid: sum of the chunks in order, + LoS, -> out
__global__ void hrt_channel_reduce_kernel(const hrt_kchannel P)
{
    const hrt_kview &V = P.v;
    const uint64_t per_link = (uint64_t)P.tiles * HRT_CH_ROWS * HRT_CH_K2;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= per_link * V.nrx * V.ntx) return;
    const uint32_t link = (uint32_t)(gid / per_link);
    const uint64_t e = gid - (uint64_t)link * per_link;   // = tile * ROWS * K2 + row_in_tile * K2 + col
    const uint32_t g = (uint32_t)(e / HRT_CH_K2), k2 = (uint32_t)(e % HRT_CH_K2);
    if (g >= P.rows) return;
    const uint32_t m = g / P.K1, k1 = g - m * P.K1, k = k1 * HRT_CH_K2 + k2;
    if (k >= P.K) return;

    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 *src = reinterpret_cast<const float4 *>(P.partial) + (uint64_t)link * V.nchunks * per_link + e;
    for (uint32_t c = 0; c < V.nchunks; ++c) {
        const float4 v = src[(uint64_t)c * per_link];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    hrt_los_entry L;
    if (V.los && los_entry(V, link, L)) {   // a real: TE = TM
        const double t = P.t0 + (double)m * P.dt, f = P.f0 + (double)k * P.df;
        float sn, cs;
        sincospif(half_revs((double)L.nu * t - f * (double)L.tau), &sn, &cs);
        const float re = L.a * cs, im = L.a * sn;
        s.x += re; s.y += im; s.z += re; s.w += im;
    }
    const uint32_t rx = link / V.ntx, tx = link % V.ntx;
    const uint64_t tk = (uint64_t)P.T * P.K;
    float2 *o = reinterpret_cast<float2 *>(P.out) + ((uint64_t)rx * V.ntx + tx) * 2u * tk + (uint64_t)m * P.K + k;
    float2 te = make_float2(s.x, s.y), tm = make_float2(s.z, s.w);
    if (V.accumulate) {
        const float2 a = o[0], bb = o[tk];
        te.x += a.x; te.y += a.y; tm.x += bb.x; tm.y += bb.y;
    }
    o[0] = te;
    o[tk] = tm;
}

extern "C" int hrt_hip_launch_channel(const hrt_kchannel *P, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint32_t links = P->v.nrx * P->v.ntx;
    if (P->v.nchunks) {
        const int e = hrt_hip_launch_segments(&P->v, stream);
        if (e) return e;
        hipLaunchKernelGGL(hrt_channel_partial_kernel, dim3(P->v.nchunks, P->tiles, links), dim3(HRT_CH_THREADS), 0,
                           st, *P);
    }
    const uint64_t n = (uint64_t)links * P->tiles * HRT_CH_ROWS * HRT_CH_K2;
    hipLaunchKernelGGL(hrt_channel_reduce_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, st, *P);
    return (int)hipGetLastError();
}

extern "C" int hrt_hip_launch_segments(const hrt_kview *V, void *stream)
{
    hipLaunchKernelGGL(hrt_channel_segments_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *V);
    return (int)hipGetLastError();
}
