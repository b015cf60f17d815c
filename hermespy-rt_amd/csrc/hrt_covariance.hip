// hrt_covariance.hip -- per-link spatial covariance matrices of an antenna array from the workspace of a finished
// hrt_trace, for gfx950.  For every link (rx, tx), polarisation and side:
//
//     R_rx[rx, tx, pol, i, i'] = sum_p |a_p^pol|^2 s_i(u_p^rx) conj(s_i'(u_p^rx)),   s_i(u) = exp(j 2 pi f_a r_i . u / c)
//     R_tx[rx, tx, pol, j, j'] = sum_p |a_p^pol|^2 t_j(u_p^tx) conj(t_j'(u_p^tx)),   t_j(u) = exp(j 2 pi f_a q_j . u / c)
//
// over the LoS entry (shard rank 0, hrt_cov_reduce_kernel) and every unblocked scatter record: the terms of
// hrt_power_profiles with the steering of hrt_array_channel (csrc/hrt_covariance.h).  u_rx is the record's
// HRT_REC_DIR, u_tx the launch direction of the record's global path; the workspace view and its readers are
// csrc/hrt_pathsum.h.
//   hrt_cov_partial_kernel  one workgroup (4 waves) per (block of the upper triangle and side, record chunk, link):
//                           per batch of staged records, the steering factors of the block's row and column
//                           elements (FP64 reduction, f32 sincospi, once per (record, element)) in LDS, then one
//                           f32 MFMA per (record, 16 x 32 tile, polarisation); the chunk's block to the scratch.
//   hrt_cov_reduce_kernel   one thread per output of the upper triangle (the threads below it leave at once): the
//                           chunks in index order, plus the LoS term, into out, with the mirror element
//                           R[i', i] = conj(R[i, i']) and the diagonal's imaginary part exactly 0.
// No floating-point atomics anywhere: two calls with the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_covariance.h"
#include "hrt_pathsum.h"

static_assert(HRT_CV_THREADS == 256u && HRT_CV_BLOCK == 64u && HRT_CV_BATCH <= 64u, "the index arithmetic of the stages");

namespace {

constexpr uint32_t BLOCK2 = HRT_CV_BLOCK * HRT_CV_BLOCK;   // complex values of a block in the scratch

typedef float cv_f32x16 __attribute__((ext_vector_type(16)));

// what a side of a call is: its elements, its blocks and where its partial sums start within a link's
struct cv_side {
    uint32_t n, nb, nblk;           // elements, block rows, blocks of the upper triangle
    const float *el;
    uint64_t off, per_link, stride; // float2: the side within a link, a link, a chunk of the side
};

__device__ __forceinline__ cv_side side_of(const hrt_kcov &P, uint32_t side)
{
    cv_side s;
    s.n = side ? P.n[1] : P.n[0];
    s.nb = (s.n + HRT_CV_BLOCK - 1u) / HRT_CV_BLOCK;
    s.nblk = side ? P.nblk[1] : P.nblk[0];
    s.el = side ? P.el[1] : P.el[0];
    s.per_link = (uint64_t)P.v.nchunks * 2u * (P.nblk[0] + P.nblk[1]) * BLOCK2;
    s.off = side ? (uint64_t)P.v.nchunks * 2u * P.nblk[0] * BLOCK2 : 0u;
    s.stride = 2ull * s.nblk * BLOCK2;
    return s;
}

// block b of the upper triangle of nb block rows, row by row: (rb, cb), cb >= rb
__device__ __forceinline__ void block_of(uint32_t nb, uint32_t b, uint32_t &rb, uint32_t &cb)
{
    rb = 0;
    while (rb + 1u < nb && b >= nb - rb) {
        b -= nb - rb;
        ++rb;
    }
    cb = rb + b;
}

__device__ __forceinline__ uint32_t block_index(uint32_t nb, uint32_t rb, uint32_t cb)
{
    return rb * nb - rb * (rb - 1u) / 2u + cb - rb;
}

// (cos, sin) of the steering phase of the element at r for direction u: the array families' rule
__device__ __forceinline__ float2 steer(double fa_c, const float *r, const float *u)
{
    float sn, cs;
    sincospif(half_revs(fa_c * dot3(r, u)), &sn, &cs);
    return make_float2(cs, sn);
}

}  // namespace

__global__ void __launch_bounds__(HRT_CV_THREADS) hrt_cov_partial_kernel(const hrt_kcov P)
{
    const hrt_kview &V = P.v;
    const uint32_t c = blockIdx.y, link = blockIdx.z;
    const uint32_t side = blockIdx.x >= P.nblk[0] ? 1u : 0u;
    const uint32_t blk = blockIdx.x - (side ? P.nblk[0] : 0u);
    const cv_side S = side_of(P, side);
    uint32_t rb, cb;
    block_of(S.nb, blk, rb, cb);
    const uint32_t rx = link / V.ntx, tx = link % V.ntx;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t h = lane >> 5, hi = (lane >> 4) & 1u;

    __shared__ float2 sS[2][HRT_CV_BATCH][HRT_CV_BLOCK];   // (cos, sin): [0] the row block's elements, [1] the column block's
    __shared__ float sEl[2][HRT_CV_BLOCK][3];              // their offsets (0 past the last element)
    __shared__ float sP[HRT_CV_BATCH][2];                  // p per polarisation
    __shared__ float sU[HRT_CV_BATCH][3];                  // the side's direction
    __shared__ uint32_t sB[HRT_CV_BATCH], sI[HRT_CV_BATCH];   // (bounce, hit) of the staged records

    const uint32_t nwhich = rb == cb ? 1u : 2u;   // a diagonal block's columns are its rows
    if (tid < 2u * HRT_CV_BLOCK) {
        const uint32_t which = tid >> 6, e = (which ? cb : rb) * HRT_CV_BLOCK + (tid & 63u);
#pragma unroll
        for (int q = 0; q < 3; ++q) sEl[which][tid & 63u][q] = e < S.n ? S.el[3u * e + q] : 0.f;
    }
    const float2(*sCol)[HRT_CV_BLOCK] = rb == cb ? sS[0] : sS[1];

    // the MFMA tiles of this wave: row tile w of the block, column tiles 0 and 1, both polarisations
    const bool live_r = rb * HRT_CV_BLOCK + 16u * w < S.n;
    const bool live_c0 = live_r, live_c1 = live_r && cb * HRT_CV_BLOCK + 32u < S.n;
    cv_f32x16 acc[2][2];   // [column tile][pol]
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][q][r] = 0.f;

    uint32_t b = 0, cur = 0, end = 0;
    chunk_range(V, 0, tx, c, cur, end);
    for (;;) {
        const uint32_t n = fill_batch<HRT_CV_BATCH>(V, rx, tx, c, lane, w, b, cur, end, sB, sI);
        if (n == 0) break;
        __syncthreads();
        if (tid < n) {
            const uint32_t rb_ = sB[tid], ri = sI[tid];
            const double ter = rec_field(V, rb_, rx, HRT_REC_A_TE_RE)[ri], tei = rec_field(V, rb_, rx, HRT_REC_A_TE_IM)[ri];
            const double tmr = rec_field(V, rb_, rx, HRT_REC_A_TM_RE)[ri], tmi = rec_field(V, rb_, rx, HRT_REC_A_TM_IM)[ri];
            sP[tid][0] = (float)(ter * ter + tei * tei);
            sP[tid][1] = (float)(tmr * tmr + tmi * tmi);
            if (side) {
                const hrt_launch_dir_t d = hit_launch_dir(V, P.sh, rb_, tx, ri);
                sU[tid][0] = d.fx; sU[tid][1] = d.fy; sU[tid][2] = d.fz;
            } else {
                sU[tid][0] = rec_field(V, rb_, rx, HRT_REC_DIRX)[ri];
                sU[tid][1] = rec_field(V, rb_, rx, HRT_REC_DIRY)[ri];
                sU[tid][2] = rec_field(V, rb_, rx, HRT_REC_DIRZ)[ri];
            }
        }
        __syncthreads();
        // the steering factors, once per (record, element)
#pragma unroll 1
        for (uint32_t x = tid; x < nwhich * HRT_CV_BATCH * HRT_CV_BLOCK; x += HRT_CV_THREADS) {
            const uint32_t e = x & 63u, j = (x >> 6) % HRT_CV_BATCH, which = x / (HRT_CV_BLOCK * HRT_CV_BATCH);
            if (j < n) {
                const bool in = (which ? cb : rb) * HRT_CV_BLOCK + e < S.n;
                sS[which][j][e] = in ? steer(P.fa_c, sEl[which][e], sU[j]) : make_float2(0.f, 0.f);
            }
        }
        __syncthreads();
        if (live_r) {
            for (uint32_t j = 0; j < n; ++j) {
                const float2 s = sS[0][j][16u * w + (lane & 15u)];
                // A: rows 0..15 (cos, -sin), rows 16..31 (sin, cos) of the row tile's elements; k = h
                const float a = hi ? (h ? s.x : s.y) : (h ? -s.y : s.x);
                const float pte = sP[j][0], ptm = sP[j][1];
                if (live_c0) {   // B: k = 0 p cos, k = 1 -p sin of the column tile's elements
                    const float2 q = sCol[j][lane & 31u];
                    const float v = h ? -q.y : q.x;
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, pte * v, acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, ptm * v, acc[0][1], 0, 0, 0);
                }
                if (live_c1) {
                    const float2 q = sCol[j][32u + (lane & 31u)];
                    const float v = h ? -q.y : q.x;
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, pte * v, acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, ptm * v, acc[1][1], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // D: lane = column, register r = row (r & 3) + 8 (r >> 2) + 4 h; rows 0..15 Re, 16..31 Im of 16 row elements
    if (!live_r) return;
    float2 *dst = reinterpret_cast<float2 *>(P.partial) + (uint64_t)link * S.per_link + S.off + (uint64_t)c * S.stride +
                  (uint64_t)blk * BLOCK2;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const uint32_t col = 32u * t + (lane & 31u);
        const bool col_ok = cb * HRT_CV_BLOCK + col < S.n;
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const uint32_t row = 16u * w + (r & 3) + 8u * (r >> 2) + 4u * h;
                if (col_ok && rb * HRT_CV_BLOCK + row < S.n)
                    dst[(uint64_t)q * S.nblk * BLOCK2 + row * HRT_CV_BLOCK + col] = make_float2(acc[t][q][r], acc[t][q][r + 8]);
            }
    }
}

// one thread per (link, side, pol, i, i'); those with i' >= i: the chunks in index order, + LoS, -> out[i, i'] and,
// conjugated, out[i', i]; the diagonal real
__global__ void hrt_cov_reduce_kernel(const hrt_kcov P)
{
    const hrt_kview &V = P.v;
    const uint64_t links = (uint64_t)V.nrx * V.ntx;
    const uint64_t n_rx = links * 2u * P.n[0] * P.n[0], n_tx = links * 2u * P.n[1] * P.n[1];
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_rx + n_tx) return;
    const uint32_t side = gid >= n_rx ? 1u : 0u;
    const cv_side S = side_of(P, side);
    const uint64_t e = gid - (side ? n_rx : 0u), nn = (uint64_t)S.n * S.n;
    const uint32_t link = (uint32_t)(e / (2u * nn));
    const uint32_t m = (uint32_t)(e % nn), pol = (uint32_t)(e / nn) & 1u;
    const uint32_t i = m / S.n, k = m - i * S.n;
    if (k < i) return;
    const float2 *src = reinterpret_cast<const float2 *>(P.partial) + (uint64_t)link * S.per_link + S.off +
                        ((uint64_t)pol * S.nblk + block_index(S.nb, i / HRT_CV_BLOCK, k / HRT_CV_BLOCK)) * BLOCK2 +
                        (i % HRT_CV_BLOCK) * HRT_CV_BLOCK + k % HRT_CV_BLOCK;
    float2 s = sum_chunks(src, V.nchunks, S.stride);
    hrt_los_entry L;
    if (V.los && los_entry(V, link, L)) {   // the partial kernel's float steering and products
        const float sg = side ? 1.f : -1.f;   // u_rx = -u_tx
        const float u[3] = {sg * L.ux, sg * L.uy, sg * L.uz};
        const float p = (float)((double)L.a * L.a);
        const float2 a = steer(P.fa_c, S.el + 3u * i, u), q = steer(P.fa_c, S.el + 3u * k, u);
        s.x += fmaf(-a.y, -(p * q.y), a.x * (p * q.x));
        s.y += fmaf(a.x, -(p * q.y), a.y * (p * q.x));
    }
    float2 *o = reinterpret_cast<float2 *>(P.out) + (gid - m);
    if (k == i) s.y = 0.f;
    store_out(o + m, s, V.accumulate);
    if (k != i) store_out(o + (uint64_t)k * S.n + i, make_float2(s.x, -s.y), V.accumulate);
}

extern "C" int hrt_hip_launch_covariance(const hrt_kcov *P, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint32_t links = P->v.nrx * P->v.ntx;
    if (P->v.nchunks) {
        const int e = hrt_hip_launch_segments(&P->v, stream);
        if (e) return e;
        hipLaunchKernelGGL(hrt_cov_partial_kernel, dim3(P->nblk[0] + P->nblk[1], P->v.nchunks, links),
                           dim3(HRT_CV_THREADS), 0, st, *P);
    }
    const uint64_t n = (uint64_t)links * 2u * ((uint64_t)P->n[0] * P->n[0] + (uint64_t)P->n[1] * P->n[1]);
    hipLaunchKernelGGL(hrt_cov_reduce_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, st, *P);
    return (int)hipGetLastError();
}
