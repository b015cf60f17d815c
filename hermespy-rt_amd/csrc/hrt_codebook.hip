// hrt_codebook.hip -- per-subband precoder codebook selection (PMI search) on an array channel, for gfx950: every entry
// W_c of a finite codebook is scored against the channel matrices of a subband and the best index is kept.
//
//     E_c,k = H_k W_c,   mu_c = (1/n) sum_k |E_c,k|_F^2  or  (1/n) sum_k log2 det(I + E_c,k^H E_c,k / N0),
//     c* = argmax_c mu_c (lowest index on a tie)
//
// The form, the LDS image and the order of every sum are csrc/hrt_codebook.h's.  VALU form: a lane owns one entry of
// the tile and one subband (its wave's), so E, the L x L Gram matrix, its LDL^H and the subband mean stay in that
// lane's registers and the epilogue needs no gather; the codebook tile is the operand shared through LDS, H's elements
// are wave-uniform loads.  Up to three launches on the caller's stream, instantiated per L:
//   tiles      for every tile: barrier, the workgroup stages the tile (zeros beyond C), barrier, every live lane
//              scores its entry and keeps its best (mu, c) over ascending c with a strict >, and whether any mu was
//              not finite.
//   select     a butterfly over the wave: the larger mu, the lower c on a tie; lane 0 stores index, metric and status.
//   table      (HRT_CS_TABLE, a launch of its own) the tiles once more: the same statements give mu_c again, stored
//              as it is formed, or zero for a flagged subband -- whether a subband is flagged is known only after the
//              first walk, and every byte is written once.
//   effective  (HRT_CS_EFFECTIVE, a launch of its own) lane j forms rows (k, i) = j, j + 64, .. of E_c*,k by the
//              statement that scored it, W_c* read from global memory, and stores them; zeros for a flagged subband.
// The selection alone needs no second kernel; the two optional regions are launches of their own because one kernel
// holding all three ran out of scalar registers.
// A subband's bits depend on its own matrices and the codebook only: a lane's sums never leave the lane, the butterfly
// compares and moves, it does not add.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include <float.h>
#include <stdint.h>

#include "hermespy_rt.h"
#include "hrt_codebook.h"

#define CS_T HRT_CS_THREADS
#define CS_RB HRT_CS_ROWS

// er[r][l] + j ei[r][l] = sum_t h[r][t] w(t, l) for RB rows of H at once (row r's element t is h[min(r, rows - 1) si +
// t st]: a row beyond `rows` repeats the last one and is ignored by the caller)
template <uint32_t L, uint32_t RB, class WF>
__device__ __forceinline__ void cs_rows(const float2 *__restrict__ h, uint64_t si, uint64_t st, uint32_t rows,
                                        uint32_t nt, WF wf, float (&er)[RB][L], float (&ei)[RB][L])
{
    const float2 *hr[RB];
#pragma unroll
    for (uint32_t r = 0; r < RB; ++r) {
        hr[r] = h + (uint64_t)(r < rows ? r : rows - 1u) * si;
#pragma unroll
        for (uint32_t l = 0; l < L; ++l) er[r][l] = ei[r][l] = 0.f;
    }
    for (uint32_t t = 0; t < nt; ++t) {
        float2 w[L];
#pragma unroll
        for (uint32_t l = 0; l < L; ++l) w[l] = wf(t, l);
#pragma unroll
        for (uint32_t r = 0; r < RB; ++r) {
            const float2 x = hr[r][(uint64_t)t * st];
#pragma unroll
            for (uint32_t l = 0; l < L; ++l) {
                er[r][l] = er[r][l] + (x.x * w[l].x - x.y * w[l].y);
                ei[r][l] = ei[r][l] + (x.x * w[l].y + x.y * w[l].x);
            }
        }
    }
}

// f(E_c,k) of one frequency: h points at H[0][0] of it
template <uint32_t L, class WF>
__device__ __forceinline__ float cs_score(const float2 *__restrict__ h, uint64_t si, uint64_t st, uint32_t nr,
                                          uint32_t nt, WF wf, bool capacity, float n0)
{
    float gd[L], gr[L][L], gi[L][L];
#pragma unroll
    for (uint32_t a = 0; a < L; ++a) {
        gd[a] = 0.f;
#pragma unroll
        for (uint32_t b = 0; b < L; ++b) gr[a][b] = gi[a][b] = 0.f;
    }
    for (uint32_t i0 = 0; i0 < nr; i0 += CS_RB) {
        const uint32_t rows = nr - i0 < CS_RB ? nr - i0 : CS_RB;
        float er[CS_RB][L], ei[CS_RB][L];
        cs_rows<L, CS_RB>(h + (uint64_t)i0 * si, si, st, rows, nt, wf, er, ei);
#pragma unroll
        for (uint32_t r = 0; r < CS_RB; ++r) {
            if (r >= rows) break;
#pragma unroll
            for (uint32_t a = 0; a < L; ++a) {
                gd[a] = gd[a] + (er[r][a] * er[r][a] + ei[r][a] * ei[r][a]);
                if (capacity) {
#pragma unroll
                    for (uint32_t b = 0; b < a; ++b) {
                        gr[a][b] = gr[a][b] + (er[r][a] * er[r][b] + ei[r][a] * ei[r][b]);
                        gi[a][b] = gi[a][b] + (er[r][a] * ei[r][b] - ei[r][a] * er[r][b]);
                    }
                }
            }
        }
    }
    if (!capacity) {
        float f = gd[0];
#pragma unroll
        for (uint32_t a = 1; a < L; ++a) f = f + gd[a];
        return f;
    }
    // A = I + G / N0 and its unpivoted LDL^H, in place: gr, gi become l, gd becomes d
    float det = 1.f;
#pragma unroll
    for (uint32_t j = 0; j < L; ++j) {
#pragma unroll
        for (uint32_t m = 0; m < j; ++m) {
            float vr = gr[j][m] / n0, vi = gi[j][m] / n0;
#pragma unroll
            for (uint32_t p = 0; p < m; ++p) {
                vr = vr - (gr[j][p] * gr[m][p] + gi[j][p] * gi[m][p]) * gd[p];
                vi = vi - (gi[j][p] * gr[m][p] - gr[j][p] * gi[m][p]) * gd[p];
            }
            gr[j][m] = vr / gd[m];
            gi[j][m] = vi / gd[m];
        }
        float d = 1.f + gd[j] / n0;
#pragma unroll
        for (uint32_t m = 0; m < j; ++m) d = d - (gr[j][m] * gr[j][m] + gi[j][m] * gi[j][m]) * gd[m];
        gd[j] = d;
        det = j == 0u ? d : det * d;
    }
    return hrt_cs_log2(det);
}

// the tile's image: lane j's element (t, l)
struct cs_lds_w {
    const float2 *s;
    uint32_t ct, l;
    __device__ __forceinline__ float2 operator()(uint32_t t, uint32_t ll) const { return s[(t * l + ll) * ct]; }
};

// an entry in global memory: W[c][t][l]
struct cs_mem_w {
    const float2 *w;
    uint32_t l;
    __device__ __forceinline__ float2 operator()(uint32_t t, uint32_t ll) const { return w[t * l + ll]; }
};

// the subband of a wave: wave `wave` of workgroup `blockIdx.x` owns subband blockIdx.x HRT_CS_WAVES + wave
struct cs_subband {
    uint64_t sb, link, per_link;    // its index, its link, the subbands of a link: 2 T B
    uint32_t rem, n;                // its index within the link: (pol T + m) B + b; its frequencies
    uint64_t q0;                    // its first point within the link: (pol T + m) K + b S
    bool live;
};

__device__ __forceinline__ cs_subband cs_locate(const hrt_kcodebook &P)
{
    cs_subband s;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64u));
    s.sb = (uint64_t)blockIdx.x * HRT_CS_WAVES + wave;
    s.live = s.sb < P.subbands;
    s.per_link = 2ull * P.T * P.B;
    s.link = s.live ? s.sb / s.per_link : 0u;
    s.rem = s.live ? (uint32_t)(s.sb % s.per_link) : 0u;
    const uint32_t pm = s.rem / P.B, k0 = (s.rem % P.B) * P.S;
    s.n = P.K - k0 < P.S ? P.K - k0 : P.S;
    s.q0 = (uint64_t)pm * P.K + k0;
    return s;
}

// the walk over the codebook.  TABLE false: the selection -- index, metric, status.  TABLE true, launched behind it on
// the same stream: the same statements give every mu_c again, stored as it is formed, or zero where the first walk
// flagged the subband (that is known only after the whole walk, and every byte is written once).
template <uint32_t L, bool TABLE>
__global__ void __launch_bounds__(HRT_CS_THREADS)
hrt_codebook_kernel(const hrt_kcodebook P, const float2 *__restrict__ H, const float2 *__restrict__ W)
{
    extern __shared__ float2 sW[];

    const uint32_t tid = threadIdx.x, lane = tid % 64u;
    const uint32_t nr = P.nr, nt = P.nt, C = P.c, ct = P.ct, ntl = nt * L;
    const cs_subband s = cs_locate(P);
    const uint64_t st = P.pts, si = (uint64_t)nt * P.pts;
    const float2 *const Hs = H + s.link * nr * si + s.q0;  // H[i][t] at the subband's frequency kk: Hs[i si + t st + kk]
    const cs_lds_w wf = {sW + lane, ct, L};
    const bool cap = P.capacity != 0u;
    // (the regions of hermespy_rt.h: index, metric, status, table, effective)
    uint32_t *const o = reinterpret_cast<uint32_t *>(P.out);

    float bm = -INFINITY;
    uint32_t bc = 0xffffffffu;
    bool bad = false;
    uint32_t flagged = 0u;
    if (TABLE && s.live) flagged = o[2u * P.subbands + s.sb];
    for (uint32_t c0 = 0; c0 < C; c0 += ct) {
        __syncthreads();
        for (uint32_t w = tid; w < ntl * ct; w += CS_T) {
            const uint32_t c = c0 + w % ct;
            sW[w] = c < C ? W[(uint64_t)c * ntl + w / ct] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        const uint32_t c = c0 + lane;
        if (!s.live || lane >= ct || c >= C) continue;
        float sum = 0.f;
        for (uint32_t kk = 0; kk < s.n; ++kk) {
            const float f = cs_score<L>(Hs + kk, si, st, nr, nt, wf, cap, P.n0);
            sum = kk == 0u ? f : sum + f;
        }
        const float mu = sum / (float)s.n;
        if (TABLE) {
            float *const table = reinterpret_cast<float *>(o) + 3u * P.subbands;
            table[(s.link * C + c) * s.per_link + s.rem] = flagged ? 0.f : mu;
        } else {
            bad = bad || !(fabsf(mu) <= FLT_MAX);
            if (mu > bm) {
                bm = mu;
                bc = c;
            }
        }
    }
    if (TABLE) return;

    // ---- select: the larger mu, the lower index on a tie
    for (uint32_t off = 32u; off > 0u; off >>= 1) {
        const float om = __shfl_xor(bm, (int)off, 64);
        const uint32_t oc = (uint32_t)__shfl_xor((int)bc, (int)off, 64);
        if (om > bm || (om == bm && oc < bc)) {
            bm = om;
            bc = oc;
        }
    }
    const uint32_t status = __any((int)bad) ? HRT_CS_NONFINITE : 0u;
    if (s.live && lane == 0u) {
        o[s.sb] = status ? 0xffffffffu : bc;
        reinterpret_cast<float *>(o)[P.subbands + s.sb] = status ? 0.f : bm;
        o[2u * P.subbands + s.sb] = status;
    }
}

// effective, launched behind the selection on the same stream: lane j of the subband's wave forms the rows (k, i) = j,
// j + 64, .. of E_c*,k by the statement that scored them, W_c* read from global memory; zeros for a flagged subband
template <uint32_t L>
__global__ void __launch_bounds__(HRT_CS_THREADS)
hrt_codebook_effective_kernel(const hrt_kcodebook P, const float2 *__restrict__ H, const float2 *__restrict__ W)
{
    const uint32_t lane = threadIdx.x % 64u, nr = P.nr, nt = P.nt;
    const cs_subband s = cs_locate(P);
    if (!s.live) return;
    const uint64_t st = P.pts, si = (uint64_t)nt * P.pts;
    const float2 *const Hs = H + s.link * nr * si + s.q0;
    const uint32_t *const o = reinterpret_cast<const uint32_t *>(P.out);
    const uint32_t best = o[s.sb], status = o[2u * P.subbands + s.sb];
    const uint64_t words = P.subbands * (3u + ((P.flags & HRT_CS_TABLE) ? P.c : 0u));   // even: 2 T B per link
    float2 *const E = reinterpret_cast<float2 *>(reinterpret_cast<float *>(P.out) + words) + s.link * nr * L * P.pts + s.q0;
    const cs_mem_w wg = {W + (uint64_t)(status ? 0u : best) * (nt * L), L};
    for (uint32_t e = lane; e < s.n * nr; e += 64u) {
        const uint32_t kk = e % s.n, i = e / s.n;
        float er[1][L], ei[1][L];
        if (!status) cs_rows<L, 1u>(Hs + (uint64_t)i * si + kk, si, st, 1u, nt, wg, er, ei);
#pragma unroll
        for (uint32_t l = 0; l < L; ++l)
            E[((uint64_t)i * L + l) * P.pts + kk] = status ? make_float2(0.f, 0.f) : make_float2(er[0][l], ei[0][l]);
    }
}

template <uint32_t L>
static void cs_launch(const hrt_kcodebook &P, const float2 *h, const float2 *w, hipStream_t st)
{
    const dim3 grid((uint32_t)((P.subbands + HRT_CS_WAVES - 1u) / HRT_CS_WAVES)), block(HRT_CS_THREADS);
    const size_t lds = (size_t)P.ct * P.nt * L * sizeof(float2);
    hipLaunchKernelGGL((hrt_codebook_kernel<L, false>), grid, block, lds, st, P, h, w);
    if (P.flags & HRT_CS_TABLE) hipLaunchKernelGGL((hrt_codebook_kernel<L, true>), grid, block, lds, st, P, h, w);
    if (P.flags & HRT_CS_EFFECTIVE) hipLaunchKernelGGL(hrt_codebook_effective_kernel<L>, grid, block, 0, st, P, h, w);
}

extern "C" int hrt_hip_launch_codebook(const hrt_kcodebook *P, const void *H, const void *W, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const float2 *h = (const float2 *)H, *w = (const float2 *)W;
    if (P->ct == 0u || (size_t)P->ct * P->nt * P->l * sizeof(float2) > HRT_CS_LDS_BYTES) return (int)hipErrorInvalidValue;
    switch (P->l) {
    case 1u: cs_launch<1u>(*P, h, w, st); break;
    case 2u: cs_launch<2u>(*P, h, w, st); break;
    case 3u: cs_launch<3u>(*P, h, w, st); break;
    case 4u: cs_launch<4u>(*P, h, w, st); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
