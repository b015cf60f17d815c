/* hrt_codebook.h -- internal contract between csrc/host/channel.c (hrt_codebook_select) and the codebook selection
 * kernel (csrc/hrt_codebook.hip).  Plain C; passed to the kernel by value.
 *
 *     E_c,k = H_k W_c (Nr x L);   mu_c = (1/n) sum_k f(E_c,k),   f = |E|_F^2 (POWER) or log2 det(I + E^H E / N0)
 *     (CAPACITY);   c* = argmax_c mu_c, the lowest index on a tie
 *     one subband per (rx, tx, pol, m, b): the frequencies k0 = b S .. k0 + n - 1, n = min(S, K - k0)
 *
 * Form.  A workgroup of HRT_CS_THREADS threads owns HRT_CS_WAVES consecutive subbands, one per wave, and walks the
 * codebook in tiles of CT entries staged through LDS; lane j of every wave owns entry c0 + j of the tile (lanes
 * >= CT idle), so a tile is read from memory once for all the workgroup's subbands and every lane scores its entry
 * against its wave's subband alone, all n frequencies in turn: mu_c is complete in one lane, and the running best
 * (mu, c) of a lane is over ascending c.  CT = hrt_codebook_tile(Nt, L): 64 while the tile fits HRT_CS_LDS_BYTES,
 * 32 beyond (Nt L > 128: half of every wave idles -- a third form that splits an entry over lanes would change the
 * order of the sums).  The tile's LDS image: entry j, element (t, l) is the float2 slot (t L + l) CT + j, that is
 * the words 2 ((t L + l) CT + j) + {0 re, 1 im}; entries beyond C are zeros.  Staging thread w of a pass writes
 * slot w and reads W[c0 + w % CT][w / CT], so every word has one owner and both the staging stores and the scoring
 * loads (one float2 per lane, consecutive lanes consecutive slots) are free of bank conflicts.
 * H's elements are the same address for a whole wave (its subband's), read from global memory.
 *
 * Arithmetic, all float, no contraction.  For a row i of H and a layer l, over t ascending from zero:
 *     er = er + (hr wr - hi wi);   ei = ei + (hr wi + hi wr)            (h = H[i][t], w = W[t][l])
 * then over the rows i ascending, for the layers a and b < a:
 *     gd[a] = gd[a] + (er_a er_a + ei_a ei_a)
 *     gr[a][b] = gr[a][b] + (er_a er_b + ei_a ei_b);   gi[a][b] = gi[a][b] + (er_a ei_b - ei_a er_b)
 * (gr, gi under CAPACITY only: G = E^H E, G[a][b] = conj(e_a) . e_b).  POWER: f = ((gd[0] + gd[1]) + ..) over l
 * ascending.  CAPACITY: A[a][a] = 1 + gd[a] / N0, A[a][b] = (gr / N0, gi / N0), and the unpivoted LDL^H, j ascending:
 *     for m < j:  v = A[j][m];  for p < m:  vr = vr - (l_jp.r l_mp.r + l_jp.i l_mp.i) d_p,
 *                                           vi = vi - (l_jp.i l_mp.r - l_jp.r l_mp.i) d_p;   l_jm = (vr / d_m, vi / d_m)
 *     d_j = A[j][j];  for m < j:  d_j = d_j - (l_jm.r l_jm.r + l_jm.i l_jm.i) d_m
 * det = ((d_0 d_1) d_2) d_3 and f = hrt_cs_log2(det), below.  mu = (f_k0 + f_k0+1 + ..) / (float)n.
 * The `effective` pass runs the first statement again for c* (W from global memory): the same bits. */
#ifndef HRT_CODEBOOK_H
#define HRT_CODEBOOK_H

#include <stdint.h>
#include <string.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HRT_CS_THREADS 256u           /* 4 waves per workgroup */
#define HRT_CS_WAVES 4u               /* subbands per workgroup: one per wave */
#define HRT_CS_LDS_BYTES 65536u       /* the largest tile image */
#define HRT_CS_MAX_NR 16u
#define HRT_CS_MAX_NT 64u
#define HRT_CS_MAX_L 4u
#define HRT_CS_MAX_C 4096u
#define HRT_CS_ROWS 4u                /* rows of H a lane carries through one walk over t */

/* entries per codebook tile (0: outside the limits); the image takes CT * nt * l * 8 bytes of LDS */
static inline uint32_t hrt_codebook_tile(uint32_t nt, uint32_t l)
{
    if (nt < 1u || nt > HRT_CS_MAX_NT || l < 1u || l > HRT_CS_MAX_L || l > nt) return 0u;
    return 64u * nt * l * 8u <= HRT_CS_LDS_BYTES ? 64u : 32u;
}

/* the float2 slot of element (t, l) of the tile's entry j (the form above) */
static inline uint32_t hrt_codebook_slot(uint32_t ct, uint32_t l_count, uint32_t j, uint32_t t, uint32_t l)
{
    return (t * l_count + l) * ct + j;
}

/* log2 of a float, restated in plain float operations so that an emulation follows it bit for bit (never the
 * hardware's approximate instruction).  x = 2^e f by the bits, f in [1, 2); f > HRT_CS_SQRT2 is halved (exact) and e
 * raised, so f lies in (sqrt(1/2), sqrt(2)].  With s = (f - 1) / (f + 1) and z = s s,
 *     log2 f = s (c0 + z (c1 + z (c2 + z (c3 + z c4)))),   c_j = 2 / ((2 j + 1) ln 2) rounded to float
 * (the series of 2 atanh(s) / ln 2 cut after z^4: |s| <= 0.1716, the first term left out is below 2^-28 of the sum)
 * and the result is (float)e + that.  An x that is not a normal positive float (zero, negative, subnormal, Inf, NaN)
 * gives NaN: the determinants this is for are >= 1. */
#define HRT_CS_SQRT2_BITS 0x3fb504f3u /* the float nearest sqrt(2) */
#define HRT_CS_LOG2_C0 2.8853900817779268f
#define HRT_CS_LOG2_C1 0.9617966939259756f
#define HRT_CS_LOG2_C2 0.5770780163555854f
#define HRT_CS_LOG2_C3 0.4121985831111324f
#define HRT_CS_LOG2_C4 0.3205988979753252f
#ifdef __HIPCC__
__host__ __device__
#endif
static inline float hrt_cs_log2(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    if (u < 0x00800000u || u >= 0x7f800000u) {
        const uint32_t nan = 0x7fc00000u;
        float r;
        memcpy(&r, &nan, 4);
        return r;
    }
    int32_t e = (int32_t)(u >> 23) - 127;
    uint32_t m = (u & 0x007fffffu) | 0x3f800000u;
    if (m > HRT_CS_SQRT2_BITS) {
        m -= 0x00800000u;
        e += 1;
    }
    float f;
    memcpy(&f, &m, 4);
    const float s = (f - 1.0f) / (f + 1.0f);
    const float z = s * s;
    float p = HRT_CS_LOG2_C3 + z * HRT_CS_LOG2_C4;
    p = HRT_CS_LOG2_C2 + z * p;
    p = HRT_CS_LOG2_C1 + z * p;
    p = HRT_CS_LOG2_C0 + z * p;
    return (float)e + s * p;
}

typedef struct {
    uint32_t nr, nt, l, c;          /* H is Nr x Nt, an entry Nt x L, C entries */
    uint32_t ct;                    /* entries per tile: hrt_codebook_tile(nt, l) */
    uint32_t capacity;              /* 1: HRT_CS_CAPACITY, 0: HRT_CS_POWER */
    uint32_t T, K, S, B;            /* times, frequencies, frequencies per subband, subbands per (rx, tx, pol, m) */
    float n0;                       /* the noise power (CAPACITY) */
    uint64_t pts;                   /* points per link: 2 T K */
    uint64_t subbands;              /* links * 2 T B */
    uint32_t flags;                 /* HRT_CS_TABLE | HRT_CS_EFFECTIVE */
    void *out;                      /* the regions of hermespy_rt.h, one behind the other: index, metric and status
                                     * [subbands] (4 bytes each), table float [links][C][2 T B] (HRT_CS_TABLE),
                                     * effective complex [links][Nr][L][pts] (HRT_CS_EFFECTIVE; 8-byte aligned: the
                                     * subbands of a link are an even number) */
} hrt_kcodebook;

/* H: complex [links][Nr][Nt][pts]; W: complex [C][Nt][L]; neither is written */
int hrt_hip_launch_codebook(const hrt_kcodebook *P, const void *H, const void *W, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_CODEBOOK_H */
