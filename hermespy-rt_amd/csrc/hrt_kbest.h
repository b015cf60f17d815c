/* hrt_kbest.h -- internal contract between csrc/host/channel.c (hrt_channel_kbest) and the K-best tree-search
 * detection kernel (csrc/hrt_kbest.hip).  Plain C; passed to the kernel by value.
 *
 *     [H | y] = Q [R | z] by modified Gram-Schmidt (optionally sorted), rho = |y - Q z|^2;
 *     breadth-first over the positions Nt - 1 .. 0, the K paths of smallest partial distance survive a level;
 *     index, metric: the best leaf of the final list;  llr: max-log over the final list's leaves, clamped
 *     one point per (rx, tx, pol, m, k)
 *
 * Form.  A group of g = hrt_kbest_form(Nr, Nt, K) lanes owns one point: g is the smallest power of two >= K whose LDS
 * share holds the point (below), so g = K wherever the matrix is small enough and a lane is a survivor.  Narrow
 * (g < 64): a wave holds 64 / g points; wide (g = 64): one point per wave.  A workgroup of HRT_KB_THREADS threads holds
 * HRT_KB_THREADS / g points, contiguous ones.  Lanes K .. g - 1 of a group (g > K only) never hold a survivor.
 *
 * LDS.  A thread has HRT_KB_WORDS float words, word e of thread w at float index e HRT_KB_THREADS + w:
 *   matrix   A = [H | y], Nr x n with n = Nt + 1; lane l of the group owns the rows l + g k, k < mk = ceil(Nr / g),
 *            rows beyond Nr are zero; entry (k, c, part) is the lane's word (k n + c) 2 + part (hrt_mgs.inc's layout).
 *   point    behind the lanes' matrix words, word w of the point is word mk n 2 + w / g of the group's lane w % g:
 *            R[t][u] (position t, STREAM u) at w = (t Nt + u) 2 + part, z[t] at w = (Nt Nt + t) 2 + part;
 *            hrt_kbest_point_words(Nt) = 2 Nt (Nt + 1) words.
 *   g is the smallest power of two >= K with 2 n ceil(Nr / g) + ceil(point words / g) <= HRT_KB_WORDS.
 * The constellation's image is hrt_detect.h's (float2 slot x holds S[x]), 8 M bytes behind the threads' words.
 *
 * Sums.  An inner product or a squared norm of columns is a per-lane sum over the lane's rows k ascending (from zero,
 * each term (xr yr + xi yi) or (xr yi - xi yr) or (xr xr + xi xi) formed first), then a butterfly over the group
 * (lane ^ 1, ^ 2, ...): the same bits in every lane.  The detection order (a nibble per position) and the null
 * columns are group-uniform registers; lane 0 of the group writes R and z.
 *
 * Tree.  A lane holds one survivor as (PED, key); the key holds every decided stream's digit at its own position
 * j B, so it is the whole path.  A lane without a survivor holds PED = +inf (a point whose PED is really not finite is
 * flagged, so +inf never stands for a value that is reported).  Per level a lane forms b once and walks its M
 * children; the children with symbol x of all lanes are batch x.  A batch is sorted descending by (PED', key) with a
 * bitonic network of cross-lane compare-exchanges, the lane-wise minimum with the running best (ascending) holds the g
 * smallest of both and is bitonic, a bitonic merge sorts it; ranks K .. g - 1 are cleared.  A batch none of whose
 * children is at or below the current K-th best PED (wave-uniform ballot) is skipped: it cannot change the list.  Keys
 * are distinct, so the surviving set is defined by (PED', key) alone and the bytes do not depend on the network.
 *
 * Arithmetic, all float, no contraction: hermespy_rt.h hrt_kbest_spec, statement by statement. */
#ifndef HRT_KBEST_H
#define HRT_KBEST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HRT_KB_THREADS 256u           /* 4 waves per workgroup */
#define HRT_KB_WORDS 56u              /* LDS words per thread (the constellation's 2 KiB follow) */
#define HRT_KB_MAX_NR 64u
#define HRT_KB_MAX_NT 16u
#define HRT_KB_MAX_B 8u               /* bits per symbol */
#define HRT_KB_MAX_BITS 32u           /* Nt B: the key is one 32-bit word */
#define HRT_KB_MAX_K 64u
#define HRT_KB_MAX_M 256u

/* words of a point's R and z */
static inline uint32_t hrt_kbest_point_words(uint32_t nt)
{
    return 2u * nt * (nt + 1u);
}

/* whether K is a list size the kernel has: a power of two, 1 .. 64 */
static inline int hrt_kbest_k_ok(uint32_t k)
{
    return k >= 1u && k <= HRT_KB_MAX_K && !(k & (k - 1u));
}

/* lanes per point (0: outside the limits) */
static inline uint32_t hrt_kbest_form(uint32_t nr, uint32_t nt, uint32_t k)
{
    if (nr < 1u || nr > HRT_KB_MAX_NR || nt < 1u || nt > HRT_KB_MAX_NT || !hrt_kbest_k_ok(k)) return 0u;
    for (uint32_t g = k; g <= 64u; g *= 2u)
        if (2u * (nt + 1u) * ((nr + g - 1u) / g) + (hrt_kbest_point_words(nt) + g - 1u) / g <= HRT_KB_WORDS) return g;
    return 0u;
}

typedef struct {
    uint32_t nr, nt, b;             /* H is Nr x Nt, B bits per symbol, Nt B <= 32 */
    uint32_t k;                     /* the list size */
    uint32_t g;                     /* lanes per point: hrt_kbest_form(nr, nt, k) */
    uint32_t mk;                    /* rows per lane: ceil(nr / g) */
    uint32_t llr;                   /* 1: HRT_KB_LLR */
    uint32_t sorted;                /* 1: HRT_KB_SORTED */
    uint32_t skip;                  /* 1: skip a batch that cannot enter the list (0 only for measurements: same bytes) */
    float n0;                       /* the noise power */
    float clip;                     /* the LLR clip */
    uint32_t pts;                   /* points per link: 2 T K */
    uint32_t points;                /* links * pts, < 2^31 */
    void *out;                      /* the regions of hermespy_rt.h, one behind the other: index, metric and status
                                     * [points] (4 bytes each), llr float [links][Nt][B][pts] (HRT_KB_LLR) */
} hrt_kkbest;

/* H: complex [links][Nr][Nt][pts]; Y: complex [links][Nr][pts]; S: complex [2^b]; none is written */
int hrt_hip_launch_kbest(const hrt_kkbest *P, const void *H, const void *Y, const void *S, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_KBEST_H */
