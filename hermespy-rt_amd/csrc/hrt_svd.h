/* hrt_svd.h -- internal contract between csrc/host/channel.c (hrt_channel_svd) and the SVD kernel (csrc/hrt_svd.hip).
 * Plain C; passed to the kernel by value.
 *
 *     H[rx][tx][:, :][pol][t][k] = u diag(sigma) v^H      one "point" per (rx, tx, pol, t, k), Nr x Nt
 *
 * One-sided (Hestenes) complex Jacobi in float on the tall orientation: A = H where Nr >= Nt, else H^H; m x n with
 * m = max(Nr, Nt), n = min(Nr, Nt).  Column pairs (p, q), p < q, are rotated in cyclic order; the rotations are
 * accumulated in the n x n unitary V, so that A V = (long side) diag(sigma).
 *
 * A group of g lanes (hrt_svd_form: a power of two, 1 .. 64) owns one matrix; lane l of the group owns the rows
 * r = l + g k of A (k < mk = ceil(m / g)) and of V (k < nk = ceil(n / g)).  A rotation acts on each row alone, so a
 * word of LDS is read and written by one lane only between the two barriers of the kernel; the three inner products
 * of a pair are per-lane sums over k, then a butterfly over the g lanes (lane ^ 1, ^ 2, ...), which leaves the same
 * bits in every lane of the group.
 *
 * LDS: entry (k, c, part) of A is the word ((k n + c) 2 + part) HRT_SVD_THREADS + tid, V follows A: the 64 lanes of a
 * wave read 64 consecutive words for a given entry (no bank conflict).  A thread has HRT_SVD_WORDS words, and g is
 * the smallest power of two with 2 n (mk + nk) <= HRT_SVD_WORDS: 64 KB of static LDS a workgroup of 4 waves.  The rule
 * is read by the host and mirrored in tests/svd_util.py. */
#ifndef HRT_SVD_H
#define HRT_SVD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HRT_SVD_THREADS 256u          /* 4 waves per workgroup */
#define HRT_SVD_WORDS 64u             /* LDS words per thread */
#define HRT_SVD_MAX_SHORT 16u         /* min(Nr, Nt) */
#define HRT_SVD_MAX_LONG 64u          /* max(Nr, Nt) */
#define HRT_SVD_MAX_POINTS (1u << 24) /* Nr * Nt * num_times * num_freqs */
#define HRT_SVD_MAX_SWEEPS 16u        /* the cap of the sweep loop */

/* lanes per matrix: a pure function of the matrix size (0: outside the limits) */
static inline uint32_t hrt_svd_form(uint32_t nr, uint32_t nt)
{
    const uint32_t m = nr > nt ? nr : nt, n = nr > nt ? nt : nr;
    if (n < 1u || n > HRT_SVD_MAX_SHORT || m > HRT_SVD_MAX_LONG) return 0u;
    for (uint32_t g = 1u; g <= 64u; g *= 2u)
        if (2u * n * ((m + g - 1u) / g + (n + g - 1u) / g) <= HRT_SVD_WORDS) return g;
    return 0u;
}

typedef struct {
    uint32_t nr, nt;                /* the matrix of a point */
    uint32_t m, n;                  /* max, min */
    uint32_t mk, nk;                /* rows of A and of V per lane */
    uint32_t tall;                  /* 1: A = H (Nr >= Nt), 0: A = H^H */
    uint32_t pad;
    uint64_t pts;                   /* points per link: 2 num_times num_freqs */
    uint64_t points;                /* links * pts */
    const float *H;                 /* complex [links][Nr][Nt][pts] */
    float *sigma;                   /* [links][n][pts] */
    float *u;                       /* complex [links][Nr][n][pts], or NULL */
    float *v;                       /* complex [links][Nt][n][pts], or NULL */
    uint32_t *sweeps;               /* [links][pts] */
} hrt_ksvd;

int hrt_hip_launch_svd(const hrt_ksvd *P, uint32_t g, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_SVD_H */
