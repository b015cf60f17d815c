/* hrt_equalizer.h -- internal contract between csrc/host/channel.c (hrt_channel_equalizer) and the equalizer kernel
 * (csrc/hrt_equalizer.hip).  Plain C; passed to the kernel by value.
 *
 *     W = (H^H H + lambda I)^-1 H^H,  sinr_i = 1 / (N0 G_ii) - [LMMSE],  G = (H^H H + lambda I)^-1
 *     one "point" per (rx, tx, pol, t, k), H = H[rx][tx][:, :][pol][t][k], Nr x Nt
 *
 * Modified Gram-Schmidt in float on the augmented matrix A = [H; sqrt(lambda) I] = Q R, column by column, never through
 * the Gram matrix.  The same column operations act on an n x n block T that starts as the identity, so that T ends as
 * R^-1.  The bottom block of A is sqrt(lambda) T at every step and is not stored a second time: an inner product of two
 * columns is the sum over the Nr rows of H's block plus lambda times the sum over the rows of T.  Then
 * G_ii = |row i of T|^2 and W^H = Q1 T^H (Q1: the top Nr rows of Q), formed column by column in place.
 *
 * A group of g lanes (hrt_equalizer_form: a power of two, 1 .. 64) owns one matrix; lane l of the group owns the rows
 * r = l + g k of the top block (k < mk = ceil(Nr / g)) and of T (k < nk = ceil(Nt / g)).  A column operation acts on
 * each row alone, so a word of LDS is read and written by one lane only between the barriers of the kernel; an inner
 * product is a per-lane sum over k, then a butterfly over the g lanes (lane ^ 1, ^ 2, ...), which leaves the same bits
 * in every lane of the group; an entry of T is handed to the group by a shuffle from its owner.
 *
 * LDS: entry (k, c, part) of the top block is the word ((k n + c) 2 + part) HRT_EQ_THREADS + tid with n = Nt, T follows
 * it: the 64 lanes of a wave read 64 consecutive words for a given entry (no bank conflict).  A thread has
 * HRT_EQ_WORDS words, and g is the smallest power of two with 2 n (mk + nk) <= HRT_EQ_WORDS: 64 KB of static LDS a
 * workgroup of 4 waves.  The rule is read by the host and mirrored in tests/equalizer_util.py. */
#ifndef HRT_EQUALIZER_H
#define HRT_EQUALIZER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HRT_EQ_THREADS 256u          /* 4 waves per workgroup */
#define HRT_EQ_WORDS 64u             /* LDS words per thread */
#define HRT_EQ_MAX_NT 16u
#define HRT_EQ_MAX_NR 64u
#define HRT_EQ_MAX_POINTS (1u << 24) /* Nr * Nt * num_times * num_freqs */

/* lanes per matrix: a pure function of the matrix size (0: outside the limits) */
static inline uint32_t hrt_equalizer_form(uint32_t nr, uint32_t nt)
{
    if (nt < 1u || nt > HRT_EQ_MAX_NT || nr < 1u || nr > HRT_EQ_MAX_NR) return 0u;
    for (uint32_t g = 1u; g <= 64u; g *= 2u)
        if (2u * nt * ((nr + g - 1u) / g + (nt + g - 1u) / g) <= HRT_EQ_WORDS) return g;
    return 0u;
}

typedef struct {
    uint32_t nr, nt;                /* the matrix of a point */
    uint32_t mk, nk;                /* rows of the top block and of T per lane */
    uint32_t lmmse;                 /* 1: lambda = n0, and 1 is subtracted from the SINR; 0: lambda = 0 */
    float n0;                       /* the noise power */
    uint64_t pts;                   /* points per link: 2 num_times num_freqs */
    uint64_t points;                /* links * pts */
    const float *H;                 /* complex [links][Nr][Nt][pts] */
    float *W;                       /* complex [links][Nt][Nr][pts], or NULL */
    float *sinr;                    /* [links][Nt][pts] */
    uint32_t *status;               /* [links][pts] */
} hrt_kequalizer;

int hrt_hip_launch_equalizer(const hrt_kequalizer *P, uint32_t g, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_EQUALIZER_H */
