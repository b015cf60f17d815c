/* hrt_precoder.h -- internal contract between csrc/host/channel.c (hrt_channel_precoder) and the precoder kernel
 * (csrc/hrt_precoder.hip).  Plain C; passed to the kernel by value.
 *
 *     P0 = H^H (MRT),  H^H (H H^H)^-1 (ZF),  H^H (H H^H + alpha I)^-1 (RZF);  P = P0 scaled to the power;
 *     E = H P,  sinr_i = |E_ii|^2 / (sum_{j != i} |E_ij|^2 + N0)
 *     one "point" per (rx, tx, pol, t, k), H = H[rx][tx][:, :][pol][t][k], Nr x Nt (Nr streams, Nt transmit elements)
 *
 * ZF and RZF are the equalizer's factorisation with the two sides swapped: modified Gram-Schmidt in float on the
 * augmented matrix A = [H^H; sqrt(alpha) I] = Q R, (Nt + Nr) x Nr, column by column, never through the Gram matrix
 * H H^H, with the column operations carried on an Nr x Nr block T that ends as R^-1 (csrc/hrt_equalizer.h, whose
 * loops csrc/hrt_mgs.inc holds for both kernels).  A^H A = H H^H + alpha I = R^H R and H^H = Q1 R, so
 * P0 = Q1 R^-H = Q1 T^H: what the equalizer calls W^H is P0 itself, Nt x Nr, and leaves the kernel as it lies.
 *
 * A group of g lanes owns one matrix; lane l of the group owns the rows r = l + g k of the top block (the transmit
 * elements, k < mk = ceil(Nt / g)) and of T (k < nk = ceil(Nr / g)).  The lane groups, the LDS layout -- entry
 * (k, c, part) of the top block is the word ((k n + c) 2 + part) HRT_PC_THREADS + tid with n = Nr, T follows it -- and the
 * word budget are the equalizer's, so the form rule is hrt_equalizer_form(Nt, Nr): g is the smallest power of two with
 * 2 Nr (mk + nk) <= HRT_PC_WORDS.  The rule is read by the host and mirrored in tests/precoder_util.py.
 *
 * E = H P is formed from H itself and from the scaled P that is stored, not from an identity of the factorisation
 * (E = I - alpha T T^H cancels when alpha is far above sigma^2 and would not describe the stored P).  H's block has
 * become P by then, so a lane reads H[i][t] for its own rows t once more from global memory (the workgroup has just
 * loaded them: they sit in L2), one row i of H at a time; its partial sums of E[i][:] lie in its first 2 Nr words of
 * T's region, which is dead after P0 is formed.  No second copy of H is kept: it would double the top block, which
 * halves the points of a workgroup for the shapes that fill the word budget and leaves no g for any Nr >= 11. */
#ifndef HRT_PRECODER_H
#define HRT_PRECODER_H

#include <stdint.h>

#include "hrt_equalizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HRT_PC_THREADS HRT_EQ_THREADS /* 4 waves per workgroup */
#define HRT_PC_WORDS HRT_EQ_WORDS     /* LDS words per thread */
#define HRT_PC_MAX_NR 16u             /* streams (rows of H) */
#define HRT_PC_MAX_NT 64u             /* transmit elements (columns of H) */
#define HRT_PC_MAX_POINTS (1u << 24)  /* Nr * Nt * num_times * num_freqs */

/* lanes per matrix: the equalizer's rule for the factored matrix [H^H; sqrt(alpha) I], whose top block is Nt x Nr
 * (0: outside the limits) */
static inline uint32_t hrt_precoder_form(uint32_t nr, uint32_t nt)
{
    return hrt_equalizer_form(nt, nr);
}

typedef struct {
    uint32_t nr, nt;                /* the matrix of a point: Nr x Nt */
    uint32_t mk, nk;                /* rows of the top block (of Nt) and of T (of Nr) per lane */
    uint32_t kind;                  /* HRT_PC_MRT, HRT_PC_ZF, HRT_PC_RZF */
    uint32_t stream;                /* 1: HRT_PC_STREAM, 0: HRT_PC_TOTAL */
    float alpha;                    /* the regularization (RZF), else 0 */
    float n0;                       /* the noise power */
    float power;                    /* Ptot (TOTAL), Ptot / Nr (STREAM) */
    uint64_t pts;                   /* points per link: 2 num_times num_freqs */
    uint64_t points;                /* links * pts */
    const float *H;                 /* complex [links][Nr][Nt][pts] */
    float *P;                       /* complex [links][Nt][Nr][pts], or NULL */
    float *sinr;                    /* [links][Nr][pts] */
    uint32_t *status;               /* [links][pts] */
} hrt_kprecoder;

int hrt_hip_launch_precoder(const hrt_kprecoder *P, uint32_t g, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_PRECODER_H */
