/* hrt_array_channel.h -- internal contract between csrc/host/channel.c (hrt_array_channel) and the array channel
 * kernels (csrc/hrt_array_channel.hip).  Plain C; passed to the kernels by value.
 *
 * Per link (rx, tx) and polarisation the array channel is a complex GEMM over the link's records p:
 *     H_pol[a, c] = sum_p S[a, p] W_pol[p, c],   a = i * Nt + j (element pair),  c = (m, k) (time, frequency)
 *     S = exp(j 2 pi f_a (r_i . u_rx + q_j . u_tx) / c),   W_pol = a^pol exp(j 2 pi (nu t_m - f_k tau))
 * with W from the two-level factorisation of csrc/hrt_channel.h (K padded to K1 * HRT_CH_K2, row g = m * K1 + k1,
 * padded column g * HRT_CH_K2 + k2).  One v_mfma_f32_32x32x2_f32 takes one record's (re, im) as its K = 2 in the
 * 2x2 real embedding: A rows 0..15 = Re H of 16 pairs (A = (Re S, -Im S)), rows 16..31 = Im H (A = (Im S, Re S)),
 * B row 0 = Re W, row 1 = Im W, over 32 padded columns.
 * A workgroup (4 waves) forms HRT_AC_PAIRS pairs x HRT_AC_COLS padded columns of one link from one chunk of the
 * link's records and writes them to the partial sums of the scratch; the reduce kernel adds the chunks in a fixed
 * order (csrc/hrt_pathsum.h). */
#ifndef HRT_ARRAY_CHANNEL_H
#define HRT_ARRAY_CHANNEL_H

#include <stddef.h>
#include <stdint.h>

#include "hrt_pathsum.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HRT_AC_THREADS 256u   /* 4 waves per workgroup */
#define HRT_AC_PAIRS 32u      /* element pairs per workgroup: 2 MFMA row tiles of 16 */
#define HRT_AC_GROWS 16u      /* rows g per workgroup: HRT_AC_GROWS * 16 = 256 padded columns, 2 tiles of 32 a wave */
#define HRT_AC_BATCH 32u      /* unblocked records staged in LDS at a time */
#define HRT_AC_MAX_ELEMENTS 1024u
#define HRT_AC_MAX_POINTS (1u << 24)   /* Nr * Nt * T * K */

typedef struct {
    hrt_kview v;
    hrt_kshard sh;                  /* (20 bytes: the fields below follow it directly) */
    uint32_t nr, nt, npairs;        /* elements; npairs = nr * nt */
    hrt_kgrid g;                    /* K .. fa_c (csrc/hrt_pathsum.h) */
    const float *rx_el, *tx_el;     /* device [nr][3], [nt][3] element offsets (m) */
    float *partial;                 /* scratch: complex [link][chunk][pol][pair][T * K] */
    float *out;                     /* complex [nrx][ntx][nr][nt][2][T][K] */
} hrt_karray;

/* kernel-argument offsets alone have moved the partial kernel's SGPR spills and its time (hrt_kshard) */
_Static_assert(offsetof(hrt_karray, g) == 144 && offsetof(hrt_karray, rx_el) == 208, "hrt_karray: the argument offsets");

int hrt_hip_launch_array_channel(const hrt_karray *P, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_ARRAY_CHANNEL_H */
