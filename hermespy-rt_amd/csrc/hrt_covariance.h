/* hrt_covariance.h -- internal contract between csrc/host/channel.c (hrt_array_covariance) and the covariance kernels
 * (csrc/hrt_covariance.hip).  Plain C; passed to the kernels by value.
 *
 * Per link (rx, tx), side (RX: the elements r_i and u = u_rx; TX: q_j and u = u_tx) and polarisation the spatial
 * covariance is a Hermitian rank-one update per term, a real GEMM over the link's records p:
 *     R_pol[i, i'] = sum_p p_pol s_i(u_p) conj(s_i'(u_p)),   s_i(u) = exp(j 2 pi f_a r_i . u / c),   p_pol = |a^pol|^2
 * One v_mfma_f32_32x32x2_f32 takes one record as its K = 2 in the 2x2 real embedding of csrc/hrt_array_channel.h:
 * A rows 0..15 = (cos_i, -sin_i) and rows 16..31 = (sin_i, cos_i) of 16 row elements, B row 0 = p cos_i' and row 1 =
 * -p sin_i' over 32 column elements (one B per polarisation), so D rows 0..15 are Re R and rows 16..31 Im R of a
 * 16 x 32 tile.  A workgroup (4 waves) forms one HRT_CV_BLOCK x HRT_CV_BLOCK block of the upper triangle (column
 * block >= row block; wave w the row tile w, both column tiles, both polarisations) from one chunk of the link's
 * records and writes it to the scratch; the reduce kernel adds the chunks in a fixed order, adds the LoS term, and
 * writes the upper triangle, its mirror and the real diagonal (csrc/hrt_pathsum.h).
 *
 * The scratch: seg, then partial, complex [link][side][chunk][pol][block][HRT_CV_BLOCK][HRT_CV_BLOCK], the sides that
 * are asked for in the order RX, TX, block (rb, cb) of a side with nb = ceil(N / HRT_CV_BLOCK) block rows at index
 * rb nb - rb (rb - 1) / 2 + cb - rb.  Entries past the side's N elements are never written and never read. */
#ifndef HRT_COVARIANCE_H
#define HRT_COVARIANCE_H

#include <stddef.h>
#include <stdint.h>

#include "hrt_pathsum.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HRT_CV_THREADS 256u        /* 4 waves per workgroup */
#define HRT_CV_BLOCK 64u           /* elements per block row and column: 4 row tiles of 16, 2 column tiles of 32 */
#define HRT_CV_BATCH 64u           /* unblocked records staged in LDS at a time */
#define HRT_CV_MAX_ELEMENTS 256u   /* per side */
#define HRT_CV_MAX_OUTPUTS (1ull << 26)   /* links * 2 * (Nr^2 + Nt^2) complex outputs */

typedef struct {
    hrt_kview v;
    hrt_kshard sh;                  /* (20 bytes: the fields below follow it directly) */
    uint32_t sides;                 /* HRT_COV_RX | HRT_COV_TX */
    uint32_t n[2];                  /* elements of the RX / TX side; 0: the side is not asked for */
    uint32_t nblk[2];               /* blocks of the side's upper triangle: nb (nb + 1) / 2 */
    double fa_c;                    /* f_a / c: revolutions per metre of path difference */
    const float *el[2];             /* device [n][3] element offsets (m) of the side */
    float *partial;                 /* scratch: layout above */
    float *out;                     /* complex R_rx [nrx][ntx][2][Nr][Nr], then R_tx [nrx][ntx][2][Nt][Nt] */
} hrt_kcov;

_Static_assert(offsetof(hrt_kcov, sh) == 112 && offsetof(hrt_kcov, sides) == 132 && offsetof(hrt_kcov, n) == 136 &&
               offsetof(hrt_kcov, nblk) == 144 && offsetof(hrt_kcov, fa_c) == 152 && offsetof(hrt_kcov, el) == 160 &&
               offsetof(hrt_kcov, partial) == 176 && offsetof(hrt_kcov, out) == 184 && sizeof(hrt_kcov) == 192,
               "hrt_kcov: the argument offsets");

int hrt_hip_launch_covariance(const hrt_kcov *P, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_COVARIANCE_H */
