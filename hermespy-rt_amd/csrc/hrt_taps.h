/* hrt_taps.h -- internal contract between csrc/host/channel.c (hrt_taps) and the taps kernels (csrc/hrt_taps.hip).
 * Plain C; passed to the kernels by value.
 *
 * Per link (rx, tx) the taps are a real GEMM over the link's records p:
 *     h[g, i] = sum_p U[g, p] V[p, i],   g = 4 m + q,  q = (TE re, TE im, TM re, TM im)
 *     U = Re / Im of a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)),   V = sinc(l_i - f_s tau_p)
 * on v_mfma_f32_16x16x4_f32: a row tile is 16 rows g (4 time samples), a column tile 16 taps, one MFMA takes 4
 * records.  A workgroup (4 waves) forms HRT_TP_WTILES accumulator tiles per wave: RT row tiles x CT column tiles with
 * RT * CT = 4 (RT = 4 when the grid has at least 4 row tiles, else RT = 1); wave w takes column tiles
 * (cb * 4 + w) * CT .. + CT - 1 and row tiles rb * RT .. + RT - 1.  It writes one chunk of the link's records to
 * the partial sums of the scratch; the reduce kernel adds the chunks in a fixed order (csrc/hrt_pathsum.h).  The tile
 * setup and the MFMA loop are csrc/hrt_taps_gemm.inc, shared with the array and beam taps kernels.
 *
 * hrt_ktaps holds the fields of the taps grid (hrt_ktgrid of csrc/hrt_pathsum.h, without rows: here rows = T) written
 * out, where they always were: taps_plan() of csrc/host/channel.c fills them from a hrt_ktgrid, and the shared device
 * code takes the hrt_ktaps itself as its grid.  As a hrt_ktgrid member the fields move by 4 and 8 bytes and the
 * kernel-argument loads of hrt_taps_partial_kernel regroup (profiles/HISTORY.md). */
#ifndef HRT_TAPS_H
#define HRT_TAPS_H

#include <stdint.h>

#include "hrt_pathsum.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HRT_TP_THREADS 256u   /* 4 waves per workgroup */
#define HRT_TP_WTILES 4u      /* accumulator tiles (16 x 16) per wave */
#define HRT_TP_BATCH 32u      /* unblocked records staged in LDS at a time (8 MFMA k-steps) */
#define HRT_TP_MAX_POINTS (1u << 20)    /* num_taps * num_times */
#define HRT_TP_MAX_TAP (1 << 24)        /* |l_min|, |l_min + num_taps|: tap indices exact in f32 */

typedef struct {
    hrt_kview v;
    uint32_t L, T;                  /* taps, time samples */
    int32_t l_min;
    uint32_t rtiles, ctiles;        /* ceil(4 T / 16), ceil(L / 16) */
    uint32_t rt;                    /* row tiles per wave: 4 or 1 (column tiles per wave: 4 / rt) */
    uint32_t rblocks, cblocks;      /* ceil(rtiles / rt), ceil(ctiles / (4 * (4 / rt))) */
    double fs, fc, t0, dt;
    float *partial;                 /* scratch: complex [link][chunk][pol][T][L] */
    float *out;                     /* complex [nrx][ntx][2][T][L] */
} hrt_ktaps;

int hrt_hip_launch_taps(const hrt_ktaps *P, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_TAPS_H */
