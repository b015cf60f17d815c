/* hrt_array_taps.h -- internal contract between csrc/host/channel.c (hrt_array_taps) and the array taps kernels
 * (csrc/hrt_array_taps.hip).  Plain C; passed to the kernels by value.
 *
 * Per link (rx, tx) the array taps are the real GEMM of csrc/hrt_taps.h with more rows:
 *     h[g, i] = sum_p U[g, p] V[p, i],   g = 4 (a T + m) + q,  a = i_r Nt + j_t (element pair),
 *                                        q = (TE re, TE im, TM re, TM im)
 *     U = Re / Im of a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p + f_a (r_i . u_p^rx + q_j . u_p^tx) / c)),
 *     V = sinc(l_i - f_s tau_p)
 * on v_mfma_f32_16x16x4_f32: a row tile is 16 rows g (4 (pair, time) rows), a column tile 16 taps, one MFMA takes 4
 * records.  The steering folds into U (the sinc is real), so a record costs 8 FLOP per (pair, time, tap), as in
 * hrt_taps.  A workgroup (4 waves) writes one chunk of the link's records to the partial sums of the scratch; the
 * reduce kernel adds the chunks in a fixed order (csrc/hrt_pathsum.h).  The GEMM's tile setup, MFMA loop and write-back
 * are csrc/hrt_taps_gemm.inc, the grid hrt_ktgrid (csrc/hrt_pathsum.h), both shared with hrt_beam_taps.  Two forms:
 *   rt = 4 (the grid has at least 4 row tiles: Nr Nt T >= 13): a wave holds RT = 4 row tiles x CT = 4 column tiles,
 *          the 4 waves stand along the rows: a block of 16 row tiles (64 (pair, time) rows) x 4 column tiles, so a
 *          staged record (its loads, u_tx, sinc parameters) serves 64 MFMAs;
 *   rt = 1 (smaller grids): hrt_taps' RT = 1 form, 1 row tile x 4 column tiles a wave, the waves along the columns. */
#ifndef HRT_ARRAY_TAPS_H
#define HRT_ARRAY_TAPS_H

#include <stddef.h>
#include <stdint.h>

#include "hrt_pathsum.h"
#include "hrt_taps.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    hrt_kview v;
    hrt_kshard sh;                  /* (20 bytes: the fields below follow it directly) */
    uint32_t nr, nt, npairs;        /* elements; npairs = nr * nt */
    hrt_ktgrid g;                   /* L .. dt (csrc/hrt_pathsum.h): rows = npairs * T; rt 4: rblocks = ceil(rtiles / 16),
                                       cblocks = ceil(ctiles / 4); rt 1: rblocks = rtiles, cblocks = ceil(ctiles / 16) */
    double fa_c;                    /* f_a / c: revolutions per metre of path difference */
    const float *rx_el, *tx_el;     /* device [nr][3], [nt][3] element offsets (m) */
    float *partial;                 /* scratch: complex [link][chunk][pair][pol][T][L] */
    float *out;                     /* complex [nrx][ntx][nr][nt][2][T][L] */
} hrt_karray_taps;

_Static_assert(offsetof(hrt_karray_taps, g) == 144 && offsetof(hrt_karray_taps, g.fs) == 184 &&
               offsetof(hrt_karray_taps, rx_el) == 224, "hrt_karray_taps: the argument offsets");

int hrt_hip_launch_array_taps(const hrt_karray_taps *P, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_ARRAY_TAPS_H */
