/* hrt_beam_taps.h -- internal contract between csrc/host/channel.c (hrt_beam_taps) and the beam taps kernels
 * (csrc/hrt_beam_taps.hip).  Plain C; passed to the kernels by value.
 *
 * Per link (rx, tx) the beamformed taps are the real GEMM of csrc/hrt_array_taps.h with beam pairs for element pairs
 * (DESIGN.md section 17):
 *     h[g, i] = sum_p U[g, p] V[p, i],   g = 4 ((a Bt + b) T + m) + q,  q = (TE re, TE im, TM re, TM im)
 *     U = Re / Im of a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)) G[a Bt + b, p],   V = sinc(l_i - f_s tau_p)
 *     G = g_rx[a](u_rx) g_tx[b](u_tx)   (csrc/hrt_beam_channel.h)
 * on v_mfma_f32_16x16x4_f32.  |G| is not 1, so G enters U as a complex product, not as a phase.  The two forms and
 * their tiles are hrt_array_taps': rt = 4 (Br Bt T >= 13) with blocks of 64 (pair, time) rows x 4 column tiles, rt = 1
 * with blocks of 4 rows x 16 column tiles.
 *
 * The gain stage is csrc/hrt_beam_gains.inc (element tiles of HRT_BM_ETILE in LDS, FP32 within a tile, FP64 across
 * the tiles) for the beams the block's rows touch.  A block of `cap` rows (64 or 4) that starts at row0 covers the
 * pairs pf = row0 / T .. pl = (min(row0 + cap, rows) - 1) / T: at most cap of them, and it may begin and end inside
 * a pair.  Its RX slot s is beam pf / Bt + s, up to beam pl / Bt; its TX slot s is beam s where every TX beam fits
 * (Bt <= cap), else the beam of pair pf + s, (pf + s) mod Bt -- at most cap slots a side.  The LoS gains of every
 * (link, pair) are formed once by hrt_beam_taps_los_kernel into the scratch (behind the partial sums) and read by the
 * reduce kernel. */
#ifndef HRT_BEAM_TAPS_H
#define HRT_BEAM_TAPS_H

#include <stddef.h>
#include <stdint.h>

#include "hrt_beam_channel.h"
#include "hrt_pathsum.h"
#include "hrt_taps.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    hrt_kview v;
    hrt_kshard sh;                  /* (20 bytes: the fields below follow it directly) */
    uint32_t nr, nt, br, bt, npairs;   /* elements, beams; npairs = br * bt */
    hrt_ktgrid g;                   /* L .. dt (csrc/hrt_pathsum.h): hrt_karray_taps' with npairs = br * bt */
    double fa_c;                    /* f_a / c: revolutions per metre of path difference */
    const float *rx_el, *tx_el;     /* device [nr][3], [nt][3] element offsets (m) */
    const float *rx_w, *tx_w;       /* device [br][nr][2], [bt][nt][2] weights (re, im) */
    float *partial;                 /* scratch: complex [link][chunk][pair][pol][T][L] */
    float *los;                     /* scratch: complex [link][pair] gains at the LoS directions */
    float *out;                     /* complex [nrx][ntx][br][bt][2][T][L] */
} hrt_kbeam_taps;

_Static_assert(offsetof(hrt_kbeam_taps, nr) == 132 && offsetof(hrt_kbeam_taps, g.fs) == 192 &&
               offsetof(hrt_kbeam_taps, g) == 152 && offsetof(hrt_kbeam_taps, rx_el) == 232,
               "hrt_kbeam_taps: the argument offsets");

int hrt_hip_launch_beam_taps(const hrt_kbeam_taps *P, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_BEAM_TAPS_H */
