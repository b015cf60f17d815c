/* hrt_sparse_beam_taps.h -- internal contract between csrc/host/channel.c (hrt_sparse_beam_taps) and the kernel that
 * forms beamformed impulse responses from dominant-path lists (csrc/hrt_sparse_beam_taps.hip).  Plain C; passed to the
 * kernel by value.
 *
 * The input is a buffer of hrt_dominant_paths' layout (include/hermespy_rt.h): a header uint64_t [L][2] = {kept,
 * eligible}, then hrt_dominant_path [L][K].  Per link the beamformed taps of the list are the real GEMM of
 * csrc/hrt_beam_taps.h over the link's first n = min(kept, K) slots p:
 *     h[g, i] = sum_{p < n} U[g, p] V[p, i],   g = 4 ((a Bt + b) T + m) + q,  q = (TE re, TE im, TM re, TM im)
 *     U = Re / Im of a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)) g_rx[a](u_rx_p) g_tx[b](u_tx_p),  V = sinc(l_i - f_s tau_p)
 * with the tiles, the two forms (rt = 4: <4, 4, 4>, rt = 1: <1, 4, 1>) and the grid (hrt_ktgrid, taps_grid() with Br Bt
 * pairs) of csrc/hrt_array_taps.h, and the beam slots of csrc/hrt_beam_taps.h: a workgroup (4 waves) forms its block of
 * (beam pair, time) rows x taps of one link from ALL of the link's slots, walked in index order HRT_TP_BATCH at a time
 * as csrc/hrt_sparse_taps.h walks them, the gains of each batch formed by part 1 of csrc/hrt_beam_gains.inc, and writes
 * its accumulators straight to out.  One chunk per link: no partial sums, no reduce kernel, no LoS kernel, no
 * workspace view, no scratch.  The LoS entry is an ordinary slot; power, path, bounce and tri are not read, and neither
 * is any slot at or beyond n. */
#ifndef HRT_SPARSE_BEAM_TAPS_H
#define HRT_SPARSE_BEAM_TAPS_H

#include <stddef.h>
#include <stdint.h>

#include "hrt_array_taps.h"
#include "hrt_beam_channel.h"
#include "hrt_sparse_channel.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    hrt_ktgrid g;                   /* L .. dt (csrc/hrt_pathsum.h), as csrc/hrt_taps_gemm.inc reads it: rows = br * bt * T */
    double fa_c;                    /* f_a / c: revolutions per metre of path difference */
    uint32_t links;                 /* num_rx * num_tx (grid z: at most HRT_SP_MAX_LINKS) */
    uint32_t max_paths;             /* slots per link */
    uint32_t nr, nt, br, bt, npairs;   /* elements, beams; npairs = br * bt (csrc/hrt_beam_gains.inc reads nr, nt, bt) */
    uint32_t accumulate;            /* add into out */
    const float *rx_el, *tx_el;     /* device [nr][3], [nt][3] element offsets (m) */
    const float *rx_w, *tx_w;       /* device [br][nr][2], [bt][nt][2] weights (re, im) */
    const uint8_t *paths;           /* header u64 [links][2], then 72-byte slots [links][max_paths]; 8-byte aligned */
    float *out;                     /* complex [links][br][bt][2][T][L] */
} hrt_ksparse_beam_taps;

int hrt_hip_launch_sparse_beam_taps(const hrt_ksparse_beam_taps *P, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_SPARSE_BEAM_TAPS_H */
