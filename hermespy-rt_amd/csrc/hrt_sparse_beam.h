/* hrt_sparse_beam.h -- internal contract between csrc/host/channel.c (hrt_sparse_beam_channel) and the kernel that
 * forms a beamformed channel from dominant-path lists (csrc/hrt_sparse_beam.hip).  Plain C; passed to the kernel by
 * value.
 *
 * The input is a buffer of hrt_dominant_paths' layout (include/hermespy_rt.h): a header uint64_t [L][2] = {kept,
 * eligible}, then hrt_dominant_path [L][K].  Per link and polarisation the beam channel of the list is the complex GEMM
 * of csrc/hrt_beam_channel.h over the link's first n = min(kept, K) slots p:
 *     B_pol[a Bt + b, c] = sum_{p < n} G[a Bt + b, p] W_pol[p, c],   G = g_rx[a](u_rx_p) g_tx[b](u_tx_p),  c = (m, k)
 * with the tiles of csrc/hrt_array_channel.h: a workgroup (4 waves) forms HRT_AC_PAIRS beam pairs x HRT_AC_GROWS * 16
 * padded columns of one link from ALL of the link's slots, walked in index order HRT_AC_BATCH at a time as
 * csrc/hrt_sparse_channel.h walks them, the gains of each batch formed by part 1 of csrc/hrt_beam_gains.inc, and
 * writes its accumulators straight to out.  One chunk per link: no partial sums, no reduce kernel, no LoS kernel, no
 * workspace view, no scratch.  The LoS entry is an ordinary slot; power, path, bounce and tri are not read, and
 * neither is any slot at or beyond n. */
#ifndef HRT_SPARSE_BEAM_H
#define HRT_SPARSE_BEAM_H

#include <stddef.h>
#include <stdint.h>

#include "hrt_beam_channel.h"
#include "hrt_sparse_channel.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    hrt_kgrid g;                    /* K .. fa_c (csrc/hrt_pathsum.h), as csrc/hrt_pair_gemm.inc reads it */
    uint32_t links;                 /* num_rx * num_tx */
    uint32_t max_paths;             /* slots per link */
    uint32_t nr, nt, br, bt, npairs;   /* elements, beams; npairs = br * bt (csrc/hrt_beam_gains.inc reads nr, nt, bt) */
    uint32_t accumulate;            /* add into out */
    const float *rx_el, *tx_el;     /* device [nr][3], [nt][3] element offsets (m) */
    const float *rx_w, *tx_w;       /* device [br][nr][2], [bt][nt][2] weights (re, im) */
    const uint8_t *paths;           /* header u64 [links][2], then 72-byte slots [links][max_paths]; 8-byte aligned */
    float *out;                     /* complex [links][br][bt][2][T][K] */
} hrt_ksparse_beam;

int hrt_hip_launch_sparse_beam(const hrt_ksparse_beam *P, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_SPARSE_BEAM_H */
