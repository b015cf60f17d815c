/* hrt_sparse_channel.h -- internal contract between csrc/host/channel.c (hrt_sparse_array_channel) and the kernel that
 * forms an array channel from dominant-path lists (csrc/hrt_sparse_channel.hip).  Plain C; passed to the kernel by value.
 *
 * The input is a buffer of hrt_dominant_paths' layout (include/hermespy_rt.h): a header uint64_t [L][2] = {kept,
 * eligible}, then hrt_dominant_path [L][K].  Per link and polarisation the channel of the list is the complex GEMM of
 * csrc/hrt_array_channel.h over the link's first n = min(kept, K) slots p:
 *     H_pol[a, c] = sum_{p < n} S[a, p] W_pol[p, c],   a = i * Nt + j (element pair),  c = (m, k) (time, frequency)
 * with the tiles of that header: a workgroup (4 waves) forms HRT_AC_PAIRS pairs x HRT_AC_GROWS * 16 padded columns of
 * one link from ALL of the link's slots, walked in index order HRT_AC_BATCH at a time, and writes its accumulators
 * straight to out.  One chunk per link: no partial sums, no reduce kernel, no segments, no workspace view, no scratch.
 * The twelve floats of a slot from a_te_re on are the HRT_PS_REC_FLOATS floats of stage_record (csrc/hrt_pathsum.h) in
 * its order; power, path, bounce and tri are not read, and neither is any slot at or beyond n. */
#ifndef HRT_SPARSE_CHANNEL_H
#define HRT_SPARSE_CHANNEL_H

#include <stddef.h>
#include <stdint.h>

#include "hrt_array_channel.h"
#include "hrt_dominant.h"
#include "hrt_pathsum.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HRT_SP_SLOT_BYTES 72u         /* sizeof(hrt_dominant_path) */
#define HRT_SP_SLOT_FIRST 24u         /* offsetof(hrt_dominant_path, a_te_re): the staged floats start here */
#define HRT_SP_MAX_LINKS 65535u       /* num_rx * num_tx (grid y) */

typedef struct {
    hrt_kgrid g;                    /* K .. fa_c (csrc/hrt_pathsum.h), as csrc/hrt_pair_gemm.inc reads it */
    uint32_t links;                 /* num_rx * num_tx */
    uint32_t max_paths;             /* slots per link */
    uint32_t nr, nt, npairs;        /* elements; npairs = nr * nt */
    uint32_t accumulate;            /* add into out */
    const float *rx_el, *tx_el;     /* device [nr][3], [nt][3] element offsets (m) */
    const uint8_t *paths;           /* header u64 [links][2], then 72-byte slots [links][max_paths]; 8-byte aligned */
    float *out;                     /* complex [links][nr][nt][2][T][K] */
} hrt_ksparse;

int hrt_hip_launch_sparse_channel(const hrt_ksparse *P, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_SPARSE_CHANNEL_H */
