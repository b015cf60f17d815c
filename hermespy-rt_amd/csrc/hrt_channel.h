/* hrt_channel.h -- internal contract between csrc/host/channel.c and the channel kernels
 * (csrc/hrt_channel.hip).  Plain C; passed to the kernels by value.
 *
 * The channel of one (rx, tx) is formed as a complex GEMM (two-level DFT):
 * with K padded to K1 * HRT_CH_K2 and k = k1 * HRT_CH_K2 + k2,
 *     H[(m, k1), k2] = sum_p U[(m, k1), p] V[p, k2]
 *     U = a_p exp(j 2 pi (nu_p t_m - (f0 + k1 K2 df) tau_p)),   V = exp(-j 2 pi k2 df tau_p).
 * Rows (m, k1) are cut into tiles of HRT_CH_ROWS; one workgroup (one wave) forms one tile of one
 * link from a chunk of that link's records and writes it to the partial sums of the scratch; the
 * reduce kernel adds the chunks in a fixed order (csrc/hrt_pathsum.h). */
#ifndef HRT_CHANNEL_H
#define HRT_CHANNEL_H

#include <stdint.h>

#include "hrt_pathsum.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HRT_CH_K2 16u        /* columns of a tile: the inner DFT length */
#define HRT_CH_ROWS 64u      /* rows (m, k1) of a tile */
#define HRT_CH_BATCH 16u     /* records staged in LDS at a time */
#define HRT_CH_THREADS 64u   /* one wave per workgroup: 16 x 4 threads of 4 x 4 outputs */
#define HRT_CH_TILE_FLOATS (HRT_CH_ROWS * HRT_CH_K2 * 4u)   /* te re, te im, tm re, tm im */

typedef struct {
    hrt_kview v;                    /* nchunks: record chunks per (link, tile) */
    uint32_t K, T, K1, rows, tiles; /* rows = T * K1, tiles = ceil(rows / HRT_CH_ROWS) */
    double f0, df, t0, dt;
    float *partial;                 /* scratch: [link][chunk][tile][HRT_CH_TILE_FLOATS] */
    float *out;                     /* complex [nrx][ntx][2][T][K] */
} hrt_kchannel;

int hrt_hip_launch_channel(const hrt_kchannel *P, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_CHANNEL_H */
