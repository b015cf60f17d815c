/* hrt_propagate.h -- internal contract between csrc/host/channel.c (hrt_propagate) and the propagation kernels
 * (csrc/hrt_propagate.hip).  Plain C; passed to the kernels by value.
 *
 *     y[r][n] = sum_p sum_{l < L} h[r][p][m(n)][l] x[p][n - l_min - l],   m(n) = min(n / S, M - 1)
 *     r = (rx, i, pol): R = nrx Nr 2 complex rows;   p = (tx, j): P = ntx Nt TX ports;   x[p][k] = 0 outside 0 <= k < N
 *
 * Per block m the real GEMM Y[2R][cols] = A[2R][2K] B[2K][cols], K = P L, B the Toeplitz operand of x, never
 * materialised.  Two forms; hrt_propagate_form below is the whole rule, read by the host and mirrored in
 * tests/propagate_util.py:
 *   HRT_PG_MFMA     M = 1 or S a multiple of 16, so that a 16-column tile lies in one block.  v_mfma_f32_16x16x4_f32,
 *                   a tile = 16 complex rows x 16 samples, the 4-deep k step = (re, im) of the taps l, l + 1, two
 *                   MFMAs a step (one accumulating Re y with A = (h_re, -h_im), one Im y with A = (h_im, h_re)) on
 *                   one B = (x_re, x_im) of the samples n - l_min - l.  A workgroup (4 waves) forms 16 rows x
 *                   HRT_PG_COLS samples, wave w the HRT_PG_WTILES column tiles from column 64 w: 8 independent
 *                   accumulators a wave.  It walks the ports and, per port, the taps HRT_PG_LC at a time, with the
 *                   window of x those taps need (HRT_PG_COLS + HRT_PG_LC complex samples, re/im interleaved) in LDS.
 *   HRT_PG_GENERAL  any other S: one lane per (row, sample), an fmaf chain over (tx, j, l) in that order.
 * Both walk the whole K in one workgroup: no partial sums, no scratch, no atomics; every y[r][n] is written once. */
#ifndef HRT_PROPAGATE_H
#define HRT_PROPAGATE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HRT_PG_THREADS 256u       /* 4 waves per workgroup */
#define HRT_PG_WTILES 4u          /* column tiles (16 samples) per wave */
#define HRT_PG_COLS 256u          /* samples per workgroup: 4 waves x HRT_PG_WTILES x 16 */
#define HRT_PG_LC 256u            /* taps per staged window (even: a k step never straddles two windows) */
#define HRT_PG_WINDOW (HRT_PG_COLS + HRT_PG_LC)   /* complex samples of the LDS window */
#define HRT_PG_MAX_ELEMENTS 1024u /* nr, nt */
#define HRT_PG_MAX_POINTS (1u << 24)              /* nr * nt * num_times * num_taps */
#define HRT_PG_MAX_TAP (1 << 24)                  /* |l_min|, |l_min + num_taps| */
#define HRT_PG_MAX_SAMPLES (1ull << 31)           /* num_samples, num_out */

#define HRT_PG_MFMA 0u
#define HRT_PG_GENERAL 1u

/* the form of a call: a pure function of the spec */
static inline uint32_t hrt_propagate_form(uint32_t num_times, uint32_t samples_per_block)
{
    return (num_times == 1u || samples_per_block % 16u == 0u) ? HRT_PG_MFMA : HRT_PG_GENERAL;
}

typedef struct {
    uint32_t R, P;                  /* complex rows nrx Nr 2, TX ports ntx Nt */
    uint32_t ntx, nr, nt;           /* the factors the index of h needs */
    uint32_t M, L, S;               /* blocks, taps, samples per block */
    int32_t l_min;
    uint32_t accumulate;
    uint64_t N, N_out;              /* samples of x per port, samples of y per row */
    const float *h;                 /* complex [nrx][ntx][Nr][Nt][2][M][L] */
    const float *x;                 /* complex [P][N] */
    float *out;                     /* complex [R][N_out] */
} hrt_kpropagate;

int hrt_hip_launch_propagate(const hrt_kpropagate *P, uint32_t form, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_PROPAGATE_H */
