/* hrt_beam_channel.h -- internal contract between csrc/host/channel.c (hrt_beam_channel) and the beam channel
 * kernels (csrc/hrt_beam_channel.hip).  Plain C; passed to the kernels by value.
 *
 * Per link (rx, tx) and polarisation the beamformed channel is the complex GEMM of csrc/hrt_array_channel.h with
 * beam pairs for rows:
 *     B_pol[a Bt + b, c] = sum_p G[a Bt + b, p] W_pol[p, c],   c = (m, k) (time, frequency)
 *     G = g_rx[a](u_rx) g_tx[b](u_tx),   W_pol = a^pol exp(j 2 pi (nu t_m - f_k tau))
 *     g_rx[a](u) = sum_i conj(W_rx[a, i]) exp(j 2 pi f_a r_i . u / c),   g_tx[b](u) = sum_j W_tx[b, j] exp(j 2 pi f_a q_j . u / c)
 * W is the two-level factorisation of csrc/hrt_channel.h; the A operand of v_mfma_f32_32x32x2_f32 is the 2x2 real
 * embedding (Re G, -Im G; Im G, Re G), which holds for any complex G.  The weights are folded into every record's
 * steering term before the GEMM, so the element-domain matrix is never formed and the cost does not grow with Nr Nt.
 * A workgroup (4 waves) forms HRT_AC_PAIRS beam pairs x 256 padded columns of one link from one chunk of the link's
 * records.  Per batch of staged records it forms the element phase factors HRT_BM_ETILE elements at a time in LDS and
 * accumulates the gains of the beams its pairs touch: the RX beams a0 .. a0 + na - 1 and, of the TX beams, all Bt of
 * them where Bt <= HRT_AC_PAIRS and (p0 + slot) mod Bt otherwise -- at most HRT_AC_PAIRS a side.  Within an element
 * tile the sum is FP32, across the tiles FP64.  The LoS gains of every (link, pair) are formed once by
 * hrt_beam_los_kernel into the scratch (behind the partial sums) and read by the reduce kernel. */
#ifndef HRT_BEAM_CHANNEL_H
#define HRT_BEAM_CHANNEL_H

#include <stddef.h>
#include <stdint.h>

#include "hrt_array_channel.h"
#include "hrt_pathsum.h"

#ifdef __cplusplus
extern "C" {
#endif

/* (the tile of a workgroup is csrc/hrt_array_channel.h's: HRT_AC_THREADS, HRT_AC_PAIRS, HRT_AC_GROWS, HRT_AC_BATCH) */
#define HRT_BM_ETILE 32u      /* elements whose phase factors are in LDS at a time */
#define HRT_BM_MAX_ELEMENTS 256u
#define HRT_BM_MAX_BEAMS 256u
#define HRT_BM_MAX_POINTS (1u << 24)   /* Br * Bt * T * K */

typedef struct {
    hrt_kview v;
    hrt_kshard sh;                  /* (20 bytes: the fields below follow it directly) */
    uint32_t nr, nt, br, bt, npairs;   /* elements, beams; npairs = br * bt */
    hrt_kgrid g;                    /* K .. fa_c (csrc/hrt_pathsum.h) */
    const float *rx_el, *tx_el;     /* device [nr][3], [nt][3] element offsets (m) */
    const float *rx_w, *tx_w;       /* device [br][nr][2], [bt][nt][2] weights (re, im) */
    float *partial;                 /* scratch: complex [link][chunk][pol][pair][T * K] */
    float *los;                     /* scratch: complex [link][pair] gains at the LoS directions */
    float *out;                     /* complex [nrx][ntx][br][bt][2][T][K] */
} hrt_kbeam;

_Static_assert(offsetof(hrt_kbeam, g) == 152 && offsetof(hrt_kbeam, rx_el) == 216, "hrt_kbeam: the argument offsets");

int hrt_hip_launch_beam_channel(const hrt_kbeam *P, void *stream);

#ifdef __cplusplus
}
#endif

#ifdef __HIPCC__
/* what the kernels of the two beam families (csrc/hrt_beam_channel.hip, csrc/hrt_beam_taps.hip) share besides the
 * kernel text of csrc/hrt_beam_gains.inc */
namespace {

// weight e of beam `beam` of a codebook [beams][n][2]; the combiner (RX side) takes the conjugate
__device__ __forceinline__ float2 beam_weight(const float *w, uint32_t n, uint32_t beam, uint32_t e, bool conj)
{
    const float *p = w + ((uint64_t)beam * n + e) * 2u;
    return make_float2(p[0], conj ? -p[1] : p[1]);
}
}  // namespace
#endif /* __HIPCC__ */
#endif /* HRT_BEAM_CHANNEL_H */
