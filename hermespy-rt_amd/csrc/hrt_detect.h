/* hrt_detect.h -- internal contract between csrc/host/channel.c (hrt_channel_detect) and the maximum-likelihood
 * detection kernel (csrc/hrt_detect.hip).  Plain C; passed to the kernel by value.
 *
 *     d_q = |y - H s(q)|^2 over the Q = M^Nt hypotheses q, stream j sending the symbol x_j = (q >> (j B)) & (M - 1);
 *     q* = argmin_q d_q, the lowest q on a tie;   llr[j][b] = (min_{bit 0} d_q - min_{bit 1} d_q) / N0
 *     one point per (rx, tx, pol, m, k)
 *
 * Form.  A lane owns one hypothesis.  g = hrt_detect_form(Nt, B) = min(64, Q) lanes make the group of a point:
 *   narrow (Q < 64)   a wave holds 64 / g points, lane l owns hypothesis q = l % g of point l / g; groups beyond the
 *                     last point repeat it and store nothing;
 *   wide (Q >= 64)    a wave owns one point and walks Q / 64 tiles, lane l owns q = 64 tile + l: the low six bits of q
 *                     are the lane's and never change, the bits above are the tile's and the same for the whole wave.
 * A workgroup of HRT_DT_THREADS threads is HRT_DT_WAVES waves, each with points of its own.  The bit (j, b) of a
 * hypothesis is bit j B + (B - 1 - b) of q (hrt_detect_bit): positions below 6 are lane bits, positions from 6 on
 * tile bits.  A lane keeps its running minimum over its tiles (ascending q, a strict <, so the lowest q of equal
 * distances stays) and, for every tile bit, the minimum of its distances with that bit 0 and with that bit 1: at most
 * 1 + 2 * 6 registers.  The end is a compare-and-move butterfly over the group: (d, q) for the hard decision, the lower
 * q on equal d; for a lane bit p the lanes' minima over every offset but 2^p, then one exchange across 2^p; for a tile
 * bit its two minima over all offsets.  Minima do not depend on their order, so neither do the bytes.
 * The only LDS image is the constellation's: float2 slot x holds S[x] (words 2 x re, 2 x + 1 im), M slots,
 * hrt_detect_lds_bytes(B) = 8 M <= 2048 bytes, staged once by the workgroup (thread w writes slot w, w + 256, ..).  A
 * table of the products H_ij S[x] would be Nr Nt M float2 PER POINT (up to 128 KiB at 64 x 1, B = 8) and shared by no
 * other wave; the kernel multiplies per hypothesis instead, H_ij and y_i being the same address for the whole group
 * (wide: scalar loads).
 *
 * Arithmetic, all float, no contraction: hermespy_rt.h hrt_detect_spec, statement by statement. */
#ifndef HRT_DETECT_H
#define HRT_DETECT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HRT_DT_THREADS 256u           /* 4 waves per workgroup */
#define HRT_DT_WAVES 4u
#define HRT_DT_MAX_NR 64u
#define HRT_DT_MAX_B 8u               /* bits per symbol */
#define HRT_DT_MAX_BITS 12u           /* Nt B: Q <= 4096, Nt <= 12 */
#define HRT_DT_MAX_M 256u             /* constellation points */
#define HRT_DT_LANE_BITS 6u           /* bit positions of q that are the lane's */

/* lanes per point, g = min(64, Q) (0: outside the limits); a wave holds 64 / g points and walks Q / g tiles */
static inline uint32_t hrt_detect_form(uint32_t nt, uint32_t b)
{
    if (nt < 1u || b < 1u || b > HRT_DT_MAX_B || nt > HRT_DT_MAX_BITS || nt * b > HRT_DT_MAX_BITS) return 0u;
    return nt * b >= HRT_DT_LANE_BITS ? 64u : 1u << (nt * b);
}

/* tiles a group walks: Q / g */
static inline uint32_t hrt_detect_tiles(uint32_t nt, uint32_t b)
{
    const uint32_t g = hrt_detect_form(nt, b);
    return g ? (1u << (nt * b)) / g : 0u;
}

/* the position in q of bit b (0: the label's most significant) of stream j */
static inline uint32_t hrt_detect_bit(uint32_t bits, uint32_t j, uint32_t b)
{
    return j * bits + (bits - 1u - b);
}

/* the constellation's LDS image: bytes, and the float2 slot of symbol x */
static inline uint32_t hrt_detect_lds_bytes(uint32_t bits)
{
    return bits >= 1u && bits <= HRT_DT_MAX_B ? 8u << bits : 0u;
}

static inline uint32_t hrt_detect_slot(uint32_t x)
{
    return x;
}

typedef struct {
    uint32_t nr, nt, b;             /* H is Nr x Nt, B bits per symbol */
    uint32_t g;                     /* lanes per point: hrt_detect_form(nt, b) */
    uint32_t tiles;                 /* hrt_detect_tiles(nt, b) */
    uint32_t llr;                   /* 1: HRT_DT_LLR */
    float n0;                       /* the noise power */
    uint32_t pts;                   /* points per link: 2 T K */
    uint32_t points;                /* links * pts, < 2^31 */
    void *out;                      /* the regions of hermespy_rt.h, one behind the other: index, metric and status
                                     * [points] (4 bytes each), llr float [links][Nt][B][pts] (HRT_DT_LLR) */
} hrt_kdetect;

/* H: complex [links][Nr][Nt][pts]; Y: complex [links][Nr][pts]; S: complex [2^b]; none is written */
int hrt_hip_launch_detect(const hrt_kdetect *P, const void *H, const void *Y, const void *S, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_DETECT_H */
