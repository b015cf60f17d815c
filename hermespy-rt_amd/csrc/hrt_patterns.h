/* hrt_patterns.h -- internal contract between csrc/host/channel.c (hrt_apply_patterns) and the pattern kernels
 * (csrc/hrt_patterns.hip).  Plain C; passed to the kernels by value.
 *
 * The amplitudes of every unblocked scatter record p of link (rx, tx), and of every clear LoS entry, are multiplied in
 * place by the real weight
 *     w_p = fl32( F_rx(R_rx[rx] u_p^rx) F_tx(R_tx[tx] u_p^tx) )
 * u_p^rx the record's HRT_REC_DIR, u_p^tx the launch direction of its ray's global path (LoS: HRT_LOS_DIR and its
 * negative), R the row-major world -> local rotation of the endpoint (NULL: identity), F the pattern of the side in
 * the local frame (boresight +x, zenith from +z, azimuth atan2(y, x)): include/hrt_device.h, hrt_pattern.  Index 0 of
 * the arrays below is the RX side, 1 the TX side. */
#ifndef HRT_PATTERNS_H
#define HRT_PATTERNS_H

#include <stddef.h>
#include <stdint.h>

#include "hrt_pathsum.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HRT_PT_THREADS 256u          /* hits per workgroup */
#define HRT_PT_MAX_ZENITH 181u       /* table nodes: 2 .. 181 zenith, 1 .. 360 azimuth */
#define HRT_PT_MAX_AZIMUTH 360u
#define HRT_PT_MAX_GAIN_DB 200.0f

typedef struct {
    hrt_kview v;                    /* (ws is written: the amplitude fields and HRT_LOS_A) */
    hrt_kshard sh;                  /* (20 bytes: the fields below follow it directly) */
    uint32_t kind[2];               /* HRT_PATTERN_* */
    uint32_t nz[2], na[2];          /* table nodes (HRT_PATTERN_TABLE) */
    float g[2];                     /* 10^(gain_db / 20) */
    uint32_t pad;
    const float *table[2];          /* device [nz][na] (HRT_PATTERN_TABLE) */
    const float *rot[2];            /* device [nrx][9] / [ntx][9]; NULL: identity */
} hrt_kpatterns;

_Static_assert(offsetof(hrt_kpatterns, sh) == 112 && offsetof(hrt_kpatterns, kind) == 132 &&
               offsetof(hrt_kpatterns, nz) == 140 && offsetof(hrt_kpatterns, na) == 148 &&
               offsetof(hrt_kpatterns, g) == 156 && offsetof(hrt_kpatterns, table) == 168 &&
               offsetof(hrt_kpatterns, rot) == 184 && sizeof(hrt_kpatterns) == 200,
               "hrt_kpatterns: the argument offsets");

int hrt_hip_launch_patterns(const hrt_kpatterns *P, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_PATTERNS_H */
