/* hrt_power.h -- internal contract between csrc/host/channel.c (hrt_power_profiles) and the power kernels
 * (csrc/hrt_power.hip).  Plain C; passed to the kernels by value.
 *
 * Per link (rx, tx) and polarisation the power statistics are incoherent sums over the link's terms (the LoS entry
 * and every unblocked scatter record), p = |a^pol|^2 in FP64:
 *   moments   [link][pol][HRT_POWER_FIELDS]   FP64 partial sums per record chunk in the scratch, added in a fixed
 *                                              order by the reduce kernel (csrc/hrt_pathsum.h)
 *   histograms (PDP, arrival and departure spectra) in FIXED POINT: with this call's total P of the (link, pol) and
 *             E the least integer with 2^E >= 2 P, a term adds rint(p 2^(62 - E)) to a u64 bin.  u64 adds commute,
 *             so the bins do not depend on the order of the (LDS or global) atomic adds; the finalize kernel turns
 *             them into doubles, q 2^(E - 62).
 * The scratch: seg (csrc/hrt_pathsum.h), then partial [link][chunk][2][HRT_POWER_FIELDS] doubles, total [link][2]
 * doubles (this call's P), hist [link][2][nbins] u64 (nbins = Ld + 2 Nth Nph: delay bins, then arrival, then
 * departure), each region 256-byte aligned. */
#ifndef HRT_POWER_H
#define HRT_POWER_H

#include <stdint.h>

#include "hrt_pathsum.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HRT_PW_THREADS 256u          /* moments pass: 4 waves per workgroup */
#define HRT_PW_HIST_THREADS 512u     /* histogram pass: 8 waves per workgroup */
#define HRT_PW_LDS_MAX (80u << 10)   /* LDS histograms of one link (both pols) up to this: 2 workgroups per CU */
#define HRT_PW_MAX_DELAY_BINS (1u << 16)
#define HRT_PW_MAX_ANGLE_BINS (1u << 14)    /* Nth * Nph */
#define HRT_PW_MAX_LINK_BINS (1ull << 26)   /* links * (Ld + 2 Nth Nph): 1 GiB of u64 bins */

typedef struct {
    hrt_kview v;
    hrt_kshard sh;                  /* (20 bytes: the fields below follow it directly) */
    uint32_t Ld, Nth, Nph;          /* delay bins; zenith x azimuth bins (0: no spectra) */
    uint32_t nbins;                 /* Ld + 2 Nth Nph */
    double tau0, dtau;
    double *partial;                /* scratch: [link][chunk][2][HRT_POWER_FIELDS] */
    double *total;                  /* scratch: [link][2], this call's P */
    unsigned long long *hist;       /* scratch: [link][2][nbins] */
    double *out;                    /* moments [L][2][F], pdp [L][2][Ld], arrival [L][2][Nth][Nph], departure */
} hrt_kpower;

int hrt_hip_launch_power(const hrt_kpower *P, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_POWER_H */
