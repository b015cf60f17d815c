/* hrt_dominant.h -- internal contract between csrc/host/channel.c (hrt_dominant_paths) and the selection kernels
 * (csrc/hrt_dominant.hip).  Plain C; passed to the kernels by value.
 *
 * Per link (rx, tx) the K strongest eligible terms (the LoS entry and every unblocked scatter record) in the strict
 * order of include/hermespy_rt.h (hrt_dominant_path): power descending, then bounce, then global path ascending.
 * A term is carried as a candidate of 24 bytes whose 128-bit key orders it (larger first):
 *   hi   the bits of the FP64 power + 1 (monotone for non-negative doubles; 0 marks an empty slot)
 *   lo   ~((bounce + 1) << 48 | path), path < 2^48
 *   ix   where the term's fields are: the hit index of a scatter record of this call's workspace, HRT_DM_IX_LOS for
 *        this call's LoS entry, HRT_DM_IX_OLD | slot for a record the output already holds (accumulate)
 * Within a link the keys of distinct terms are distinct, so the first K of a set do not depend on the order the set
 * is visited in: the partial kernel writes the first K of its record chunk, the merge kernel the first K of up to
 * HRT_DM_FANIN such lists, the final kernel the first K of the remaining lists, the LoS entry and what the output
 * holds, and gathers the winners' 72-byte records.
 * The scratch: seg (csrc/hrt_pathsum.h), then la [link][nchunks][K] candidates, ca [link][nchunks] u64 (unblocked
 * records of the chunk), lb [link][nmid][K] and cb [link][nmid] (nmid = 0: no merge level), each 256-byte aligned. */
#ifndef HRT_DOMINANT_H
#define HRT_DOMINANT_H

#include <stdint.h>

#include "hrt_pathsum.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HRT_DM_MAX_PATHS 1024u         /* K */
#define HRT_DM_MAX_LINK_PATHS (1u << 22)   /* links * K */
#define HRT_DM_THREADS 256u            /* partial and merge kernels: 4 waves per workgroup */
#define HRT_DM_FINAL_THREADS 1024u     /* final kernel: one thread per output slot */
#define HRT_DM_SLOTS 2048u             /* LDS candidates of a workgroup: the K kept so far, then the pending ones */
#define HRT_DM_FANIN 16u               /* lists one merge or final workgroup reads */
#define HRT_DM_MAX_CHUNKS (HRT_DM_FANIN * HRT_DM_FANIN)
#define HRT_DM_IX_LOS 0xFFFFFFFEu
#define HRT_DM_IX_OLD 0x80000000u
#define HRT_DM_PATH_BITS 48u

typedef struct {
    uint64_t hi, lo;
    uint32_t ix, pad;
} hrt_dm_cand;

typedef struct {
    hrt_kview v;
    hrt_kshard sh;                  /* (20 bytes: the fields below follow it directly) */
    uint32_t K;                     /* max_paths */
    uint32_t nmid;                  /* lists per link after the merge level; 0: the final kernel reads la */
    uint32_t pad;
    hrt_dm_cand *la, *lb;           /* scratch: [link][nchunks][K], [link][nmid][K] */
    uint64_t *ca, *cb;              /* scratch: [link][nchunks], [link][nmid] */
    uint8_t *out;                   /* header u64 [L][2], then hrt_dominant_path [L][K] */
} hrt_kdominant;

int hrt_hip_launch_dominant(const hrt_kdominant *D, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_DOMINANT_H */
