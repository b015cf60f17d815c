/* hrt_launch_plan.h -- which kernel runs for a launch of the tracer, which walk it is built for and how large its
 * LDS image is: ONE pure function of an hrt_kparams ("the launch plan", holds the decision table).
 * Plain C (C99 and C++): the launch shims (hrt_kernels.hip) launch what it says, the host (csrc/host/problem.c)
 * asks it what will run instead of trying a launch, and the tests build it for the host. */
#ifndef HRT_LAUNCH_PLAN_H
#define HRT_LAUNCH_PLAN_H

#include "hrt_kparams.h"
#include "hrt_libm.h"   /* HRT_EXP2_TAB_BYTES */

/* the sizes behind the LDS images; hrt_kernels.hip names them kMaskRounds, kCandBuf, ... from these */
#define HRT_MASK_ROUNDS 16u               /* culling rounds of 64 rows per block of the walks: one block = 1024 rows */
#define HRT_CAND_BUF 64u                  /* candidate rows parked per wave by the fine walk (4 float4 each) */
#define HRT_WAVE_SCRATCH4(cand_buf) (2u * HRT_MASK_ROUNDS + ((cand_buf) ? 4u * HRT_CAND_BUF : 0u))   /* float4 per wave */
#define HRT_LDS_TX 64u                    /* TX positions in the image of a fused launch 0 */
#define HRT_SHADE_LDS_TRI 2048u           /* the shade kernel keeps the normals in LDS up to this many triangles ... */
#define HRT_SHADE_LDS_MESH 256u           /* ... and meshes */
#define HRT_LDS_TABLE_CEIL (144u * 1024u) /* a staged table (rows + guard pairs + leaf records) is at most this */
#define HRT_PLAN_WAVES (HRT_BLOCK / 64u)
/* what follows the named terms in an image: the trace kernel's 4 counters, the fused kernels' 64, the shade
 * kernel's 8 words, the image kernel's 4 */
#define HRT_LDS_TAIL_TRACE 16u
#define HRT_LDS_TAIL_FUSED 256u
#define HRT_LDS_TAIL_SHADE 32u
#define HRT_LDS_TAIL_IMAGE 16u
/* launch 0 on patch tables (hrt_fused_kernel<..., TXCELL>): seven workgroups of it share a CU's 160 KiB, and the two
 * word tables ride in its image only while it stays within a seventh */
#define HRT_LDS_CU (160u * 1024u)
#define HRT_FUSED0_PER_CU 7u
#define HRT_LDS_FUSED0_MAX (HRT_LDS_CU / HRT_FUSED0_PER_CU)
/* the primary rays of launches >= 2 on patch tables (hrt_trace_kernel<true, 2, PATCH>): eight workgroups per CU */
#define HRT_TRACE_PATCH_PER_CU 8u
#define HRT_LDS_TRACE_PATCH_MAX (HRT_LDS_CU / HRT_TRACE_PATCH_PER_CU)

typedef struct {
    /* table facts */
    uint64_t tri_bytes;   /* the staged image: rows + guard pairs (padded to 16 B) + leaf records */
    uint8_t in_lds;       /* the table is staged in LDS */
    uint8_t one_block;    /* at most one block of HRT_MASK_ROUNDS * 64 rows */
    uint8_t trees;        /* the big-table trees are walked */
    uint8_t fine;         /* the fine leaves are walked (off LDS, no trees) */
    /* walks: a kernel runs as its instantiation <TRI_IN_LDS = in_lds, VARIANT = ...> */
    uint8_t trace_v;      /* hrt_trace_kernel */
    uint8_t fused_v;      /* hrt_fused_kernel (under `fine` no fused kernel runs: the trace kernel's) */
    int8_t chain_v;       /* hrt_chain_kernel; -1: no chain on this table / walk (off LDS, more than one block, trees) */
    /* launches */
    uint8_t own_records;  /* launches >= 1: shadow traces + records are hrt_records_kernel's */
    uint8_t image;        /* ... and the primary rays of launch 1 hrt_image_kernel's */
    uint8_t shade_lds_normals;    /* hrt_shade_kernel<true> */
    uint32_t cnt_per_wave;        /* hrt_kparams.cnt_per_wave of the trace and shade kernels */
    /* the terms of the LDS images, in bytes */
    uint64_t t_rows;      /* the rows alone */
    uint64_t t_table;     /* tri_bytes if staged, else 0 */
    uint64_t t_rx;        /* RX positions */
    uint64_t t_masks;     /* HRT_MASK_ROUNDS mask words per wave */
    uint64_t t_scratch;   /* per-wave scratch, with the candidate buffer under `fine` */
    uint64_t t_mat_exp;   /* materials + expf's table */
    uint64_t t_tx;        /* HRT_LDS_TX TX positions */
    uint64_t t_orig;      /* the records kernel's l_orig: a word per row */
    uint64_t t_normals;   /* the shade kernel's triangle normals + mesh rows, 0 if it reads them from global memory */
    /* the LDS images */
    uint64_t lds_trace, lds_fused, lds_chain, lds_records, lds_image, lds_shade;
    /* launch 0 of a patch-table problem (flat one-block walk on a staged table, a TX cell table, no per-cell masks):
     * its own instantiation of hrt_fused_kernel with an image of what that path reads, lds_fused0; else all 0 */
    uint8_t fused0_txcell;
    uint8_t fused0_words;   /* the image holds the two word tables: reference-order indices and material indices */
    uint64_t t_mat0;        /* the materials without expf's table */
    uint64_t t_tx0;         /* min(num_tx, HRT_LDS_TX) TX positions */
    uint64_t t_words0;      /* one of the two word tables: a word per row, padded to 16 B; 0 if they are out */
    uint64_t lds_fused0;    /* rows + tail + t_mat0 + t_tx0 + 2 t_words0 */
    /* the primary rays of launches >= 2 of a records-kernel problem (hrt_plan_trace_patch): hrt_trace_kernel's own
     * instantiation with an image of what that path reads, lds_trace_patch; else both 0 */
    uint8_t trace_patch;
    uint64_t lds_trace_patch;   /* rows + t_masks + tail: an eighth of a CU holds it up to 249 rows */
} hrt_launch_plan;

static inline hrt_launch_plan hrt_plan(const hrt_kparams *P)
{
    hrt_launch_plan pl;
    const int v = P->tune.variant;
    const uint64_t T = P->num_tri;
    memset(&pl, 0, sizeof pl);
    pl.t_rows = T * HRT_TRI_FLOATS * 4u;
    pl.tri_bytes = pl.t_rows + ((T + 1u) / 2u) * 16u + (uint64_t)P->acc.num_leaf * HRT_NODE_FLOATS * 4u;
    pl.in_lds = pl.t_rows <= P->tune.lds_tri_bytes_max && pl.tri_bytes <= HRT_LDS_TABLE_CEIL;
    pl.one_block = T <= HRT_MASK_ROUNDS * 64u;
    pl.trees = P->acc.big && v >= 4 && v != 9;
    pl.fine = !pl.in_lds && !pl.trees && P->acc.fine != NULL && (v == 7 || v == 9);
    const int flat = v == 2 || v == 3 || (v == 7 && !pl.trees && pl.one_block);
    const int staged = v == 1 || (v == 7 && T <= P->tune.fuse_staged_max_tri);   /* the fused and chain kernels only */
    /* the walk behind `flat` and the tree variants, by where the table is and how large */
    const int w_flat = pl.in_lds && pl.one_block ? 2 : 3;
    const int w_tree = pl.trees ? 6 : (pl.in_lds && pl.one_block ? 4 : 5);   /* (tables beyond LDS are > 1 block) */
    pl.trace_v = (uint8_t)(pl.fine ? 9 : v == 0 ? 0 : v == 1 ? 1 : flat ? w_flat : w_tree);
    pl.fused_v = (uint8_t)(pl.fine ? 9 : v == 0 ? 0 : staged ? 1 : flat ? w_flat : w_tree);
    pl.chain_v = (int8_t)(pl.in_lds && pl.one_block && pl.fused_v != 6 ? pl.fused_v : -1);
    pl.own_records = P->patch.mask != NULL && pl.in_lds && flat && pl.one_block;
    pl.image = pl.own_records && P->patch.num_img != 0u;
    pl.shade_lds_normals = !P->tune.shade_global_normals && T <= HRT_SHADE_LDS_TRI && P->num_mesh <= HRT_SHADE_LDS_MESH;
    pl.cnt_per_wave = pl.fine ? 1u : 0u;

    pl.t_table = pl.in_lds ? pl.tri_bytes : 0u;
    pl.t_rx = (uint64_t)P->num_rx * 16u;
    pl.t_masks = HRT_PLAN_WAVES * HRT_MASK_ROUNDS * 8u;
    pl.t_scratch = HRT_PLAN_WAVES * HRT_WAVE_SCRATCH4(pl.fine) * 16u;
    pl.t_mat_exp = HRT_NUM_MATERIALS * HRT_MAT_FLOATS * 4u + HRT_EXP2_TAB_BYTES;
    pl.t_tx = HRT_LDS_TX * 16u;
    pl.t_orig = T * 4u;
    pl.t_normals = pl.shade_lds_normals ? (T + P->num_mesh) * 16u : 0u;
    pl.lds_trace = pl.t_table + pl.t_rx + pl.t_masks + pl.t_scratch + HRT_LDS_TAIL_TRACE;
    pl.lds_fused = pl.t_table + pl.t_rx + pl.t_masks + pl.t_scratch + HRT_LDS_TAIL_FUSED + pl.t_mat_exp + pl.t_tx;
    pl.lds_chain = pl.lds_fused;   /* (the chain runs on staged tables without the fine walk: the fused image) */
    pl.lds_records = pl.t_rows + pl.t_rx + pl.t_mat_exp + pl.t_orig;
    pl.lds_image = pl.t_rows + HRT_LDS_TAIL_IMAGE;
    pl.lds_shade = pl.t_mat_exp + pl.t_rx + HRT_LDS_TAIL_SHADE + pl.t_normals;

    pl.fused0_txcell = !pl.fine && pl.in_lds && pl.fused_v == 2 && P->patch.txcell != NULL && P->rxt.cell_mask == NULL;
    if (pl.fused0_txcell) {
        const uint64_t words = (pl.t_orig + 15u) / 16u * 16u;
        pl.t_mat0 = HRT_NUM_MATERIALS * HRT_MAT_FLOATS * 4u;
        pl.t_tx0 = (uint64_t)(P->num_tx < HRT_LDS_TX ? P->num_tx : HRT_LDS_TX) * 16u;
        pl.lds_fused0 = pl.t_rows + HRT_LDS_TAIL_FUSED + pl.t_mat0 + pl.t_tx0;
        /* (with the words in, 88 T < HRT_LDS_FUSED0_MAX: such a table has at most 250 rows, a word per thread) */
        pl.fused0_words = pl.lds_fused0 + 2u * words <= HRT_LDS_FUSED0_MAX;
        pl.t_words0 = pl.fused0_words ? words : 0u;
        pl.lds_fused0 += 2u * pl.t_words0;
    }
    pl.trace_patch = pl.own_records && pl.trace_v == 2;   /* (own_records: a staged table, the flat one-block walk) */
    if (pl.trace_patch) pl.lds_trace_patch = pl.t_rows + pl.t_masks + HRT_LDS_TAIL_TRACE;
    return pl;
}

/* launch b: hrt_records_kernel traces the shadow rays and writes the records (never at launch 0) */
static inline int hrt_plan_own_records(const hrt_launch_plan *pl, uint32_t b) { return b != 0u && pl->own_records; }
/* launch b: the primary rays are hrt_image_kernel's (launch 1 of a records-kernel problem with image tables) */
static inline int hrt_plan_image(const hrt_launch_plan *pl, uint32_t b) { return b == 1u && pl->image; }
/* launch b: the primary rays are hrt_trace_kernel<true, 2, PATCH>'s (launches >= 2 of a records-kernel problem; launch 1
 * is the image kernel's, or without image tables the shared instantiation's, as launch 0 is when it does not fuse) */
static inline int hrt_plan_trace_patch(const hrt_launch_plan *pl, uint32_t b) { return b >= 2u && pl->trace_patch; }
/* launch b can run as one fused kernel: launch 0 unless the fine leaves are walked, later launches on a staged
 * table with a one-block walk */
static inline int hrt_plan_fuses(const hrt_launch_plan *pl, uint32_t b)
{
    if (b == 0u) return !pl->fine;
    return pl->in_lds && (pl->fused_v == 0 || pl->fused_v == 1 || pl->fused_v == 2 || pl->fused_v == 4);
}
/* launches b0 .. num_bounces can run as one chain kernel (whether its grid is resident is the shim's to ask) */
static inline int hrt_plan_chains(const hrt_launch_plan *pl, uint32_t b0, uint32_t num_bounces)
{
    return b0 != 0u && b0 <= num_bounces && !pl->own_records && pl->chain_v >= 0;
}

#endif
