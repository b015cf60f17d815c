/* records_streams_stub.c -- the launch sequence of a trace (csrc/host/problem.c: trace_impl) against a RECORDING stub of
 * the hrt_hip_* layer: no GPU, no HIP.  Built by tests/test_records_streams_design.py together with problem.c, tune.c
 * and accel.c (-ffunction-sections / --gc-sections: only the shim functions the trace path reaches are defined here).
 *
 *     records_streams_stub <num_bounces> <triangles> <patch masks 0|1> <timer 0|1> <traces>
 *
 * makes a problem by hand (no scene, nothing on a device), traces it `traces` times on the caller's stream "main" and
 * prints one line per shim call.  Streams are named aux0, aux1, ... and ordering-only events ev0, ev1, ... in the
 * order of their creation; the events of a timer tev0, ...  HRT_TUNE and HRT_OVERLAP are read as in the library. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hrt_internal.h"
#include "hrt_launch_plan.h"

int hrt_hip_stream_create_prio(void **stream, int lowest);

#define MAIN_STREAM ((void *)(uintptr_t)0x10)
enum { AUX = 0x100, EV = 0x1000, TEV = 0x2000 };
static unsigned n_aux, n_ev, n_tev;

static const char *name(const void *h)
{
    static char buf[4][32];
    static int k;
    const uintptr_t v = (uintptr_t)h;
    char *b = buf[k++ & 3];
    if (h == MAIN_STREAM) return "main";
    if (v >= TEV) snprintf(b, 32, "tev%u", (unsigned)(v - TEV));
    else if (v >= EV) snprintf(b, 32, "ev%u", (unsigned)(v - EV));
    else if (v >= AUX) snprintf(b, 32, "aux%u", (unsigned)(v - AUX));
    else snprintf(b, 32, "?%lu", (unsigned long)v);
    return b;
}

const char *hrt_hip_error_string(int err) { (void)err; return "stub"; }
int hrt_hip_set_device(int dev) { printf("set_device %d\n", dev); return 0; }
int hrt_hip_free(void *p) { printf("free\n"); free(p); return 0; }
int hrt_hip_host_free(void *p) { printf("host_free\n"); free(p); return 0; }
int hrt_hip_memset_async(void *dst, int value, uint64_t bytes, void *stream)
{
    (void)dst; (void)bytes;
    printf("memset %d on %s\n", value, name(stream));
    return 0;
}
int hrt_hip_stream_create(void **stream)
{
    *stream = (void *)(uintptr_t)(AUX + n_aux++);
    printf("stream_create default -> %s\n", name(*stream));
    return 0;
}
int hrt_hip_stream_create_prio(void **stream, int lowest)
{
    *stream = (void *)(uintptr_t)(AUX + n_aux++);
    printf("stream_create %s -> %s\n", lowest ? "lowest" : "default", name(*stream));
    return 0;
}
int hrt_hip_stream_destroy(void *stream) { printf("stream_destroy %s\n", name(stream)); return 0; }
int hrt_hip_event_create_sync(void **ev)
{
    *ev = (void *)(uintptr_t)(EV + n_ev++);
    printf("event_create_sync -> %s\n", name(*ev));
    return 0;
}
int hrt_hip_event_create(void **ev)
{
    *ev = (void *)(uintptr_t)(TEV + n_tev++);
    printf("event_create -> %s\n", name(*ev));
    return 0;
}
int hrt_hip_event_destroy(void *ev) { printf("event_destroy %s\n", name(ev)); return 0; }
int hrt_hip_event_record(void *ev, void *stream) { printf("record %s on %s\n", name(ev), name(stream)); return 0; }
int hrt_hip_stream_wait_event(void *stream, void *ev) { printf("wait %s on %s\n", name(ev), name(stream)); return 0; }
uint64_t hrt_hip_sort_temp_bytes(uint64_t cap) { return cap; }
int hrt_hip_sort_hits(const hrt_kparams *P, uint32_t bounce, void *stream)
{
    (void)P;
    printf("sort b=%u on %s\n", bounce, name(stream));
    return 0;
}
int hrt_hip_launch_los(const hrt_kparams *P, void *stream) { (void)P; printf("los on %s\n", name(stream)); return 0; }

/* the four launch shims answer as the real ones do: from the launch plan */
int hrt_hip_launch_trace(const hrt_kparams *P, uint32_t bounce, void *stream)
{
    const hrt_launch_plan pl = hrt_plan(P);
    if (hrt_plan_own_records(&pl, bounce) && bounce >= P->num_bounces) return 0;   /* the last launch: records only */
    printf("%s b=%u on %s\n", hrt_plan_own_records(&pl, bounce) && hrt_plan_image(&pl, bounce) ? "image" : "trace", bounce, name(stream));
    return 0;
}
int hrt_hip_launch_shade(const hrt_kparams *P, uint32_t bounce, void *stream)
{
    const hrt_launch_plan pl = hrt_plan(P);
    if (hrt_plan_own_records(&pl, bounce) && bounce >= P->num_bounces) return 0;
    printf("shade b=%u on %s\n", bounce, name(stream));
    return 0;
}
int hrt_hip_launch_fused(const hrt_kparams *P, uint32_t bounce, void *stream)
{
    const hrt_launch_plan pl = hrt_plan(P);
    if (!hrt_plan_fuses(&pl, bounce)) return -1;
    printf("fused b=%u on %s\n", bounce, name(stream));
    return 0;
}
int hrt_hip_launch_records(const hrt_kparams *P, uint32_t bounce, void *stream)
{
    const hrt_launch_plan pl = hrt_plan(P);
    if (!hrt_plan_own_records(&pl, bounce)) return -1;
    printf("records b=%u on %s\n", bounce, name(stream));
    return 0;
}
int hrt_hip_launch_chain(const hrt_kparams *P, uint32_t b0, void *stream)
{
    const hrt_launch_plan pl = hrt_plan(P);
    if (!hrt_plan_chains(&pl, b0, P->num_bounces)) return -1;
    printf("chain b0=%u on %s\n", b0, name(stream));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 6) { fprintf(stderr, "usage: %s num_bounces triangles masks timer traces\n", argv[0]); return 2; }
    const uint32_t nb = (uint32_t)atoi(argv[1]), T = (uint32_t)atoi(argv[2]);
    const int masks = atoi(argv[3]), timed = atoi(argv[4]), traces = atoi(argv[5]);
    static const unsigned long long mask_words[1] = {0u};
    hrt_problem *p = (hrt_problem *)calloc(1, sizeof *p);
    if (!p) return 3;
    if (hrt_tune_load(&p->tune)) { fprintf(stderr, "%s\n", hrt_last_error()); free(p); return 4; }
    p->num_tri = T; p->num_mesh = 1; p->num_rx = 2; p->num_tx = 1;
    p->f_ghz = 1.f; p->fsl_mult = 1.f; p->dop_mult = 1.f;
    p->d_blob = malloc(16);   /* (what hrt_problem_destroy hands to hrt_hip_free) */
    if (masks) p->kpatch.mask = mask_words;
    const hrt_shard s = {1000u, 0u, 1u, 0u, nb};
    int rc = 0;
    for (int t = 0; t < traces && !rc; ++t) {
        hrt_timer *tm = NULL;
        printf("-- trace %d\n", t);
        if (timed) rc = hrt_timer_create(nb, &tm);
        /* (nothing dereferences the directions or the workspace: every shim is a stub) */
        if (!rc) rc = hrt_trace_flags(p, &s, (const float *)(uintptr_t)0x1000, NULL, (void *)(uintptr_t)0x10000, UINT64_MAX, MAIN_STREAM, tm, 0u);
        hrt_timer_destroy(tm);
    }
    if (rc) fprintf(stderr, "rc %d: %s\n", rc, hrt_last_error());
    printf("-- destroy\n");
    hrt_problem_destroy(p);
    return rc ? 1 : 0;
}
