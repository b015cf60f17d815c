"""div_c of csrc/hrt_kernels.hip -- the delay of a record's last leg, distance / c, as the rounded product with
1/c corrected once by its exact residual -- equals the IEEE division for EVERY float of [2^-60, 2^40): 838 860 800
distances from far below an atom to far beyond any scene, and 0.  A small C program runs the same three float
operations (no contraction, explicit fused multiply-adds) against `/` over the whole range on the host; the device
side of the same comparison is tests/test_gpu_mask_primitives.py."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#define NT 8
static const float kC = 299792458.0f;
static uint32_t lo, hi;
static unsigned long long bad[NT], seen[NT];
static uint32_t first_bad[NT];
static float div_c(float a)
{
    const float kInvC = 1.0f / kC;
    const float q = a * kInvC;
    const float r = fmaf(-q, kC, a);
    return fmaf(r, kInvC, q);
}
static int differs(float a)
{
    volatile float want = a / kC;
    float got = div_c(a), w = want;
    return memcmp(&got, &w, 4) != 0;
}
static void *work(void *arg)
{
    const int t = (int)(intptr_t)arg;
    const uint64_t n = (uint64_t)hi - lo, a = lo + n * t / NT, b = lo + n * (t + 1) / NT;
    for (uint64_t u = a; u < b; ++u) {
        const uint32_t v = (uint32_t)u;
        float x;
        memcpy(&x, &v, 4);
        if (differs(x)) { if (!bad[t]) first_bad[t] = v; ++bad[t]; }
        ++seen[t];
    }
    return NULL;
}
int main(void)
{
    const float flo = 0x1p-60f, fhi = 0x1p40f;
    memcpy(&lo, &flo, 4);
    memcpy(&hi, &fhi, 4);
    pthread_t th[NT];
    for (int t = 0; t < NT; ++t) pthread_create(&th[t], NULL, work, (void *)(intptr_t)t);
    unsigned long long nb = 0, ns = 0;
    uint32_t fb = 0;
    for (int t = 0; t < NT; ++t) {
        pthread_join(th[t], NULL);
        if (bad[t] && !nb) fb = first_bad[t];
        nb += bad[t];
        ns += seen[t];
    }
    nb += differs(0.0f);
    printf("compared %llu mismatches %llu first 0x%08x\n", ns, nb, fb);
    return 0;
}
'''


def test_three_instruction_division_by_c_is_exact(tmp_path):
    src = tmp_path / "divc.c"
    src.write_text(SRC)
    exe = tmp_path / "divc"
    flags = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-pthread"]
    try:   # a hardware fused multiply-add where the host has one (the C library's fmaf is exact too, and slow)
        if re.search(r"^flags\s*:.*\bfma\b", open("/proc/cpuinfo").read(), re.M):
            flags.append("-mfma")
    except OSError:
        pass
    subprocess.check_call(["gcc"] + flags + [str(src), "-o", str(exe), "-lm"])
    out = subprocess.check_output([str(exe)], text=True)
    m = re.match(r"compared (\d+) mismatches (\d+) first (0x[0-9a-f]+)", out)
    assert m, out
    assert int(m.group(1)) == 100 * 2 ** 23 == 838860800   # every float of the 100 binades
    assert int(m.group(2)) == 0, out


def test_kernels_use_the_checked_sequence():
    """The constants and the three operations of div_c in the kernel source are the ones compared above, and the
    records, shade and fused kernels form the last leg's delay with it."""
    src = open(os.path.join(REPO, "hermespy-rt_amd", "csrc", "hrt_kernels.hip")).read()
    body = open(os.path.join(REPO, "hermespy-rt_amd", "csrc", "hrt_fused_body.inc")).read()
    assert "constexpr float kC = 299792458.0f;" in src and "constexpr float kInvC = 1.0f / kC;" in src
    fn = src[src.index("float div_c(float a)"):]
    fn = fn[:fn.index("}")]
    assert re.sub(r"\s+", " ", fn).endswith(
        "{ const float q = a * kInvC; const float r = __builtin_fmaf(-q, kC, a); return __builtin_fmaf(r, kInvC, q); ")
    assert src.count("div_c(d2rx)") == 2 and body.count("div_c(d2rx)") == 1
    assert "d2rx / kC" not in src and "d2rx / kC" not in body
