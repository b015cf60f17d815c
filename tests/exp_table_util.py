"""Shared by tests/test_exp_table_design.py and tests/test_gpu_exp_table.py: the inputs that walk the 2^(i/32) table of
expf (csrc/hrt_libm.h: hrt_exp2_tab, which the device reads from a copy in LDS) and a HOST build of that header to hold
the device against -- expf itself, the table index an input reaches, and scatter_pattern (csrc/hrt_kernels.hip)
restated on the header's functions."""
import ctypes as C
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: k of x = -(k + 1/2) ln2 / 32: 18 times round the table (e^-12.5: beyond the tracer's exponents, [-4 pi, 0])
K_MAX = 32 * 18

_SRC = r"""
#include "hrt_libm.h"
void probe_expf(const float *x, float *y, long n) { for (long i = 0; i < n; ++i) y[i] = hrt_expf(x[i]); }
void probe_index(const float *x, unsigned *k, long n)
{
    for (long i = 0; i < n; ++i) { uint64_t ki; (void)hrt_expf_reduce(x[i], &ki); k[i] = (unsigned)(ki & 31u); }
}
/* csrc/hrt_kernels.hip: scatter_pattern, operation for operation */
void probe_scatter(const float *in, float *out, long n)
{
    for (long i = 0; i < n; ++i) {
        const float s = in[4 * i], alpha = in[4 * i + 1], th_s = in[4 * i + 2], th_i = in[4 * i + 3];
        const float dth = fabsf(th_s - th_i);
        const float f = s * hrt_expf(-alpha * dth);
        const float cs = hrt_cosf_nb(th_s);
        float si, ci;
        hrt_sincosf(th_i, &si, &ci);
        const float rough = 1.0f / (1.0f + alpha);
        const float spec = rough * cs;
        const float diff = (1.0f - rough) * cs;
        float te = f * (spec + diff);
        float tm = f * (spec * ci + diff);
        const float ph = alpha * si * 0.1f;
        const float sp = hrt_sinf(ph);
        float tei = te * sp;
        float tmi = tm * sp;
        const float nrm = sqrtf(te * te + tei * tei + tm * tm + tmi * tmi);
        if (nrm > 1e-6f) { te /= nrm; tei /= nrm; tm /= nrm; tmi /= nrm; }
        out[4 * i] = te; out[4 * i + 1] = tei; out[4 * i + 2] = tm; out[4 * i + 3] = tmi;
    }
}
"""


def table_inputs():
    """x = -(k + 1/2) ln2 / 32 for k = 0 .. K_MAX, as floats: each lies half a table step below -k ln2 / 32."""
    k = np.arange(K_MAX + 1, dtype=np.float64)
    return (-(k + 0.5) * np.log(2.0) / 32.0).astype(np.float32)


def edge_inputs():
    """0 and -4 pi (the ends of the tracer's exponents) with their float neighbours."""
    out = []
    for c in (np.float32(0.0), np.float32(-4.0 * np.pi)):
        out += [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    out.append(np.float32(-0.0))
    return np.array(out, np.float32)


def host_build(tmp):
    """The header compiled for the host (the flags of oracle/Makefile's libm_probe) as a ctypes library."""
    src, so = os.path.join(str(tmp), "exp_probe.c"), os.path.join(str(tmp), "libexp_probe.so")
    with open(src, "w") as f:
        f.write(_SRC)
    subprocess.check_call(["cc", "-O2", "-mfma", "-ffp-contract=off", "-Wall", "-shared", "-fPIC",
                           "-I", os.path.join(REPO, "hermespy-rt_amd", "csrc"), src, "-o", so, "-lm"])
    return C.CDLL(so)


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def host_expf(H, x):
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    H.probe_expf(_f32p(x), _f32p(y), C.c_long(x.size))
    return y


def host_index(H, x):
    x = np.ascontiguousarray(x, np.float32)
    k = np.empty(x.size, np.uint32)
    H.probe_index(_f32p(x), k.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_long(x.size))
    return k


def host_scatter(H, items):
    items = np.ascontiguousarray(items, np.float32).reshape(-1, 4)
    out = np.empty_like(items)
    H.probe_scatter(_f32p(items), _f32p(out), C.c_long(items.shape[0]))
    return out


def scatter_items(x):
    """(s, alpha, th_s, th_i) whose exponent -alpha |th_s - th_i| is EXACTLY x (x <= 0): alpha 1, th_i 0, th_s -x;
    and the same x through alpha 2 and 4 (values of the materials) wherever x / alpha is exact in float."""
    x = np.ascontiguousarray(x, np.float32)
    rows = [np.stack([np.full_like(x, 0.5), np.ones_like(x), -x, np.zeros_like(x)], axis=1)]
    big = x[np.abs(x) > 1e-30]   # (division by a power of two is exact but for the denormals)
    for alpha in (2.0, 4.0):
        rows.append(np.stack([np.full_like(big, 0.3), np.full_like(big, alpha), -big / np.float32(alpha), np.zeros_like(big)], axis=1))
    return np.concatenate(rows).astype(np.float32)
