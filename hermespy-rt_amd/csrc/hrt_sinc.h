// hrt_sinc.h -- the sinc weights of the sampled impulse responses, for the kernels of the three taps families
// (csrc/hrt_taps_gemm.inc, the reduce helpers of csrc/hrt_pathsum.h, which includes this file).  HIP device code only.
//
// Every delay is reduced in FP64 to x = f_s tau.  With n = rint(x), f = x - n, sinc(l - x) = -(-1)^(l - n) sin(pi f) /
// (pi (l - n - f)): one f32 sinpi per record and, per tap, an exact integer difference, one v_rcp_f32 and a sign.
// Where |l - x| < 1e-4 the weight is 1 (the f32 rounding of sinc there; exactly 1 where l - x is exactly 0).
#ifndef HRT_SINC_H
#define HRT_SINC_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// The sinc of one delay, x = f_s tau: sinc(l - x) = (-1)^l c / ((l - k) - r) with k = rint(x) clamped to
// +-2^26 (so l - k is an exact int32 for |l| <= 2^24), r = x - k and c = -(-1)^n sin(pi (x - n)) / pi, n = rint(x).
// Unclamped, |r| <= 1/2; clamped, r has the sign of k and l - k the other one, so (l - k) - r never vanishes.
struct sinc_rec {
    int32_t k;
    float r, c;
};

__device__ __forceinline__ sinc_rec sinc_prep(double fs, float tau)
{
    const double x = fs * (double)tau;
    const double n = rint(x);
    const double k = fmin(fmax(n, -67108864.0), 67108864.0);
    const double h = 0.5 * n;   // n odd <=> n / 2 has a fraction (exact below 2^53; beyond it x is even, f = 0)
    const float s = sinpif((float)(x - n)) * 0.318309886183790672f;   // sin(pi f) / pi
    sinc_rec q;
    q.k = (int32_t)k;
    q.r = (float)(x - k);
    q.c = h != floor(h) ? s : -s;
    return q;
}

__device__ __forceinline__ float sinc_tap(int32_t l, const sinc_rec &q)
{
    const float d = (float)(l - q.k) - q.r;
    const float c = (l & 1) ? -q.c : q.c;
    return fabsf(d) < 1e-4f ? 1.f : c * __builtin_amdgcn_rcpf(d);
}

}  // namespace

#endif  // HRT_SINC_H
