// hrt_patterns.hip -- antenna radiation patterns and orientations applied to the workspace of a finished hrt_trace,
// in place, for gfx950 (csrc/hrt_patterns.h, include/hrt_device.h: hrt_apply_patterns).  The four amplitude fields of
// every unblocked scatter record of link (rx, tx), and HRT_LOS_A of every clear LoS entry, are multiplied by
//
//     w = fl32( F_rx(R_rx[rx] u^rx) F_tx(R_tx[tx] u^tx) )
//
// so that every path-sum family (csrc/hrt_pathsum.h), which reads an amplitude only through the workspace view, sees
// the weighted path.  Nothing else of the workspace is written, and nothing is read that a trace does not write: the
// direction fields of a blocked record, the slots from a block's count up to cap, blocked and coincident LoS entries.
//   hrt_patterns_records_kernel  one thread per hit (b, i), i < counts[b + 1] (read here: no host synchronisation).
//                                The TX weight once per hit (the launch direction of the ray's global path; the TX
//                                index is HRT_HIT_RAY / num_local), then per receiver the mask bit, the three
//                                direction floats, the RX weight and four loads and stores of coalesced field runs.
//   hrt_patterns_los_kernel      one thread per link: u^tx = HRT_LOS_DIR, u^rx = -u^tx.
// No atomics: a slot is written by one thread, and two runs on equal inputs give equal bits.  The evaluation sequence
// below is float32 without contraction (-ffp-contract=off); tests/patterns_util.py emulates it step by step.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_patterns.h"
#include "hrt_pathsum.h"

static_assert(HRT_PT_THREADS == 256u, "the grid of hrt_hip_launch_patterns");

namespace {

constexpr float PT_PI = 3.14159265358979323846f;
constexpr float PT_HALF_PI = 1.57079632679489661923f;
constexpr float PT_INV_PI = 0.318309886183790671538f;
constexpr float PT_INV_2PI = 0.159154943091895335769f;
constexpr float PT_DEG = 57.2957795130823208768f;         // 180 / pi
constexpr float PT_DIPOLE = 1.28062484748656971738f;      // sqrt(1.64)
constexpr float PT_DIPOLE_POLE = 1.00580040321708930000f; // sqrt(1.64) pi / 4
constexpr float PT_DIPOLE_SIN_MIN = 0.000244140625f;      // 2^-12
constexpr float PT_DB_TO_LOG2 = 0.166096404744368117394f; // log2(10) / 20

struct pt_side {
    uint32_t kind, nz, na;
    float g;
    const float *table, *rot;
};

__device__ __forceinline__ pt_side side_of(const hrt_kpatterns &P, uint32_t s)
{
    return pt_side{s ? P.kind[1] : P.kind[0], s ? P.nz[1] : P.nz[0], s ? P.na[1] : P.na[0], s ? P.g[1] : P.g[0],
                   s ? P.table[1] : P.table[0], s ? P.rot[1] : P.rot[0]};
}

// u in the local frame of endpoint e: R[e] u, every row summed left to right (NULL: identity)
__device__ __forceinline__ void to_local(const float *rot, uint32_t e, float ux, float uy, float uz, float &x, float &y,
                                         float &z)
{
    x = ux; y = uy; z = uz;
    if (rot) {
        const float *R = rot + 9u * e;
        x = (R[0] * ux + R[1] * uy) + R[2] * uz;
        y = (R[3] * ux + R[4] * uy) + R[5] * uz;
        z = (R[6] * ux + R[7] * uy) + R[8] * uz;
    }
}

// zenith = atan2(hypot(x, y), z), azimuth = atan2(y, x): scale-invariant, (x, y, z) is not re-normalised
__device__ __forceinline__ float table_value(const pt_side &S, float theta, float phi)
{
    const uint32_t nz = S.nz, na = S.na;
    const float tz = theta * ((float)(nz - 1u) * PT_INV_PI);
    uint32_t i0 = (tz >= 0.f && tz < (float)(nz - 1u)) ? (uint32_t)tz : (tz >= (float)(nz - 1u) ? nz - 2u : 0u);
    const float sz = fminf(tz - (float)i0, 1.f);
    const float ta = (phi + PT_PI) * ((float)na * PT_INV_2PI);
    uint32_t k0 = (ta >= 0.f && ta < (float)(2u * na)) ? (uint32_t)ta : 0u;
    const float sa = ta - (float)k0;
    if (k0 >= na) k0 -= na;
    const uint32_t k1 = k0 + 1u == na ? 0u : k0 + 1u;
    const float *r0 = S.table + (uint64_t)i0 * na, *r1 = r0 + na;
    const float a0 = r0[k0], a1 = r0[k1], b0 = r1[k0], b1 = r1[k1];
    const float a = a0 + sa * (a1 - a0);
    const float b = b0 + sa * (b1 - b0);
    return a + sz * (b - a);
}

// F of the side's pattern for the local direction (x, y, z)
__device__ __forceinline__ float pattern_value(const pt_side &S, float x, float y, float z)
{
    switch (S.kind) {
    case HRT_PATTERN_DIPOLE: {
        // sin and |cos| of the zenith from the components; cos((pi / 2) cos t) = sin((pi / 2) sin^2 t / (1 + |cos t|))
        const float r = hypotf(x, y), n = hypotf(r, z);
        const float s = r / n, c = fabsf(z) / n;
        if (!(s >= PT_DIPOLE_SIN_MIN)) return (S.g * PT_DIPOLE_POLE) * s;
        const float q = (s * s) / (1.f + c);
        return ((S.g * PT_DIPOLE) * sinf(PT_HALF_PI * q)) / s;
    }
    case HRT_PATTERN_TR38901: {
        const float td = atan2f(hypotf(x, y), z) * PT_DEG, pd = atan2f(y, x) * PT_DEG;
        const float a = (td - 90.f) / 65.f, b = pd / 65.f;
        const float av = fminf(12.f * (a * a), 30.f), ah = fminf(12.f * (b * b), 30.f);
        const float A = fminf(av + ah, 30.f);
        return S.g * exp2f((8.f - A) * PT_DB_TO_LOG2);
    }
    case HRT_PATTERN_TABLE:
        return S.g * table_value(S, atan2f(hypotf(x, y), z), atan2f(y, x));
    default:
        return S.g;
    }
}

__device__ __forceinline__ float side_weight(const pt_side &S, uint32_t e, float ux, float uy, float uz)
{
    if (S.kind == HRT_PATTERN_ISOTROPIC) return S.g;
    float x, y, z;
    to_local(S.rot, e, ux, uy, uz, x, y, z);
    return pattern_value(S, x, y, z);
}

__device__ __forceinline__ float *rec_field_rw(const hrt_kview &V, uint32_t b, uint32_t rx, uint32_t f)
{
    return const_cast<float *>(rec_field(V, b, rx, f));
}

}  // namespace

__global__ void __launch_bounds__(HRT_PT_THREADS) hrt_patterns_records_kernel(const hrt_kpatterns P)
{
    const hrt_kview &V = P.v;
    const uint32_t b = blockIdx.y;
    const uint32_t i = blockIdx.x * HRT_PT_THREADS + threadIdx.x;
    const uint32_t *counts = reinterpret_cast<const uint32_t *>(V.ws + V.off_counts);
    const uint64_t n = counts[b + 1u];
    if (i >= n || i >= V.cap) return;
    const uint32_t ray = hit_field(V, b, HRT_HIT_RAY)[i];
    const uint32_t tx = ray / V.num_local;
    if (tx >= V.ntx) return;   // (not a ray of this trace: nothing of it is touched)

    const pt_side TX = side_of(P, 1u), RX = side_of(P, 0u);
    float wt = TX.g;
    if (TX.kind != HRT_PATTERN_ISOTROPIC) {
        const hrt_launch_dir_t d = hit_launch_dir(V, P.sh, b, tx, i);
        wt = side_weight(TX, tx, d.fx, d.fy, d.fz);
    }
    const uint32_t word = i >> 6, bit = i & 63u;
    for (uint32_t rx = 0; rx < V.nrx; ++rx) {
        if (!((mask_row(V, b, rx)[word] >> bit) & 1u)) continue;
        float wr = RX.g;
        if (RX.kind != HRT_PATTERN_ISOTROPIC)
            wr = side_weight(RX, rx, rec_field(V, b, rx, HRT_REC_DIRX)[i], rec_field(V, b, rx, HRT_REC_DIRY)[i],
                             rec_field(V, b, rx, HRT_REC_DIRZ)[i]);
        const float w = wr * wt;
        float *f0 = rec_field_rw(V, b, rx, HRT_REC_A_TE_RE), *f1 = rec_field_rw(V, b, rx, HRT_REC_A_TE_IM);
        float *f2 = rec_field_rw(V, b, rx, HRT_REC_A_TM_RE), *f3 = rec_field_rw(V, b, rx, HRT_REC_A_TM_IM);
        const float a0 = f0[i], a1 = f1[i], a2 = f2[i], a3 = f3[i];
        f0[i] = a0 * w;
        f1[i] = a1 * w;
        f2[i] = a2 * w;
        f3[i] = a3 * w;
    }
}

__global__ void hrt_patterns_los_kernel(const hrt_kpatterns P)
{
    const hrt_kview &V = P.v;
    const uint32_t link = blockIdx.x * blockDim.x + threadIdx.x;
    if (link >= V.nrx * V.ntx) return;
    float *L = const_cast<float *>(reinterpret_cast<const float *>(V.ws + V.off_los)) + (uint64_t)link * HRT_LOS_FLOATS;
    if (__float_as_uint(L[HRT_LOS_STATUS]) != 2u) return;   // blocked, or coincident (a = 1 by definition: los_entry)
    const uint32_t rx = link / V.ntx, tx = link - rx * V.ntx;
    const float ux = L[HRT_LOS_DIRX], uy = L[HRT_LOS_DIRY], uz = L[HRT_LOS_DIRZ];
    const float wt = side_weight(side_of(P, 1u), tx, ux, uy, uz);
    const float wr = side_weight(side_of(P, 0u), rx, -ux, -uy, -uz);
    L[HRT_LOS_A] = L[HRT_LOS_A] * (wr * wt);
}

extern "C" int hrt_hip_launch_patterns(const hrt_kpatterns *P, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (P->v.nb)
        hipLaunchKernelGGL(hrt_patterns_records_kernel, dim3((unsigned)(P->v.cap / HRT_PT_THREADS), P->v.nb),
                           dim3(HRT_PT_THREADS), 0, st, *P);
    const uint32_t links = P->v.nrx * P->v.ntx;
    hipLaunchKernelGGL(hrt_patterns_los_kernel, dim3((links + 255u) / 256u), dim3(256), 0, st, *P);
    return (int)hipGetLastError();
}
