// hrt_power.hip -- per-link power statistics (moments, power-delay profile, arrival and departure angular power
// spectra) from the workspace of a finished hrt_trace, for gfx950.  For every link (rx, tx) and polarisation pol,
// over the LoS entry (shard rank 0, hrt_power_reduce_kernel) and every unblocked scatter record (the other kernels):
//
//     p = |a^pol|^2 (FP64),  moments sum p x (1, tau, tau^2, nu, nu^2, u_rx, u_tx),  histograms sum p by bin
//
// The TX segments of the hit blocks come from hrt_channel_segments_kernel (csrc/hrt_channel.hip); the workspace
// view and its readers are csrc/hrt_pathsum.h, the fixed-point histograms csrc/hrt_power.h.
//   hrt_power_partial_kernel   one workgroup per (record chunk, link): every lane tests its records' mask bits and
//                              sums its terms in FP64; the workgroup adds the lanes in a fixed order (butterfly
//                              shuffles, then the waves in order) and writes the chunk's moments to the scratch.
//   hrt_power_reduce_kernel    one workgroup per link: the chunks in a fixed order (strided over the threads, then
//                              the partial kernel's tree), plus the LoS term, into out; this call's P to the
//                              scratch; the LoS term's fixed-point bins.
//   hrt_power_hist_kernel      the chunking of the partial kernel: every term's bins, fixed-point u64 adds into an
//                              LDS copy of the link's histograms (flushed with global u64 atomic adds of the non-zero
//                              bins) or, when they do not fit, straight into the scratch.
//   hrt_power_finalize_kernel  one thread per bin: q 2^(E - 62) into out.
// No floating-point atomics anywhere: two calls with the same inputs give the same bits.
//
// u_rx is the record's HRT_REC_DIR (directions_rx); u_tx the launch direction of the record's ray, evaluated from the
// global path as hrt_array_channel does (csrc/hrt_launch_dir.h); nu the float difference FS0 - DFS.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrt_pathsum.h"
#include "hrt_power.h"

namespace {

constexpr uint32_t F = HRT_POWER_FIELDS;
constexpr uint32_t NW = 11u;   // the p-weighted fields P .. P_UTX_Z, per pol
constexpr double PI = 3.141592653589793;   // (numpy's pi)

// one term: p per pol, tau, nu and both directions
struct pw_term {
    double p[2], tau, nu, ur[3], ut[3];
};

// field f (HRT_POWER_P .. HRT_POWER_P_UTX_Z) of a term
__device__ __forceinline__ double term_field(const pw_term &t, uint32_t pol, uint32_t f)
{
    const double p = t.p[pol];
    switch (f) {
    case HRT_POWER_P: return p;
    case HRT_POWER_P_TAU: return p * t.tau;
    case HRT_POWER_P_TAU2: return p * t.tau * t.tau;
    case HRT_POWER_P_NU: return p * t.nu;
    case HRT_POWER_P_NU2: return p * t.nu * t.nu;
    case HRT_POWER_P_URX_X: return p * t.ur[0];
    case HRT_POWER_P_URX_Y: return p * t.ur[1];
    case HRT_POWER_P_URX_Z: return p * t.ur[2];
    case HRT_POWER_P_UTX_X: return p * t.ut[0];
    case HRT_POWER_P_UTX_Y: return p * t.ut[1];
    default: return p * t.ut[2];
    }
}

__device__ __forceinline__ void scatter_term(const hrt_kpower &P, uint32_t b, uint32_t rx, uint32_t tx, uint32_t i,
                                             pw_term &t)
{
    float R[HRT_PS_REC_FLOATS];
    stage_record(P.v, P.sh, b, rx, tx, i, R);
    const double ter = R[0], tei = R[1], tmr = R[2], tmi = R[3];
    t.p[0] = ter * ter + tei * tei;
    t.p[1] = tmr * tmr + tmi * tmi;
    t.tau = R[4];
    t.nu = R[5];
    for (int q = 0; q < 3; ++q) {
        t.ur[q] = R[6 + q];
        t.ut[q] = R[9 + q];
    }
}

// the LoS entry of a link as a term (false where there is none: blocked)
__device__ __forceinline__ bool los_term(const hrt_kview &V, uint32_t link, pw_term &t)
{
    hrt_los_entry L;
    if (!los_entry(V, link, L)) return false;
    const double a = L.a;
    t.p[0] = t.p[1] = a * a;
    t.tau = L.tau;
    t.nu = L.nu;
    t.ut[0] = L.ux; t.ut[1] = L.uy; t.ut[2] = L.uz;
    t.ur[0] = -(double)L.ux; t.ur[1] = -(double)L.uy; t.ur[2] = -(double)L.uz;
    return true;
}

// the fixed-point scale of a (link, pol): the least E with 2^E >= 2 P (0 for P = 0)
__device__ __forceinline__ int hist_exp(double total)
{
    int e = 0;
    frexp(total, &e);   // total = m 2^e, m in [1/2, 1): 2 total < 2^(e + 1)
    return total > 0.0 ? e + 1 : 0;
}

__device__ __forceinline__ unsigned long long hist_q(double p, int E)
{
    const double x = rint(ldexp(p, 62 - E));
    return x < 9.2e18 ? (unsigned long long)x : 0ull;   // (x <= 2^62 for p <= P; a NaN adds nothing)
}

// the bins of a term: delay (Ld: outside the window), zenith x azimuth of u_rx and of u_tx
__device__ __forceinline__ uint32_t delay_bin(const hrt_kpower &P, double tau)
{
    const double x = (tau - P.tau0) / P.dtau;
    return x >= 0.0 && x < (double)P.Ld ? (uint32_t)x : P.Ld;
}

__device__ __forceinline__ uint32_t angle_bin(const hrt_kpower &P, const double *u)
{
    const double th = floor(acos(fmin(fmax(u[2], -1.0), 1.0)) / PI * (double)P.Nth);
    const double ph = floor((atan2(u[1], u[0]) + PI) / (2.0 * PI) * (double)P.Nph);
    const uint32_t i = th > 0.0 ? (th < (double)P.Nth ? (uint32_t)th : P.Nth - 1u) : 0u;
    const uint32_t j = ph > 0.0 && ph < (double)P.Nph ? (uint32_t)ph : 0u;   // index Nph wraps to 0
    return i * P.Nph + j;
}

__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);   // every lane: the same sum, in the same order
    return x;
}

}  // namespace

__global__ void __launch_bounds__(HRT_PW_THREADS) hrt_power_partial_kernel(const hrt_kpower P)
{
    const hrt_kview &V = P.v;
    const uint32_t c = blockIdx.x, link = blockIdx.y;
    const uint32_t rx = link / V.ntx, tx = link % V.ntx;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    constexpr uint32_t NA = 1u + 2u * NW;   // count, then [pol][field]
    __shared__ double sW[HRT_PW_THREADS / 64u][NA];

    double acc[NA];
#pragma unroll
    for (uint32_t k = 0; k < NA; ++k) acc[k] = 0.0;
    for (uint32_t b = 0; b < V.nb; ++b) {
        uint32_t start, end;
        chunk_range(V, b, tx, c, start, end);
        const uint64_t *mask = mask_row(V, b, rx);
        for (uint32_t i = start + tid; i < end; i += HRT_PW_THREADS) {
            if (!((mask[i >> 6] >> (i & 63u)) & 1u)) continue;
            pw_term t;
            scatter_term(P, b, rx, tx, i, t);
            acc[0] += 1.0;
#pragma unroll
            for (uint32_t pol = 0; pol < 2u; ++pol)
#pragma unroll
                for (uint32_t f = 0; f < NW; ++f) acc[1u + pol * NW + f] += term_field(t, pol, HRT_POWER_P + f);
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < NA; ++k) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) sW[w][k] = s;
    }
    __syncthreads();
    if (tid < 2u * F) {   // (pol, field) of the chunk: the waves in order
        const uint32_t pol = tid / F, f = tid % F;
        double s = 0.0;
        if (f == HRT_POWER_COUNT || (f >= HRT_POWER_P && f < HRT_POWER_P + NW)) {
            const uint32_t k = f == HRT_POWER_COUNT ? 0u : 1u + pol * NW + (f - HRT_POWER_P);
            for (uint32_t q = 0; q < HRT_PW_THREADS / 64u; ++q) s += sW[q][k];
        }
        P.partial[((uint64_t)link * V.nchunks + c) * 2u * F + tid] = s;   // (P_LOS: 0)
    }
}

// one workgroup per link: thread t adds chunks t, t + 256, ... in order, the workgroup adds the threads in a fixed
// order; then per (pol, field) + LoS -> out; this call's P -> total; the LoS term's bins -> hist
__global__ void __launch_bounds__(HRT_PW_THREADS) hrt_power_reduce_kernel(const hrt_kpower P)
{
    const hrt_kview &V = P.v;
    const uint32_t link = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    __shared__ double sW[HRT_PW_THREADS / 64u][2u * F];

    double acc[2u * F];
#pragma unroll
    for (uint32_t k = 0; k < 2u * F; ++k) acc[k] = 0.0;
    const double *src = P.partial + (uint64_t)link * V.nchunks * 2u * F;
    for (uint32_t c = tid; c < V.nchunks; c += HRT_PW_THREADS)
#pragma unroll
        for (uint32_t k = 0; k < 2u * F; ++k) acc[k] += src[(uint64_t)c * 2u * F + k];
#pragma unroll
    for (uint32_t k = 0; k < 2u * F; ++k) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) sW[w][k] = s;
    }
    __syncthreads();
    if (tid >= 2u * F) return;
    const uint32_t pol = tid / F, f = tid % F;
    double s = 0.0;
    for (uint32_t q = 0; q < HRT_PW_THREADS / 64u; ++q) s += sW[q][tid];
    pw_term t;
    const bool los = V.los && los_term(V, link, t);
    if (los) {
        if (f == HRT_POWER_COUNT) s += 1.0;
        else if (f == HRT_POWER_P_LOS) s += t.p[pol];
        else s += term_field(t, pol, f);
    }
    if (f == HRT_POWER_P) {
        P.total[(uint64_t)link * 2u + pol] = s;
        if (los && P.nbins) {   // the hist kernel adds after this one: plain adds
            const unsigned long long q = hist_q(t.p[pol], hist_exp(s));
            unsigned long long *H = P.hist + ((uint64_t)link * 2u + pol) * P.nbins;
            const uint32_t kd = delay_bin(P, t.tau);
            if (kd < P.Ld) H[kd] += q;
            if (P.Nth) {
                const uint32_t A = P.Nth * P.Nph;
                H[P.Ld + angle_bin(P, t.ur)] += q;
                H[P.Ld + A + angle_bin(P, t.ut)] += q;
            }
        }
    }
    double *o = P.out + (uint64_t)link * 2u * F + tid;
    o[0] = V.accumulate ? o[0] + s : s;
}

// LDS: the link's histograms (2 nbins u64, dynamic LDS) in LDS, flushed at the end; else straight to the scratch
template <bool LDS>
__global__ void __launch_bounds__(HRT_PW_HIST_THREADS) hrt_power_hist_kernel(const hrt_kpower P)
{
    extern __shared__ unsigned long long sH[];
    const hrt_kview &V = P.v;
    const uint32_t c = blockIdx.x, link = blockIdx.y;
    const uint32_t rx = link / V.ntx, tx = link % V.ntx;
    const uint32_t tid = threadIdx.x;
    const uint32_t nb2 = 2u * P.nbins, A = P.Nth * P.Nph;
    unsigned long long *gH = P.hist + (uint64_t)link * nb2;
    unsigned long long *H = LDS ? sH : gH;
    if (LDS) {
        for (uint32_t j = tid; j < nb2; j += HRT_PW_HIST_THREADS) sH[j] = 0ull;
        __syncthreads();
    }
    const int E0 = hist_exp(P.total[(uint64_t)link * 2u]), E1 = hist_exp(P.total[(uint64_t)link * 2u + 1u]);
    for (uint32_t b = 0; b < V.nb; ++b) {
        uint32_t start, end;
        chunk_range(V, b, tx, c, start, end);
        const uint64_t *mask = mask_row(V, b, rx);
        for (uint32_t i = start + tid; i < end; i += HRT_PW_HIST_THREADS) {
            if (!((mask[i >> 6] >> (i & 63u)) & 1u)) continue;
            pw_term t;
            scatter_term(P, b, rx, tx, i, t);
            const unsigned long long q0 = hist_q(t.p[0], E0), q1 = hist_q(t.p[1], E1);
            if ((q0 | q1) == 0ull) continue;
            const uint32_t kd = delay_bin(P, t.tau);
            if (kd < P.Ld) {
                atomicAdd(&H[kd], q0);
                atomicAdd(&H[P.nbins + kd], q1);
            }
            if (A) {
                const uint32_t ka = P.Ld + angle_bin(P, t.ur), kt = P.Ld + A + angle_bin(P, t.ut);
                atomicAdd(&H[ka], q0);
                atomicAdd(&H[P.nbins + ka], q1);
                atomicAdd(&H[kt], q0);
                atomicAdd(&H[P.nbins + kt], q1);
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t j = tid; j < nb2; j += HRT_PW_HIST_THREADS) {
            const unsigned long long v = sH[j];
            if (v) atomicAdd(&gH[j], v);
        }
    }
}

// one thread per (link, pol, bin): q 2^(E - 62) -> out (pdp, arrival or departure)
__global__ void hrt_power_finalize_kernel(const hrt_kpower P)
{
    const hrt_kview &V = P.v;
    const uint64_t links = (uint64_t)V.nrx * V.ntx;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= links * 2u * P.nbins) return;
    const uint64_t lp = gid / P.nbins;   // link * 2 + pol
    const uint32_t j = (uint32_t)(gid % P.nbins), A = P.Nth * P.Nph;
    const double v = ldexp((double)P.hist[gid], hist_exp(P.total[lp]) - 62);
    double *pdp = P.out + links * 2u * F, *arr = pdp + links * 2u * P.Ld, *dep = arr + links * 2u * A;
    double *o = j < P.Ld ? pdp + lp * P.Ld + j
                         : (j < P.Ld + A ? arr + lp * A + (j - P.Ld) : dep + lp * A + (j - P.Ld - A));
    o[0] = V.accumulate ? o[0] + v : v;
}

extern "C" int hrt_hip_launch_power(const hrt_kpower *P, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint32_t links = P->v.nrx * P->v.ntx;
    const uint64_t hist_bytes = (uint64_t)links * 2u * P->nbins * 8u;
    hipError_t he;
    if (hist_bytes && (he = hipMemsetAsync(P->hist, 0, hist_bytes, st)) != hipSuccess) return (int)he;
    if (P->v.nchunks) {
        const int e = hrt_hip_launch_segments(&P->v, stream);
        if (e) return e;
        hipLaunchKernelGGL(hrt_power_partial_kernel, dim3(P->v.nchunks, links), dim3(HRT_PW_THREADS), 0, st, *P);
    }
    hipLaunchKernelGGL(hrt_power_reduce_kernel, dim3(links), dim3(HRT_PW_THREADS), 0, st, *P);
    if ((he = hipGetLastError()) != hipSuccess || !hist_bytes) return (int)he;
    if (P->v.nchunks) {
        // the LDS form where the link's bins fit the budget and the device (the bins do not depend on the form)
        const uint64_t lds = 2ull * P->nbins * 8u;
        int dev = 0, max_lds = 0;
        bool use_lds = lds <= HRT_PW_LDS_MAX && hipGetDevice(&dev) == hipSuccess &&
                       hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess &&
                       lds <= (uint64_t)max_lds;
        if (use_lds && lds > (64u << 10) &&
            hipFuncSetAttribute((const void *)hrt_power_hist_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds) != hipSuccess)
            use_lds = false;
        (void)hipGetLastError();   // (a refused attribute leaves its error behind: the global form runs instead)
        const dim3 grid(P->v.nchunks, links);
        if (use_lds)
            hipLaunchKernelGGL(hrt_power_hist_kernel<true>, grid, dim3(HRT_PW_HIST_THREADS), (unsigned)lds, st, *P);
        else
            hipLaunchKernelGGL(hrt_power_hist_kernel<false>, grid, dim3(HRT_PW_HIST_THREADS), 0, st, *P);
    }
    const uint64_t nf = (uint64_t)links * 2u * P->nbins;
    hipLaunchKernelGGL(hrt_power_finalize_kernel, dim3((unsigned)((nf + 255u) / 256u)), dim3(256), 0, st, *P);
    return (int)hipGetLastError();
}
