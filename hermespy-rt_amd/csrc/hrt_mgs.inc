// hrt_mgs.inc -- the lane-level pieces of modified Gram-Schmidt on a matrix held in LDS by a group of G lanes, shared by
// the equalizer kernel (csrc/hrt_equalizer.hip) and the precoder kernel (csrc/hrt_precoder.hip).  Both factor an
// augmented matrix A = [top; sqrt(lambda) I] = Q R with n columns, column by column, and carry the column operations on
// an n x n block T that starts as I and ends as R^-1 (csrc/hrt_equalizer.h has the reasons and the LDS layout).
//
// The including file defines EQ_T, the threads of a workgroup, before the include: entry (k, c, part) of a lane's rows is
// the word ((k n + c) 2 + part) EQ_T of its pointer (wA: the top block, mk rows a lane; wT: T, nk rows a lane).  Every
// sum is a per-lane sum over k ascending, then a butterfly over the group: the tests emulate exactly this order.

// sum over the G lanes of a group; every lane ends with the same bits (a + b = b + a at each level)
template <uint32_t G>
__device__ __forceinline__ float eq_reduce(float v)
{
#pragma unroll
    for (uint32_t off = 1u; off < G; off *= 2u) v = v + __shfl_xor(v, (int)off);
    return v;
}

// the value of the group's lane `src` (the same bits in every lane of the group)
template <uint32_t G>
__device__ __forceinline__ float eq_from(float v, uint32_t src)
{
    if constexpr (G == 1u) return v;
    else return __shfl(v, (int)src, (int)G);
}

// sum_k |x[k, c]|^2 over `rows` rows of this lane
__device__ __forceinline__ float eq_lane_norm2(const float *w, uint32_t c, uint32_t rows, uint32_t n)
{
    float a = 0.f;
    for (uint32_t k = 0; k < rows; ++k) {
        const float xr = w[((k * n + c) * 2u) * EQ_T], xi = w[((k * n + c) * 2u + 1u) * EQ_T];
        a = a + (xr * xr + xi * xi);
    }
    return a;
}

// |a_c|^2 of the augmented matrix over the group: the top block, plus lambda times T's
template <uint32_t G>
__device__ __forceinline__ float eq_norm2(const float *wA, const float *wT, uint32_t c, uint32_t mk, uint32_t nk, uint32_t n,
                                          bool aug, float lam)
{
    float a = eq_lane_norm2(wA, c, mk, n);
    if (aug) a = a + lam * eq_lane_norm2(wT, c, nk, n);
    return eq_reduce<G>(a);
}

// sum_k conj(x[k, p]) x[k, q] over `rows` rows of this lane
__device__ __forceinline__ void eq_lane_dot(const float *w, uint32_t p, uint32_t q, uint32_t rows, uint32_t n, float &re,
                                            float &im)
{
    re = 0.f;
    im = 0.f;
    for (uint32_t k = 0; k < rows; ++k) {
        const float *x = w + ((k * n + p) * 2u) * EQ_T, *y = w + ((k * n + q) * 2u) * EQ_T;
        const float xr = x[0], xi = x[EQ_T], yr = y[0], yi = y[EQ_T];
        re = re + (xr * yr + xi * yi);
        im = im + (xr * yi - xi * yr);
    }
}

// x[:, c] /= d on `rows` rows of this lane
__device__ __forceinline__ void eq_scale(float *w, uint32_t c, uint32_t rows, uint32_t n, float d)
{
    for (uint32_t k = 0; k < rows; ++k) {
        float *x = w + ((k * n + c) * 2u) * EQ_T;
        x[0] = x[0] / d;
        x[EQ_T] = x[EQ_T] / d;
    }
}

// x[:, q] -= (rr + j ri) x[:, p] on `rows` rows of this lane
__device__ __forceinline__ void eq_project(float *w, uint32_t p, uint32_t q, uint32_t rows, uint32_t n, float rr, float ri)
{
    for (uint32_t k = 0; k < rows; ++k) {
        const float *x = w + ((k * n + p) * 2u) * EQ_T;
        float *y = w + ((k * n + q) * 2u) * EQ_T;
        const float xr = x[0], xi = x[EQ_T];
        y[0] = y[0] - (rr * xr - ri * xi);
        y[EQ_T] = y[EQ_T] - (rr * xi + ri * xr);
    }
}

// start: the squared column norms of A; their largest (for the singular threshold) and their sum (not finite: the
// point is flagged) come back in nmax and nsum
template <uint32_t G>
__device__ __forceinline__ void eq_start(const float *wA, const float *wT, uint32_t mk, uint32_t nk, uint32_t n, bool aug,
                                         float lam, float &nmax, float &nsum)
{
    nmax = 0.f;
    nsum = 0.f;
    for (uint32_t c = 0; c < n; ++c) {
        const float a = eq_norm2<G>(wA, wT, c, mk, nk, n, aug, lam);
        nmax = a > nmax ? a : nmax;
        nsum = nsum + a;
    }
}

// factor: A = Q R, T = R^-1; true where a diagonal entry of R is at or below thr
template <uint32_t G>
__device__ __forceinline__ bool eq_factor(float *wA, float *wT, uint32_t mk, uint32_t nk, uint32_t n, bool aug, float lam,
                                          float thr)
{
    bool sing = false;
    for (uint32_t j = 0; j < n; ++j) {
        const float rjj = sqrtf(eq_norm2<G>(wA, wT, j, mk, nk, n, aug, lam));
        sing = sing || !(rjj > thr);
        eq_scale(wA, j, mk, n, rjj);
        eq_scale(wT, j, nk, n, rjj);
        for (uint32_t i = j + 1u; i < n; ++i) {
            float rr, ri;
            eq_lane_dot(wA, j, i, mk, n, rr, ri);
            if (aug) {
                float tr, ti;
                eq_lane_dot(wT, j, i, nk, n, tr, ti);
                rr = rr + lam * tr;
                ri = ri + lam * ti;
            }
            rr = eq_reduce<G>(rr);
            ri = eq_reduce<G>(ri);
            eq_project(wA, j, i, mk, n, rr, ri);
            eq_project(wT, j, i, nk, n, rr, ri);
        }
    }
    return sing;
}

// weights: the top block becomes Q1 T^H in place, columns ascending: column i <- sum_{c >= i} conj(T[i, c]) q_c (T is
// upper triangular, so the columns it reads are not yet overwritten); T[i, c] comes from its owner by a shuffle
template <uint32_t G>
__device__ __forceinline__ void eq_weights(float *wA, const float *wT, uint32_t mk, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i) {
        const float *const ti = wT + ((i / G) * n * 2u) * EQ_T;     // (the slot of row i, in every lane)
        for (uint32_t c = i; c < n; ++c) {
            const float tr = eq_from<G>(ti[(c * 2u) * EQ_T], i % G), tm = eq_from<G>(ti[(c * 2u + 1u) * EQ_T], i % G);
            for (uint32_t k = 0; k < mk; ++k) {
                float *x = wA + ((k * n + i) * 2u) * EQ_T;
                const float *y = wA + ((k * n + c) * 2u) * EQ_T;
                const float yr = y[0], yi = y[EQ_T];
                const float pr = tr * yr + tm * yi, pi = tr * yi - tm * yr;
                x[0] = c == i ? pr : x[0] + pr;
                x[EQ_T] = c == i ? pi : x[EQ_T] + pi;
            }
        }
    }
}
