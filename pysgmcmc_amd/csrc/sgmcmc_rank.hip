// sgmcmc_rank.hip -- K18: rank normalisation of a strided (m, n, P) device trace, behind include/sgmcmc_hip_rank.h. For every
// parameter: pool the draws of the 2 m split chains, sort, average ranks over ties, inverse normal CDF (AS241), the same for
// |x - median|, and the two 5 % tail indicators. K12 (sgmcmc_chain_diag.hip) turns the four outputs into the rank-normalised
// split R-hat and the bulk and tail effective sample sizes.
//
// One launch, grid = P, one workgroup per parameter column. The column sits in the LDS as doubles (for both element types)
// next to the 16-bit pooled index of each draw, padded with +inf to a power of two npad >= 128: 10 bytes a slot. The LDS is
// static, in three capacity classes (1024, 4096, 8192 slots: 10, 40, 80 KiB), so small columns leave room for several
// workgroups on a CU and no launch needs a function attribute. The workgroup has npad / 2 threads, at most 1024.
//   1. gather   the column with stride ld into the LDS, converting to double; a NaN or an infinity anywhere makes the whole
//               workgroup write NaN to its outputs and leave
//   2. sort     bitonic, a barrier per stage, on the STRICT TOTAL order (value, pooled index): equal values (and -0.0 with
//               +0.0) are ordered by index, the +inf padding carries the indices N .. npad - 1 and so ends up behind every
//               draw. The sorted image does not depend on the shape of the network or the workgroup size.
//   3. emit     from sorted position k: the run of equal values around k (neighbours first, two binary searches when there is a
//               tie) gives rank2 = first + last + 2; z, tail_lo, tail_hi go to the place of draw idx[k] with one 8-byte store
//               each. The elements of one column are ld_out apart in any order, so nothing is gained by putting them back
//               into draw order first.
//   4. fold     keys[k] = |keys[k] - med| in place (the index stays), sort again, emit z_folded.
// No atomics, no scratch, nothing waited on but the workgroup's own barriers.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sgmcmc_hip_rank.h"

#pragma clang fp contract(off)

#include "sgmcmc_host.hpp"

using namespace sgmcmc_host;

namespace {

constexpr int RK_MAX_POOLED = SGMCMC_RANK_MAX_POOLED;
constexpr int RK_MIN_PAD = 128;                           // the smallest padded count: one wave of pairs
constexpr int RK_MAX_BLOCK = 1024;

// Wichura, AS241, PPND16, for p in (0, 0.5]: the published coefficients in the published order.
__device__ __forceinline__ double ppnd16_lower(double p)
{
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r
                                + 4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r
                             + 1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r
                                + 2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r
                             + 4.2313330701600911252e+1) * r + 1.0);
        return num / den;
    }
    double r = q <= 0.0 ? p : 1.0 - p;
    r = sqrt(-log(r));
    double num, den;
    if (r <= 5.0) {
        r = r - 1.6;
        num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r
                   + 1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r
                + 4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
        den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r
                   + 1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r
                + 2.05319162663775882187e+0) * r + 1.0);
    } else {
        r = r - 5.0;
        num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r
                   + 2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r
                + 5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
        den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r
                   + 7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r
                + 5.99832206555888793769e-1) * r + 1.0);
    }
    double x = num / den;
    if (q < 0.0) x = -x;
    return x;
}

// zeta of the header: the upper half of the ranks is the negated lower half
__device__ __forceinline__ double z_of_rank2(int rank2, int N)
{
    const double D = 2.0 * (double)N + 0.5;
    const bool lower = rank2 <= N + 1;
    const double v = ppnd16_lower(((double)(lower ? rank2 : 2 * N + 2 - rank2) - 0.75) / D);
    return lower ? v : -v;
}

// ascending bitonic sort of keys[0 .. npad) with idx as the tie-breaker and payload; ends behind a barrier
__device__ __forceinline__ void rank_sort(double *keys, uint16_t *idx, int npad)
{
    const int pairs = npad >> 1;
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int t = (int)threadIdx.x; t < pairs; t += (int)blockDim.x) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const double a = keys[lo], b = keys[hi];
                const uint16_t ia = idx[lo], ib = idx[hi];
                const bool after = a > b || (a == b && ia > ib);          // (a, ia) comes after (b, ib)
                if (after == ((lo & k) == 0)) {
                    keys[lo] = b; keys[hi] = a;
                    idx[lo] = ib; idx[hi] = ia;
                }
            }
            __syncthreads();
        }
    }
}

// rank2 of sorted position k among keys[0 .. N)
__device__ __forceinline__ int rank2_at(const double *keys, int k, int N)
{
    const double v = keys[k];
    int first = k, last = k;
    if (k > 0 && keys[k - 1] == v) {                      // first: the smallest position in [0, k) whose key is not below v
        int a = 0, b = k - 1;                             // keys[b] == v
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (keys[mid] < v) a = mid + 1; else b = mid;
        }
        first = a;
    }
    if (k + 1 < N && keys[k + 1] == v) {                  // last: the largest position in (k, N) whose key is not above v
        int a = k + 1, b = N - 1;                         // keys[a] == v
        while (a < b) {
            const int mid = (a + b + 1) >> 1;
            if (keys[mid] > v) b = mid - 1; else a = mid;
        }
        last = a;
    }
    return first + last + 2;
}

template <typename T, int CAP>
__global__ void __launch_bounds__(RK_MAX_BLOCK)
rank_normalize_kernel(const T *__restrict__ trace, int n, int half, size_t ld, size_t chain_stride, double *__restrict__ z,
                      double *__restrict__ z_folded, double *__restrict__ tail_lo, double *__restrict__ tail_hi, size_t ld_out,
                      size_t chain_stride_out, int N, int npad)
{
    __shared__ double keys[CAP];
    __shared__ uint16_t idx[CAP];
    const int tid = (int)threadIdx.x, block = (int)blockDim.x;
    const size_t p = blockIdx.x;
    const int second = n - half;                          // source draw of the second half's first element

    int bad = 0;
    for (int j = tid; j < npad; j += block) {
        double v = INFINITY;
        if (j < N) {
            const int s = j / half, i = j - s * half;
            const size_t src = (size_t)(s >> 1) * chain_stride + (size_t)((s & 1) * second + i) * ld + p;
            v = (double)trace[src];
            bad |= !isfinite(v);
        }
        keys[j] = v;
        idx[j] = (uint16_t)j;
    }
    bad = __syncthreads_or(bad);

    // the place of pooled draw j in an output
    auto place = [&](int j) {
        const int s = j / half, i = j - s * half;
        return (size_t)s * chain_stride_out + (size_t)i * ld_out + p;
    };

    if (bad) {
        const double nan = __builtin_nan("");
        for (int j = tid; j < N; j += block) {
            const size_t o = place(j);
            if (z) z[o] = nan;
            if (z_folded) z_folded[o] = nan;
            if (tail_lo) tail_lo[o] = nan;
            if (tail_hi) tail_hi[o] = nan;
        }
        return;
    }

    rank_sort(keys, idx, npad);
    const double med = (keys[N / 2 - 1] + keys[N / 2]) * 0.5;
    const double lo_cut = keys[(N - 1) / 20], hi_cut = keys[(19 * (N - 1) + 19) / 20];
    if (z || tail_lo || tail_hi) {
        for (int k = tid; k < N; k += block) {
            const double v = keys[k];
            const size_t o = place((int)idx[k]);
            if (z) z[o] = z_of_rank2(rank2_at(keys, k, N), N);
            if (tail_lo) tail_lo[o] = v <= lo_cut ? 1.0 : 0.0;
            if (tail_hi) tail_hi[o] = v >= hi_cut ? 1.0 : 0.0;
        }
    }
    if (!z_folded) return;
    __syncthreads();                                      // every read of the first sorted image is done
    for (int k = tid; k < N; k += block) keys[k] = fabs(keys[k] - med);
    __syncthreads();
    rank_sort(keys, idx, npad);
    for (int k = tid; k < N; k += block) z_folded[place((int)idx[k])] = z_of_rank2(rank2_at(keys, k, N), N);
}

template <typename T>
int rank_normalize(const T *trace, int m, size_t n, size_t P, size_t ld, size_t chain_stride, double *z, double *z_folded,
                   double *tail_lo, double *tail_hi, size_t ld_out, size_t chain_stride_out, hipStream_t st)
{
    const char *who = "rank_normalize";
    if (m < 1 || m > SGMCMC_RANK_MAX_CHAINS)
        return fail(SGMCMC_EINVAL, "%s: m = %d chains, must be 1 .. %d", who, m, SGMCMC_RANK_MAX_CHAINS);
    if (n < 4) return fail(SGMCMC_EINVAL, "%s: n = %zu samples, must be at least 4", who, n);
    const size_t half = n / 2;
    if (half > (size_t)RK_MAX_POOLED || 2 * (size_t)m * half > (size_t)RK_MAX_POOLED)
        return fail(SGMCMC_EINVAL, "%s: N = 2 * m * (n / 2) with m = %d, n = %zu exceeds %d pooled draws", who, m, n, RK_MAX_POOLED);
    if (P == 0) return 0;
    if (!trace) return fail(SGMCMC_EINVAL, "%s: trace must be non-NULL", who);
    if (!z && !z_folded && !tail_lo && !tail_hi)
        return fail(SGMCMC_EINVAL, "%s: at least one of z, z_folded, tail_lo and tail_hi must be non-NULL", who);
    if (ld < P) return fail(SGMCMC_EINVAL, "%s: ld = %zu is smaller than P = %zu", who, ld, P);
    size_t rows = 0, need = 0, last = 0, extent = 0;
    if (__builtin_mul_overflow(n - 1, ld, &rows) || __builtin_add_overflow(rows, P, &need))
        return fail(SGMCMC_EINVAL, "%s: (n - 1) * ld + P overflows with n = %zu, ld = %zu", who, n, ld);
    if (chain_stride < need)
        return fail(SGMCMC_EINVAL, "%s: chain_stride = %zu is smaller than (n - 1) * ld + P = %zu", who, chain_stride, need);
    if (ld_out < P) return fail(SGMCMC_EINVAL, "%s: ld_out = %zu is smaller than P = %zu", who, ld_out, P);
    size_t rows_out = 0, need_out = 0;
    if (__builtin_mul_overflow(half - 1, ld_out, &rows_out) || __builtin_add_overflow(rows_out, P, &need_out))
        return fail(SGMCMC_EINVAL, "%s: (half - 1) * ld_out + P overflows with half = %zu, ld_out = %zu", who, half, ld_out);
    if (chain_stride_out < need_out)
        return fail(SGMCMC_EINVAL, "%s: chain_stride_out = %zu is smaller than (half - 1) * ld_out + P = %zu", who,
                    chain_stride_out, need_out);
    if (__builtin_mul_overflow((size_t)(m - 1), chain_stride, &last) || __builtin_add_overflow(last, need, &extent)
        || extent > SIZE_MAX / sizeof(T))
        return fail(SGMCMC_EINVAL, "%s: the trace's extent overflows with m = %d, chain_stride = %zu", who, m, chain_stride);
    if (__builtin_mul_overflow((size_t)(2 * m - 1), chain_stride_out, &last) || __builtin_add_overflow(last, need_out, &extent)
        || extent > SIZE_MAX / sizeof(double))
        return fail(SGMCMC_EINVAL, "%s: the outputs' extent overflows with m = %d, chain_stride_out = %zu", who, m, chain_stride_out);
    if (P > (size_t)INT32_MAX) return fail(SGMCMC_EINVAL, "%s: P = %zu is too large for one launch", who, P);

    const int N = (int)(2 * (size_t)m * half);
    int npad = RK_MIN_PAD;
    while (npad < N) npad <<= 1;
    const int block = npad / 2 < RK_MAX_BLOCK ? npad / 2 : RK_MAX_BLOCK;
#define RANK_LAUNCH(CAP)                                                                                                       \
    hipLaunchKernelGGL((rank_normalize_kernel<T, CAP>), dim3((unsigned)P), dim3(block), 0, st, trace, (int)n, (int)half, ld,   \
                       chain_stride, z, z_folded, tail_lo, tail_hi, ld_out, chain_stride_out, N, npad)
    if (npad <= 1024) RANK_LAUNCH(1024);
    else if (npad <= 4096) RANK_LAUNCH(4096);
    else RANK_LAUNCH(RK_MAX_POOLED);
#undef RANK_LAUNCH
    return launched("rank_normalize_kernel");
}

}  // namespace

extern "C" {

int sgmcmc_rank_abi_version(void) { return SGMCMC_RANK_ABI_VERSION; }

int sgmcmc_rank_max_pooled(void) { return RK_MAX_POOLED; }

int sgmcmc_rank_normalize_f32(const float *trace, int m, size_t n, size_t P, size_t ld, size_t chain_stride, double *z,
                              double *z_folded, double *tail_lo, double *tail_hi, size_t ld_out, size_t chain_stride_out,
                              sgmcmc_stream_t stream)
{
    return rank_normalize<float>(trace, m, n, P, ld, chain_stride, z, z_folded, tail_lo, tail_hi, ld_out, chain_stride_out,
                                 static_cast<hipStream_t>(stream));
}
int sgmcmc_rank_normalize_f64(const double *trace, int m, size_t n, size_t P, size_t ld, size_t chain_stride, double *z,
                              double *z_folded, double *tail_lo, double *tail_hi, size_t ld_out, size_t chain_stride_out,
                              sgmcmc_stream_t stream)
{
    return rank_normalize<double>(trace, m, n, P, ld, chain_stride, z, z_folded, tail_lo, tail_hi, ld_out, chain_stride_out,
                                  static_cast<hipStream_t>(stream));
}

}  // extern "C"
