// sgmcmc_calib.hip -- K20: PIT, central-interval coverage, PIT histogram and the closed-form CRPS of the equal-weight Gaussian
// mixture that a kept ensemble predicts, behind include/sgmcmc_hip_calib.h (the statement is there).
//
// One launch, grid = n_rows, one workgroup per row, 64 .. 1024 threads (half the draws, rounded up to a power of two), then a
// 256-lane launch for the summary. The LDS is static, in three capacity classes (256, 1024, 4096 draws of 24 bytes).
//   mu, var      the row's means as doubles and the variances, read once into the LDS
//   P, T         256 partials on the first 256 threads (all of a smaller workgroup), a chain of S / 256 terms each, then the tree
//   g_s          thread p runs the chains g_p and g_(S-1-p): p + (S - 1 - p) = S - 1 pair terms whatever p. While t < p both
//                chains advance in one loop body, so two independent erf / exp / sqrt / divide sequences are in flight; the
//                rest of the longer chain follows alone. mu[t] and var[t] are read at one address by all lanes (a broadcast).
//                With 4096 draws a thread takes two such pairs, one after the other.
//   G, Dg        g in the LDS, folded like P and T
// No atomics, no scratch buffer, nothing waited on but the workgroup's own barriers.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sgmcmc_hip_calib.h"

#pragma clang fp contract(off)

#include "sgmcmc_host.hpp"

using namespace sgmcmc_host;

namespace {

constexpr int CB_MAX_DRAWS = SGMCMC_CALIB_MAX_DRAWS;
constexpr int CB_MAX_LEVELS = SGMCMC_CALIB_MAX_LEVELS;
constexpr int CB_MAX_BINS = SGMCMC_CALIB_MAX_BINS;
constexpr int CB_MIN_PAD = 128;                           // the smallest padded count: one wave of chain pairs
constexpr int CB_MAX_BLOCK = 1024;
constexpr int CB_PARTS = 256;                             // partials of every sum
constexpr double CB_SQRT2 = 0x1.6a09e667f3bcdp+0;
constexpr double CB_INV_SQRTPI = 0x1.20dd750429b6dp-1;
constexpr double CB_DIAG = CB_SQRT2 * CB_INV_SQRTPI;      // A(0, c) = c * CB_DIAG; one rounding, as the statement writes it

// E|N(d, c^2)|
__device__ __forceinline__ double calib_A(double d, double c)
{
    const double e = c * CB_SQRT2;
    const double u = d / e;
    return e * (u * erf(u) + exp(-(u * u)) * CB_INV_SQRTPI);
}

// sum_{i < n} f(i) in the stated order by the whole workgroup (K19's): partial p by thread p (threads p, p + block, ... of a
// small workgroup), the tree in part[]. Every thread gets the total; ends behind a barrier, part free again.
template <typename F>
__device__ __forceinline__ double calib_block_sum(int n, double *part, F f)
{
    const int tid = (int)threadIdx.x, block = (int)blockDim.x;
    for (int p = tid; p < CB_PARTS; p += block) {
        double a = 0.0;
        for (int i = p; i < n; i += CB_PARTS) a += f(i);
        part[p] = a;
    }
    __syncthreads();
    for (int h = CB_PARTS / 2; h >= 1; h >>= 1) {
        for (int t = tid; t < h; t += block) part[t] += part[t + h];
        __syncthreads();
    }
    const double r = part[0];
    __syncthreads();
    return r;
}

template <typename T, int CAP>
__global__ void __launch_bounds__(CB_MAX_BLOCK)
calib_kernel(const T *__restrict__ means, size_t ld, int S, const double *__restrict__ var, const T *__restrict__ y,
             double *__restrict__ pit, double *__restrict__ crps)
{
    __shared__ double mu[CAP];
    __shared__ double vr[CAP];
    __shared__ double g[CAP];
    __shared__ double part[CB_PARTS];
    const int tid = (int)threadIdx.x, block = (int)blockDim.x;
    const size_t r = blockIdx.x;
    const T *col = means + r;

    for (int s = tid; s < S; s += block) {
        mu[s] = (double)col[(size_t)s * ld];
        vr[s] = var[s];
    }
    const double yy = (double)y[r];
    __syncthreads();

    const double P = calib_block_sum(S, part, [&](int s) {
        return 0.5 * erfc(-(((yy - mu[s]) / sqrt(vr[s])) / CB_SQRT2));
    });
    const double Tsum = calib_block_sum(S, part, [&](int s) { return calib_A(yy - mu[s], sqrt(vr[s])); });

    // ---- the chains: pair p is g_lo and g_hi with lo = p, hi = S - 1 - p; the middle draw of an odd S is a pair of one
    const int pairs = (S + 1) >> 1;
    for (int p = tid; p < pairs; p += block) {
        const int lo = p, hi = S - 1 - p;
        const double mlo = mu[lo], vlo = vr[lo], mhi = mu[hi], vhi = vr[hi];
        const int both = lo == hi ? 0 : lo;
        double alo = 0.0, ahi = 0.0;
        int t = 0;
        for (; t < both; ++t) {
            const double mt = mu[t], vt = vr[t];
            alo += calib_A(mlo - mt, sqrt(vlo + vt));
            ahi += calib_A(mhi - mt, sqrt(vhi + vt));
        }
        for (; t < hi; ++t) ahi += calib_A(mhi - mu[t], sqrt(vhi + vr[t]));
        g[lo] = alo;                                      // lo == hi: overwritten by the line below
        g[hi] = ahi;
    }
    __syncthreads();

    const double G = calib_block_sum(S, part, [&](int s) { return g[s]; });
    const double Dg = calib_block_sum(S, part, [&](int s) { return sqrt(vr[s] + vr[s]) * CB_DIAG; });
    if (tid == 0) {
        const double dS = (double)S;
        pit[r] = P / dS;
        crps[r] = Tsum / dS - ((G + G) + Dg) / (2.0 * dS * dS);
    }
}

struct CalibLevels {
    double v[CB_MAX_LEVELS];
};

// summary = { TREE crps, NaN rows, the rows in each central interval, the rows in each PIT bin }. Counts are integers, so
// their order of addition is free: one LDS column per thread, folded by the same tree.
__global__ void __launch_bounds__(CB_PARTS)
calib_summary_kernel(const double *__restrict__ pit, const double *__restrict__ crps, size_t n_rows, CalibLevels levels,
                     int n_levels, int n_bins, double *__restrict__ summary)
{
    __shared__ double part[CB_PARTS];
    __shared__ unsigned cnt[1 + CB_MAX_LEVELS + CB_MAX_BINS][CB_PARTS];
    __shared__ double lo[CB_MAX_LEVELS], hi[CB_MAX_LEVELS];
    const int tid = (int)threadIdx.x;
    const int n_cnt = 1 + n_levels + n_bins;
    for (int k = 0; k < n_cnt; ++k) cnt[k][tid] = 0u;
    if (tid < n_levels) {
        lo[tid] = 0.5 - 0.5 * levels.v[tid];
        hi[tid] = 0.5 + 0.5 * levels.v[tid];
    }
    __syncthreads();
    const double db = (double)n_bins;
    double c = 0.0;
    for (size_t r = tid; r < n_rows; r += CB_PARTS) {
        const double p = pit[r], v = crps[r];
        c += v;
        if (p != p || v != v) {
            cnt[0][tid] += 1u;
            continue;
        }
        for (int k = 0; k < n_levels; ++k)
            if (lo[k] <= p && p <= hi[k]) cnt[1 + k][tid] += 1u;
        if (n_bins > 0) {
            const double f = floor(p * db);
            // p lies in [0, 1] whenever it is no NaN; a negative index would be in no bin, and stays out of cnt
            if (f >= 0.0) cnt[1 + n_levels + (f >= db ? n_bins - 1 : (int)f)][tid] += 1u;
        }
    }
    part[tid] = c;
    __syncthreads();
    for (int h = CB_PARTS / 2; h >= 1; h >>= 1) {
        if (tid < h) {
            part[tid] += part[tid + h];
            for (int k = 0; k < n_cnt; ++k) cnt[k][tid] += cnt[k][tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) summary[0] = part[0];
    if (tid < n_cnt) summary[1 + tid] = (double)cnt[tid][0];
}

template <typename T>
int mixture_calibration(const T *means, size_t ld, size_t S, size_t n_rows, const double *var, const T *y, const double *levels,
                        int n_levels, int n_bins, double *pit, double *crps, double *summary, hipStream_t st)
{
    const char *who = "mixture_calibration";
    if (S < 1 || S > (size_t)CB_MAX_DRAWS) return fail(SGMCMC_EINVAL, "%s: S = %zu draws, must be 1 .. %d", who, S, CB_MAX_DRAWS);
    if (n_levels < 0 || n_levels > CB_MAX_LEVELS)
        return fail(SGMCMC_EINVAL, "%s: n_levels = %d, must be 0 .. %d", who, n_levels, CB_MAX_LEVELS);
    if (n_bins < 0 || n_bins > CB_MAX_BINS) return fail(SGMCMC_EINVAL, "%s: n_bins = %d, must be 0 .. %d", who, n_bins, CB_MAX_BINS);
    CalibLevels lv = {};
    if (levels)
        for (int k = 0; k < n_levels; ++k) {
            if (!(levels[k] > 0.0 && levels[k] < 1.0))
                return fail(SGMCMC_EINVAL, "%s: levels[%d] = %g, must lie in (0, 1)", who, k, levels[k]);
            lv.v[k] = levels[k];
        }
    if (n_rows == 0) return 0;
    const struct { const void *p; const char *name; } required[] = {
        {means, "means"}, {var, "var"}, {y, "y"}, {pit, "pit"}, {crps, "crps"}};
    for (const auto &arg : required)
        if (!arg.p) return fail(SGMCMC_EINVAL, "%s: %s is NULL", who, arg.name);
    if (!levels && n_levels > 0) return fail(SGMCMC_EINVAL, "%s: levels is NULL with n_levels = %d", who, n_levels);
    if (ld < n_rows) return fail(SGMCMC_EINVAL, "%s: ld = %zu is smaller than n_rows = %zu", who, ld, n_rows);
    size_t rows = 0, extent = 0;
    if (__builtin_mul_overflow(S - 1, ld, &rows) || __builtin_add_overflow(rows, n_rows, &extent)
        || extent > SIZE_MAX / sizeof(double))
        return fail(SGMCMC_EINVAL, "%s: means' extent overflows with S = %zu, ld = %zu", who, S, ld);
    if (n_rows > (size_t)INT32_MAX) return fail(SGMCMC_EINVAL, "%s: n_rows = %zu is too large for one launch", who, n_rows);

    int npad = CB_MIN_PAD;
    while (npad < (int)S) npad <<= 1;
    const int block = npad / 2 < CB_MAX_BLOCK ? npad / 2 : CB_MAX_BLOCK;
#define CALIB_LAUNCH(CAP)                                                                                                      \
    hipLaunchKernelGGL((calib_kernel<T, CAP>), dim3((unsigned)n_rows), dim3(block), 0, st, means, ld, (int)S, var, y, pit, crps)
    if (S <= 256) CALIB_LAUNCH(256);
    else if (S <= 1024) CALIB_LAUNCH(1024);
    else CALIB_LAUNCH(CB_MAX_DRAWS);
#undef CALIB_LAUNCH
    if (int rc = launched("calib_kernel")) return rc;
    if (summary) {
        hipLaunchKernelGGL(calib_summary_kernel, dim3(1), dim3(CB_PARTS), 0, st, static_cast<const double *>(pit),
                           static_cast<const double *>(crps), n_rows, lv, n_levels, n_bins, summary);
        if (int rc = launched("calib_summary_kernel")) return rc;
    }
    return 0;
}

}  // namespace

extern "C" {

int sgmcmc_calib_abi_version(void) { return SGMCMC_CALIB_ABI_VERSION; }

int sgmcmc_calib_max_draws(void) { return CB_MAX_DRAWS; }

int sgmcmc_mixture_calibration_f32(const float *means, size_t ld, size_t S, size_t n_rows, const double *var, const float *y,
                                   const double *levels, int n_levels, int n_bins, double *pit, double *crps, double *summary,
                                   sgmcmc_stream_t stream)
{
    return mixture_calibration(means, ld, S, n_rows, var, y, levels, n_levels, n_bins, pit, crps, summary,
                               static_cast<hipStream_t>(stream));
}

int sgmcmc_mixture_calibration_f64(const double *means, size_t ld, size_t S, size_t n_rows, const double *var, const double *y,
                                   const double *levels, int n_levels, int n_bins, double *pit, double *crps, double *summary,
                                   sgmcmc_stream_t stream)
{
    return mixture_calibration(means, ld, S, n_rows, var, y, levels, n_levels, n_bins, pit, crps, summary,
                               static_cast<hipStream_t>(stream));
}

}  // extern "C"
