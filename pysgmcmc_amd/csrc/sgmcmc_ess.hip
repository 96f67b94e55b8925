// sgmcmc_ess.hip -- K10, the effective sample size of EVERY parameter from device-resident traces: kernel and host side of
// sgmcmc_ess_variogram_{f32,f64} and sgmcmc_diag_abi_version (include/sgmcmc_hip_diag.h, the diagnostics add-on outside the
// section 8(b) boundary). The reference gets there by a host loop over the parameter dimensions
// (pysgmcmc/diagnostics/sampler_diagnostics.py:47-82, pymc3 3.1's variogram estimate).
//
// Shape: parameters are independent and contiguous along a row of a trace, so lane = parameter and every global access
// is a coalesced row segment; no contraction => no MFMA. A lane walks the lags of its own parameter until its stop rule
// fires; a wave goes on while any of its lanes is active, the others skip the accumulation. The slab a workgroup needs
// (m chains x n samples x block_threads parameters) is either staged in the LDS once -- every lane reads back only the
// column it wrote itself, lane-contiguous and hence conflict-free, so no barrier is needed -- or re-read from global
// memory lag by lag. Both go through the same arithmetic (ess_column, fp contraction off), so they give the same bits,
// and since one lane sums one parameter in a fixed order the result cannot depend on the launch geometry either.
#include <cmath>
#include <cstdint>

#include "sgmcmc_stream.hpp"

#include "sgmcmc_hip_diag.h"

namespace {

constexpr size_t ESS_LDS_MAX = (size_t)160 * 1024;      // LDS of one CU (gfx950)

template <typename T>
struct EssChains {
    const T *p[SGMCMC_ESS_MAX_CHAINS];                    // by value in the kernel arguments: no device-side pointer table
};

// element (c, i) of the lane's own column; chain c selected first (its pointer is wave-uniform)
template <typename T>
struct EssGlobalColumn {
    const EssChains<T> &ch;
    size_t ld, col;
    __device__ __forceinline__ const T *chain(int c) const { return ch.p[c] + col; }
    __device__ __forceinline__ double at(const T *base, unsigned i) const { return (double)base[(size_t)i * ld]; }
};
template <typename T>
struct EssLdsColumn {
    const T *slab;                                        // + threadIdx.x already
    unsigned n, bt;
    __device__ __forceinline__ const T *chain(int c) const { return slab + (size_t)c * n * bt; }
    __device__ __forceinline__ double at(const T *base, unsigned i) const { return (double)base[i * bt]; }
};

struct EssResult {
    double raw;
    long long ess;
    int stop_lag;
};

// One parameter, one lane. `live` = the lane owns a parameter; dead lanes only take part in the wave votes.
template <typename Col>
__device__ __forceinline__ EssResult ess_column(const Col &x, int m, unsigned n, bool live)
{
    const double dn = (double)n;
    double vhat = 0.0;
    if (live) {
        // chain means and unbiased variances (two passes per chain), all on samples shifted by the column's first one:
        // variances and B do not see a common shift, a column of equal samples gives Vhat = 0 EXACTLY whatever its
        // value (sum of n copies of 0.1 / n is not 0.1), and a large offset costs no digits
        const double x0 = x.at(x.chain(0), 0);
        double mean_sum = 0.0, var_sum = 0.0;
        for (int c = 0; c < m; ++c) {
            const auto *b = x.chain(c);
            double s = 0.0;
            for (unsigned i = 0; i < n; ++i) s += x.at(b, i) - x0;
            const double mean = s / dn;
            double q = 0.0;
            for (unsigned i = 0; i < n; ++i) {
                const double d = (x.at(b, i) - x0) - mean;
                q += d * d;
            }
            mean_sum += mean;
            var_sum += q / (dn - 1.0);
        }
        double B = 0.0;
        if (m > 1) {
            const double grand = mean_sum / (double)m;
            double q = 0.0;
            for (int c = 0; c < m; ++c) {                 // the means again (m * n adds) rather than 64 doubles of scratch
                const auto *b = x.chain(c);
                double s = 0.0;
                for (unsigned i = 0; i < n; ++i) s += x.at(b, i) - x0;
                const double d = s / dn - grand;
                q += d * d;
            }
            B = dn * (q / (double)(m - 1));
        }
        const double W = var_sum / (double)m;
        vhat = W * (dn - 1.0) / dn + B / dn;
    }
    const bool ok = live && vhat != 0.0 && isfinite(vhat);
    EssResult r;
    r.stop_lag = ok ? (int)n : 1;
    bool active = ok;
    double rho_sum = 0.0, prev = 1.0;
    const double two_vhat = 2.0 * vhat;
    for (unsigned t = 1; t < n; ++t) {
        if (__ballot(active) == 0) break;                 // wave-uniform: every lane of the wave has stopped
        if (active) {
            const unsigned cnt = n - t;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            for (int c = 0; c < m; ++c) {
                const auto *b = x.chain(c);
                unsigned i = 0;
                for (; i + 4 <= cnt; i += 4) {
                    const double d0 = x.at(b, i + t) - x.at(b, i);
                    const double d1 = x.at(b, i + 1 + t) - x.at(b, i + 1);
                    const double d2 = x.at(b, i + 2 + t) - x.at(b, i + 2);
                    const double d3 = x.at(b, i + 3 + t) - x.at(b, i + 3);
                    a0 += d0 * d0;
                    a1 += d1 * d1;
                    a2 += d2 * d2;
                    a3 += d3 * d3;
                }
                for (; i < cnt; ++i) {
                    const double d = x.at(b, i + t) - x.at(b, i);
                    a0 += d * d;
                }
            }
            const double s = (a0 + a1) + (a2 + a3);
            const double rho = 1.0 - s / (two_vhat * ((double)m * (double)cnt));   // the one division of the lag
            rho_sum += rho;
            if ((t & 1u) == 0 && prev + rho < 0.0) {
                r.stop_lag = (int)(t + 1);
                active = false;
            }
            prev = rho;
        }
    }
    r.raw = ok ? ((double)m * dn) / (1.0 + 2.0 * rho_sum) : __builtin_nan("");
    r.ess = (isfinite(r.raw) && fabs(r.raw) < 9.2e18) ? (long long)r.raw : 0ll;
    return r;
}

template <typename T, bool LDS>
__global__ void __launch_bounds__(256) ess_variogram_kernel(const EssChains<T> ch, int m, unsigned n, size_t P, size_t ld,
                                                            long long *__restrict__ ess, double *__restrict__ raw,
                                                            int *__restrict__ stop_lag)
{
    extern __shared__ __align__(16) unsigned char ess_lds_raw[];
    const unsigned bt = blockDim.x;
    const size_t p = (size_t)blockIdx.x * bt + threadIdx.x;
    const bool live = p < P;
    EssResult r;
    if (LDS) {
        T *slab = reinterpret_cast<T *>(ess_lds_raw) + threadIdx.x;
        if (live) {
            for (int c = 0; c < m; ++c) {
                const T *__restrict__ src = ch.p[c] + p;
                T *dst = slab + (size_t)c * n * bt;
#pragma unroll 8
                for (unsigned i = 0; i < n; ++i) dst[i * bt] = src[(size_t)i * ld];
            }
        }
        r = ess_column(EssLdsColumn<T>{slab, n, bt}, m, n, live);
    } else {
        r = ess_column(EssGlobalColumn<T>{ch, ld, live ? p : 0}, m, n, live);
    }
    if (live) {
        ess[p] = r.ess;
        if (raw) raw[p] = r.raw;
        if (stop_lag) stop_lag[p] = r.stop_lag;
    }
}

template <typename T, bool LDS>
int ess_launch(const EssChains<T> &ch, int m, size_t n, size_t P, size_t ld, int64_t *ess, double *raw, int32_t *stop_lag,
               int bt, size_t lds_bytes, const LaunchCfg &cfg, hipStream_t st)
{
    auto kern = ess_variogram_kernel<T, LDS>;
    if (lds_bytes > 64 * 1024) {
        hipError_t e0 = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)lds_bytes);
        if (e0 != hipSuccess) return hip_fail(e0, "hipFuncSetAttribute(ess_variogram_kernel)");
    }
    const dim3 grid((unsigned)((P + (size_t)bt - 1) / (size_t)bt)), block((unsigned)bt);
    long long *ess_ll = reinterpret_cast<long long *>(ess);
    if (cfg.ev0 != nullptr || cfg.ev1 != nullptr)
        hipExtLaunchKernelGGL(kern, grid, block, lds_bytes, st, cfg.ev0, cfg.ev1, 0, ch, m, (unsigned)n, P, ld, ess_ll, raw, stop_lag);
    else
        hipLaunchKernelGGL(kern, grid, block, lds_bytes, st, ch, m, (unsigned)n, P, ld, ess_ll, raw, stop_lag);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, "launch ess_variogram");
}

template <typename T>
int ess_variogram(const T *const *chains, int m, size_t n, size_t P, size_t ld, int64_t *ess, double *raw, int32_t *stop_lag,
                  int staging, const sgmcmc_launch_t *lc, hipStream_t st)
{
    if (P == 0) return 0;
    if (m < 1 || m > SGMCMC_ESS_MAX_CHAINS)
        return fail(SGMCMC_EINVAL, "ess_variogram: m = %d chains, must be 1 .. %d", m, SGMCMC_ESS_MAX_CHAINS);
    if (n < 2 || n > (size_t)INT32_MAX) return fail(SGMCMC_EINVAL, "ess_variogram: n = %zu samples, must be 2 .. 2^31 - 1", n);
    if (ld < P) return fail(SGMCMC_EINVAL, "ess_variogram: ld = %zu is smaller than P = %zu", ld, P);
    if (!chains || !ess) return fail(SGMCMC_EINVAL, "ess_variogram: chains and ess must be non-NULL");
    if ((P + 63) / 64 > (size_t)INT32_MAX) return fail(SGMCMC_EINVAL, "ess_variogram: P = %zu is too large for one launch", P);
    EssChains<T> ch;
    for (int c = 0; c < SGMCMC_ESS_MAX_CHAINS; ++c) {
        ch.p[c] = c < m ? chains[c] : nullptr;
        if (c < m && !ch.p[c]) return fail(SGMCMC_EINVAL, "ess_variogram: chains[%d] is NULL", c);
    }
    if (staging != SGMCMC_ESS_STAGING_AUTO && staging != SGMCMC_ESS_STAGING_LDS && staging != SGMCMC_ESS_STAGING_GLOBAL)
        return fail(SGMCMC_EINVAL, "ess_variogram: staging must be SGMCMC_ESS_STAGING_AUTO, _LDS or _GLOBAL");
    LaunchCfg cfg;
    if (int rc = resolve_launch(lc, cfg)) return rc;
    const int bt = cfg.block_threads > 0 ? cfg.block_threads : 64;
    // m <= 64, n < 2^31, bt <= 256, sizeof(T) <= 8: no overflow in 64 bits
    const size_t slab = (size_t)m * n * (size_t)bt * sizeof(T);
    bool lds = slab <= ESS_LDS_MAX;
    if (staging == SGMCMC_ESS_STAGING_LDS && !lds)
        return fail(SGMCMC_EINVAL, "ess_variogram: the slab of %d x %zu x %d elements (%zu B) does not fit the LDS (%zu B)", m, n, bt,
                    slab, ESS_LDS_MAX);
    if (staging == SGMCMC_ESS_STAGING_GLOBAL) lds = false;
    return lds ? ess_launch<T, true>(ch, m, n, P, ld, ess, raw, stop_lag, bt, slab, cfg, st)
               : ess_launch<T, false>(ch, m, n, P, ld, ess, raw, stop_lag, bt, 0, cfg, st);
}

}  // namespace

extern "C" {

int sgmcmc_diag_abi_version(void) { return SGMCMC_DIAG_ABI_VERSION; }

int sgmcmc_ess_variogram_f32(const float *const *chains, int m, size_t n, size_t P, size_t ld, int64_t *ess, double *raw,
                             int32_t *stop_lag, int staging, const sgmcmc_launch_t *launch, sgmcmc_stream_t stream)
{
    return ess_variogram<float>(chains, m, n, P, ld, ess, raw, stop_lag, staging, launch, static_cast<hipStream_t>(stream));
}
int sgmcmc_ess_variogram_f64(const double *const *chains, int m, size_t n, size_t P, size_t ld, int64_t *ess, double *raw,
                             int32_t *stop_lag, int staging, const sgmcmc_launch_t *launch, sgmcmc_stream_t stream)
{
    return ess_variogram<double>(chains, m, n, P, ld, ess, raw, stop_lag, staging, launch, static_cast<hipStream_t>(stream));
}

}  // extern "C"
