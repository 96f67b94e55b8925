// sgmcmc_chain_diag.hip -- K12, R-hat and the effective sample size of EVERY parameter from one strided (m, n, P) device trace
// of up to 4096 chains: kernel and host side of sgmcmc_chain_diag_{f32,f64} and sgmcmc_chains_abi_version
// (include/sgmcmc_hip_chains.h, the many-chains diagnostics add-on outside the section 8(b) boundary). K10 (sgmcmc_ess.hip)
// gives one lane all m chains of its parameter and takes the chain pointers by value, which stops at 64 chains; the reference
// loops over the parameter dimensions on the host (pysgmcmc/diagnostics/sampler_diagnostics.py:12-82).
//
// Shape: a workgroup is 64 parameters x `waves` waves. Lane = parameter, so every global access is a coalesced row segment,
// as in K10; no contraction => no MFMA. The chains are cut into groups of 16 consecutive chains and wave w takes the groups
// w, w + waves, ... For every quantity that is summed over the chains (the means, the variances, the squared deviations of
// the means -- three quantities in turn, the trace read three or four times -- and the squared differences of each lag) a wave forms the GROUP sums of its groups, by K10's loops restricted to
// the group's chains, and stores them in an LDS table [n_groups][64]; after a barrier EVERY wave adds the whole column of its
// lane in ascending group order. The order is fixed by the groups, so the bits do not depend on `waves`, and every wave holds
// the same Vhat, the same rho_t, the same stop decision per parameter and the same "all 64 parameters have stopped" vote.
//
// Barriers are workgroup-uniform by construction: what decides the trip count of the lag loop and every branch around a
// barrier is computed by each wave from the LDS table and the kernel arguments alone -- never from a wave's own partial
// sums or its number of groups. A wave without groups (m = 17 with 16 waves) and the dead lanes of the last workgroup
// (p >= P) walk every barrier.
//
// The table is double-buffered when two copies fit the LDS (one barrier per reduction: a wave that writes buffer k ^ 1 for
// the next reduction has passed the barrier every reader of that buffer's previous contents arrived at after reading), and
// single otherwise (a second barrier after the reads). The slab of a workgroup does not fit the LDS at the sizes this is
// for (256 chains x 100 samples x 64 parameters x 4 B = 6.5 MB), so every lag re-reads global memory through the caches.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sgmcmc_hip_chains.h"

#pragma clang fp contract(off)

#include "sgmcmc_host.hpp"

using namespace sgmcmc_host;

namespace {

constexpr int CD_GROUP = 16;                              // chains per group: part of the arithmetic contract
constexpr int CD_LANES = 64;                              // parameters per workgroup = lanes of a wave
constexpr int CD_MAX_WAVES = 16;
constexpr size_t CD_LDS_MAX = (size_t)160 * 1024;         // LDS of one CU (gfx950)

// The lane's column of the group-sum table. put() stores a group sum of one of the wave's own groups; sum() is called by
// EVERY thread of the workgroup the same number of times and returns the column's total in ascending group order.
struct GroupTable {
    double *col;                                          // current buffer + lane
    int other;                                            // doubles from the current buffer to the other one; 0 = one buffer
    int n_groups;
    __device__ __forceinline__ void put(int g, double v) const { col[g * CD_LANES] = v; }
    __device__ __forceinline__ void put_other(int g, double v) const { col[other + g * CD_LANES] = v; }   // two buffers only
    __device__ __forceinline__ double sum()
    {
        __syncthreads();
        double s = 0.0;
        for (int g = 0; g < n_groups; ++g) s += col[g * CD_LANES];
        if (other == 0) {
            __syncthreads();                              // `other` is a kernel argument: uniform
        } else {
            col += other;
            other = -other;
        }
        return s;
    }
};

// sum_i (x[i] - x0) and sum_i ((x[i] - x0) - mean)^2 of one chain of the lane's column, i ascending as in K10. The loads of
// eight rows are issued before the first of them is added: the adds form one dependent chain either way, and a wave that
// waits for every load before it issues the next one leaves the memory system idle.
constexpr int CD_ROWS = 8;

template <typename T>
__device__ __forceinline__ double shifted_sum(const T *__restrict__ b, unsigned n, size_t ld, double x0)
{
    double s = 0.0;
    unsigned i = 0;
    for (; i + CD_ROWS <= n; i += CD_ROWS) {
        T v[CD_ROWS];
#pragma unroll
        for (int k = 0; k < CD_ROWS; ++k) v[k] = b[(size_t)(i + k) * ld];
#pragma unroll
        for (int k = 0; k < CD_ROWS; ++k) s += (double)v[k] - x0;
    }
    for (; i < n; ++i) s += (double)b[(size_t)i * ld] - x0;
    return s;
}

template <typename T>
__device__ __forceinline__ double shifted_squares(const T *__restrict__ b, unsigned n, size_t ld, double x0, double mean)
{
    double q = 0.0;
    unsigned i = 0;
    for (; i + CD_ROWS <= n; i += CD_ROWS) {
        T v[CD_ROWS];
#pragma unroll
        for (int k = 0; k < CD_ROWS; ++k) v[k] = b[(size_t)(i + k) * ld];
#pragma unroll
        for (int k = 0; k < CD_ROWS; ++k) {
            const double d = ((double)v[k] - x0) - mean;
            q += d * d;
        }
    }
    for (; i < n; ++i) {
        const double d = ((double)b[(size_t)i * ld] - x0) - mean;
        q += d * d;
    }
    return q;
}

template <typename T>
__global__ void __launch_bounds__(CD_LANES *CD_MAX_WAVES)
    chain_diag_kernel(const T *__restrict__ trace, int m, unsigned n, size_t P, size_t ld, size_t chain_stride,
                      double *__restrict__ rhat, long long *__restrict__ ess, double *__restrict__ raw,
                      int *__restrict__ stop_lag, int n_groups, int two_buffers, int walk_lags)
{
    extern __shared__ __align__(16) unsigned char chain_diag_lds[];
    const int w = (int)threadIdx.y, waves = (int)blockDim.y;
    const size_t p = (size_t)blockIdx.x * CD_LANES + threadIdx.x;
    const bool live = p < P;
    const T *__restrict__ x = trace + (live ? p : 0);     // dead lanes load nothing; they only walk the barriers
    GroupTable tab{reinterpret_cast<double *>(chain_diag_lds) + threadIdx.x, two_buffers ? n_groups * CD_LANES : 0, n_groups};
    const double dn = (double)n;
    const double x0 = live ? (double)x[0] : 0.0;

    // chain means, shifted by x0: sum over the chains
    for (int g = w; g < n_groups; g += waves) {
        double mean_sum = 0.0;
        if (live) {
            const int c1 = min(m, (g + 1) * CD_GROUP);
            for (int c = g * CD_GROUP; c < c1; ++c) {
                mean_sum += shifted_sum(x + (size_t)c * chain_stride, n, ld, x0) / dn;
            }
        }
        tab.put(g, mean_sum);
    }
    const double mean_sum = tab.sum();
    // Unbiased chain variances (two passes per chain) and, for B, the squared deviations of the chain means from the grand
    // mean. With two table buffers both group sums come from ONE walk over the chains (a chain's mean serves both) and are
    // reduced side by side -- three barriers, once; with one buffer they take a walk each and the means are formed again,
    // as in K10. The same operations on the same values in the same order either way.
    const double grand = mean_sum / (double)m;
    double var_sum = 0.0, dev_sum = 0.0;
    if (two_buffers) {                                    // a kernel argument: uniform
        __syncthreads();                                  // every wave has read the means out of what is now the other buffer
        for (int g = w; g < n_groups; g += waves) {
            double v = 0.0, q = 0.0;
            if (live) {
                const int c1 = min(m, (g + 1) * CD_GROUP);
                for (int c = g * CD_GROUP; c < c1; ++c) {
                    const T *__restrict__ b = x + (size_t)c * chain_stride;
                    const double mean = shifted_sum(b, n, ld, x0) / dn;
                    v += shifted_squares(b, n, ld, x0, mean) / (dn - 1.0);
                    const double d = mean - grand;
                    q += d * d;
                }
            }
            tab.put(g, v);
            tab.put_other(g, q);
        }
        __syncthreads();
        for (int g = 0; g < n_groups; ++g) var_sum += tab.col[g * CD_LANES];
        for (int g = 0; g < n_groups; ++g) dev_sum += tab.col[tab.other + g * CD_LANES];
        __syncthreads();                                  // both buffers are free for the lags
    } else {
        for (int g = w; g < n_groups; g += waves) {
            double v = 0.0;
            if (live) {
                const int c1 = min(m, (g + 1) * CD_GROUP);
                for (int c = g * CD_GROUP; c < c1; ++c) {
                    const T *__restrict__ b = x + (size_t)c * chain_stride;
                    const double mean = shifted_sum(b, n, ld, x0) / dn;
                    v += shifted_squares(b, n, ld, x0, mean) / (dn - 1.0);
                }
            }
            tab.put(g, v);
        }
        var_sum = tab.sum();
        for (int g = w; g < n_groups; g += waves) {
            double q = 0.0;
            if (live) {
                const int c1 = min(m, (g + 1) * CD_GROUP);
                for (int c = g * CD_GROUP; c < c1; ++c) {
                    const double d = shifted_sum(x + (size_t)c * chain_stride, n, ld, x0) / dn - grand;
                    q += d * d;
                }
            }
            tab.put(g, q);
        }
        dev_sum = tab.sum();
    }
    const double B = m > 1 ? dn * (dev_sum / (double)(m - 1)) : 0.0;
    const double W = var_sum / (double)m;
    const double vhat = W * (dn - 1.0) / dn + B / dn;
    const bool ok = live && vhat != 0.0 && isfinite(vhat);
    if (rhat && live && w == 0) rhat[p] = ok ? sqrt(vhat / W) : __builtin_nan("");
    if (!walk_lags) return;                               // a kernel argument: every wave leaves here or none does

    int stop = ok ? (int)n : 1;
    bool active = ok;                                     // from the table and the arguments alone: the same in every wave
    double rho_sum = 0.0, prev = 1.0;
    const double two_vhat = 2.0 * vhat;
    for (unsigned t = 1; t < n; ++t) {
        if (__ballot(active) == 0) break;                 // all 64 parameters have stopped -- in every wave alike
        const unsigned cnt = n - t;
        for (int g = w; g < n_groups; g += waves) {
            if (active) {
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
                const int c1 = min(m, (g + 1) * CD_GROUP);
                for (int c = g * CD_GROUP; c < c1; ++c) {
                    const T *__restrict__ b = x + (size_t)c * chain_stride;
                    const T *__restrict__ bt = b + (size_t)t * ld;
                    unsigned i = 0;
                    for (; i + 4 <= cnt; i += 4) {
                        const double d0 = (double)bt[(size_t)i * ld] - (double)b[(size_t)i * ld];
                        const double d1 = (double)bt[(size_t)(i + 1) * ld] - (double)b[(size_t)(i + 1) * ld];
                        const double d2 = (double)bt[(size_t)(i + 2) * ld] - (double)b[(size_t)(i + 2) * ld];
                        const double d3 = (double)bt[(size_t)(i + 3) * ld] - (double)b[(size_t)(i + 3) * ld];
                        a0 += d0 * d0;
                        a1 += d1 * d1;
                        a2 += d2 * d2;
                        a3 += d3 * d3;
                    }
                    for (; i < cnt; ++i) {
                        const double d = (double)bt[(size_t)i * ld] - (double)b[(size_t)i * ld];
                        a0 += d * d;
                    }
                }
                tab.put(g, (a0 + a1) + (a2 + a3));
            }
        }
        const double s = tab.sum();                       // stopped lanes add what their column happens to hold and drop it
        if (active) {
            const double rho = 1.0 - s / (two_vhat * ((double)m * (double)cnt));   // the one division of the lag
            rho_sum += rho;
            if ((t & 1u) == 0 && prev + rho < 0.0) {
                stop = (int)(t + 1);
                active = false;
            }
            prev = rho;
        }
    }
    if (live && w == 0) {
        const double r = ok ? ((double)m * dn) / (1.0 + 2.0 * rho_sum) : __builtin_nan("");
        if (ess) ess[p] = (isfinite(r) && fabs(r) < 9.2e18) ? (long long)r : 0ll;
        if (raw) raw[p] = r;
        if (stop_lag) stop_lag[p] = stop;
    }
}

// the largest of 1, 2, 4, 8, 16 that exceeds neither the group count nor what keeps the whole grid resident at once
int auto_waves(int n_groups, size_t blocks)
{
    int cus = current_device_cus();
    if (cus <= 0) cus = 256;
    const size_t slots = (size_t)32 * (size_t)cus;        // 8 waves on each of a CU's 4 SIMDs
    int waves = CD_MAX_WAVES;
    while (waves > 1 && (waves > n_groups || blocks * (size_t)waves > slots)) waves >>= 1;
    return waves;
}

template <typename T>
int chain_diag(const T *trace, int m, size_t n, size_t P, size_t ld, size_t chain_stride, double *rhat, int64_t *ess,
               double *raw, int32_t *stop_lag, int waves, hipStream_t st)
{
    if (P == 0) return 0;
    if (m < 1 || m > SGMCMC_CHAINS_MAX_CHAINS)
        return fail(SGMCMC_EINVAL, "chain_diag: m = %d chains, must be 1 .. %d", m, SGMCMC_CHAINS_MAX_CHAINS);
    if (n < 2 || n > (size_t)INT32_MAX) return fail(SGMCMC_EINVAL, "chain_diag: n = %zu samples, must be 2 .. 2^31 - 1", n);
    if (ld < P) return fail(SGMCMC_EINVAL, "chain_diag: ld = %zu is smaller than P = %zu", ld, P);
    size_t rows = 0, need = 0, last = 0, extent = 0;
    if (__builtin_mul_overflow(n - 1, ld, &rows) || __builtin_add_overflow(rows, P, &need))
        return fail(SGMCMC_EINVAL, "chain_diag: (n - 1) * ld + P overflows with n = %zu, ld = %zu", n, ld);
    if (chain_stride < need)
        return fail(SGMCMC_EINVAL, "chain_diag: chain_stride = %zu is smaller than (n - 1) * ld + P = %zu", chain_stride, need);
    if (__builtin_mul_overflow((size_t)(m - 1), chain_stride, &last) || __builtin_add_overflow(last, need, &extent)
        || extent > SIZE_MAX / sizeof(T))
        return fail(SGMCMC_EINVAL, "chain_diag: the trace's extent overflows with m = %d, chain_stride = %zu", m, chain_stride);
    if (!trace) return fail(SGMCMC_EINVAL, "chain_diag: trace must be non-NULL");
    if (!rhat && !ess && !raw && !stop_lag)
        return fail(SGMCMC_EINVAL, "chain_diag: at least one of rhat, ess, raw and stop_lag must be non-NULL");
    if (waves != 0 && waves != 1 && waves != 2 && waves != 4 && waves != 8 && waves != 16)
        return fail(SGMCMC_EINVAL, "chain_diag: waves = %d, must be 0 (auto), 1, 2, 4, 8 or 16", waves);
    const size_t blocks = (P + CD_LANES - 1) / CD_LANES;
    if (blocks > (size_t)INT32_MAX) return fail(SGMCMC_EINVAL, "chain_diag: P = %zu is too large for one launch", P);
    const int n_groups = (m + CD_GROUP - 1) / CD_GROUP;     // <= 256
    if (waves == 0) waves = auto_waves(n_groups, blocks);
    const size_t table = (size_t)n_groups * CD_LANES * sizeof(double);   // <= 128 KiB
    const int two_buffers = 2 * table <= CD_LDS_MAX;
    const size_t lds_bytes = two_buffers ? 2 * table : table;
    auto kern = chain_diag_kernel<T>;
    if (lds_bytes > 64 * 1024) {
        hipError_t e0 = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)lds_bytes);
        if (e0 != hipSuccess) return hip_fail(e0, "hipFuncSetAttribute(chain_diag_kernel)");
    }
    const int walk_lags = ess || raw || stop_lag;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(CD_LANES, (unsigned)waves), lds_bytes, st, trace, m, (unsigned)n, P, ld,
                       chain_stride, rhat, reinterpret_cast<long long *>(ess), raw, stop_lag, n_groups, two_buffers, walk_lags);
    return launched("chain_diag");
}

}  // namespace

extern "C" {

int sgmcmc_chains_abi_version(void) { return SGMCMC_CHAINS_ABI_VERSION; }

int sgmcmc_chain_diag_f32(const float *trace, int m, size_t n, size_t P, size_t ld, size_t chain_stride, double *rhat,
                          int64_t *ess, double *raw, int32_t *stop_lag, int waves, sgmcmc_stream_t stream)
{
    return chain_diag<float>(trace, m, n, P, ld, chain_stride, rhat, ess, raw, stop_lag, waves, static_cast<hipStream_t>(stream));
}
int sgmcmc_chain_diag_f64(const double *trace, int m, size_t n, size_t P, size_t ld, size_t chain_stride, double *rhat,
                          int64_t *ess, double *raw, int32_t *stop_lag, int waves, sgmcmc_stream_t stream)
{
    return chain_diag<double>(trace, m, n, P, ld, chain_stride, rhat, ess, raw, stop_lag, waves, static_cast<hipStream_t>(stream));
}

}  // extern "C"
