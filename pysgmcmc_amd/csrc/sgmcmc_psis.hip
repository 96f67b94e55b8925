// sgmcmc_psis.hip -- K19: Pareto-smoothed importance-sampling leave-one-out of an (S, n_rows) device matrix of pointwise log
// densities, behind include/sgmcmc_hip_psis.h (the statements are there; the numbers below are its steps).
//
// One launch, grid = n_rows, one workgroup per observation column, npad / 2 threads (64 .. 1024), then a 256-lane launch for
// the totals. The LDS is static, in three capacity classes (1024, 4096, 8192 slots of 12 bytes), as in K18.
//   9. row_lppd   the column is read once for the finite check and the two maxima, a second time as exp(l - m) into the LDS;
//                 lane 0 adds them one by one (K13's order, so K13's bits)
//   1. - 3.       a third read puts lw = -l - max(-l) next to its draw index; K18's bitonic sort on (value, index); pos[] is
//                 the inverse permutation, so a sum in DRAW order reads keys[pos[s]]. The tail is the end of the sorted
//                 image; its start is found by the M threads that look at one neighbour pair each
//   5.            x overwrites the tail in place; each wave takes grid points j = wave, wave + waves, ...: a lane holds
//                 partials lane, lane + 64, lane + 128, lane + 192 in registers, folds 128 and 64 in registers and 32 .. 1 by
//                 shuffles -- the stated tree without a barrier. The smoothed tail (or, for a non-finite khat, the tail
//                 recomputed from the column) then overwrites x
//   6. - 8.       in place in the sorted image; the sums over the draws by 256 threads, a chain of S / 256 terms each
// No atomics, no scratch buffer, nothing waited on but the workgroup's own barriers.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "sgmcmc_hip_psis.h"

#pragma clang fp contract(off)

#include "sgmcmc_host.hpp"

using namespace sgmcmc_host;

namespace {

constexpr int PS_MAX_DRAWS = SGMCMC_PSIS_MAX_DRAWS;
constexpr int PS_MIN_PAD = 128;                           // the smallest padded count: one wave of pairs
constexpr int PS_MAX_BLOCK = 1024;
constexpr int PS_PARTS = 256;                             // partials of every sum
constexpr int PS_MAX_GRID = 72;                           // 30 + floor(sqrt(ceil(0.2 * 8192))) = 70 grid points at most
constexpr int PS_WAVE = 64;
constexpr double PS_LOG_DBL_MIN = -0x1.6232bdd7abcd2p+9;  // log(DBL_MIN) as a constant: tail membership is exact

// ascending bitonic sort of keys[0 .. npad) with idx as the tie-breaker and payload (K18's); ends behind a barrier
__device__ __forceinline__ void psis_sort(double *keys, uint16_t *idx, int npad)
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

// fmax over the workgroup of every thread's v; red holds one slot per wave. Ends behind a barrier, red free again.
__device__ __forceinline__ double psis_block_fmax(double v, double *red)
{
    for (int off = PS_WAVE / 2; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    const int waves = (int)blockDim.x / PS_WAVE;
    if (((int)threadIdx.x & (PS_WAVE - 1)) == 0) red[(int)threadIdx.x / PS_WAVE] = v;
    __syncthreads();
    double r = red[0];
    for (int w = 1; w < waves; ++w) r = fmax(r, red[w]);
    __syncthreads();
    return r;
}

// sum_{i < n} f(i) in the stated order by the whole workgroup: partial p by thread p (threads p, p + block, ... of a small
// workgroup), the tree in part[]. Every thread gets the total; ends behind a barrier, part free again.
template <typename F>
__device__ __forceinline__ double psis_block_sum(int n, double *part, F f)
{
    const int tid = (int)threadIdx.x, block = (int)blockDim.x;
    for (int p = tid; p < PS_PARTS; p += block) {
        double a = 0.0;
        for (int i = p; i < n; i += PS_PARTS) a += f(i);
        part[p] = a;
    }
    __syncthreads();
    for (int h = PS_PARTS / 2; h >= 1; h >>= 1) {
        for (int t = tid; t < h; t += block) part[t] += part[t + h];
        __syncthreads();
    }
    const double r = part[0];
    __syncthreads();
    return r;
}

// the same sum by ONE wave, every lane of it in the call: lane t holds partials t, t + 64, t + 128, t + 192, so h = 128 and
// h = 64 of the tree are register adds and h = 32 .. 1 shuffles (lanes >= h add what is not read again). Every lane gets the
// total.
template <typename F>
__device__ __forceinline__ double psis_wave_sum(int n, F f)
{
    const int lane = (int)threadIdx.x & (PS_WAVE - 1);
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
    for (int i = lane; i < n; i += PS_PARTS) {
        p0 += f(i);
        if (i + 64 < n) p1 += f(i + 64);
        if (i + 128 < n) p2 += f(i + 128);
        if (i + 192 < n) p3 += f(i + 192);
    }
    p0 += p2;
    p1 += p3;
    p0 += p1;
    for (int h = PS_WAVE / 2; h >= 1; h >>= 1) p0 += __shfl_down(p0, h);
    return __shfl(p0, 0);
}

template <int CAP>
__global__ void __launch_bounds__(PS_MAX_BLOCK)
psis_loo_kernel(const double *__restrict__ loglik, size_t ld, int S, int M, int npad, double *__restrict__ elpd_loo,
                double *__restrict__ khat_out, int *__restrict__ n_tail_out, double *__restrict__ row_lppd,
                double *__restrict__ log_weights, size_t ld_w)
{
    __shared__ double keys[CAP];
    __shared__ uint16_t idx[CAP];
    __shared__ uint16_t pos[CAP];
    __shared__ double part[PS_PARTS];
    __shared__ double gb[PS_MAX_GRID], gL[PS_MAX_GRID], gw[PS_MAX_GRID];
    __shared__ double red[PS_MAX_BLOCK / PS_WAVE];
    __shared__ double s_lppd;
    __shared__ int s_t0;
    const int tid = (int)threadIdx.x, block = (int)blockDim.x;
    const int wave = tid / PS_WAVE, waves = block / PS_WAVE;
    const size_t r = blockIdx.x;
    const double *col = loglik + r;

    // ---- the finite check, m = max l and max lr = max(-l)
    int bad = 0;
    double lmax = -INFINITY, lrmax = -INFINITY;
    for (int j = tid; j < S; j += block) {
        const double v = col[(size_t)j * ld];
        bad |= !isfinite(v);
        lmax = fmax(lmax, v);
        lrmax = fmax(lrmax, -v);
    }
    if (tid == 0) s_t0 = S;
    bad = __syncthreads_or(bad);
    if (bad) {
        const double nan = __builtin_nan("");
        if (tid == 0) {
            elpd_loo[r] = nan;
            khat_out[r] = nan;
            n_tail_out[r] = -1;
            if (row_lppd) row_lppd[r] = nan;
        }
        if (log_weights)
            for (int j = tid; j < S; j += block) log_weights[(size_t)j * ld_w + r] = nan;
        return;
    }
    const double m = psis_block_fmax(lmax, red);
    const double maxlr = psis_block_fmax(lrmax, red);

    // ---- 9. row_lppd: K13's second pass, one chain in draw order
    if (row_lppd) {
        for (int j = tid; j < S; j += block) keys[j] = exp(col[(size_t)j * ld] - m);
        __syncthreads();
        if (tid == 0) {
            double Z = 0.0;
            for (int s = 0; s < S; ++s) Z += keys[s];
            s_lppd = (m + log(Z)) - log((double)S);
        }
        __syncthreads();                                  // keys is written again below
    }

    // ---- 1. and 3. lw next to its draw index, sorted; the inverse permutation
    for (int j = tid; j < npad; j += block) {
        keys[j] = j < S ? (-col[(size_t)j * ld]) - maxlr : INFINITY;
        idx[j] = (uint16_t)j;
    }
    __syncthreads();
    psis_sort(keys, idx, npad);
    for (int k = tid; k < S; k += block) pos[idx[k]] = (uint16_t)k;
    const double cut = fmax(keys[S - M - 1], PS_LOG_DBL_MIN);
    for (int k = S - M + tid; k < S; k += block)          // k - 1 >= S - M - 1 >= 0; at most one k sees the seam
        if (keys[k] > cut && !(keys[k - 1] > cut)) s_t0 = k;
    __syncthreads();
    const int t0 = s_t0, n = S - t0;
    double *x = keys + t0;

    // ---- 4. and 5. the generalised Pareto fit and the smoothed tail
    double khat = INFINITY;
    if (n > 4) {
        const double ec = exp(cut), dn = (double)n;
        for (int i = tid; i < n; i += block) x[i] = exp(x[i]) - ec;
        __syncthreads();
        int root = 0;
        while ((root + 1) * (root + 1) <= n) ++root;
        const int G = 30 + root;
        const int q = (int)floor(dn / 4.0 + 0.5) - 1;
        const double xq3 = 3.0 * x[q], xinv = 1.0 / x[n - 1], dG = (double)G;
        for (int j = wave; j < G; j += waves) {
            const double bj = (1.0 - sqrt(dG / ((double)(j + 1) - 0.5))) / xq3 + xinv;
            const double nb = -bj;
            const double kj = psis_wave_sum(n, [&](int i) { return log1p(nb * x[i]); }) / dn;
            if ((tid & (PS_WAVE - 1)) == 0) {
                gb[j] = bj;
                gL[j] = dn * ((log(-(bj / kj)) - kj) - 1.0);
            }
        }
        __syncthreads();
        for (int j = wave; j < G; j += waves) {
            const double Lj = gL[j];
            double w = 1.0 / psis_wave_sum(G, [&](int t) { return exp(gL[t] - Lj); });
            if (w < 10.0 * DBL_EPSILON) w = 0.0;
            if ((tid & (PS_WAVE - 1)) == 0) gw[j] = w;
        }
        __syncthreads();
        const double wsum = psis_block_sum(G, part, [&](int t) { return gw[t]; });
        const double b = psis_block_sum(G, part, [&](int t) { return gb[t] * (gw[t] / wsum); });
        const double nb = -b;
        const double kk = psis_block_sum(n, part, [&](int i) { return log1p(nb * x[i]); }) / dn;
        const double sigma = -kk / b;
        khat = (dn * kk + 5.0) / (dn + 10.0);
        if (isfinite(khat)) {
            for (int i = tid; i < n; i += block) {
                const double t1 = log1p(-(((double)i + 0.5) / dn));
                const double y = khat == 0.0 ? (-sigma) * t1 : sigma * expm1((-khat) * t1) / khat;
                x[i] = log(y + ec);
            }
        } else {
            for (int i = tid; i < n; i += block) x[i] = (-col[(size_t)idx[t0 + i] * ld]) - maxlr;
        }
        __syncthreads();
    }

    // ---- 6. and 7.
    double lwmax = -INFINITY;
    for (int k = tid; k < S; k += block) {
        const double v = fmin(keys[k], 0.0);
        keys[k] = v;
        lwmax = fmax(lwmax, v);
    }
    lwmax = psis_block_fmax(lwmax, red);                  // its first barrier also publishes keys
    const double lse = lwmax + log(psis_block_sum(S, part, [&](int s) { return exp(keys[pos[s]] - lwmax); }));
    for (int k = tid; k < S; k += block) keys[k] = keys[k] - lse;
    __syncthreads();

    // ---- 8.
    double vmax = -INFINITY;
    for (int s = tid; s < S; s += block) {
        const double lwn = keys[pos[s]];
        vmax = fmax(vmax, lwn + col[(size_t)s * ld]);
        if (log_weights) log_weights[(size_t)s * ld_w + r] = lwn;
    }
    vmax = psis_block_fmax(vmax, red);
    const double Zl = psis_block_sum(S, part, [&](int s) { return exp((keys[pos[s]] + col[(size_t)s * ld]) - vmax); });
    if (tid == 0) {
        elpd_loo[r] = vmax + log(Zl);
        khat_out[r] = khat;
        n_tail_out[r] = n;
        if (row_lppd) row_lppd[r] = s_lppd;
    }
}

// K13's row_lppd of one column by one lane (the totals' launch, when the caller keeps no row_lppd)
__device__ double psis_column_lppd(const double *col, size_t ld, int S)
{
    double m = -INFINITY;
    int bad = 0;
    for (int s = 0; s < S; ++s) {
        const double v = col[(size_t)s * ld];
        bad |= !isfinite(v);
        m = fmax(m, v);
    }
    if (bad) return __builtin_nan("");
    double Z = 0.0;
    for (int s = 0; s < S; ++s) Z += exp(col[(size_t)s * ld] - m);
    return (m + log(Z)) - log((double)S);
}

// summary = { sum elpd_loo, sum row_lppd, rows with khat > 0.7, rows with n_tail < 0 }
__global__ void __launch_bounds__(PS_PARTS)
psis_summary_kernel(const double *__restrict__ loglik, size_t ld, int S, size_t n_rows, const double *__restrict__ elpd_loo,
                    const double *__restrict__ khat, const int *__restrict__ n_tail, const double *__restrict__ row_lppd,
                    double *__restrict__ summary)
{
    __shared__ double part[4][PS_PARTS];
    const int tid = (int)threadIdx.x;
    double e = 0.0, l = 0.0, high = 0.0, nonfinite = 0.0;
    for (size_t r = tid; r < n_rows; r += PS_PARTS) {
        e += elpd_loo[r];
        l += row_lppd ? row_lppd[r] : psis_column_lppd(loglik + r, ld, S);
        high += khat[r] > 0.7 ? 1.0 : 0.0;
        nonfinite += n_tail[r] < 0 ? 1.0 : 0.0;
    }
    part[0][tid] = e; part[1][tid] = l; part[2][tid] = high; part[3][tid] = nonfinite;
    __syncthreads();
    for (int h = PS_PARTS / 2; h >= 1; h >>= 1) {
        if (tid < h)
            for (int k = 0; k < 4; ++k) part[k][tid] += part[k][tid + h];
        __syncthreads();
    }
    if (tid < 4) summary[tid] = part[tid][0];
}

int psis_loo(const double *loglik, size_t ld, size_t S, size_t n_rows, double r_eff, double *elpd_loo, double *khat,
             int *n_tail, double *row_lppd, double *log_weights, size_t ld_w, double *summary, hipStream_t st)
{
    const char *who = "psis_loo";
    if (S < 2 || S > (size_t)PS_MAX_DRAWS) return fail(SGMCMC_EINVAL, "%s: S = %zu draws, must be 2 .. %d", who, S, PS_MAX_DRAWS);
    if (!(r_eff > 0.0) || !std::isfinite(r_eff))
        return fail(SGMCMC_EINVAL, "%s: r_eff = %g, must be a positive finite number", who, r_eff);
    if (n_rows == 0) return 0;
    const struct { const void *p; const char *name; } required[] = {
        {loglik, "loglik"}, {elpd_loo, "elpd_loo"}, {khat, "khat"}, {n_tail, "n_tail"}};
    for (const auto &arg : required)
        if (!arg.p) return fail(SGMCMC_EINVAL, "%s: %s is NULL", who, arg.name);
    if (ld < n_rows) return fail(SGMCMC_EINVAL, "%s: ld = %zu is smaller than n_rows = %zu", who, ld, n_rows);
    if (log_weights && ld_w < n_rows) return fail(SGMCMC_EINVAL, "%s: ld_w = %zu is smaller than n_rows = %zu", who, ld_w, n_rows);
    size_t rows = 0, extent = 0;
    if (__builtin_mul_overflow(S - 1, ld, &rows) || __builtin_add_overflow(rows, n_rows, &extent)
        || extent > SIZE_MAX / sizeof(double))
        return fail(SGMCMC_EINVAL, "%s: loglik's extent overflows with S = %zu, ld = %zu", who, S, ld);
    if (log_weights && (__builtin_mul_overflow(S - 1, ld_w, &rows) || __builtin_add_overflow(rows, n_rows, &extent)
                        || extent > SIZE_MAX / sizeof(double)))
        return fail(SGMCMC_EINVAL, "%s: log_weights' extent overflows with S = %zu, ld_w = %zu", who, S, ld_w);
    if (n_rows > (size_t)INT32_MAX) return fail(SGMCMC_EINVAL, "%s: n_rows = %zu is too large for one launch", who, n_rows);

    // 2. of the header, in double on the host
    const double m1 = std::ceil(0.2 * (double)S), m2 = std::ceil(3.0 * std::sqrt((double)S / r_eff));
    double md = m1 < m2 ? m1 : m2;
    if (md < 1.0) md = 1.0;
    if (md > (double)(S - 1)) md = (double)(S - 1);
    const int M = (int)md;

    int npad = PS_MIN_PAD;
    while (npad < (int)S) npad <<= 1;
    const int block = npad / 2 < PS_MAX_BLOCK ? npad / 2 : PS_MAX_BLOCK;
#define PSIS_LAUNCH(CAP)                                                                                                       \
    hipLaunchKernelGGL((psis_loo_kernel<CAP>), dim3((unsigned)n_rows), dim3(block), 0, st, loglik, ld, (int)S, M, npad,        \
                       elpd_loo, khat, n_tail, row_lppd, log_weights, ld_w)
    if (npad <= 1024) PSIS_LAUNCH(1024);
    else if (npad <= 4096) PSIS_LAUNCH(4096);
    else PSIS_LAUNCH(PS_MAX_DRAWS);
#undef PSIS_LAUNCH
    if (int rc = launched("psis_loo_kernel")) return rc;
    if (summary) {
        hipLaunchKernelGGL(psis_summary_kernel, dim3(1), dim3(PS_PARTS), 0, st, loglik, ld, (int)S, n_rows,
                           static_cast<const double *>(elpd_loo), static_cast<const double *>(khat),
                           static_cast<const int *>(n_tail), static_cast<const double *>(row_lppd), summary);
        if (int rc = launched("psis_summary_kernel")) return rc;
    }
    return 0;
}

}  // namespace

extern "C" {

int sgmcmc_psis_abi_version(void) { return SGMCMC_PSIS_ABI_VERSION; }

int sgmcmc_psis_max_draws(void) { return PS_MAX_DRAWS; }

int sgmcmc_psis_loo(const double *loglik, size_t ld, size_t S, size_t n_rows, double r_eff, double *elpd_loo, double *khat,
                    int *n_tail, double *row_lppd, double *log_weights, size_t ld_w, double *summary, sgmcmc_stream_t stream)
{
    return psis_loo(loglik, ld, S, n_rows, r_eff, elpd_loo, khat, n_tail, row_lppd, log_weights, ld_w, summary,
                    static_cast<hipStream_t>(stream));
}

}  // extern "C"
