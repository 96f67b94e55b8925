/* sgmcmc_hip_diag.h -- OPTIONAL diagnostics add-on of libsgmcmc_hip.so, OUTSIDE the SURVEY.md section 8(b) boundary.
 *
 * include/sgmcmc_hip.h is the drop-in contract behind `next(sampler)` (ABI v6, its contract map); a maintainer of the
 * reference binds that header and nothing here. This header declares what the same shared library offers on top of it for
 * chain diagnostics that need the lagged HISTORY of a chain, which no step kernel sees: the effective sample size of every
 * parameter from device-resident traces (the function of pysgmcmc/diagnostics/sampler_diagnostics.py:47-82, which loops
 * over the parameter dimensions on the host). It has a version of its own, so it can grow without touching the boundary.
 *
 * Conventions are those of sgmcmc_hip.h: extern "C", plain pointers and sizes; 0 on success, a positive hipError_t or a
 * negative SGMCMC_E* code with a thread-local text in sgmcmc_last_error(); asynchronous on `stream`, legal inside stream
 * capture; the library allocates, frees and copies nothing and keeps no process-wide state; arguments are checked on the
 * host before anything is launched.
 */
#ifndef SGMCMC_HIP_DIAG_H
#define SGMCMC_HIP_DIAG_H

#include "sgmcmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGMCMC_DIAG_ABI_VERSION 1

int sgmcmc_diag_abi_version(void);

#define SGMCMC_ESS_MAX_CHAINS 64

/* `staging` of sgmcmc_ess_variogram_*: where the slab (m chains x n samples x the parameters of one workgroup) lives while
 * the lags are walked. Performance only: the three give identical bits.
 *   AUTO    LDS when the slab fits 160 KiB (m * n * block_threads * sizeof(element)), else GLOBAL
 *   LDS     the slab is read from HBM once into the LDS; moments and every lag are computed from there
 *           (SGMCMC_EINVAL if it does not fit)
 *   GLOBAL  moments and every lag re-read global memory (consecutive lags of a workgroup hit L2)                         */
#define SGMCMC_ESS_STAGING_AUTO   0
#define SGMCMC_ESS_STAGING_LDS    1
#define SGMCMC_ESS_STAGING_GLOBAL 2

/* K10: effective sample size of each of P parameters from the traces of m chains (variogram estimate, pymc3 3.1's formula
 * as the reference uses it). For one parameter with traces x[c][i], c < m, i < n:
 *   mean_c, var_c (unbiased);  B = n var_c(mean_c) (unbiased; 0 when m = 1);  W = mean_c(var_c);  Vhat = W (n-1)/n + B/n
 *   t = 1, 2, ...:  V_t = 1/(m (n-t)) sum_c sum_{i<n-t} (x[c][i+t] - x[c][i])^2,  rho_t = 1 - V_t / (2 Vhat);
 *                   after each even t stop if rho_{t-1} + rho_t < 0 (rho_0 = 1); stop in any case when t reaches n;
 *                   T = t after the last increment (so T = n when no pair was negative)
 *   raw = m n / (1 + 2 sum_{1 <= t < T} rho_t);   ess = (int64) raw, truncated toward zero
 *
 *   chains    HOST array of m DEVICE pointers (read during the call, not kept): chain c is a matrix of n rows of P
 *             parameters, element (i, p) at chains[c][i * ld + p]. Separate per-chain buffers need no stacking copy; a
 *             contiguous (m, n, P) array is chains[c] = base + c * n * P, ld = P. Any element alignment.
 *   m         1 .. SGMCMC_ESS_MAX_CHAINS;   n  2 .. 2^31 - 1;   ld >= P (elements);   P = 0 is a successful no-op
 *   ess       int64[P], required;   raw  double[P] or NULL;   stop_lag  int32[P] (T) or NULL
 *   staging   SGMCMC_ESS_STAGING_*
 *   launch    NULL = defaults. Only block_threads (parameters per workgroup: 64, 128, 192 or 256; default and auto = 64) and
 *             the timestamp events are read; the other fields are validated and ignored.
 *
 * Elements are f32 or f64; every sum, and everything after it, is f64 in both cases. Lanes map to parameters (coalesced
 * rows); each parameter is summed by ONE lane in a fixed order (per lag four interleaved partial sums over i, chains in
 * order, combined as (a0 + a1) + (a2 + a3)), so `raw` does not depend on block_threads, on the staging, on alignment or
 * on the launch: equal inputs give equal bits. The cost depends on the data: m * sum_{t<T} (n - t) terms per parameter,
 * and a wave runs until its last lane has stopped.
 *
 * Degenerate columns: where Vhat is zero or not finite (a constant column, a NaN or Inf sample) raw = NaN, ess = 0 and
 * stop_lag = 1, and the neighbouring parameters are not affected (the scalar Python function raises there; a batched one
 * cannot). The moments are taken on samples shifted by the column's first one, so equal samples give Vhat = 0 exactly
 * whatever their value. ess is also 0 where raw itself is not finite or does not fit an int64.                            */
int sgmcmc_ess_variogram_f32(const float *const *chains, int m, size_t n, size_t P, size_t ld, int64_t *ess, double *raw,
                             int32_t *stop_lag, int staging, const sgmcmc_launch_t *launch, sgmcmc_stream_t stream);
int sgmcmc_ess_variogram_f64(const double *const *chains, int m, size_t n, size_t P, size_t ld, int64_t *ess, double *raw,
                             int32_t *stop_lag, int staging, const sgmcmc_launch_t *launch, sgmcmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGMCMC_HIP_DIAG_H */
