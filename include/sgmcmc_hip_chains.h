/* sgmcmc_hip_chains.h -- OPTIONAL many-chains diagnostics add-on of libsgmcmc_hip.so, OUTSIDE the SURVEY.md section 8(b) boundary.
 *
 * include/sgmcmc_hip_fused_trace.h leaves the thinned samples of up to 256 chains of a small BNN in ONE strided device array
 * and include/sgmcmc_hip_predict.h reads it there. include/sgmcmc_hip_diag.h (K10) diagnoses at most 64 chains, whose pointers
 * travel by value, and gives no R-hat. This header declares the step between the two for the chain counts the whole-step
 * kernel was built for: the Gelman-Rubin statistic AND the effective sample size of every parameter from a strided
 * (m, n, P) trace with up to 4096 chains (pysgmcmc/diagnostics/sampler_diagnostics.py:12-82, which loops over the parameter
 * dimensions on the host). It has a version of its own, so it can grow without touching the boundary or the other add-ons.
 *
 * Conventions are those of sgmcmc_hip.h: extern "C", plain pointers and sizes; 0 on success, a positive hipError_t or a
 * negative SGMCMC_E* code with a thread-local text in sgmcmc_last_error(); launches are asynchronous on `stream` and legal
 * inside stream capture; the library allocates, frees and copies nothing and keeps no process-wide state; arguments are
 * checked on the host before anything is launched.
 */
#ifndef SGMCMC_HIP_CHAINS_H
#define SGMCMC_HIP_CHAINS_H

#include "sgmcmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGMCMC_CHAINS_ABI_VERSION 1

int sgmcmc_chains_abi_version(void);

#define SGMCMC_CHAINS_MAX_CHAINS 4096

/* K12: R-hat and effective sample size of each of P parameters from the traces of m chains in one strided array. For one
 * parameter with traces x[c][i], c < m, i < n, the formulas are K10's (sgmcmc_hip_diag.h):
 *   mean_c, var_c (unbiased);  B = n var_c(mean_c) (unbiased; 0 when m = 1);  W = mean_c(var_c);  Vhat = W (n-1)/n + B/n
 *   rhat = sqrt(Vhat / W)
 *   t = 1, 2, ...:  V_t = 1/(m (n-t)) sum_c sum_{i<n-t} (x[c][i+t] - x[c][i])^2,  rho_t = 1 - V_t / (2 Vhat);
 *                   after each even t stop if rho_{t-1} + rho_t < 0 (rho_0 = 1); stop in any case when t reaches n;
 *                   T = t after the last increment (so T = n when no pair was negative)
 *   raw = m n / (1 + 2 sum_{1 <= t < T} rho_t);   ess = (int64) raw, truncated toward zero
 *
 *   trace         DEVICE array; element (c, i, p) at trace[c * chain_stride + i * ld + p]. Rows are dense; any element
 *                 alignment. Views of wider (ld > P) or longer (chain_stride > n * ld) buffers go down without a copy.
 *   m             1 .. SGMCMC_CHAINS_MAX_CHAINS;   n  2 .. 2^31 - 1;   P = 0 is a successful no-op
 *   ld            >= P (elements);   chain_stride  >= (n - 1) * ld + P (elements)
 *   rhat          double[P] or NULL
 *   ess           int64[P] or NULL;   raw  double[P] or NULL;   stop_lag  int32[P] (T) or NULL   (as in K10)
 *                 At least one of the four must be non-NULL. With ess, raw and stop_lag all NULL the launch takes the
 *                 moments only and walks no lag: the R-hat-only mode.
 *   waves         0 (auto) or 1, 2, 4, 8, 16: the waves of a workgroup that share the chains of its 64 parameters.
 *                 Performance only: every value gives identical bits. Auto: the largest of 1, 2, 4, 8, 16 that exceeds
 *                 neither the number of 16-chain groups, ceil(m / 16), nor what keeps the whole grid resident at once,
 *                 ceil(P / 64) * waves <= 32 waves * the device's compute units (a grid that fills the device by itself
 *                 gains nothing from splitting a parameter's chains, and pays a barrier per lag for it).
 *
 * Elements are f32 or f64; every sum, and everything after it, is f64 in both cases, without contraction. A workgroup is
 * 64 parameters x `waves` waves: lane = parameter (coalesced rows), and the chains are cut into GROUPS OF 16 CONSECUTIVE
 * CHAINS (the last may be shorter) that the waves share out. The summation order is fixed by the groups, not by the waves:
 *   moments   per chain, mean and unbiased variance by K10's two passes on samples shifted by x0 = x[0][0]; sum mean_c and
 *             sum var_c are added inside a group in ascending chain order from 0.0, the group sums in ascending group order
 *             from 0.0; sum (mean_c - grand)^2 for B likewise. W = sum var / m, B = n q / (m - 1) (0 at m = 1).
 *   lag t     inside a group K10's four interleaved partial sums a0..a3 over i carry on from chain to chain; the group sum
 *             is (a0 + a1) + (a2 + a3); s = the group sums in ascending group order from 0.0;
 *             rho_t = 1 - s / ((2 Vhat) ((double)m (double)(n - t))).
 * So the results do not depend on waves, on alignment, on ld or chain_stride, or on how many columns the call holds, and for
 * m <= 16 (one group) raw, ess and stop_lag are K10's bits exactly.
 *
 * rhat is sqrt(Vhat / W) as IEEE gives it (+inf where W = 0 < Vhat: chains that are each constant at different values) and
 * NaN where Vhat is zero or not finite. At m = 1, B = 0 and the formula gives sqrt((n - 1) / n) for every column that is not
 * degenerate: one chain says nothing about convergence. Degenerate columns (Vhat zero or not finite: a constant column, a
 * NaN or Inf sample) are K10's for the rest: raw = NaN, ess = 0, stop_lag = 1; neighbouring parameters are not affected.
 *
 * Refused with SGMCMC_EINVAL, with the offending value in the text: m outside 1 .. 4096; n outside 2 .. 2^31 - 1; ld < P;
 * chain_stride < (n - 1) * ld + P; an extent that overflows a size_t; a NULL trace; all four outputs NULL; waves not one of
 * 0, 1, 2, 4, 8, 16; P too large for one launch (ceil(P / 64) >= 2^31).                                                      */
int sgmcmc_chain_diag_f32(const float *trace, int m, size_t n, size_t P, size_t ld, size_t chain_stride, double *rhat,
                          int64_t *ess, double *raw, int32_t *stop_lag, int waves, sgmcmc_stream_t stream);
int sgmcmc_chain_diag_f64(const double *trace, int m, size_t n, size_t P, size_t ld, size_t chain_stride, double *rhat,
                          int64_t *ess, double *raw, int32_t *stop_lag, int waves, sgmcmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGMCMC_HIP_CHAINS_H */
