/* sgmcmc_hip_score.h -- OPTIONAL held-out-score add-on of libsgmcmc_hip.so, OUTSIDE the SURVEY.md section 8(b) boundary.
 *
 * include/sgmcmc_hip_predict.h gives the posterior predictive of the samples a device trace holds. This header declares the
 * step that follows: the score of that ensemble against held-out targets -- the pointwise Gaussian log density of every
 * sampled network at every test row, the log pointwise predictive density (lppd), the WAIC penalty and the error of the
 * ensemble mean. The reference leaves it open (pysgmcmc/diagnostics/model_diagnostics.py is one comment line); the density
 * is the one its BNN trains on (pysgmcmc/models/bayesian_neural_network.py:368, the 1e-16 in the variance included). It has
 * a version of its own, so it can grow without touching the boundary or the other add-ons.
 *
 * Conventions are those of sgmcmc_hip.h: extern "C", plain pointers and sizes; 0 on success, a positive hipError_t or a
 * negative SGMCMC_E* code with a thread-local text in sgmcmc_last_error(); launches are asynchronous on `stream` and legal
 * inside stream capture; the library allocates, frees and copies nothing and keeps no process-wide state; arguments are
 * checked on the host before anything is launched.
 */
#ifndef SGMCMC_HIP_SCORE_H
#define SGMCMC_HIP_SCORE_H

#include "sgmcmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGMCMC_SCORE_ABI_VERSION 1

int sgmcmc_score_abi_version(void);

#define SGMCMC_SCORE_MAX_CHAINS 64

/* K13: the held-out score of S = m * n sampled networks at n_rows test inputs with targets y.
 *   chains, m, n, ld, layer_sizes, n_layers, X     what they are in sgmcmc_bnn_predict_* (sgmcmc_hip_predict.h): a HOST array
 *                 of m DEVICE matrices of n rows, sample s = c * n + i at chains[c] + i * ld, a row a flat parameter vector
 *                 W1, b1, ..., WL, bL, log_var of n_params elements; m = 1 .. SGMCMC_SCORE_MAX_CHAINS, m * n < 2^31
 *   y             [n_rows] of the element type, in the units the networks work in (normalised if the networks were trained
 *                 on normalised targets)
 *   means         (S, n_rows) row-major, required: network s's output at row r, with the bits sgmcmc_bnn_predict_* writes.
 *                 It is the forward launch's output and the only input of the reductions besides y and the log-variances.
 *   row_lppd, row_pwaic, ens_mean, ens_var     double[n_rows], required
 *   loglik        double (S, n_rows) row-major or NULL
 *   sample_loglik double[S] or NULL
 *   summary       double[3] or NULL
 *
 * Every reduction runs in float64, whatever the element type, one rounding per written operation (no contraction), in
 * exactly this order. With P = n_params and row_s the parameter row of sample s:
 *
 *   per sample    lv_s = (double)row_s[P - 1]
 *                 a_s  = -0.5 * (1.8378770664093453 + lv_s)                   (log 2 pi)
 *                 b_s  = 0.5 / (exp(lv_s) + 1e-16)
 *   pointwise     d = (double)y[r] - (double)means[s][r]
 *                 l[s][r] = a_s - (d * d) * b_s
 *   per row r, samples s ascending, two passes
 *     pass 1      F = sum f,  ens_mean = F / S        (f = (double)means[s][r])
 *                 M = max_s l                          (fmax, starting from -inf)
 *                 L = sum l,  lbar = L / S
 *     pass 2      q = sum (f - ens_mean)^2,  ens_var = q / S
 *                 Z = sum exp(l - M)
 *                 w = sum (l - lbar)^2
 *     results     row_lppd[r]  = (M + log(Z)) - log((double)S)
 *                 row_pwaic[r] = w / (S - 1), and exactly 0.0 when S == 1
 *   ens_mean and ens_var are the statements of sgmcmc_bnn_predict_* in its order: their bits equal what it writes.
 *   loglik[s][r]     = l[s][r]
 *   sample_loglik[s] = sum_r l[s][r]: 256 partial sums, partial j adding rows j, j + 256, ... ascending from 0.0, then added
 *                 by a fixed pairwise tree: for h = 128, 64, ..., 1: partial[j] += partial[j + h] for j < h
 *   summary       = { sum_r row_lppd[r], sum_r row_pwaic[r], sum_r (ens_mean[r] - (double)y[r])^2 }, each in that same
 *                 256-partials-then-tree order
 *
 * At most four launches, one behind the other on `stream`. The forward pass is sgmcmc_bnn_predict_*'s own (called with no
 * optional output), so a net it refuses is refused with its text. The row kernel: one lane per test row in 64-lane
 * workgroups; the per-sample constants a_s, b_s are formed once per workgroup and block of 64 samples and staged through
 * the LDS; no atomics. The per-sample kernel (when sample_loglik is given): one 256-lane workgroup per sample; it forms l
 * again from means, y, a_s, b_s with the statements above, so it does not need loglik. The summary kernel (when summary is
 * given): one 256-lane workgroup. Equal inputs give equal bits, whatever the launch, the number of rows or samples in the
 * call, or the layout of the chains.
 *
 * n_rows = 0 or n = 0 is a successful no-op. Refused with SGMCMC_EINVAL and a text that starts "bnn_score: ", an earlier
 * check winning over a later one: m outside 1 .. 64; a NULL chains, layer_sizes, X, y, means, row_lppd, row_pwaic, ens_mean
 * or ens_var; a NULL chains[c]; ld < n_params; m * n >= 2^31; n_rows too large for one launch (more than 2^31 - 1 workgroups
 * of 64 rows). Non-finite y or log_var are NOT checked: they propagate into the outputs by IEEE rules (a NaN log_var makes
 * every row's lppd NaN; an infinite y makes that row's l -inf and its lppd NaN).                                          */
int sgmcmc_bnn_score_f32(const float *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers,
                         const float *X, const float *y, size_t n_rows, float *means, double *row_lppd, double *row_pwaic,
                         double *ens_mean, double *ens_var, double *loglik, double *sample_loglik, double *summary,
                         sgmcmc_stream_t stream);
int sgmcmc_bnn_score_f64(const double *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers,
                         const double *X, const double *y, size_t n_rows, double *means, double *row_lppd,
                         double *row_pwaic, double *ens_mean, double *ens_var, double *loglik, double *sample_loglik,
                         double *summary, sgmcmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGMCMC_HIP_SCORE_H */
