/* sgmcmc_hip_predict.h -- OPTIONAL posterior-predictive add-on of libsgmcmc_hip.so, OUTSIDE the SURVEY.md section 8(b) boundary.
 *
 * include/sgmcmc_hip_fused_trace.h leaves the thinned samples of m chains of a small tanh-MLP BNN in a device matrix and
 * include/sgmcmc_hip_diag.h diagnoses them where they lie. This header declares the step that follows: the posterior
 * predictive of those samples at test inputs (pysgmcmc/models/bayesian_neural_network.py:560-630, which evaluates the kept
 * networks one by one and reduces on the host) -- every network's mean at every test row, exp(log_var) of every network, and
 * the mean and variance of the networks' means per row -- read straight from the trace. It has a version of its own, so it
 * can grow without touching the boundary or the other add-ons.
 *
 * Conventions are those of sgmcmc_hip.h: extern "C", plain pointers and sizes; 0 on success, a positive hipError_t or a
 * negative SGMCMC_E* code with a thread-local text in sgmcmc_last_error(); launches are asynchronous on `stream` and legal
 * inside stream capture; the library allocates, frees and copies nothing and keeps no process-wide state; arguments are
 * checked on the host before anything is launched.
 */
#ifndef SGMCMC_HIP_PREDICT_H
#define SGMCMC_HIP_PREDICT_H

#include "sgmcmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGMCMC_PREDICT_ABI_VERSION 1

int sgmcmc_predict_abi_version(void);

#define SGMCMC_PREDICT_MAX_CHAINS 64

/* K11: the outputs of S = m * n sampled networks at n_rows test inputs, and their ensemble moments.
 *   chains        HOST array of m DEVICE matrices of n rows (read during the call, not kept), as in sgmcmc_ess_variogram_*:
 *                 sample s = c * n + i is the row at chains[c] + i * ld. A row is a flat parameter vector in the whole-step
 *                 kernel's order: W1 (in, out) row-major, b1, ..., WL, bL, log_var. Any element alignment. A contiguous
 *                 (m, n, P) trace goes down as ONE matrix of m * n rows (m = 1), so 256 chains need no pointer table.
 *   m             1 .. SGMCMC_PREDICT_MAX_CHAINS;   m * n < 2^31
 *   layer_sizes   [n_layers + 1], n_layers = 1 .. 8 weight layers, every size >= 1, the last one 1 (the rules of the whole-step
 *                 entries); n_params = sum(in * out + out) + 1
 *   ld            elements between rows, >= n_params; what lies between n_params and ld is never read
 *   X             (n_rows, layer_sizes[0]) row-major, already normalised by the caller
 *   means         (m * n, n_rows) row-major, required: network s's output unit at every row (the reference's
 *                 `return_individual_predictions` output). It is also the only scratch the reduction needs.
 *   noise_var     [m * n] or NULL: exp(log_var_s), formed in double and rounded once
 *   ens_mean, ens_var   double[n_rows] or NULL, both or neither: the mean over s of means[s][r] and the population
 *                 variance mean_s((means[s][r] - ens_mean[r])^2) (bayesian_neural_network.py:619-622)
 *
 * Two launches. The forward pass: one workgroup holds ONE sample's parameters in the LDS and walks tiles of test rows (the
 * X tile and two ping-pong activation buffers are in the LDS too; activations never touch global memory). Every output
 * unit owns its k-ordered fma chain, exactly the whole-step kernel's forward loops, so the bits of means[s][r] depend on
 * theta_s and x_r alone: not on the row tile, the grid, the alignment of a row, or how many samples or rows the call holds.
 * The reduction: f64, two passes, s ascending, ONE lane per test row, so equal `means` give equal bits whatever the launch.
 *
 * n_rows = 0 or n = 0 is a successful no-op. Refused with SGMCMC_EINVAL: m outside 1 .. 64; a NULL chains, chains[c],
 * layer_sizes, X or means; n_layers outside 1 .. 8, a layer size < 1, a last layer that is not one unit; ld < n_params; one
 * of ens_mean / ens_var without the other; m * n >= 2^31; a net whose parameters, with a row tile of ONE test row, need
 * more than 160 KiB of LDS.                                                                                                */
int sgmcmc_bnn_predict_f32(const float *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers,
                           const float *X, size_t n_rows, float *means, float *noise_var, double *ens_mean, double *ens_var,
                           sgmcmc_stream_t stream);
int sgmcmc_bnn_predict_f64(const double *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers,
                           const double *X, size_t n_rows, double *means, double *noise_var, double *ens_mean,
                           double *ens_var, sgmcmc_stream_t stream);

/* The number of test rows per tile the forward launch of sgmcmc_bnn_predict_* uses for this net and element size (4 or 8):
 * the largest power of two <= 32 that keeps a workgroup's LDS (parameters + X tile + two activation buffers) within
 * max(40 KiB, twice the parameter copy), so several workgroups share a CU; 1 if only that fits the 160 KiB. Performance
 * only: the results do not depend on it. Returns the tile (>= 1), or SGMCMC_EINVAL for a net sgmcmc_bnn_predict_* refuses.
 * Host arithmetic; nothing is launched.                                                                                   */
int sgmcmc_bnn_predict_row_tile(const int *layer_sizes, int n_layers, size_t element_size);

#ifdef __cplusplus
}
#endif
#endif /* SGMCMC_HIP_PREDICT_H */
