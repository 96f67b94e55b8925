/* sgmcmc_hip_predict_grad.h -- OPTIONAL predictive-gradient add-on of libsgmcmc_hip.so, OUTSIDE the SURVEY.md section 8(b)
 * boundary.
 *
 * include/sgmcmc_hip_predict.h evaluates the networks sampled into a device trace at test inputs. A Bayesian-optimisation
 * loop also climbs an acquisition function of that predictive, and for that it needs the derivatives of the predictive mean
 * and variance with respect to the INPUTS (RoBO's model interface, which pysgmcmc/models/base_model.py follows, calls this
 * `predictive_gradients`). This header declares that step: every sampled network's output AND its input gradient at every
 * test row, and the derivatives of the ensemble mean and variance, read straight from the trace. It has a version of its
 * own, so it can grow without touching the boundary or the other add-ons.
 *
 * Conventions are those of sgmcmc_hip.h: extern "C", plain pointers and sizes; 0 on success, a positive hipError_t or a
 * negative SGMCMC_E* code with a thread-local text in sgmcmc_last_error(); launches are asynchronous on `stream` and legal
 * inside stream capture; the library allocates, frees and copies nothing and keeps no process-wide state; arguments are
 * checked on the host before anything is launched.
 */
#ifndef SGMCMC_HIP_PREDICT_GRAD_H
#define SGMCMC_HIP_PREDICT_GRAD_H

#include "sgmcmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGMCMC_PREDICT_GRAD_ABI_VERSION 1

int sgmcmc_predict_grad_abi_version(void);

#define SGMCMC_PREDICT_GRAD_MAX_CHAINS 64

/* K14: the outputs of S = m * n sampled networks at n_rows test inputs, their gradients with respect to those inputs, and
 * the input gradients of the ensemble mean and variance. D0 = layer_sizes[0].
 *   chains, m, n, ld, layer_sizes, n_layers, X     exactly as in sgmcmc_bnn_predict_*: a HOST array of m DEVICE matrices of
 *                 n rows, sample s = c * n + i the row at chains[c] + i * ld, a row the flat parameter vector W1 (in, out)
 *                 row-major, b1, ..., WL, bL, log_var, at any element alignment; 1 .. 8 weight layers, every size >= 1, the
 *                 last one 1; X (n_rows, D0) row-major, already normalised. m = 1 .. SGMCMC_PREDICT_GRAD_MAX_CHAINS,
 *                 m * n < 2^31. What lies between n_params and ld is never read; log_var is not an input of anything here.
 *   means         (S, n_rows) row-major, required: the bits sgmcmc_bnn_predict_* writes for the same inputs (the forward
 *                 loops are K11's: every output unit owns its k-ordered fma chain).
 *   grads         (S, n_rows, D0) row-major, required: grads[s][r][d] = d means[s][r] / d X[r][d], in the element type,
 *                 every written operation rounded once (no contraction). h_l is the tanh output of layer l, n_l =
 *                 layer_sizes[l], W_l[k][j] element k * n_l + j of layer l's weights:
 *                   L = 1:             grads[d] = W_1[d][0]                                         (a copy: exact)
 *                   top:               delta_{L-1}[k] = W_L[k][0] * (1 - h_{L-1}[k] * h_{L-1}[k])   (h * h, 1 - ., the product)
 *                   l = L-1 ... 2:     acc = 0; for j = 0 .. n_l - 1 ascending: acc = fma(W_l[k][j], delta_l[j], acc);
 *                                      delta_{l-1}[k] = acc * (1 - h_{l-1}[k] * h_{l-1}[k])
 *                   inputs:            acc = 0; for j ascending: acc = fma(W_1[d][j], delta_1[j], acc); grads[d] = acc
 *                 so grads[s][r][:] depends on theta_s and x_r alone: not on the row tile, the grid, the alignment of a row,
 *                 pair or scalar loops, or how many samples or rows the call holds.
 *   ens_mean, ens_var   double[n_rows];  dmean, dvar   double (n_rows, D0) row-major: all four, or all four NULL. Reduced in
 *                 f64 in a fixed order without atomics, ONE lane per output element, s ascending:
 *                   ens_mean[r], ens_var[r]   K11's statements in K11's order: the bits sgmcmc_bnn_predict_* writes
 *                   G = sum_s (double)grads[s][r][d];                                         dmean[r][d] = G / S
 *                   C = sum_s ((double)means[s][r] - ens_mean[r]) * (double)grads[s][r][d];   dvar[r][d] = (2.0 * C) / S
 *                 dvar is the derivative of the population variance ens_var: the term in the mean gradient drops out because
 *                 sum_s (means[s][r] - ens_mean[r]) = 0.
 *
 * Launches. Forward + backward: grid.x = S, grid.y = min(n_tiles, ceil(4096 / S), 65535), n_tiles = ceil(n_rows / tile)
 * with the tile of sgmcmc_bnn_predict_grad_row_tile. The workgroup (s, y) copies sample s's parameters into the LDS once
 * and walks the tiles y, y + grid.y, ...; per tile the X tile, EVERY hidden layer's activations and two ping-pong delta
 * buffers live in the LDS, so neither an activation nor a delta touches global memory. The backward sweep reads rows of
 * W_l, contiguous in j, and writes grads coalesced over (row, d). Behind it on the same stream: the K11 reduction of means,
 * then one lane per (r, d) for dmean and dvar.
 *
 * n_rows = 0 or n = 0 is a successful no-op. Refused with SGMCMC_EINVAL, the text starting "bnn_predict_grad: ", an earlier
 * check winning over a later one: m outside 1 .. 64; a NULL chains, layer_sizes, X, means or grads (each named); the four
 * ensemble outputs neither all given nor all NULL; n_layers outside 1 .. 8, a layer size < 1, a last layer that is not one
 * unit; a NULL chains[c]; ld < n_params; m * n >= 2^31; n_rows or n_rows * D0 too large for one launch; a net whose LDS
 * need, at a row tile of ONE test row, exceeds 160 KiB.                                                                     */
int sgmcmc_bnn_predict_grad_f32(const float *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers,
                                const float *X, size_t n_rows, float *means, float *grads, double *ens_mean, double *ens_var,
                                double *dmean, double *dvar, sgmcmc_stream_t stream);
int sgmcmc_bnn_predict_grad_f64(const double *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers,
                                const double *X, size_t n_rows, double *means, double *grads, double *ens_mean,
                                double *ens_var, double *dmean, double *dvar, sgmcmc_stream_t stream);

/* The number of test rows per tile the forward + backward launch uses for this net and element size (4 or 8): the largest
 * power of two <= 32 that keeps a workgroup's LDS within max(40 KiB, twice the parameter copy), so several workgroups share
 * a CU; 1 if only that fits the 160 KiB. The footprint, in elements, every region rounded up to a multiple of 4:
 *   n_params + tile * D0 + sum over the hidden layers l = 1 .. L-1 of tile * n_l + 2 * tile * (the widest hidden layer).
 * Performance only: the results do not depend on it. Returns the tile (>= 1), or SGMCMC_EINVAL for a net
 * sgmcmc_bnn_predict_grad_* refuses or an element size other than 4 or 8. Host arithmetic; nothing is launched.           */
int sgmcmc_bnn_predict_grad_row_tile(const int *layer_sizes, int n_layers, size_t element_size);

#ifdef __cplusplus
}
#endif
#endif /* SGMCMC_HIP_PREDICT_GRAD_H */
