/* sgmcmc_hip_particles.h -- OPTIONAL particle-gradient add-on of libsgmcmc_hip.so, OUTSIDE the SURVEY.md section 8(b)
 * boundary.
 *
 * The whole-step kernel (sgmcmc_hip.h [whole-step], sgmcmc_hip_fused.h) forms the cost of a small tanh-MLP BNN and its
 * parameter gradient inside a launch that also updates the chain. A particle method (Stein variational gradient descent)
 * needs that cost and gradient for EVERY particle of an (n, P) matrix on one minibatch and applies an update of its own.
 * This header declares that step on its own: no sampler state, no update, no noise. It has a version of its own, so it can
 * grow without touching the boundary or the other add-ons.
 *
 * Conventions are those of sgmcmc_hip.h: extern "C", plain pointers and sizes; 0 on success, a positive hipError_t or a
 * negative SGMCMC_E* code with a thread-local text in sgmcmc_last_error(); launches are asynchronous on `stream` and legal
 * inside stream capture; the library allocates, frees and copies nothing and keeps no process-wide state; arguments are
 * checked on the host before anything is launched.
 */
#ifndef SGMCMC_HIP_PARTICLES_H
#define SGMCMC_HIP_PARTICLES_H

#include "sgmcmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGMCMC_PARTICLES_ABI_VERSION 1

int sgmcmc_particles_abi_version(void);

/* The dynamic LDS one workgroup of K15 asks for, in bytes, for this net, minibatch and element size (4 or 8): the
 * whole-step kernel's rule,
 *   160 + ((2 * sum(layer_sizes[0 .. L]) + 1) * batch + n_params + 4) * esize,
 * or 0 when the call would be refused: a net that breaks the net rules below, batch < 1, an element size other than 4 or 8,
 * or a footprint above 160 KiB (the LDS of one compute unit). Host arithmetic; nothing is launched, no error text is set
 * for a footprint that does not fit.                                                                                     */
size_t sgmcmc_bnn_particles_lds_bytes(const int *layer_sizes, int n_layers, int batch, size_t esize);

/* K15: the cost of every particle of a small tanh-MLP BNN on one minibatch and its gradient with respect to the particle's
 * parameters, in one launch.
 *   theta, n_particles, ld     particle p is the n_params dense elements at theta + p * ld, the flat parameter vector W1
 *                 (in, out) row-major, b1, ..., WL, bL, log_var: the order of a trace row. Any element alignment. What lies
 *                 between n_params and ld is never read.
 *   layer_sizes, n_layers      sizes[0] inputs ... sizes[L] == 1; 1 .. 8 weight layers, every size >= 1.
 *   Xb, ldx, yb, batch         the minibatch as fed: row b of X is the sizes[0] elements at Xb + b * ldx, its target yb[b].
 *   batch_size, n_examples, wdecay, prior_mean, prior_var      the constants of the BNN cost, as in the whole-step entries.
 *   add_prior     1: grad is the full gradient of cost_out. 0: the weight-prior term coef * theta is left out, which is the
 *                 row the whole-step kernel leaves in its `grad` (its update adds the term as grad_decay).
 *   grad, ld_grad              row p at grad + p * ld_grad, n_params elements; what lies between n_params and ld_grad is
 *                 never written.
 *   cost_out      n_particles elements: the negative log likelihood with both priors, the whole-step kernel's cost.
 *
 * Arithmetic: the whole-step kernel's, statement for statement, every written operation rounded once (no contraction).
 * h_0 = x, h_l the output of layer l (tanh for l < L), n_l = layer_sizes[l], B = batch:
 *   forward     acc = b_l[j]; for k ascending: acc = fma(h_{l-1}[b][k], W_l[k][j], acc)
 *   head        in double: s = log_var, inv = 1 / (exp(s) + 1e-16), r_b = y_b - h_L[b], delta_L[b] = (T)(r_b * -(inv /
 *               batch_size)); cost and d / d log_var from sum_b r_b^2 and sum_i theta_i^2, the prior denominators
 *               n_params + 3e-16 and 2 * prior_var + 3e-16, one cast to T at the end
 *   gW_l[k][j]  acc = 0; for b ascending: acc = fma(h_{l-1}[b][k], delta_l[b][j], acc)
 *   gb_l[j]     acc = 0; for b ascending: acc = acc + delta_l[b][j]
 *   delta_{l-1}[b][k]   acc = 0; for j ascending: acc = fma(delta_l[b][j], W_l[k][j], acc); acc * (1 - h * h), h = h_{l-1}[b][k]
 *   add_prior   grad[i] = raw[i] + coef * theta[i], one multiply and one add, coef = (T)(wdecay / ((n_params + 3e-16) *
 *               n_examples)); skipped when coef == 0. The log_var element included.
 * Every weight and bias gradient therefore has the bits the whole-step kernel leaves in its gradient row for the same
 * particle and window; the cost and the log_var element differ from it by the order of two double sums in front of one
 * cast. A result depends on the particle and the minibatch alone: not on n_particles, ld, ld_grad, ldx, the alignment of a
 * row, or whether a loop ran on pairs of elements.
 *
 * Launch: grid.x = n_particles, one workgroup of 512 lanes per particle. The particle's parameters, the minibatch, every
 * layer's activations and the deltas live in the LDS (sgmcmc_bnn_particles_lds_bytes; above 64 KiB the entry opts the
 * kernel in). Nothing but grad and cost_out is written to global memory; no atomics, no matrix cores.
 *
 * n_particles = 0 is a successful no-op. Refused with SGMCMC_EINVAL, the text starting "bnn_particles_cost_grad: ", an
 * earlier check winning over a later one: a NULL theta, Xb, yb, grad or cost_out; a NULL layer_sizes, n_layers outside
 * 1 .. 8, a layer size < 1, a last layer that is not one unit; batch < 1; ld < n_params; ld_grad < n_params;
 * ldx < layer_sizes[0]; a footprint above 160 KiB; n_particles >= 2^31.                                                    */
int sgmcmc_bnn_particles_cost_grad_f32(const float *theta, size_t n_particles, size_t ld, const int *layer_sizes, int n_layers,
                                       const float *Xb, size_t ldx, const float *yb, int batch, double batch_size,
                                       double n_examples, double wdecay, double prior_mean, double prior_var, int add_prior,
                                       float *grad, size_t ld_grad, float *cost_out, sgmcmc_stream_t stream);
int sgmcmc_bnn_particles_cost_grad_f64(const double *theta, size_t n_particles, size_t ld, const int *layer_sizes, int n_layers,
                                       const double *Xb, size_t ldx, const double *yb, int batch, double batch_size,
                                       double n_examples, double wdecay, double prior_mean, double prior_var, int add_prior,
                                       double *grad, size_t ld_grad, double *cost_out, sgmcmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGMCMC_HIP_PARTICLES_H */
