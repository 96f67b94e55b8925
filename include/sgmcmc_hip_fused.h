/* sgmcmc_hip_fused.h -- OPTIONAL whole-step add-on of libsgmcmc_hip.so, OUTSIDE the SURVEY.md section 8(b) boundary.
 *
 * include/sgmcmc_hip.h (ABI v6) declares the whole-step BNN kernel K8 for SGHMC and SGLD with ONE by-value stepsize per
 * launch (its [whole-step] group). This header declares what the same kernel offers on top of that:
 *   - a stepsize SCHEDULE inside a launch: a device table of one block of five derived scalars per step, which the update
 *     phase of step t reads where a per-step launch reads `sgmcmc_step_opts_t.scalars_dev`;
 *   - relativistic SGHMC (K3's operator) as a third update of the kernel, by value or with such a table.
 * It has a version of its own, so it can grow without touching the boundary.
 *
 * Conventions are those of sgmcmc_hip.h: extern "C", plain pointers and sizes; 0 on success, a positive hipError_t or a
 * negative SGMCMC_E* code with a thread-local text in sgmcmc_last_error(); launches are asynchronous on `stream` and legal
 * inside stream capture; the library allocates, frees and copies nothing and keeps no process-wide state; arguments are
 * checked on the host before anything is launched.
 */
#ifndef SGMCMC_HIP_FUSED_H
#define SGMCMC_HIP_FUSED_H

#include "sgmcmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGMCMC_FUSED_ABI_VERSION 1

int sgmcmc_fused_abi_version(void);

/* HOST-ONLY table builders: fill block_host[t][0..5) , t < n_steps, with the scalars block of the stepsize eps_host[t] -- what
 * sgmcmc_{sghmc,sgld,rsghmc}_scalars_* store in a device block for one stepsize, from the same derivation (same bits):
 *   sghmc   {eps^2, c1, c3, e4, mdecay}           (pysgmcmc/samplers/sghmc.py:111-117,211-217,235)
 *   sgld    {eps, A, A - 0, 2 eps, safe denominator of scale_grad}   (pysgmcmc/samplers/sgld.py:106-108,186-191)
 *   rsghmc  {eps, mass, D, m^2 c^2, noise scale}  (pysgmcmc/samplers/relativistic_sghmc.py:105-106,117-125)
 * Both pointers are HOST memory. Nothing is launched or copied and no device is needed; the caller uploads the block
 * (n_steps * 5 elements) and passes the device copy as `scalars_steps` below. n_steps = 0 is a successful no-op.          */
int sgmcmc_sghmc_scalars_steps_f32(const float *eps_host, size_t n_steps, float scale_grad, float mdecay, float *block_host);
int sgmcmc_sghmc_scalars_steps_f64(const double *eps_host, size_t n_steps, double scale_grad, double mdecay,
                                   double *block_host);
int sgmcmc_sgld_scalars_steps_f32(const float *eps_host, size_t n_steps, float A, float scale_grad, float *block_host);
int sgmcmc_sgld_scalars_steps_f64(const double *eps_host, size_t n_steps, double A, double scale_grad, double *block_host);
int sgmcmc_rsghmc_scalars_steps_f32(const float *eps_host, size_t n_steps, float mass, float c, float D, float b_hat,
                                    float *block_host);
int sgmcmc_rsghmc_scalars_steps_f64(const double *eps_host, size_t n_steps, double mass, double c, double D, double b_hat,
                                    double *block_host);

/* sgmcmc_bnn_fused_{sghmc,sgld}_steps_* with a stepsize per step: the by-value `eps` is replaced by
 *   scalars_steps   DEVICE table [n_steps][5] of the step's dtype (sgmcmc_{sghmc,sgld}_scalars_steps_*), required; row t serves
 *                   step first_step + t of EVERY chain of the launch.
 * Everything else is as in sgmcmc_hip.h. `scale_grad` and `mdecay` / `A` keep their places in the argument list and are not
 * read: the rows carry what is derived from them. A table of n_steps equal stepsizes gives the by-value launch bit for bit. */
int sgmcmc_bnn_fused_sghmc_sched_steps_f32(float *theta, float *V, float *grad, float *tau, float *g, float *v_hat,
                                           float *minv, size_t n_params, size_t chain_stride, int n_chains,
                                           const int *layer_sizes, int n_layers, const float *X, const float *y,
                                           size_t n_data, const int *window_starts, int batch, double batch_size,
                                           double n_examples, double wdecay, double prior_mean, double prior_var,
                                           const float *scalars_steps, float scale_grad, float mdecay, uint64_t first_step,
                                           uint64_t n_steps, uint64_t burn_in_steps, uint64_t seed_base, const float *xi,
                                           float *cost_out, sgmcmc_stream_t stream);
int sgmcmc_bnn_fused_sghmc_sched_steps_f64(double *theta, double *V, double *grad, double *tau, double *g, double *v_hat,
                                           double *minv, size_t n_params, size_t chain_stride, int n_chains,
                                           const int *layer_sizes, int n_layers, const double *X, const double *y,
                                           size_t n_data, const int *window_starts, int batch, double batch_size,
                                           double n_examples, double wdecay, double prior_mean, double prior_var,
                                           const double *scalars_steps, double scale_grad, double mdecay,
                                           uint64_t first_step, uint64_t n_steps, uint64_t burn_in_steps, uint64_t seed_base,
                                           const double *xi, double *cost_out, sgmcmc_stream_t stream);
int sgmcmc_bnn_fused_sgld_sched_steps_f32(float *theta, float *grad, float *tau, float *g, float *v_hat, float *minv,
                                          size_t n_params, size_t chain_stride, int n_chains, const int *layer_sizes,
                                          int n_layers, const float *X, const float *y, size_t n_data,
                                          const int *window_starts, int batch, double batch_size, double n_examples,
                                          double wdecay, double prior_mean, double prior_var, const float *scalars_steps,
                                          float scale_grad, float A, uint64_t first_step, uint64_t n_steps,
                                          uint64_t burn_in_steps, uint64_t seed_base, const float *xi, float *cost_out,
                                          sgmcmc_stream_t stream);
int sgmcmc_bnn_fused_sgld_sched_steps_f64(double *theta, double *grad, double *tau, double *g, double *v_hat, double *minv,
                                          size_t n_params, size_t chain_stride, int n_chains, const int *layer_sizes,
                                          int n_layers, const double *X, const double *y, size_t n_data,
                                          const int *window_starts, int batch, double batch_size, double n_examples,
                                          double wdecay, double prior_mean, double prior_var, const double *scalars_steps,
                                          double scale_grad, double A, uint64_t first_step, uint64_t n_steps,
                                          uint64_t burn_in_steps, uint64_t seed_base, const double *xi, double *cost_out,
                                          sgmcmc_stream_t stream);

/* The whole-step kernel with the relativistic SGHMC update (K3, pysgmcmc/samplers/relativistic_sghmc.py:120-140; same
 * operator and Philox stream as sgmcmc_rsghmc_step_*: noise of element i at step s is xi(seed_base + chain, s, i)).
 *   rows theta, p, grad: as the rows of sgmcmc_bnn_fused_sghmc_steps_* (n_params per chain, chain c at + c * chain_stride,
 *     16-B aligned); there are no preconditioner rows and no burn-in switch. `grad` receives d cost / d theta of the step's
 *     minibatch without the weight-prior term, which the update adds.
 *   eps, mass, c, D, b_hat: as in sgmcmc_rsghmc_step_* (m^2 c^2 a power of two takes the same exact shortcut).
 *   scalars_steps: NULL, or a DEVICE table [n_steps][5] (sgmcmc_rsghmc_scalars_steps_*) that replaces the five by-value
 *     scalars step by step; the divisions by m^2 c^2 are then divisions by the row's value.
 * layer_sizes .. prior_var, first_step, n_steps, seed_base, xi, cost_out and the LDS budget: as in sgmcmc_hip.h.          */
int sgmcmc_bnn_fused_rsghmc_steps_f32(float *theta, float *p, float *grad, size_t n_params, size_t chain_stride,
                                      int n_chains, const int *layer_sizes, int n_layers, const float *X, const float *y,
                                      size_t n_data, const int *window_starts, int batch, double batch_size,
                                      double n_examples, double wdecay, double prior_mean, double prior_var, float eps,
                                      float mass, float c, float D, float b_hat, const float *scalars_steps,
                                      uint64_t first_step, uint64_t n_steps, uint64_t seed_base, const float *xi,
                                      float *cost_out, sgmcmc_stream_t stream);
int sgmcmc_bnn_fused_rsghmc_steps_f64(double *theta, double *p, double *grad, size_t n_params, size_t chain_stride,
                                      int n_chains, const int *layer_sizes, int n_layers, const double *X, const double *y,
                                      size_t n_data, const int *window_starts, int batch, double batch_size,
                                      double n_examples, double wdecay, double prior_mean, double prior_var, double eps,
                                      double mass, double c, double D, double b_hat, const double *scalars_steps,
                                      uint64_t first_step, uint64_t n_steps, uint64_t seed_base, const double *xi,
                                      double *cost_out, sgmcmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGMCMC_HIP_FUSED_H */
