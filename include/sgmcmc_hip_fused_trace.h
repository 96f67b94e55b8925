/* sgmcmc_hip_fused_trace.h -- OPTIONAL thinned-trace add-on of libsgmcmc_hip.so, OUTSIDE the SURVEY.md section 8(b) boundary.
 *
 * include/sgmcmc_hip.h and include/sgmcmc_hip_fused.h declare the whole-step BNN kernel K8, whose launches hand back the LAST
 * parameter vector and the costs: a caller that keeps samples has to end a launch at every kept one and copy theta. This
 * header declares the same kernel writing every k-th theta' into a device matrix itself, so "keep n thinned samples of m
 * chains" is ONE launch whose output sgmcmc_ess_variogram_* (include/sgmcmc_hip_diag.h) reads as it lies. It has a version of
 * its own, so it can grow without touching the boundary or the other add-ons.
 *
 * Conventions are those of sgmcmc_hip.h: extern "C", plain pointers and sizes; 0 on success, a positive hipError_t or a
 * negative SGMCMC_E* code with a thread-local text in sgmcmc_last_error(); launches are asynchronous on `stream` and legal
 * inside stream capture; the library allocates, frees and copies nothing and keeps no process-wide state; arguments are
 * checked on the host before anything is launched.
 */
#ifndef SGMCMC_HIP_FUSED_TRACE_H
#define SGMCMC_HIP_FUSED_TRACE_H

#include "sgmcmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGMCMC_FUSED_TRACE_ABI_VERSION 1

int sgmcmc_fused_trace_abi_version(void);

/* n_steps whole steps per chain, as sgmcmc_bnn_fused_{sghmc,sgld}_steps_* (sgmcmc_hip.h), their `sched` twins and
 * sgmcmc_bnn_fused_rsghmc_steps_* (sgmcmc_hip_fused.h) run them -- same chain, same costs, bit for bit -- and every
 * trace_every-th theta' kept. ONE entry per dtype: the update is an argument.
 *   kind           0 SGHMC, 1 preconditioned SGLD, 2 relativistic SGHMC
 *   rows, n_rows   HOST array (read during the call, not kept) of the kind's DEVICE state rows in the order of its entry:
 *                  kind 0  theta, V, grad, tau, g, v_hat, minv (7);  kind 1  theta, grad, tau, g, v_hat, minv (6);
 *                  kind 2  theta, p, grad (3). Each as there: n_params per chain, chain c at + c * chain_stride, 16-B aligned.
 *   n_params .. prior_var   the 15 net arguments of those entries, same meaning and checks
 *   scalars, n_scalars      HOST array of the kind's by-value scalars in the order of its entry:
 *                  kind 0  eps, scale_grad, mdecay (3);  kind 1  eps, scale_grad, A (3);  kind 2  eps, mass, c, D, b_hat (5)
 *   scalars_steps  NULL, or a DEVICE table [n_steps][5] (sgmcmc_*_scalars_steps_*, sgmcmc_hip_fused.h) that replaces the
 *                  stepsize step by step, as in the `sched` entries (kinds 0, 1: `scalars` is then not read)
 *   first_step, n_steps, burn_in_steps, seed_base, xi, cost_out   as there; burn_in_steps is ignored for kind 2
 *   trace          DEVICE matrix of the step's dtype, any element alignment: chain c owns rows of n_params elements from
 *                  trace + c * trace_chain_stride on, trace_capacity of them
 *   trace_chain_stride   elements between the chains' slabs, >= trace_capacity * n_params (not read for one chain)
 *   trace_row      first row this launch writes (rows before it are left alone: a trace is filled by successive launches)
 *   trace_every    k >= 1: keep every k-th step
 *   trace_phase    steps taken since the last kept one, < trace_every. Step t of the launch (0-based) is kept iff
 *                  (trace_phase + t + 1) % trace_every == 0; the j-th kept step writes theta' -- the bits `theta` holds
 *                  after that step -- to row trace_row + j. The launch keeps (trace_phase + n_steps) / trace_every rows;
 *                  the next launch continues with trace_row advanced by that and phase (trace_phase + n_steps) % trace_every.
 * Refused with SGMCMC_EINVAL: a kind outside 0..2 and n_rows or n_scalars that is not the kind's (first: they decide how
 * the arrays are read); then whatever the untraced entries refuse; then trace NULL, trace_every 0, trace_phase >=
 * trace_every, more kept rows than fit between trace_row and trace_capacity, and for n_chains > 1 a trace_chain_stride
 * below trace_capacity * n_params. n_steps = 0 is a successful no-op. Rows the launch does not keep into are not touched.  */
int sgmcmc_bnn_fused_trace_steps_f32(int kind, float *const *rows, int n_rows, size_t n_params, size_t chain_stride,
                                     int n_chains, const int *layer_sizes, int n_layers, const float *X, const float *y,
                                     size_t n_data, const int *window_starts, int batch, double batch_size,
                                     double n_examples, double wdecay, double prior_mean, double prior_var,
                                     const float *scalars, int n_scalars, const float *scalars_steps, uint64_t first_step,
                                     uint64_t n_steps, uint64_t burn_in_steps, uint64_t seed_base, const float *xi,
                                     float *cost_out, float *trace, size_t trace_chain_stride, uint64_t trace_capacity,
                                     uint64_t trace_row, uint64_t trace_every, uint64_t trace_phase, sgmcmc_stream_t stream);
int sgmcmc_bnn_fused_trace_steps_f64(int kind, double *const *rows, int n_rows, size_t n_params, size_t chain_stride,
                                     int n_chains, const int *layer_sizes, int n_layers, const double *X, const double *y,
                                     size_t n_data, const int *window_starts, int batch, double batch_size,
                                     double n_examples, double wdecay, double prior_mean, double prior_var,
                                     const double *scalars, int n_scalars, const double *scalars_steps, uint64_t first_step,
                                     uint64_t n_steps, uint64_t burn_in_steps, uint64_t seed_base, const double *xi,
                                     double *cost_out, double *trace, size_t trace_chain_stride, uint64_t trace_capacity,
                                     uint64_t trace_row, uint64_t trace_every, uint64_t trace_phase, sgmcmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGMCMC_HIP_FUSED_TRACE_H */
