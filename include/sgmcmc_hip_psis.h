/* sgmcmc_hip_psis.h -- OPTIONAL add-on of libsgmcmc_hip.so: K19, Pareto-smoothed importance-sampling leave-one-out (PSIS-LOO)
 * of a pointwise log-density matrix that lives on the device (K13's `loglik`), after Vehtari, Gelman and Gabry, "Practical
 * Bayesian model evaluation using leave-one-out cross-validation and WAIC" (2017), Vehtari, Simpson, Gelman, Yao and Gabry,
 * "Pareto smoothed importance sampling" (2024), with the generalised Pareto fit of Zhang and Stephens (2009). OUTSIDE the
 * SURVEY.md section 8(b) boundary; a version of its own, so it can grow without touching the boundary or the other add-ons.
 *
 * Conventions are those of sgmcmc_hip.h: extern "C", plain pointers and sizes; 0 on success, a positive hipError_t or a
 * negative SGMCMC_E* code with a thread-local text in sgmcmc_last_error(); the launches are asynchronous on `stream` and legal
 * inside stream capture; the library allocates, frees and copies nothing, never synchronises with the host, keeps no
 * process-wide state and uses no atomics; arguments are checked on the host before anything is launched. There is no
 * workspace.
 *
 * Input. loglik element (s, r), the log density of observation r under draw s, at loglik[s * ld + r], ld >= n_rows: K13's
 * `loglik`, or a view of a wider buffer. S draws, 2 <= S <= SGMCMC_PSIS_MAX_DRAWS; r_eff > 0, the relative efficiency of the
 * draws (1 for independent ones).
 *
 * Sums. Every sum below but Z of row_lppd uses the project's fixed order: 256 partials, partial j adds the elements j,
 * j + 256, ... ascending from 0.0, then the halving tree h = 128 .. 1 (part[t] += part[t + h] for t < h). A maximum is fmax.
 * logsumexp(v) is m = max v; m + log(sum exp(v - m)). Everything is in double, every written operation rounded once, no
 * contraction. The result therefore depends on no launch parameter and not on how many columns the call holds.
 *
 * One column: l[s], s < S.
 *   1. lr[s] = -l[s];  lw[s] = lr[s] - max lr
 *   2. M = min(ceil(0.2 S), ceil(3 sqrt(S / r_eff))) clamped to 1 .. S - 1, computed on the host in double
 *   3. sort by the strict total order (value, draw index);  cut = max(sorted[S - M - 1], log(DBL_MIN)), the latter the
 *      constant -0x1.6232bdd7abcd2p+9. The tail is every draw with lw > cut, in sorted order; n_tail <= M is its length
 *      (ties at the cut make it smaller). With a small r_eff the tail reaches ceil(0.2 S) draws, 1639 at the cap.
 *   4. n_tail <= 4: khat = +inf, nothing is smoothed
 *   5. otherwise, with n = n_tail, ec = exp(cut), x[i] = exp(lw_tail[i]) - ec ascending:
 *        G = 30 + floor(sqrt(n));  q = floor(n / 4 + 0.5) - 1
 *        b_j = (1 - sqrt(G / (j - 0.5))) / (3 x[q]) + 1 / x[n - 1]                            j = 1 .. G
 *        k_j = (sum_i log1p(-b_j x[i])) / n;   L_j = n (log(-(b_j / k_j)) - k_j - 1)
 *        w_j = 1 / sum_t exp(L_t - L_j); a weight below 10 DBL_EPSILON becomes 0, then w_j = w_j / sum_t w_t
 *        b = sum_j b_j w_j;  kk = (sum_i log1p(-b x[i])) / n;  sigma = -kk / b;  khat = (n kk + 5) / (n + 10)
 *        khat finite: p_i = (i + 0.5) / n,  y_i = sigma expm1(-khat log1p(-p_i)) / khat  (-sigma log1p(-p_i) when khat is
 *        exactly 0), and the tail draw at sorted position i gets lw = log(y_i + ec). A non-finite khat is reported as it is
 *        and leaves the tail as it was.
 *   6. lw = min(lw, 0)
 *   7. lwn = lw - logsumexp(lw)                  (sums over the draws run in draw order s, not in sorted order)
 *   8. elpd_loo = logsumexp(lwn + l)
 *   9. row_lppd = (m + log Z) - log((double)S), m = max l, Z = sum_s exp(l[s] - m) added ONE BY ONE in draw order from 0.0:
 *      K13's statement, so the bits are those sgmcmc_bnn_score_* writes for the same column.
 * A column that holds a NaN or an infinity gets NaN in elpd_loo, khat, row_lppd and its weights, and n_tail = -1;
 * neighbouring columns are not affected. A constant column needs no special case: n_tail = 0, khat = +inf, uniform weights.
 *
 * Launch: grid = n_rows, one workgroup per observation column, of 64 .. 1024 threads (half the padded count). The column sits
 * in the LDS as doubles next to a 16-bit draw index and the 16-bit inverse permutation, padded with +inf to a power of two:
 * 12 bytes a slot, 96 KiB at the cap. An in-LDS bitonic sort on (value, draw index), K18's, so the sorted image is
 * independent of the workgroup size; the tail is smoothed in place in the sorted image; the grid fit gives every wave one
 * grid point at a time, its 256 partials four to a lane, and folds them in the stated order by register shuffles.
 */
#ifndef SGMCMC_HIP_PSIS_H
#define SGMCMC_HIP_PSIS_H

#include "sgmcmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGMCMC_PSIS_ABI_VERSION 1

/* the largest number of draws S of one call */
#define SGMCMC_PSIS_MAX_DRAWS 8192

int sgmcmc_psis_abi_version(void);

/* SGMCMC_PSIS_MAX_DRAWS */
int sgmcmc_psis_max_draws(void);

/* K19. elpd_loo, khat [n_rows] doubles and n_tail [n_rows] ints are required; row_lppd [n_rows] or NULL; log_weights, lwn as
 * an (S, n_rows) matrix at ld_w >= n_rows, or NULL; summary double[4] or NULL: { sum elpd_loo, sum row_lppd, the number of
 * rows with khat > 0.7, the number of rows that held a NaN or an infinity }, each in the 256-partials-then-tree order over
 * the rows, written by a second small launch behind the first (the row_lppd sum is formed from the column when row_lppd is
 * NULL). Nothing but those elements is written.
 * Refused with SGMCMC_EINVAL, the text starting "psis_loo: " and holding the offending value, an earlier check winning over a
 * later one:
 *   1. S outside 2 .. 8192;   2. r_eff not a positive finite number;   3. n_rows = 0 returns 0 here;   4. a NULL loglik,
 *   elpd_loo, khat or n_tail (named);   5. ld < n_rows;   6. log_weights with ld_w < n_rows;   7. an extent that overflows a
 *   size_t;   8. n_rows >= 2^31.                                                                                             */
int sgmcmc_psis_loo(const double *loglik, size_t ld, size_t S, size_t n_rows, double r_eff, double *elpd_loo, double *khat,
                    int *n_tail, double *row_lppd, double *log_weights, size_t ld_w, double *summary, sgmcmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGMCMC_HIP_PSIS_H */
