/* sgmcmc_hip_calib.h -- OPTIONAL add-on of libsgmcmc_hip.so: K20, calibration of the posterior predictive of a kept ensemble
 * against held-out targets: the probability integral transform (PIT) of every target, the coverage of central intervals, a PIT
 * histogram, and the continuous ranked probability score (CRPS) in its exact closed form for a mixture of Gaussians (Grimit,
 * Gneiting, Berrocal and Johnson, "The continuous ranked probability score for circular variables and its application to
 * mesoscale forecast ensemble verification", 2006; `crps_mixnorm` of R's scoringRules). OUTSIDE the SURVEY.md section 8(b)
 * boundary; a version of its own, so it can grow without touching the boundary or the other add-ons.
 *
 * Conventions are those of sgmcmc_hip.h: extern "C", plain pointers and sizes; 0 on success, a positive hipError_t or a
 * negative SGMCMC_E* code with a thread-local text in sgmcmc_last_error(); the launches are asynchronous on `stream` and legal
 * inside stream capture; the library allocates, frees and copies nothing, never synchronises with the host, keeps no
 * process-wide state and uses no atomics; arguments are checked on the host before anything is launched. There is no
 * workspace.
 *
 * The predictive of row r is the equal-weight mixture of the S Gaussians N(means[s][r], var[s]).
 *
 * Input. means element (s, r), the output of draw s at row r, at means[s * ld + r], ld >= n_rows, of the element type (float or
 * double): what sgmcmc_bnn_predict_* and sgmcmc_bnn_score_* write. var double[S], the variance of draw s's Gaussian (for the
 * BNN, exp((double)log_var_s) + 1e-16). y [n_rows] of the element type. 1 <= S <= SGMCMC_CALIB_MAX_DRAWS.
 *
 * The statement. All arithmetic is in double whatever the element type, every written operation rounded once, no contraction.
 *   SQRT2 = 0x1.6a09e667f3bcdp+0      INV_SQRTPI = 0x1.20dd750429b6dp-1
 *   A(d, c):   e = c * SQRT2;  u = d / e;  A = e * (u * erf(u) + exp(-(u * u)) * INV_SQRTPI)            (= E|N(d, c^2)|)
 *   per row r, with mu_s = (double)means[s][r], yy = (double)y[r], sd_s = sqrt(var[s]):
 *     P  = TREE_s( 0.5 * erfc(-(((yy - mu_s) / sd_s) / SQRT2)) )
 *     T  = TREE_s( A(yy - mu_s, sd_s) )
 *     g_s = sum over t = 0 .. s-1, ONE BY ONE ascending from 0.0, of A(mu_s - mu_t, sqrt(var[s] + var[t]))   (g_0 = 0.0)
 *     G  = TREE_s( g_s )
 *     Dg = TREE_s( sqrt(var[s] + var[s]) * (SQRT2 * INV_SQRTPI) )                       (the diagonal pairs, A(0, c))
 *     pit[r]  = P / S
 *     crps[r] = T / S - ((G + G) + Dg) / (2.0 * S * S)
 * TREE_s is the project's fixed order: 256 partials, partial j adds the elements j, j + 256, ... ascending from 0.0, then the
 * halving tree h = 128 .. 1 (part[t] += part[t + h] for t < h). Every g_s is a serial chain of its own, so the result depends
 * on no launch parameter and not on how many rows the call holds. Non-finite inputs are not checked; they propagate by the
 * IEEE rules into their own row only.
 *
 * summary (optional), double[2 + n_levels + n_bins], written by a second small launch behind the first:
 *   summary[0]                = TREE_r( crps[r] )
 *   summary[1]                = the number of rows whose pit or crps is NaN
 *   summary[2 + k]            = the number of rows with 0.5 - 0.5 * levels[k] <= pit[r] <= 0.5 + 0.5 * levels[k]
 *   summary[2 + n_levels + b] = the number of rows with min(n_bins - 1, (int)floor(pit[r] * n_bins)) == b
 * A NaN row is in no interval and in no bin. The counts are exact integers held in doubles.
 *
 * Launch: grid = n_rows, one workgroup per row, of 64 .. 1024 threads (half the draws, rounded up to a power of two). The
 * row's mu, var and g sit in the LDS as doubles: 24 bytes a draw, 96 KiB at the cap. A thread runs the chains g_p and
 * g_(S-1-p), which together hold S - 1 terms whatever p, interleaved while both still run; mu_t and var[t] are read at the same
 * address by every lane, an LDS broadcast.
 */
#ifndef SGMCMC_HIP_CALIB_H
#define SGMCMC_HIP_CALIB_H

#include "sgmcmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGMCMC_CALIB_ABI_VERSION 1

/* the largest number of draws S of one call */
#define SGMCMC_CALIB_MAX_DRAWS 4096
/* the largest n_levels and n_bins of one call */
#define SGMCMC_CALIB_MAX_LEVELS 16
#define SGMCMC_CALIB_MAX_BINS 64

int sgmcmc_calib_abi_version(void);

/* SGMCMC_CALIB_MAX_DRAWS */
int sgmcmc_calib_max_draws(void);

/* K20. pit, crps [n_rows] doubles are required; summary double[2 + n_levels + n_bins] or NULL. levels is a HOST array of
 * n_levels doubles, read during the call and passed by value into the launch. Nothing but those elements is written.
 * Refused with SGMCMC_EINVAL, the text starting "mixture_calibration: " and holding the offending value, an earlier check
 * winning over a later one:
 *   1. S outside 1 .. 4096;   2. n_levels outside 0 .. 16 or n_bins outside 0 .. 64;   3. a level that is not in (0, 1);
 *   4. n_rows = 0 returns 0 here;   5. a NULL means, var, y, pit or crps (named);   6. levels NULL with n_levels > 0;
 *   7. ld < n_rows;   8. an extent that overflows a size_t;   9. n_rows >= 2^31.                                              */
int sgmcmc_mixture_calibration_f32(const float *means, size_t ld, size_t S, size_t n_rows, const double *var, const float *y,
                                   const double *levels, int n_levels, int n_bins, double *pit, double *crps, double *summary,
                                   sgmcmc_stream_t stream);
int sgmcmc_mixture_calibration_f64(const double *means, size_t ld, size_t S, size_t n_rows, const double *var, const double *y,
                                   const double *levels, int n_levels, int n_bins, double *pit, double *crps, double *summary,
                                   sgmcmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGMCMC_HIP_CALIB_H */
