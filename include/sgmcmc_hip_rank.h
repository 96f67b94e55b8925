/* sgmcmc_hip_rank.h -- OPTIONAL add-on of libsgmcmc_hip.so: K18, the rank normalisation of a strided device trace that turns
 * K12 (sgmcmc_hip_chains.h) into the rank-normalised split R-hat and the bulk and tail effective sample sizes of Vehtari,
 * Gelman, Simpson, Carpenter and Buerkner, "Rank-normalization, folding, and localization: an improved R-hat for assessing
 * convergence of MCMC" (2021). OUTSIDE the SURVEY.md section 8(b) boundary; a version of its own, so it can grow without
 * touching the boundary or the other add-ons.
 *
 * Conventions are those of sgmcmc_hip.h: extern "C", plain pointers and sizes; 0 on success, a positive hipError_t or a
 * negative SGMCMC_E* code with a thread-local text in sgmcmc_last_error(); the launch is asynchronous on `stream` and legal
 * inside stream capture; the library allocates, frees and copies nothing, never synchronises with the host, keeps no
 * process-wide state and uses no atomics; arguments are checked on the host before anything is launched. There is no
 * workspace.
 *
 * Input. trace, m, n, P, ld, chain_stride are K12's: element (c, i, p) at trace[c * chain_stride + i * ld + p], rows dense,
 * any element alignment, views of wider (ld > P) or longer (chain_stride > n * ld) buffers without a copy.
 *
 * Split. half = n / 2 (integer division). Split chain s = 2 c + h, h in {0, 1}, holds draws i < half, taken from source
 * draw h * (n - half) + i: for odd n the middle draw is dropped (as ArviZ's _split_chains does). N = 2 * m * half values
 * of each parameter are pooled.
 *
 * Outputs. Four optional double arrays z, z_folded, tail_lo, tail_hi (at least one non-NULL), each of shape (2 m, half, P):
 * element (s, i, p) at out[s * chain_stride_out + i * ld_out + p]. ONE (2 m, half, 4 P) buffer can hold them as four column
 * blocks with ld_out = 4 P; K12 then reads a block, or several adjacent ones, as a view. Nothing but those elements is
 * written.
 *
 * Arithmetic per parameter, in double for both element types (a float is converted first), every written operation rounded
 * once, no contraction. Values compare by IEEE value (-0.0 ties with +0.0). s[0 .. N) are the pooled values ascending.
 *   rank2(x)  = first + last + 2, first and last the 0-based positions of the first and the last element of s equal to x:
 *               twice the 1-based average rank, an exact integer in 2 .. 2 N. The order of equal elements cannot matter.
 *   z         = zeta(rank2), where with D = 2 N + 0.5 (exact)
 *                   zeta(r) =  PPND16((r - 0.75) / D)                  for r <= N + 1     (the argument is <= 0.5)
 *                   zeta(r) = -PPND16(((2 N + 2 - r) - 0.75) / D)      for r >  N + 1
 *               This is Phi^-1((rank - 3/8) / (N + 1/4)) with one division. The upper half is the negated lower half
 *               because one rounded division does not give (D - a) / D = 1 - a / D exactly, so evaluating the quantile
 *               function at both would break z(rank2) = -z(2 N + 2 - rank2) in the last bits; written this way the
 *               antisymmetry holds bit for bit and zeta is strictly increasing.
 *   PPND16    Wichura's algorithm AS241 in double, in the published order (Horner from the highest coefficient; num / den;
 *               the central branch for |p - 0.5| <= 0.425 uses only multiply, add and one divide; the two tail branches
 *               take r = sqrt(-log(p)) first, so their last bits depend on the device's log).
 *   med       = (s[N/2 - 1] + s[N/2]) * 0.5
 *   z_folded  = the same transform of the folded values |x - med| (a second sort, of doubles for both element types)
 *   k_lo      = (N - 1) / 20,   k_hi = (19 * (N - 1) + 19) / 20      (integer divisions)
 *   tail_lo   = x <= s[k_lo] ? 1.0 : 0.0;     tail_hi = x >= s[k_hi] ? 1.0 : 0.0
 * The two order statistics give the indicators of x <= quantile(0.05) and x >= quantile(0.95) under linear interpolation
 * between order statistics (numpy's default): the interpolated quantile lies in [s[floor(h)], s[ceil(h)]], h = q (N - 1),
 * no sample lies strictly between two adjacent order statistics, k_lo = floor(0.05 (N - 1)) and k_hi = ceil(0.95 (N - 1)).
 * Stated on order statistics, the indicators do not depend on how the interpolation rounds.
 *
 * A column that holds a NaN or an infinity gets NaN in all four outputs (K12 then reports it as degenerate); neighbouring
 * columns are not affected. A constant column needs no special case: every z is zeta(N + 1) = PPND16(0.5) = 0 and both
 * indicators are 1 everywhere (K12: NaN / 0 / 1).
 *
 * Launch: grid = P, one workgroup per parameter column, of 64 .. 1024 threads (half the padded count). The column sits in
 * the LDS as doubles next to a 16-bit draw index, padded with +inf to a power of two: 10 bytes a slot, 80 KiB at the cap.
 * An in-LDS bitonic sort on the strict total order (value, draw index) -- so the sorted image, and with it every output, is
 * independent of the workgroup size -- then, straight from the sorted image: tie runs by binary search, PPND16, and one
 * 8-byte store per element to the draw's place (a column's elements are ld_out apart whatever the order, so no order of the
 * stores coalesces them). Results depend on no launch parameter.
 */
#ifndef SGMCMC_HIP_RANK_H
#define SGMCMC_HIP_RANK_H

#include "sgmcmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGMCMC_RANK_ABI_VERSION 1

/* the largest pooled count N = 2 * m * (n / 2) of one call */
#define SGMCMC_RANK_MAX_POOLED 8192
#define SGMCMC_RANK_MAX_CHAINS 2048

int sgmcmc_rank_abi_version(void);

/* SGMCMC_RANK_MAX_POOLED */
int sgmcmc_rank_max_pooled(void);

/* K18. Refused with SGMCMC_EINVAL, the text starting "rank_normalize: " and holding the offending value, an earlier check
 * winning over a later one:
 *   1. m outside 1 .. 2048;   2. n < 4;   3. N = 2 * m * (n / 2) > SGMCMC_RANK_MAX_POOLED;   4. P = 0 returns 0 here;
 *   5. a NULL trace;   6. all four outputs NULL;   7. ld < P;   8. chain_stride < (n - 1) * ld + P;   9. ld_out < P;
 *  10. chain_stride_out < (half - 1) * ld_out + P;   11. an extent that overflows a size_t;   12. P >= 2^31.               */
int sgmcmc_rank_normalize_f32(const float *trace, int m, size_t n, size_t P, size_t ld, size_t chain_stride, double *z,
                              double *z_folded, double *tail_lo, double *tail_hi, size_t ld_out, size_t chain_stride_out,
                              sgmcmc_stream_t stream);
int sgmcmc_rank_normalize_f64(const double *trace, int m, size_t n, size_t P, size_t ld, size_t chain_stride, double *z,
                              double *z_folded, double *tail_lo, double *tail_hi, size_t ld_out, size_t chain_stride_out,
                              sgmcmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGMCMC_HIP_RANK_H */
