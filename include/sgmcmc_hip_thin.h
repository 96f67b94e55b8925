/* sgmcmc_hip_thin.h -- OPTIONAL add-on of libsgmcmc_hip.so: K17, greedy Stein thinning of up to 4096 samples from their
 * Stein kernel matrix, OUTSIDE the SURVEY.md section 8(b) boundary.
 *
 * K16 (sgmcmc_hip_ksd.h) forms the Stein kernel matrix k_p of a device trace or a particle set. Greedy Stein thinning
 * (Riabiz, Chen, Cockayne, Swietach, Niederer, Mackey, Oates, "Optimal thinning of MCMC output") picks m of its n rows one
 * at a time,
 *     pi(t) = argmin_j  k_p(j, j) / 2  +  sum_{t' < t} k_p(pi(t'), j),
 * and the V-statistic of the first t picks falls out of the same loop. One call selects for `batch` problems at once, one
 * workgroup each, in ONE launch. The header has a version of its own, so it can grow without touching the boundary or the
 * other add-ons.
 *
 * Conventions are those of sgmcmc_hip.h: extern "C", plain pointers and sizes; 0 on success, a positive hipError_t or a
 * negative SGMCMC_E* code with a thread-local text in sgmcmc_last_error(); the launch is asynchronous on `stream` and legal
 * inside stream capture; the library allocates, frees and copies nothing, never synchronises with the host and keeps no
 * process-wide state; arguments are checked on the host before anything is launched. There is no workspace.
 *
 * Problem layout. Problem p of `batch` reads the n x n block that starts at matrix + p * batch_stride with row pitch ld_m,
 * both in elements, size_t arithmetic throughout. batch_stride = k * ld_m + k walks the diagonal blocks of one larger matrix:
 * the chains of one trace are thinned separately after a single K16 call. Problem p writes indices_out[p * m .. p * m + m - 1],
 * row numbers local to its block (0 .. n - 1), and, when path_out is not NULL, path_out[p * m .. p * m + m - 1].
 *
 * Arithmetic contract, in double, every written operation rounded once, the same for both element types (K is the block):
 *     h_j   = 0.5 * (double) K[j][j]              acc_j = 0.0
 *     for t = 1 .. m:
 *         obj_j = acc_j + h_j                     over the candidates j
 *         j*    = the candidate with the smallest obj_j; among equal values the smallest j
 *         S     = S + 2.0 * obj_{j*}              (S starts at 0.0)
 *         indices[t - 1] = j*;   path[t - 1] = S / ((double) t * (double) t)
 *         acc_j = acc_j + (double) K[j*][j]       for every j, read from ROW j* of the block
 * Every j in 0 .. n - 1 is a candidate at every step; with SGMCMC_THIN_DISTINCT (flags bit 0) a picked row is not a candidate
 * again. path[t - 1] is the V-statistic of the first t picks: S equals the sum of k_p over the picked pairs up to rounding.
 *   The matrix is taken as given (its symmetry is not checked: row j* is what is added). Every access to it is one element
 *   wide, so neither the bits nor the legality of a call depend on ld_m, on batch_stride or on the alignment of a block.
 *   Nothing outside the `batch` blocks is read; inside a block nothing past column n - 1 of a row.
 *   Entries are expected finite. With a NaN or an infinity the picks are unspecified (a NaN objective is ranked as +infinity),
 *   but every index written is in 0 .. n - 1 and the launch ends.
 *   A call is bit-reproducible run to run.
 *
 * Launch shape, reported by sgmcmc_stein_thin_plan: grid = batch, one workgroup per problem, of 64 (n <= 64), 256
 * (n <= 256) or 1024 threads; column j belongs to thread j mod block, so a thread holds ceil(n / block) <= 4 columns' acc_j and
 * h_j in registers and a row read is coalesced. Per pick: the (value, index) argmin of a wave by cross-lane moves, the waves'
 * winners combined through the LDS, two barriers. The picks of one problem depend on each other, so a problem cannot use more
 * than one workgroup without a hand-off inside the launch; there is none, and no spin wait, atomic or scratch memory.
 */
#ifndef SGMCMC_HIP_THIN_H
#define SGMCMC_HIP_THIN_H

#include "sgmcmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGMCMC_THIN_ABI_VERSION 1

#define SGMCMC_THIN_DISTINCT 1

int sgmcmc_stein_thin_abi_version(void);

/* 4096 */
int sgmcmc_stein_thin_max_samples(void);

/* The launch of one sgmcmc_stein_thin_* call, host arithmetic only: fills out[0 .. 3] with
 *   { block size in threads, columns per thread, grid size in workgroups, waves per workgroup }
 * as far as n_out reaches (out may be NULL). Returns the number of launches, 1, or SGMCMC_EINVAL for arguments the call
 * would refuse (checks 2 to 4 below), the text starting "stein_thin_plan: ".                                               */
int sgmcmc_stein_thin_plan(size_t n, size_t m, size_t batch, int *out, int n_out);

/* Greedy Stein thinning of `batch` blocks of n x n elements: m picks each into indices_out (batch * m ints), the V-statistic
 * of the first t picks into path_out (batch * m doubles, or NULL).
 * Refused with SGMCMC_EINVAL, the text starting "stein_thin: ", an earlier check winning over a later one:
 *   1. a NULL matrix or indices_out;   2. n outside 2 .. 4096;   3. m outside 1 .. 65536;   4. batch outside 1 .. 65535;
 *   5. ld_m < n;   6. batch > 1 with batch_stride == 0;   7. unknown flag bits;   8. SGMCMC_THIN_DISTINCT with m > n.   */
int sgmcmc_stein_thin_f32(const float *matrix, size_t ld_m, size_t n, size_t m, size_t batch, size_t batch_stride, int flags,
                          int *indices_out, double *path_out, sgmcmc_stream_t stream);
int sgmcmc_stein_thin_f64(const double *matrix, size_t ld_m, size_t n, size_t m, size_t batch, size_t batch_stride, int flags,
                          int *indices_out, double *path_out, sgmcmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGMCMC_HIP_THIN_H */
