/* sgmcmc_hip_ksd.h -- OPTIONAL add-on of libsgmcmc_hip.so: K16, the kernel Stein discrepancy of up to 4096 samples with
 * their scores, OUTSIDE the SURVEY.md section 8(b) boundary.
 *
 * A device trace or a particle set is an (n, dim) matrix of samples x_i; with the scores s_i = grad log p(x_i) next to it
 * (K15 gives them for the small BNN) one call forms the Stein kernel matrix of a base kernel k(x, y) = phi(r2),
 * r2 = |x - y|^2,
 *     k_p(x_i, x_j) = phi <s_i, s_j> + 2 phi' <s_j - s_i, x_i - x_j> - 2 dim phi' - 4 phi'' r2        (phi, phi', phi'' at r2_ij)
 * its row sums, and V = (1 / n^2) sum_ij k_p, U = (1 / (n (n - 1))) sum_{i != j} k_p. The header has a version of its own,
 * so it can grow without touching the boundary or the other add-ons.
 *
 * Conventions are those of sgmcmc_hip.h: extern "C", plain pointers and sizes; 0 on success, a positive hipError_t or a
 * negative SGMCMC_E* code with a thread-local text in sgmcmc_last_error(); launches are asynchronous on `stream` and legal
 * inside stream capture; the library allocates, frees and copies nothing, never synchronises with the host and keeps no
 * process-wide state; arguments are checked on the host before anything is launched.
 *
 * Base kernels (`kind`):
 *   0 IMQ   phi = (c^2 + r2)^beta, c > 0, -1 < beta < 0.   u = c * c + r2;  phi = 1 / sqrt(u) when beta == -0.5, else
 *           pow(u, beta);  phi' = (beta * phi) / u;  phi'' = ((beta - 1) * phi') / u.
 *   1 RBF   phi = exp(-r2 / (2 h2)), h2 > 0.   w = 2 * h2;  phi = exp(-r2 / w);  phi' = -phi / w;  phi'' = -phi' / w.
 *
 * Arithmetic contract (T is the element type of the call):
 *   centring    the samples are centred per column, x~_ic = x_ic - m_c, m_c = (sum_i x_ic) * (1 / n), the sum over i in
 *               eight interleaved ascending chains added in chain order (sgmcmc_hip_svgd_many.h's mean). Centring leaves
 *               r2 and <s_j - s_i, x_i - x_j> unchanged and removes a common offset. The scores are not centred.
 *   sums        three families of sums over the dim columns run on matrix cores, in T, in a fixed k order:
 *               A_ij = <x~_i, x~_j>,  B_ij = <s_i, s_j>,  C_ij = <s_i, x~_j>.  A workgroup owns one pair (I <= J) of 64-row
 *               blocks and one column split; it stages the four tiles X~_I, X~_J, S_I, S_J of a column tile (32 columns in
 *               f32, 16 in f64) once in the LDS and feeds four products from them: A, B, S_I X~_J^T and X~_I S_J^T (a
 *               diagonal block: three products from two tiles), v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64.
 *               The column splits are capped (512 / pairs, at least 1); a workgroup walks the tiles split, split + splits,
 *               ...; partial blocks are added in ascending split order by the REDUCE launch; columns beyond 65 536 go in
 *               phases that start from the workgroup's own partial block. No floating-point atomics. Ragged n and dim
 *               are padded with zeros in the operands; nothing is read or written past dim in a row or past row n. On a
 *               diagonal block A and B are taken from the entries with i <= j and mirrored, so both are exactly symmetric.
 *   pairs       in double from the reduced sums, every written operation rounded once, no contraction:
 *                 r2_ij = max((A_ii + A_jj) - 2 A_ij, 0)
 *                 t_ij  = (C_ij + C_ji) - (C_ii + C_jj)
 *                 k_p   = ((phi * B_ij + (2 * phi') * t_ij) - (2 * dim) * phi') - (4 * phi'') * r2_ij
 *               The diagonal values are read from the same matrices, so r2_ii and t_ii are exactly 0, and (i, j) and (j, i)
 *               share one rounding sequence: the matrix is exactly symmetric. matrix_out is one cast of the double to T.
 *   sums of k_p in double. Row i: lane t of 256 adds k_p(i, j) for j = t, t + 256, ... ascending, the 256 lane sums are then
 *               added by a halving tree (lane t += lane t + 128, + 64, ... + 1). `total` is the sum of the row sums and
 *               `trace` the sum of the diagonal, both by the same scheme. V = total / (n * n),
 *               U = (total - trace) / (n * (n - 1)).
 *   A call is bit-reproducible run to run; its bits depend on (n, dim, kind, c, beta, h2) and the values only, not on ld_x,
 *   ld_s, ld_m, the alignment of a row, or which outputs were asked for (every access to the samples and scores is one
 *   element wide).
 *
 * Launches of one call, in order; sgmcmc_ksd_plan reports them with these ids:
 *   1 MEAN     the column means of the samples for one PHASE of 65 536 columns
 *   2 GRAM     block pairs times `cap` column splits, as above; MEAN and GRAM repeat per phase
 *   3 REDUCE   adds the splits' partial blocks into the n x n matrices A, B, C
 *   4 PAIR     one workgroup per row: k_p of the row, matrix_out, the row sum and the diagonal entry
 *   5 FINISH   one workgroup: total, trace, V, U
 */
#ifndef SGMCMC_HIP_KSD_H
#define SGMCMC_HIP_KSD_H

#include "sgmcmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGMCMC_KSD_ABI_VERSION 1

#define SGMCMC_KSD_MEAN 1
#define SGMCMC_KSD_GRAM 2
#define SGMCMC_KSD_REDUCE 3
#define SGMCMC_KSD_PAIR 4
#define SGMCMC_KSD_FINISH 5

#define SGMCMC_KSD_IMQ 0
#define SGMCMC_KSD_RBF 1

int sgmcmc_ksd_abi_version(void);

/* 4096 */
int sgmcmc_ksd_max_samples(void);

/* Bytes of device workspace for n samples of elem_bytes (4 or 8) each: the reduced matrices A, B and C, the row sums and the
 * diagonal, the column means of one phase and a bounded number of partial blocks. It does not depend on dim. 0 for n outside
 * 2 .. 4096 or another element size. The workspace must be 32-byte aligned.                                              */
size_t sgmcmc_ksd_workspace_bytes(size_t n, size_t elem_bytes);

/* The launches of one sgmcmc_ksd_* call, host arithmetic only. Launch k fills out[4 k .. 4 k + 3] with
 *   { id (above), tile width in columns of dim (0: the launch does not run over dim), grid size in workgroups,
 *     grid cap (GRAM: the largest number of column splits, grid = splits * pairs, a workgroup walks when
 *     ceil(min(dim, 65 536) / tile) > cap; 0: no cap, one workgroup per unit of work) }
 * as long as 4 k + 3 < n_out. Returns the number of launches (MEAN and GRAM once per phase), or SGMCMC_EINVAL for
 * arguments the call would refuse.                                                                                       */
int sgmcmc_ksd_plan(size_t n, size_t dim, size_t elem_bytes, int *out, int n_out);

/* The Stein kernel matrix of the [n x ld_x] samples and their [n x ld_s] scores and its sums. matrix_out: [n x ld_m] of T or
 * NULL; row_sums_out: n doubles or NULL; stats_out: 4 doubles {V, U, total, trace}. c and beta are read for kind 0 only, h2
 * for kind 1 only.
 * Refused with SGMCMC_EINVAL, the text starting "ksd: ", an earlier check winning over a later one:
 *   1. a NULL samples, scores, workspace or stats_out;   2. n outside 2 .. 4096;   3. dim < 1;   4. ld_x < dim;
 *   5. ld_s < dim;   6. kind not 0 or 1;   7. IMQ with c <= 0 or beta outside (-1, 0);   8. RBF with h2 <= 0;
 *   9. matrix_out with ld_m < n;   10. a workspace that is not 32-byte aligned, or dim above 2^34.                      */
int sgmcmc_ksd_f32(const float *samples, size_t ld_x, const float *scores, size_t ld_s, size_t n, size_t dim, int kind,
                   double c, double beta, double h2, void *workspace, float *matrix_out, size_t ld_m, double *row_sums_out,
                   double *stats_out, sgmcmc_stream_t stream);
int sgmcmc_ksd_f64(const double *samples, size_t ld_x, const double *scores, size_t ld_s, size_t n, size_t dim, int kind,
                   double c, double beta, double h2, void *workspace, double *matrix_out, size_t ld_m, double *row_sums_out,
                   double *stats_out, sgmcmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGMCMC_HIP_KSD_H */
