/* sgmcmc_hip_svgd_many.h -- OPTIONAL add-on of libsgmcmc_hip.so: the SVGD step for up to 1024 particles, OUTSIDE the
 * SURVEY.md section 8(b) boundary.
 *
 * sgmcmc_svgd_step_* / sgmcmc_svgd_kernel_* (sgmcmc_hip.h) keep the kernel matrix and a whole column tile of the particles
 * in registers or in the LDS and stop at 128 particles. The entries below are a second path with tiled Gram, median and
 * update kernels for 2 .. 1024 particles. Their argument lists and their semantics are those of their namesakes. The header
 * has a version of its own, so it can grow without touching the boundary or the other add-ons.
 *
 * Conventions are those of sgmcmc_hip.h: extern "C", plain pointers and sizes; 0 on success, a positive hipError_t or a
 * negative SGMCMC_E* code with a thread-local text in sgmcmc_last_error(); launches are asynchronous on `stream` and legal
 * inside stream capture; the library allocates, frees and copies nothing, never synchronises with the host and keeps no
 * process-wide state; arguments are checked on the host before anything is launched.
 *
 * Arithmetic contract (that of csrc/sgmcmc_svgd.hip, restated):
 *   distances   D comes from the Gram matrix g of the COLUMN-CENTRED particles (x~_ic = x_ic - m_c, m_c = (sum_i x_ic) *
 *               (1 / n), the sum over i in eight interleaved ascending chains added in chain order: centring leaves
 *               every distance unchanged and removes a common offset).  s = (g_ii + g_jj) - 2 g_ij with i < j, clamped at 0; dist = sqrt(s);
 *               D_ij = D_ji = dist * dist. One rounding sequence serves (i, j) and (j, i); the diagonal is exactly 0.
 *   median      over all n * n entries of D, the n zeros of the diagonal included: the middle value for an odd count, the
 *               mean of the two middle values for an even one (rank n*n/2 - 1, then the same value if it repeats, else the
 *               smallest larger entry).
 *   bandwidth   h = sqrt(0.5 * median / log(n + 1)), h2 = h * h.
 *   kernel      K_ij = exp(-D_ij / h2 / 2): exactly symmetric, exactly 1 on the diagonal.
 *   row sums    ksum_i: lane t of 256 adds K_ij for j = t, t + 256, ... ascending; the 256 lane sums are then added by a
 *               halving tree (lane t += lane t + 128, + 64, ... + 1).
 *   tail        A = K G and B = K X are kept apart; then, statement for statement as svgd_update_kernel,
 *                 kg   = (-B + x * ksum_i) / h2
 *                 gt   = (A + sign * kg) / n
 *                 hnew = alpha * H + (1 - alpha) * (gt * gt)
 *                 adj  = gt / (fudge + sqrt(hnew))
 *                 x    = x - eps * adj
 *               every written operation rounded once, no contraction.
 *   sums        over columns (Gram) and particles (A, B) have no reference order. This path fixes one: matrix-core
 *               accumulation in a fixed k order, partial Gram blocks added in ascending order of the column split, no
 *               floating-point atomics. (The median's histograms use integer atomics: counts do not depend on order.)
 *               A step is bit-reproducible run to run; its bits depend on (n, dim) and the values only, not on ld, the
 *               alignment of a row, or the width of a memory access (every access to the particle-sized matrices is one
 *               element wide).
 *
 * Launches of one step, in order; sgmcmc_svgd_many_plan reports them with these ids:
 *  11 MEAN        the column means of one PHASE of 65 536 columns, into a buffer of that many elements
 *   1 GRAM        64 x 64 blocks on or above the diagonal times `cap` column splits; a workgroup walks the phase's 64-column
 *                 (f32) / 32-column (f64) tiles  split, split + splits, ...;  v_mfma_{f32,f64}_16x16x4; the two row blocks
 *                 are centred with MEAN's means as they are staged in the LDS; from the second phase on a workgroup starts
 *                 from its own partial block. MEAN and GRAM repeat per phase: one pair of launches up to 65 536 columns,
 *                 ceil(dim / 65 536) pairs in general.
 *   2 REDUCE      adds the splits' partial blocks in ascending order into the n x n Gram matrix
 *   3 DIST        D from the Gram matrix
 *   4 SELECT      one pass of the radix select over the n * n keys, most significant byte first (4 passes in f32, 8 in
 *                 f64): per-workgroup LDS histograms merged with integer atomics
 *   5 NEXT        even counts only: entries <= the selected key are counted, the smallest larger key is found
 *   6 BANDWIDTH   one workgroup: median, h, h2
 *   7 KMATRIX     one workgroup per row: K and its row sum
 *   8 UPDATE      one workgroup per 16-column tile, no cap: the tile of X is staged whole in the LDS BEFORE anything is
 *                 written (every read of X[:, tile] precedes the first write of it; no workgroup touches another's
 *                 columns), G in 128-row chunks; K is the A operand read from global memory; v_mfma_*_16x16x4
 *   9 KGRAD       the UPDATE kernel's instantiation that writes kernel gradients instead (sgmcmc_svgd_many_kernel_*)
 *  10 COPY        K to kernel_out (sgmcmc_svgd_many_kernel_*)
 * Ragged n and dim are padded with zeros in the operands; nothing is read or written past dim in a row.
 */
#ifndef SGMCMC_HIP_SVGD_MANY_H
#define SGMCMC_HIP_SVGD_MANY_H

#include "sgmcmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGMCMC_SVGD_MANY_ABI_VERSION 1

#define SGMCMC_SVGD_MANY_GRAM 1
#define SGMCMC_SVGD_MANY_REDUCE 2
#define SGMCMC_SVGD_MANY_DIST 3
#define SGMCMC_SVGD_MANY_SELECT 4
#define SGMCMC_SVGD_MANY_NEXT 5
#define SGMCMC_SVGD_MANY_BANDWIDTH 6
#define SGMCMC_SVGD_MANY_KMATRIX 7
#define SGMCMC_SVGD_MANY_UPDATE 8
#define SGMCMC_SVGD_MANY_KGRAD 9
#define SGMCMC_SVGD_MANY_COPY 10
#define SGMCMC_SVGD_MANY_MEAN 11

int sgmcmc_svgd_many_abi_version(void);

/* 1024 */
int sgmcmc_svgd_many_max_particles(void);

/* Bytes of device workspace for n_particles particles of elem_bytes (4 or 8) each: header, select counters, D, K, row sums,
 * the column means of one phase and a bounded number of partial Gram blocks. It does not depend on dim. 0 for n_particles outside 2 .. 1024 or another
 * element size. The workspace must be 32-byte aligned.                                                                    */
size_t sgmcmc_svgd_many_workspace_bytes(size_t n_particles, size_t elem_bytes);

/* The launches of one sgmcmc_svgd_many_step_* call, host arithmetic only. Launch k fills out[4 k .. 4 k + 3] with
 *   { id (above), tile width in columns of dim (0: the launch does not run over dim), grid size in workgroups,
 *     grid cap (GRAM: the largest number of column splits, grid = splits * blocks, a workgroup walks when
 *     ceil(min(dim, 65 536) / tile) > cap; SELECT, NEXT: workgroups striding over the n * n keys; 0: no cap, one workgroup
 *     per unit of work) }
 * as long as 4 k + 3 < n_out. Returns the number of launches (MEAN and GRAM once per phase), or SGMCMC_EINVAL for
 * arguments the step would refuse.                                                                                        */
int sgmcmc_svgd_many_plan(size_t n_particles, size_t dim, size_t elem_bytes, int *out, int n_out);

/* One SVGD step in place on the [n_particles x ld] matrices: sgmcmc_svgd_step_*'s arguments and semantics. repulsion_sign
 * is +1 (the reference as written) or -1.
 * Refused with SGMCMC_EINVAL, the text starting "svgd_many_step: ", an earlier check winning over a later one:
 *   1. a NULL particles, grad, hist_grad or workspace;   2. n_particles outside 2 .. 1024;   3. dim < 1;   4. ld < dim;
 *   5. repulsion_sign not +1 or -1;   6. a workspace that is not 32-byte aligned, or dim above 2^34.                      */
int sgmcmc_svgd_many_step_f32(float *particles, const float *grad, float *hist_grad, size_t n_particles, size_t dim,
                              size_t ld, float eps, double alpha, float fudge_factor, int repulsion_sign, void *workspace,
                              sgmcmc_stream_t stream);
int sgmcmc_svgd_many_step_f64(double *particles, const double *grad, double *hist_grad, size_t n_particles, size_t dim,
                              size_t ld, double eps, double alpha, double fudge_factor, int repulsion_sign, void *workspace,
                              sgmcmc_stream_t stream);

/* Kernel matrix [n x n] (dense), summed kernel gradients [n x dim] at pitch kernel_grad_ld (NULL: not wanted) and
 * {median, h, h2}: sgmcmc_svgd_kernel_*'s arguments and semantics; any of the three outputs may be NULL.
 * Refused with SGMCMC_EINVAL, the text starting "svgd_many_kernel: ": a NULL particles or workspace; n_particles outside
 * 2 .. 1024; dim < 1; ld < dim; kernel_grad_out with kernel_grad_ld < dim; a misaligned workspace or dim above 2^34.      */
int sgmcmc_svgd_many_kernel_f32(const float *particles, size_t n_particles, size_t dim, size_t ld, void *workspace,
                                float *kernel_out, float *kernel_grad_out, size_t kernel_grad_ld, float *bandwidth_out,
                                sgmcmc_stream_t stream);
int sgmcmc_svgd_many_kernel_f64(const double *particles, size_t n_particles, size_t dim, size_t ld, void *workspace,
                                double *kernel_out, double *kernel_grad_out, size_t kernel_grad_ld, double *bandwidth_out,
                                sgmcmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGMCMC_HIP_SVGD_MANY_H */
