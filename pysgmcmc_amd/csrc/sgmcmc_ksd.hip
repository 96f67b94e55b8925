// sgmcmc_ksd.hip -- K16: the kernel Stein discrepancy of 2 .. 4096 samples and their scores behind
// include/sgmcmc_hip_ksd.h. The O(n^2 dim) part is three families of Gram-type sums, A = X~ X~^T, B = S S^T and C = S X~^T,
// the work of sgmcmc_svgd_many.hip's Gram kernel; the pair formula and the sums of k_p run in double from the reduced sums.
//
// One call, in launch order (ids of the header):
//   MEAN    the column means of the samples over all n rows of one PHASE of 65 536 columns, into a buffer of that many
//           elements (the workspace does not grow with dim): 32 columns x 8 interleaved row chains per workgroup.
//   GRAM    grid = splits x pairs: workgroup (split, block pair bi <= bj) stages the tiles X~_bi, X~_bj, S_bi, S_bj of a
//           column tile in the LDS (the samples centred as they are staged) and accumulates the four 64 x 64 blocks
//           X~_bi X~_bj^T, S_bi S_bj^T, S_bi X~_bj^T, X~_bi S_bj^T (a diagonal pair: the first three, from two tiles) over
//           the phase's tiles split, split + splits, ... with v_mfma_*_16x16x4. Wave w owns rows 16 w .. 16 w + 15 of each
//           block and its four 16-column blocks. The next tile's elements are fetched into registers before the products of
//           the current one, so the loads fly under the matrix cores (profiles/ksd.txt: 1.4 x). From the second phase on the
//           accumulators start from the workgroup's own partial blocks.
//   REDUCE  partial blocks added in ascending split order, scattered into A, B (mirrored) and C.
//   PAIR    workgroup i: k_p(i, j) in double for j = t, t + 256, ..., matrix_out, the row sum by a halving tree, k_p(i, i).
//   FINISH  one workgroup: total over the row sums and trace over the diagonal by the same scheme, V and U.
// Every access to the samples and scores is one element wide and coalesced over 16 or 32 adjacent columns, so the bits cannot
// depend on a pitch or an alignment.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sgmcmc_hip_ksd.h"

#pragma clang fp contract(off)

#include "sgmcmc_host.hpp"

using namespace sgmcmc_host;

namespace {

constexpr int KSD_MAX_SAMPLES = 4096;
constexpr int KSD_THREADS = 256;
constexpr int KSD_GB = 64;                    // rows and columns of a block
constexpr int KSD_BLOCK_ELEMS = KSD_GB * KSD_GB;
constexpr int KSD_PRODUCTS = 4;               // A, B, S_I X~_J^T, X~_I S_J^T
constexpr int KSD_GRAM_WGS = 512;             // splits x pairs stays at or below this (and is at least `pairs`)
constexpr int KSD_PHASE_COLS = 65536;         // columns per MEAN / GRAM phase: the size of the means buffer
constexpr int KSD_MEAN_COLS = 32, KSD_MEAN_CHAINS = KSD_THREADS / KSD_MEAN_COLS;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

// 16x16x4 matrix-core step: A lane l = a[row l & 15][k = l >> 4], B lane l = b[k = l >> 4][column l & 15]; output register r
// of lane l = row `row(l >> 4, r)`, column l & 15
template <typename T> struct Mfma16;
template <> struct Mfma16<float> {
    typedef f32x4 Acc;
    static __device__ __forceinline__ Acc mma(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __host__ __device__ __forceinline__ int row(int lane_hi, int reg) { return 4 * lane_hi + reg; }
};
template <> struct Mfma16<double> {
    typedef f64x4 Acc;
    static __device__ __forceinline__ Acc mma(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __host__ __device__ __forceinline__ int row(int lane_hi, int reg) { return lane_hi + 4 * reg; }
};

inline int ksd_nb64(int n) { return (n + KSD_GB - 1) / KSD_GB; }
inline int ksd_pairs(int n) { const int b = ksd_nb64(n); return b * (b + 1) / 2; }
inline int ksd_split_cap(int n) { const int c = KSD_GRAM_WGS / ksd_pairs(n); return c < 1 ? 1 : c; }
constexpr int ksd_gram_tile(size_t esize) { return esize == 4 ? 32 : 16; }

// workspace layout, in bytes; every offset is a multiple of 128
struct KsdWs {
    size_t A, B, C, rows, diag, means, parts, total;
};

inline KsdWs ksd_ws(int n, size_t esize) {
    auto up = [](size_t b) { return (b + 127) & ~(size_t)127; };
    const size_t nn = up((size_t)n * n * esize);
    KsdWs w;
    size_t off = 0;
    w.A = off; off += nn;
    w.B = off; off += nn;
    w.C = off; off += nn;
    w.rows = off; off += up((size_t)n * sizeof(double));
    w.diag = off; off += up((size_t)n * sizeof(double));
    w.means = off; off += up((size_t)KSD_PHASE_COLS * esize);
    w.parts = off; off += up((size_t)ksd_split_cap(n) * ksd_pairs(n) * KSD_PRODUCTS * KSD_BLOCK_ELEMS * esize);
    w.total = off;
    return w;
}

__device__ __forceinline__ void decode_pair(int p, int nb, int &bi, int &bj) {
    bi = 0;
    int row = nb;
    while (p >= row) { p -= row; ++bi; --row; }
    bj = bi + p;
}

// ---------------------------------------------------------------------------------------------
// MEAN, GRAM, REDUCE
// ---------------------------------------------------------------------------------------------
// means[c] = (sum_i X[i][c0 + c]) * (1 / n) for the pcols columns of one phase: chain k adds the rows k, k + 8, ... in
// ascending order, the eight chains are then added in chain order
template <typename T>
__global__ __launch_bounds__(KSD_THREADS) void ksd_mean_kernel(const T *__restrict__ X, size_t ld, int n, size_t c0, int pcols,
                                                                T *__restrict__ means) {
    __shared__ T msum[KSD_MEAN_CHAINS * KSD_MEAN_COLS];
    const int t = threadIdx.x, c = t % KSD_MEAN_COLS, chain = t / KSD_MEAN_COLS;
    const int lc = blockIdx.x * KSD_MEAN_COLS + c;
    T s = (T)0;
    if (lc < pcols) {
        const T *col = X + c0 + (size_t)lc;
#pragma unroll 8
        for (int r = chain; r < n; r += KSD_MEAN_CHAINS) s += col[(size_t)r * ld];
    }
    msum[chain * KSD_MEAN_COLS + c] = s;
    __syncthreads();
    if (t < KSD_MEAN_COLS && lc < pcols) {
        T m = msum[t];
#pragma unroll
        for (int k = 1; k < KSD_MEAN_CHAINS; ++k) m += msum[k * KSD_MEAN_COLS + t];
        means[lc] = m * ((T)1 / (T)n);
    }
}

template <typename T>
__global__ __launch_bounds__(KSD_THREADS) void ksd_gram_kernel(const T *__restrict__ X, size_t ld_x, const T *__restrict__ S,
                                                                size_t ld_s, int n, size_t c0, int pcols,
                                                                const T *__restrict__ means, int accumulate, int nb64,
                                                                int pairs, int splits, T *__restrict__ parts) {
    constexpr int TC = ksd_gram_tile(sizeof(T)), P = TC + 16 / (int)sizeof(T), RG = KSD_THREADS / TC, NR = KSD_GB / RG;
    __shared__ T xa[KSD_GB * P];
    __shared__ T xb[KSD_GB * P];
    __shared__ T sa[KSD_GB * P];
    __shared__ T sb[KSD_GB * P];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int c = t % TC, rg = t / TC;
    const int split = blockIdx.x / pairs;
    int bi, bj;
    decode_pair(blockIdx.x % pairs, nb64, bi, bj);
    const bool off_diag = bi != bj;                        // uniform over the workgroup
    const T *xbp = off_diag ? xb : xa, *sbp = off_diag ? sb : sa;
    T *out = parts + (size_t)blockIdx.x * (KSD_PRODUCTS * KSD_BLOCK_ELEMS);
    typename Mfma16<T>::Acc acc[KSD_PRODUCTS][4];
#pragma unroll
    for (int q = 0; q < KSD_PRODUCTS; ++q)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc[q][cb][r] = (accumulate && (q < 3 || off_diag)) ? out[(((q * 4 + wave) * 4 + cb) * 4 + r) * 64 + lane] : (T)0;

    const int n_tiles = (pcols + TC - 1) / TC;
    // a tile's elements and its column's mean in registers; a padded sample holds the mean itself, so that x - m is +0
    T vxa[NR], vxb[NR], vsa[NR], vsb[NR], m = (T)0;
    auto fetch = [&](int tile) {
        const int lc = tile * TC + c;
        const bool cv = lc < pcols;
        const size_t col = c0 + (size_t)lc;
        m = cv ? means[lc] : (T)0;
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const int row = rg + RG * k;
            const int ra = KSD_GB * bi + row, rb = KSD_GB * bj + row;
            vxa[k] = m; vxb[k] = m; vsa[k] = (T)0; vsb[k] = (T)0;
            if (cv && ra < n) {
                vxa[k] = X[(size_t)ra * ld_x + col];
                vsa[k] = S[(size_t)ra * ld_s + col];
            }
            if (off_diag && cv && rb < n) {
                vxb[k] = X[(size_t)rb * ld_x + col];
                vsb[k] = S[(size_t)rb * ld_s + col];
            }
        }
    };
    if (split < n_tiles) fetch(split);
    for (int tile = split; tile < n_tiles; tile += splits) {
        __syncthreads();                                   // the previous tile's operands are consumed
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const int row = rg + RG * k;
            xa[row * P + c] = vxa[k] - m;
            sa[row * P + c] = vsa[k];
            if (off_diag) {
                xb[row * P + c] = vxb[k] - m;
                sb[row * P + c] = vsb[k];
            }
        }
        __syncthreads();
        if (tile + splits < n_tiles) fetch(tile + splits);  // the next tile's loads fly under this tile's products
#pragma unroll 2
        for (int ks = 0; ks < TC / 4; ++ks) {
            const int kk = 4 * ks + (lane >> 4);
            const T ax = xa[(16 * wave + (lane & 15)) * P + kk];
            const T as = sa[(16 * wave + (lane & 15)) * P + kk];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const T bx = xbp[(16 * cb + (lane & 15)) * P + kk];
                const T bs = sbp[(16 * cb + (lane & 15)) * P + kk];
                acc[0][cb] = Mfma16<T>::mma(ax, bx, acc[0][cb]);                  // <x~_i, x~_j>
                acc[1][cb] = Mfma16<T>::mma(as, bs, acc[1][cb]);                  // <s_i, s_j>
                acc[2][cb] = Mfma16<T>::mma(as, bx, acc[2][cb]);                  // <s_i, x~_j> = C_ij
                if (off_diag) acc[3][cb] = Mfma16<T>::mma(ax, bs, acc[3][cb]);    // <x~_i, s_j> = C_ji
            }
        }
    }
#pragma unroll
    for (int q = 0; q < KSD_PRODUCTS; ++q) {
        if (q == 3 && !off_diag) break;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(((q * 4 + wave) * 4 + cb) * 4 + r) * 64 + lane] = acc[q][cb][r];
    }
}

template <typename T>
__global__ __launch_bounds__(KSD_THREADS) void ksd_reduce_kernel(const T *__restrict__ parts, int n, int nb64, int pairs,
                                                                  int splits, T *__restrict__ A, T *__restrict__ B,
                                                                  T *__restrict__ C) {
    const int idx = blockIdx.x * KSD_THREADS + threadIdx.x;
    if (idx >= pairs * KSD_PRODUCTS * KSD_BLOCK_ELEMS) return;
    int bi, bj;
    decode_pair(idx / (KSD_PRODUCTS * KSD_BLOCK_ELEMS), nb64, bi, bj);
    const int q = (idx / KSD_BLOCK_ELEMS) % KSD_PRODUCTS, e = idx % KSD_BLOCK_ELEMS;
    if (q == 3 && bi == bj) return;                        // a diagonal pair has no fourth product
    const int lane = e & 63, r = (e >> 6) & 3, cb = (e >> 8) & 3, w = e >> 10;
    const int i = KSD_GB * bi + 16 * w + Mfma16<T>::row(lane >> 4, r), j = KSD_GB * bj + 16 * cb + (lane & 15);
    if (i >= n || j >= n) return;
    if (q < 2 && i > j) return;                            // A, B on a diagonal pair: the upper triangle, mirrored
    const size_t stride = (size_t)pairs * (KSD_PRODUCTS * KSD_BLOCK_ELEMS);
    T s = parts[idx];
    for (int k = 1; k < splits; ++k) s += parts[(size_t)k * stride + idx];
    const size_t ij = (size_t)i * n + j, ji = (size_t)j * n + i;
    if (q == 0) { A[ij] = s; A[ji] = s; }
    else if (q == 1) { B[ij] = s; B[ji] = s; }
    else if (q == 2) C[ij] = s;
    else C[ji] = s;
}

// ---------------------------------------------------------------------------------------------
// PAIR, FINISH
// ---------------------------------------------------------------------------------------------
struct KsdKernel { int kind; double c2, beta, bm1, w; int rsqrt; };

// phi, phi' and phi'' at r2 (the header's statement)
__device__ __forceinline__ void ksd_phi(const KsdKernel &k, double r2, double &phi, double &d1, double &d2) {
    if (k.kind == SGMCMC_KSD_IMQ) {
        const double u = k.c2 + r2;
        phi = k.rsqrt ? 1.0 / __builtin_sqrt(u) : pow(u, k.beta);
        d1 = (k.beta * phi) / u;
        d2 = (k.bm1 * d1) / u;
    } else {
        phi = exp(-r2 / k.w);
        d1 = -phi / k.w;
        d2 = -d1 / k.w;
    }
}

// lane sums -> red[0] by the halving tree; every lane of the workgroup calls it
__device__ __forceinline__ double ksd_tree(double *red, double part) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = part;
    __syncthreads();
    for (int off = KSD_THREADS / 2; off > 0; off >>= 1) {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
    return red[0];
}

template <typename T>
__global__ __launch_bounds__(KSD_THREADS) void ksd_pair_kernel(const T *__restrict__ A, const T *__restrict__ B,
                                                                const T *__restrict__ C, int n, double two_dim, KsdKernel kern,
                                                                T *__restrict__ matrix_out, size_t ld_m,
                                                                double *__restrict__ rows, double *__restrict__ diag,
                                                                double *__restrict__ row_sums_out) {
    __shared__ double red[KSD_THREADS];
    const int i = blockIdx.x, t = threadIdx.x;
    const size_t ri = (size_t)i * n;
    const double a_ii = (double)A[ri + i], c_ii = (double)C[ri + i];
    double part = 0.0;
    for (int j = t; j < n; j += KSD_THREADS) {
        const size_t rj = (size_t)j * n;
        const double a_jj = (double)A[rj + j], c_jj = (double)C[rj + j];
        const double a_ij = (double)A[ri + j], b_ij = (double)B[ri + j];
        const double c_ij = (double)C[ri + j], c_ji = (double)C[rj + i];
        double r2 = (a_ii + a_jj) - 2.0 * a_ij;
        r2 = r2 > 0.0 ? r2 : 0.0;
        const double tt = (c_ij + c_ji) - (c_ii + c_jj);
        double phi, d1, d2;
        ksd_phi(kern, r2, phi, d1, d2);
        const double kp = ((phi * b_ij + (2.0 * d1) * tt) - two_dim * d1) - (4.0 * d2) * r2;
        if (matrix_out) matrix_out[(size_t)i * ld_m + j] = (T)kp;
        if (j == i) diag[i] = kp;
        part += kp;
    }
    const double sum = ksd_tree(red, part);
    if (t == 0) {
        rows[i] = sum;
        if (row_sums_out) row_sums_out[i] = sum;
    }
}

__global__ __launch_bounds__(KSD_THREADS) void ksd_finish_kernel(const double *__restrict__ rows,
                                                                  const double *__restrict__ diag, int n,
                                                                  double *__restrict__ stats_out) {
    __shared__ double red[KSD_THREADS];
    const int t = threadIdx.x;
    double pr = 0.0, pd = 0.0;
    for (int j = t; j < n; j += KSD_THREADS) { pr += rows[j]; pd += diag[j]; }
    const double total = ksd_tree(red, pr);
    const double trace = ksd_tree(red, pd);
    if (t == 0) {
        const double nd = (double)n;
        stats_out[0] = total / (nd * nd);
        stats_out[1] = (total - trace) / (nd * (nd - 1.0));
        stats_out[2] = total;
        stats_out[3] = trace;
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// the column phases of MEAN / GRAM and the column splits of GRAM, the same in every phase
struct KsdGram { int tc, pairs, cap, splits; size_t phases; };

inline KsdGram ksd_gram_geom(int n, size_t dim, size_t esize) {
    KsdGram g;
    g.tc = ksd_gram_tile(esize);
    g.pairs = ksd_pairs(n);
    g.cap = ksd_split_cap(n);
    const size_t first = dim < (size_t)KSD_PHASE_COLS ? dim : (size_t)KSD_PHASE_COLS;   // the widest phase
    const size_t n_tiles = (first + g.tc - 1) / g.tc;
    g.splits = (int)(n_tiles < (size_t)g.cap ? n_tiles : (size_t)g.cap);
    g.phases = (dim + KSD_PHASE_COLS - 1) / KSD_PHASE_COLS;
    return g;
}

inline int ksd_phase_cols(size_t dim, size_t ph) {
    const size_t left = dim - ph * KSD_PHASE_COLS;
    return (int)(left < (size_t)KSD_PHASE_COLS ? left : (size_t)KSD_PHASE_COLS);
}

inline int ksd_reduce_grid(int pairs) { return (pairs * KSD_PRODUCTS * KSD_BLOCK_ELEMS + KSD_THREADS - 1) / KSD_THREADS; }

// the launches of one call: all are counted, those that fit `room` are written
struct KsdPlan {
    int *out;
    int room;
    long long k;
    void add(int id, int tile, int grid, int cap) {
        if (out && 4 * k + 3 < room) { out[4 * k] = id; out[4 * k + 1] = tile; out[4 * k + 2] = grid; out[4 * k + 3] = cap; }
        ++k;
    }
};

inline long long ksd_plan(int n, size_t dim, size_t esize, int *out, int room) {
    const KsdGram g = ksd_gram_geom(n, dim, esize);
    KsdPlan p = {out, room, 0};
    for (size_t ph = 0; ph < g.phases; ++ph) {
        p.add(SGMCMC_KSD_MEAN, KSD_MEAN_COLS, (ksd_phase_cols(dim, ph) + KSD_MEAN_COLS - 1) / KSD_MEAN_COLS, 0);
        p.add(SGMCMC_KSD_GRAM, g.tc, g.splits * g.pairs, g.cap);
    }
    p.add(SGMCMC_KSD_REDUCE, 0, ksd_reduce_grid(g.pairs), 0);
    p.add(SGMCMC_KSD_PAIR, 0, n, 0);
    p.add(SGMCMC_KSD_FINISH, 0, 1, 0);
    return p.k;
}

int ksd_check(const char *who, bool nulls, size_t n, size_t dim, size_t ld_x, size_t ld_s) {
    if (nulls) return fail(SGMCMC_EINVAL, "%s: null pointer", who);
    if (n < 2 || n > (size_t)KSD_MAX_SAMPLES) return fail(SGMCMC_EINVAL, "%s: n = %zu outside [2, %d]", who, n, KSD_MAX_SAMPLES);
    if (dim < 1) return fail(SGMCMC_EINVAL, "%s: dim < 1", who);
    if (ld_x < dim) return fail(SGMCMC_EINVAL, "%s: ld_x < dim", who);
    if (ld_s < dim) return fail(SGMCMC_EINVAL, "%s: ld_s < dim", who);
    return 0;
}

template <typename T>
int ksd_impl(const T *X, size_t ld_x, const T *S, size_t ld_s, size_t n_, size_t dim, int kind, double c, double beta,
             double h2, void *workspace, T *matrix_out, size_t ld_m, double *row_sums_out, double *stats_out,
             sgmcmc_stream_t stream) {
    const char *who = "ksd";
    int rc = ksd_check(who, !X || !S || !workspace || !stats_out, n_, dim, ld_x, ld_s);
    if (rc) return rc;
    if (kind != SGMCMC_KSD_IMQ && kind != SGMCMC_KSD_RBF) return fail(SGMCMC_EINVAL, "%s: kind must be 0 (IMQ) or 1 (RBF)", who);
    if (kind == SGMCMC_KSD_IMQ && (!(c > 0.0) || !std::isfinite(c) || !(beta > -1.0 && beta < 0.0)))
        return fail(SGMCMC_EINVAL, "%s: IMQ needs c > 0 and -1 < beta < 0, got c = %g, beta = %g", who, c, beta);
    if (kind == SGMCMC_KSD_RBF && (!(h2 > 0.0) || !std::isfinite(h2)))
        return fail(SGMCMC_EINVAL, "%s: RBF needs h2 > 0, got %g", who, h2);
    if (matrix_out && ld_m < n_) return fail(SGMCMC_EINVAL, "%s: ld_m < n", who);
    if (reinterpret_cast<uintptr_t>(workspace) & 31) return fail(SGMCMC_EINVAL, "%s: workspace is not 32-byte aligned", who);
    if (dim > ((size_t)1 << 34)) return fail(SGMCMC_EINVAL, "%s: dim above 2^34", who);

    const int n = (int)n_;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    const KsdWs w = ksd_ws(n, sizeof(T));
    const KsdGram gg = ksd_gram_geom(n, dim, sizeof(T));
    const int nb64 = ksd_nb64(n), pairs = gg.pairs, splits = gg.splits;
    T *A = reinterpret_cast<T *>(ws + w.A), *B = reinterpret_cast<T *>(ws + w.B), *C = reinterpret_cast<T *>(ws + w.C);
    T *means = reinterpret_cast<T *>(ws + w.means), *parts = reinterpret_cast<T *>(ws + w.parts);
    double *rows = reinterpret_cast<double *>(ws + w.rows), *diag = reinterpret_cast<double *>(ws + w.diag);
    for (size_t ph = 0; ph < gg.phases; ++ph) {
        const size_t c0 = ph * KSD_PHASE_COLS;
        const int pcols = ksd_phase_cols(dim, ph);
        hipLaunchKernelGGL((ksd_mean_kernel<T>), dim3((pcols + KSD_MEAN_COLS - 1) / KSD_MEAN_COLS), dim3(KSD_THREADS), 0, st, X,
                           ld_x, n, c0, pcols, means);
        if ((rc = launched("ksd_mean_kernel"))) return rc;
        hipLaunchKernelGGL((ksd_gram_kernel<T>), dim3(splits * pairs), dim3(KSD_THREADS), 0, st, X, ld_x, S, ld_s, n, c0, pcols,
                           (const T *)means, (int)(ph > 0), nb64, pairs, splits, parts);
        if ((rc = launched("ksd_gram_kernel"))) return rc;
    }
    hipLaunchKernelGGL((ksd_reduce_kernel<T>), dim3(ksd_reduce_grid(pairs)), dim3(KSD_THREADS), 0, st, (const T *)parts, n, nb64,
                       pairs, splits, A, B, C);
    if ((rc = launched("ksd_reduce_kernel"))) return rc;
    KsdKernel kern;
    kern.kind = kind;
    kern.c2 = c * c;
    kern.beta = beta;
    kern.bm1 = beta - 1.0;
    kern.w = 2.0 * h2;
    kern.rsqrt = beta == -0.5;
    hipLaunchKernelGGL((ksd_pair_kernel<T>), dim3(n), dim3(KSD_THREADS), 0, st, (const T *)A, (const T *)B, (const T *)C, n,
                       2.0 * (double)dim, kern, matrix_out, ld_m, rows, diag, row_sums_out);
    if ((rc = launched("ksd_pair_kernel"))) return rc;
    hipLaunchKernelGGL(ksd_finish_kernel, dim3(1), dim3(KSD_THREADS), 0, st, (const double *)rows, (const double *)diag, n,
                       stats_out);
    return launched("ksd_finish_kernel");
}

}  // namespace

extern "C" {

int sgmcmc_ksd_abi_version(void) { return SGMCMC_KSD_ABI_VERSION; }

int sgmcmc_ksd_max_samples(void) { return KSD_MAX_SAMPLES; }

size_t sgmcmc_ksd_workspace_bytes(size_t n, size_t elem_bytes) {
    if (n < 2 || n > (size_t)KSD_MAX_SAMPLES || (elem_bytes != 4 && elem_bytes != 8)) return 0;
    return ksd_ws((int)n, elem_bytes).total;
}

int sgmcmc_ksd_plan(size_t n, size_t dim, size_t elem_bytes, int *out, int n_out) {
    const char *who = "ksd_plan";
    const int rc = ksd_check(who, false, n, dim, dim, dim);
    if (rc) return rc;
    if (elem_bytes != 4 && elem_bytes != 8) return fail(SGMCMC_EINVAL, "%s: elem_bytes must be 4 or 8", who);
    if (dim > ((size_t)1 << 34)) return fail(SGMCMC_EINVAL, "%s: dim above 2^34", who);
    const long long k = ksd_plan((int)n, dim, elem_bytes, out, out ? n_out : 0);
    return k > 0x7fffffffLL ? 0x7fffffff : (int)k;
}

int sgmcmc_ksd_f32(const float *samples, size_t ld_x, const float *scores, size_t ld_s, size_t n, size_t dim, int kind,
                   double c, double beta, double h2, void *workspace, float *matrix_out, size_t ld_m, double *row_sums_out,
                   double *stats_out, sgmcmc_stream_t stream) {
    return ksd_impl<float>(samples, ld_x, scores, ld_s, n, dim, kind, c, beta, h2, workspace, matrix_out, ld_m, row_sums_out,
                           stats_out, stream);
}

int sgmcmc_ksd_f64(const double *samples, size_t ld_x, const double *scores, size_t ld_s, size_t n, size_t dim, int kind,
                   double c, double beta, double h2, void *workspace, double *matrix_out, size_t ld_m, double *row_sums_out,
                   double *stats_out, sgmcmc_stream_t stream) {
    return ksd_impl<double>(samples, ld_x, scores, ld_s, n, dim, kind, c, beta, h2, workspace, matrix_out, ld_m, row_sums_out,
                            stats_out, stream);
}

}  // extern "C"
