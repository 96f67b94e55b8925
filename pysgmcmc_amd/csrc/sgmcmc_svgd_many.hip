// sgmcmc_svgd_many.hip -- the SVGD step (pysgmcmc/samplers/svgd.py:118-181) for 2 .. 1024 particles: tiled Gram, median
// and update kernels behind include/sgmcmc_hip_svgd_many.h. sgmcmc_svgd.hip keeps K and a column tile of X in registers or
// LDS and stops at 128 particles; here K (n x n, pitch np = n rounded up to 16, zero padded) lives in the workspace (4 MB in
// f32, 8 MB in f64 at 1024 particles: cache-resident, though more than one XCD's L2), and every kernel is tiled over particles.
//
// One step, in launch order (ids of the header):
//   MEAN       the column means over all n particles of one PHASE of 65 536 columns, into a buffer of that many elements
//              (the workspace does not grow with dim): 32 columns x 8 interleaved row chains per workgroup.
//   GRAM       grid = splits x pairs: workgroup (split, block pair bi <= bj) accumulates the 64 x 64 block  X~_bi X~_bj^T
//              over the phase's column tiles split, split + splits, ... with v_mfma_*_16x16x4, the two row blocks centred
//              with MEAN's means as they are staged in the LDS. Wave w owns rows 16 w .. 16 w + 15 of the block and its four
//              16-column blocks. From the second phase on the accumulators start from the workgroup's own partial block.
//              MEAN and GRAM repeat per phase: one pair of launches up to 65 536 columns.
//   REDUCE     partial blocks added in ascending split order, scattered into the Gram matrix (K's storage).
//   DIST       D_ij = (sqrt(max(0, (g_ii + g_jj) - 2 g_ij)))^2 from the upper triangle; zeroes the select counters.
//   SELECT     pass p histograms byte p (most significant first) of the keys that match the prefix of passes 0 .. p - 1;
//              every workgroup re-derives that prefix from the merged histograms of the earlier passes. LDS histogram per
//              workgroup, merged with integer atomics.
//   NEXT       even n * n: the count of entries <= the key of rank mid - 1 and the smallest larger key.
//   BANDWIDTH  median, h, h^2 into the header.
//   KMATRIX    workgroup i: row i of K and its sum.
//   UPDATE     workgroup = 16 columns. The tile of X (np x 16) is staged in the LDS before anything is written and is the
//              only source of X afterwards: the hazard rule is structural. Row groups of 16 blocks of 16 particles (2 per
//              wave, 8 waves), j in chunks of 128 particles of G staged in the LDS; K is the A operand, one 4-element access per lane
//              and 16 j, so MFMA step e of a lane group multiplies particle j0 + 4 (l >> 4) + e; LDS rows are stored with
//              the two low index pairs swapped so that the four lane groups read adjacent rows.
// Every access to X, G, H and kernel gradients is one element wide and coalesced over 16 .. 64 adjacent columns, so the bits
// cannot depend on pitch or alignment.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sgmcmc_hip_svgd_many.h"

#pragma clang fp contract(off)

#include "sgmcmc_host.hpp"

using namespace sgmcmc_host;

namespace {

constexpr int MANY_MAX_PARTICLES = 1024;
constexpr int MANY_THREADS = 256;
constexpr int MANY_GB = 64;                   // rows and columns of a Gram block
constexpr int MANY_BLOCK_ELEMS = MANY_GB * MANY_GB;
constexpr int MANY_GRAM_WGS = 512;            // splits x pairs stays at or below this (and is at least `pairs`)
constexpr int MANY_PHASE_COLS = 65536;        // columns per MEAN / GRAM phase: the size of the means buffer
constexpr int MANY_MEAN_COLS = 32, MANY_MEAN_CHAINS = MANY_THREADS / MANY_MEAN_COLS;
constexpr int MANY_UCOLS = 16;                // columns per update workgroup
constexpr int MANY_UTHREADS = 512;            // update workgroup: 8 waves, two per SIMD, so that K's latency is covered
constexpr int MANY_UQ = 16 / (MANY_UTHREADS / 64);   // 16-particle row blocks per wave and row group
constexpr int MANY_UROWS = MANY_UTHREADS / MANY_UCOLS;   // rows staged per pass
constexpr int MANY_JCHUNK = 128;              // particles of G per LDS chunk
constexpr int MANY_SEL_WORDS = 2080;          // 8 x 256 histogram words, count_le at 2048, next_key (64 bit) at 2050
constexpr int MANY_SEL_COUNT = 2048, MANY_SEL_NEXT = 2050;

__device__ __forceinline__ float sqrt_t(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ double sqrt_t(double x) { return __builtin_sqrt(x); }
__device__ __forceinline__ float exp_t(float x) { return expf(x); }
__device__ __forceinline__ double exp_t(double x) { return exp(x); }
__device__ __forceinline__ float log_t(float x) { return logf(x); }
__device__ __forceinline__ double log_t(double x) { return log(x); }

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

// 16x16x4 matrix-core step: A lane l = a[row l & 15][k = l >> 4], B lane l = b[k = l >> 4][column l & 15]; output register r
// of lane l = row `row(l >> 4, r)`, column l & 15
template <typename T> struct Mfma16;
template <> struct Mfma16<float> {
    typedef f32x4 Acc;
    static __device__ __forceinline__ Acc mma(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int lane_hi, int reg) { return 4 * lane_hi + reg; }
};
template <> struct Mfma16<double> {
    typedef f64x4 Acc;
    static __device__ __forceinline__ Acc mma(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int lane_hi, int reg) { return lane_hi + 4 * reg; }
};

template <typename T> struct KeyOf;
template <> struct KeyOf<float> {
    using type = uint32_t;
    static __device__ __forceinline__ uint32_t bits(float x) { return __float_as_uint(x); }
    static __device__ __forceinline__ float value(uint32_t k) { return __uint_as_float(k); }
};
template <> struct KeyOf<double> {
    using type = uint64_t;
    static __device__ __forceinline__ uint64_t bits(double x) { return (uint64_t)__double_as_longlong(x); }
    static __device__ __forceinline__ double value(uint64_t k) { return __longlong_as_double((long long)k); }
};

inline int many_np(int n) { return (n + 15) & ~15; }
inline int many_nb64(int n) { return (n + MANY_GB - 1) / MANY_GB; }
inline int many_pairs(int n) { const int b = many_nb64(n); return b * (b + 1) / 2; }
inline int many_split_cap(int n) { const int c = MANY_GRAM_WGS / many_pairs(n); return c < 1 ? 1 : c; }
constexpr int many_gram_tile(size_t esize) { return esize == 4 ? 64 : 32; }

// workspace layout, in bytes; every offset is a multiple of 128
struct ManyWs {
    size_t hdr, sel, D, K, ksum, means, parts, total;
};

inline ManyWs many_ws(int n, size_t esize) {
    const size_t np = (size_t)many_np(n);
    auto up = [](size_t b) { return (b + 127) & ~(size_t)127; };
    ManyWs w;
    size_t off = 0;
    w.hdr = off; off += 128;
    w.sel = off; off += up((size_t)MANY_SEL_WORDS * 4);
    w.D = off; off += up((size_t)n * n * esize);
    w.K = off; off += up(np * np * esize);
    w.ksum = off; off += up(np * esize);
    w.means = off; off += up((size_t)MANY_PHASE_COLS * esize);
    w.parts = off; off += up((size_t)many_split_cap(n) * many_pairs(n) * MANY_BLOCK_ELEMS * esize);
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
// MEAN, GRAM
// ---------------------------------------------------------------------------------------------
// means[c] = (sum_i X[i][c0 + c]) * (1 / n) for the pcols columns of one phase: chain k adds the rows k, k + 8, ... in
// ascending order, the eight chains are then added in chain order
template <typename T>
__global__ __launch_bounds__(MANY_THREADS) void many_mean_kernel(const T *__restrict__ X, size_t ld, int n, size_t c0,
                                                                  int pcols, T *__restrict__ means) {
    __shared__ T msum[MANY_MEAN_CHAINS * MANY_MEAN_COLS];
    const int t = threadIdx.x, c = t % MANY_MEAN_COLS, chain = t / MANY_MEAN_COLS;
    const int lc = blockIdx.x * MANY_MEAN_COLS + c;
    T s = (T)0;
    if (lc < pcols) {
        const T *col = X + c0 + (size_t)lc;
#pragma unroll 8
        for (int r = chain; r < n; r += MANY_MEAN_CHAINS) s += col[(size_t)r * ld];
    }
    msum[chain * MANY_MEAN_COLS + c] = s;
    __syncthreads();
    if (t < MANY_MEAN_COLS && lc < pcols) {
        T m = msum[t];
#pragma unroll
        for (int k = 1; k < MANY_MEAN_CHAINS; ++k) m += msum[k * MANY_MEAN_COLS + t];
        means[lc] = m * ((T)1 / (T)n);
    }
}

template <typename T>
__global__ __launch_bounds__(MANY_THREADS) void many_gram_kernel(const T *__restrict__ X, size_t ld, int n, size_t c0,
                                                                  int pcols, const T *__restrict__ means, int accumulate,
                                                                  int nb64, int pairs, int splits, T *__restrict__ parts) {
    constexpr int TC = many_gram_tile(sizeof(T)), P = TC + 16 / (int)sizeof(T), RG = MANY_THREADS / TC;
    __shared__ T xa[MANY_GB * P];
    __shared__ T xb[MANY_GB * P];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int c = t % TC, rg = t / TC;
    const int split = blockIdx.x / pairs;
    int bi, bj;
    decode_pair(blockIdx.x % pairs, nb64, bi, bj);
    const T *xbp = (bi == bj) ? xa : xb;
    T *out = parts + (size_t)blockIdx.x * MANY_BLOCK_ELEMS;
    typename Mfma16<T>::Acc acc[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[cb][r] = accumulate ? out[((wave * 4 + cb) * 4 + r) * 64 + lane] : (T)0;

    const int n_tiles = (pcols + TC - 1) / TC;
    for (int tile = split; tile < n_tiles; tile += splits) {
        const int lc = tile * TC + c;
        const bool cv = lc < pcols;
        const size_t col = c0 + (size_t)lc;
        const T m = cv ? means[lc] : (T)0;
        T va[MANY_GB / RG], vb[MANY_GB / RG];
#pragma unroll
        for (int k = 0; k < MANY_GB / RG; ++k) {
            const int row = rg + RG * k;
            const int ra = MANY_GB * bi + row, rb = MANY_GB * bj + row;
            va[k] = (T)0;
            vb[k] = (T)0;
            if (cv && ra < n) va[k] = X[(size_t)ra * ld + col] - m;
            if (bi != bj && cv && rb < n) vb[k] = X[(size_t)rb * ld + col] - m;
        }
        __syncthreads();                                   // the previous tile's operands are consumed
#pragma unroll
        for (int k = 0; k < MANY_GB / RG; ++k) {
            const int row = rg + RG * k;
            xa[row * P + c] = va[k];
            if (bi != bj) xb[row * P + c] = vb[k];
        }
        __syncthreads();
#pragma unroll 4
        for (int ks = 0; ks < TC / 4; ++ks) {
            const int kk = 4 * ks + (lane >> 4);
            const T a = xa[(16 * wave + (lane & 15)) * P + kk];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) acc[cb] = Mfma16<T>::mma(a, xbp[(16 * cb + (lane & 15)) * P + kk], acc[cb]);
        }
    }
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[((wave * 4 + cb) * 4 + r) * 64 + lane] = acc[cb][r];
}

template <typename T>
__global__ __launch_bounds__(MANY_THREADS) void many_reduce_kernel(const T *__restrict__ parts, int n, int np, int nb64,
                                                                    int pairs, int splits, T *__restrict__ gram) {
    const int idx = blockIdx.x * MANY_THREADS + threadIdx.x;
    if (idx >= pairs * MANY_BLOCK_ELEMS) return;
    const size_t stride = (size_t)pairs * MANY_BLOCK_ELEMS;
    T s = parts[idx];
    for (int q = 1; q < splits; ++q) s += parts[(size_t)q * stride + idx];
    int bi, bj;
    decode_pair(idx / MANY_BLOCK_ELEMS, nb64, bi, bj);
    const int e = idx % MANY_BLOCK_ELEMS;
    const int lane = e & 63, r = (e >> 6) & 3, cb = (e >> 8) & 3, w = e >> 10;
    const int i = MANY_GB * bi + 16 * w + Mfma16<T>::row(lane >> 4, r), j = MANY_GB * bj + 16 * cb + (lane & 15);
    if (i >= n || j >= n) return;
    gram[(size_t)i * np + j] = s;
    if (bi != bj) gram[(size_t)j * np + i] = s;
}

// ---------------------------------------------------------------------------------------------
// DIST
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(MANY_THREADS) void many_dist_kernel(const T *__restrict__ gram, int n, int np, T *__restrict__ D,
                                                                  unsigned int *__restrict__ sel) {
    if (blockIdx.x == 0) {
        for (int k = threadIdx.x; k < MANY_SEL_WORDS; k += MANY_THREADS)
            sel[k] = (k == MANY_SEL_NEXT || k == MANY_SEL_NEXT + 1) ? 0xffffffffu : 0u;
    }
    const int idx = blockIdx.x * MANY_THREADS + threadIdx.x;
    if (idx >= n * n) return;
    const int i = idx / n, j = idx % n;
    T sq = (T)0;
    if (i != j) {
        const int lo = i < j ? i : j, hi = i < j ? j : i;              // one rounding sequence for (i, j) and (j, i)
        T s = (gram[(size_t)lo * np + lo] + gram[(size_t)hi * np + hi]) - (T)2 * gram[(size_t)lo * np + hi];
        s = s > (T)0 ? s : (T)0;
        const T dist = sqrt_t(s);                                      // tf.norm, tensor_utils.py:399
        sq = dist * dist;                                              // `** 2`, svgd.py:166
    }
    D[idx] = sq;
}

// ---------------------------------------------------------------------------------------------
// SELECT / NEXT / BANDWIDTH: radix select of the median over n * n non-negative keys
// ---------------------------------------------------------------------------------------------
// prefix of the key of rank `rank` as far as the merged histograms of passes 0 .. npass - 1 fix it, and the rank that is
// left among the keys with that prefix. The digit is located by wave 0 with a shuffle scan over 4 bins per lane.
template <typename T>
__device__ void many_resolve(const unsigned int *__restrict__ sel, int npass, int rank, unsigned int *lh,
                             unsigned long long *bcast, typename KeyOf<T>::type &prefix, typename KeyOf<T>::type &mask,
                             int &remaining) {
    using Key = typename KeyOf<T>::type;
    prefix = 0;
    mask = 0;
    remaining = rank;
    for (int q = 0; q < npass; ++q) {
        const int shift = (int)sizeof(Key) * 8 - 8 * (q + 1);
        __syncthreads();
        lh[threadIdx.x] = sel[q * 256 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x < 64) {
            const int l = threadIdx.x;
            const int h0 = (int)lh[4 * l], h1 = (int)lh[4 * l + 1], h2 = (int)lh[4 * l + 2], h3 = (int)lh[4 * l + 3];
            const int mine = h0 + h1 + h2 + h3;
            int incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int up = __shfl_up(incl, off, 64);
                if (l >= off) incl += up;
            }
            int cum = incl - mine;                       // entries in bins below 4 l
            if (cum <= remaining && remaining < incl) {  // exactly one lane
                int digit = 4 * l;
                if (remaining >= cum + h0) { cum += h0; ++digit;
                    if (remaining >= cum + h1) { cum += h1; ++digit;
                        if (remaining >= cum + h2) { cum += h2; ++digit; } } }
                bcast[0] = (unsigned long long)digit;
                bcast[1] = (unsigned long long)cum;
            }
        }
        __syncthreads();
        const Key digit = (Key)bcast[0];
        remaining -= (int)bcast[1];
        prefix |= digit << shift;
        mask |= (Key)255 << shift;
    }
    __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(MANY_THREADS) void many_select_kernel(const T *__restrict__ D, int N, int rank, int pass,
                                                                    unsigned int *__restrict__ sel) {
    using Key = typename KeyOf<T>::type;
    __shared__ unsigned int lh[256];
    __shared__ unsigned long long bcast[2];
    Key prefix, mask;
    int remaining;
    many_resolve<T>(sel, pass, rank, lh, bcast, prefix, mask, remaining);
    const int shift = (int)sizeof(Key) * 8 - 8 * (pass + 1);
    lh[threadIdx.x] = 0u;
    __syncthreads();
    for (int idx = blockIdx.x * MANY_THREADS + threadIdx.x; idx < N; idx += gridDim.x * MANY_THREADS) {
        const Key k = KeyOf<T>::bits(D[idx]);
        if ((k & mask) == prefix) atomicAdd(&lh[(unsigned)((k >> shift) & (Key)255)], 1u);
    }
    __syncthreads();
    const unsigned int mine = lh[threadIdx.x];
    if (mine) atomicAdd(&sel[pass * 256 + threadIdx.x], mine);
}

template <typename T>
__global__ __launch_bounds__(MANY_THREADS) void many_next_kernel(const T *__restrict__ D, int N, int rank,
                                                                  unsigned int *__restrict__ sel) {
    using Key = typename KeyOf<T>::type;
    __shared__ unsigned int lh[256];
    __shared__ unsigned long long bcast[2];
    __shared__ unsigned long long next_key;
    __shared__ unsigned int count_le;
    Key lo, mask;
    int remaining;
    many_resolve<T>(sel, (int)sizeof(Key), rank, lh, bcast, lo, mask, remaining);
    if (threadIdx.x == 0) { next_key = ~0ull; count_le = 0u; }
    __syncthreads();
    unsigned int c_le = 0;
    unsigned long long mn = ~0ull;
    for (int idx = blockIdx.x * MANY_THREADS + threadIdx.x; idx < N; idx += gridDim.x * MANY_THREADS) {
        const Key k = KeyOf<T>::bits(D[idx]);
        if (k <= lo) ++c_le;
        else if ((unsigned long long)k < mn) mn = (unsigned long long)k;
    }
    if (c_le) atomicAdd(&count_le, c_le);
    if (mn != ~0ull) atomicMin(&next_key, mn);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (count_le) atomicAdd(&sel[MANY_SEL_COUNT], count_le);
        if (next_key != ~0ull) atomicMin(reinterpret_cast<unsigned long long *>(sel + MANY_SEL_NEXT), next_key);
    }
}

template <typename T>
__global__ __launch_bounds__(MANY_THREADS) void many_bandwidth_kernel(int n, unsigned int *__restrict__ sel,
                                                                       T *__restrict__ hdr) {
    using Key = typename KeyOf<T>::type;
    __shared__ unsigned int lh[256];
    __shared__ unsigned long long bcast[2];
    const int N = n * n, mid = N / 2;
    Key lo, mask;
    int remaining;
    many_resolve<T>(sel, (int)sizeof(Key), (N & 1) ? mid : mid - 1, lh, bcast, lo, mask, remaining);
    if (threadIdx.x != 0) return;
    T med;
    if (N & 1) {
        med = KeyOf<T>::value(lo);                                      // tensor_utils.py:205-206
    } else {
        // the two middle values: rank mid - 1, then the same value if it repeats, else the smallest larger entry
        const unsigned long long nk = *reinterpret_cast<const unsigned long long *>(sel + MANY_SEL_NEXT);
        const Key hi = ((int)sel[MANY_SEL_COUNT] > mid) ? lo : (Key)nk;
        med = (KeyOf<T>::value(lo) + KeyOf<T>::value(hi)) / (T)2;       // tensor_utils.py:208
    }
    const T h = sqrt_t((T)0.5 * med / log_t((T)n + (T)1));              // svgd.py:169-171
    hdr[0] = med;
    hdr[1] = h;
    hdr[2] = h * h;
}

// ---------------------------------------------------------------------------------------------
// KMATRIX: row i of K (pitch np, zero padded) and its sum
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(MANY_THREADS) void many_kmatrix_kernel(const T *__restrict__ D, int n, int np,
                                                                     const T *__restrict__ hdr, T *__restrict__ K,
                                                                     T *__restrict__ ksum) {
    __shared__ T red[MANY_THREADS];
    const int i = blockIdx.x, t = threadIdx.x;
    const T h2 = hdr[2];
    T part = (T)0;
    for (int j = t; j < np; j += MANY_THREADS) {
        T k = (T)0;
        if (i < n && j < n) k = exp_t(-D[(size_t)i * n + j] / h2 / (T)2);   // svgd.py:173
        K[(size_t)i * np + j] = k;
        part += k;                                                          // svgd.py:174
    }
    red[t] = part;
    __syncthreads();
    for (int off = MANY_THREADS / 2; off > 0; off >>= 1) {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
    if (t == 0) ksum[i] = red[0];
}

template <typename T>
__global__ void many_copy_kernel(const T *__restrict__ K, int n, int np, T *__restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n * n) out[idx] = K[(size_t)(idx / n) * np + (idx % n)];
}

// ---------------------------------------------------------------------------------------------
// UPDATE: A = K G, B = K X for 16 columns, then the element-wise tail (or the kernel gradients)
// ---------------------------------------------------------------------------------------------
// LDS row of particle j: within each group of 16 particles the index pairs (j & 3) and (j >> 2) & 3 are swapped, so that
// the particles 4 g + e of the four lane groups g sit in adjacent rows
__device__ __forceinline__ int many_slot(int j) { return (j & ~15) | ((j & 3) << 2) | ((j >> 2) & 3); }

template <typename T, bool UPDATE>
__global__ __launch_bounds__(MANY_UTHREADS) void many_update_kernel(T *__restrict__ X, const T *__restrict__ G,
                                                                    T *__restrict__ H, T *__restrict__ kgrad_out,
                                                                    size_t dim, size_t ld, size_t out_ld, int n,
                                                                    const T *__restrict__ hdr, const T *__restrict__ K,
                                                                    const T *__restrict__ ksum, T eps, T alpha,
                                                                    T one_minus_alpha, T fudge, T sign) {
    typedef T Vec4 __attribute__((ext_vector_type(4)));
    extern __shared__ __align__(32) unsigned char many_lds_raw[];
    const int np = (n + 15) & ~15, nb = np / 16;
    T *xs = reinterpret_cast<T *>(many_lds_raw);          // [np][16], rows by many_slot
    T *gs = xs + (size_t)np * MANY_UCOLS;                 // [128][16], rows by many_slot
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int lc = lane & 15, lg = lane >> 4;
    const int c = t & 15, r0 = t >> 4;
    const size_t col = (size_t)blockIdx.x * MANY_UCOLS + (size_t)c;
    const bool cv = col < dim;
    // every read of X[:, tile] happens here, before the first write below
    for (int r = r0; r < np; r += MANY_UROWS) xs[many_slot(r) * MANY_UCOLS + c] = (cv && r < n) ? X[(size_t)r * ld + col] : (T)0;
    __syncthreads();
    const T h2 = hdr[2];
    const T n_t = (T)n;
    const size_t ocol = (size_t)blockIdx.x * MANY_UCOLS + (size_t)lc;
    const bool ov = ocol < dim;
    const int n_groups = (nb + 15) / 16, n_chunks = (np + MANY_JCHUNK - 1) / MANY_JCHUNK;
    for (int g = 0; g < n_groups; ++g) {
        typename Mfma16<T>::Acc ag[MANY_UQ], ax[MANY_UQ];
#pragma unroll
        for (int q = 0; q < MANY_UQ; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) { ag[q][r] = (T)0; ax[q][r] = (T)0; }
        for (int ch = 0; ch < n_chunks; ++ch) {
            const int j0 = ch * MANY_JCHUNK;
            if (UPDATE) {
                __syncthreads();                              // the previous chunk is consumed
#pragma unroll
                for (int k = 0; k < MANY_JCHUNK / MANY_UROWS; ++k) {
                    const int r = r0 + MANY_UROWS * k, j = j0 + r;
                    gs[many_slot(r) * MANY_UCOLS + c] = (cv && j < n) ? G[(size_t)j * ld + col] : (T)0;
                }
                __syncthreads();
            }
            for (int sub = 0; sub < MANY_JCHUNK / 16; ++sub) {
                const int jb = j0 + 16 * sub;
                if (jb >= np) break;                          // uniform: np is the same for every lane
                T bx[4], bg[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    bx[e] = xs[(jb + 4 * e + lg) * MANY_UCOLS + lc];            // particle jb + 4 lg + e
                    bg[e] = UPDATE ? gs[(16 * sub + 4 * e + lg) * MANY_UCOLS + lc] : (T)0;
                }
#pragma unroll
                for (int q = 0; q < MANY_UQ; ++q) {
                    const int rb = 16 * g + MANY_UQ * wave + q;
                    Vec4 kv = {(T)0, (T)0, (T)0, (T)0};
                    if (rb < nb) kv = *reinterpret_cast<const Vec4 *>(K + (size_t)(16 * rb + lc) * np + jb + 4 * lg);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        ax[q] = Mfma16<T>::mma(kv[e], bx[e], ax[q]);
                        if (UPDATE) ag[q] = Mfma16<T>::mma(kv[e], bg[e], ag[q]);
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < MANY_UQ; ++q) {
            const int rb = 16 * g + MANY_UQ * wave + q;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * rb + Mfma16<T>::row(lg, r);
                if (rb < nb && i < n && ov) {
                    const T x = xs[many_slot(i) * MANY_UCOLS + lc];
                    const T kg = (-ax[q][r] + x * ksum[i]) / h2;                 // svgd.py:176-181
                    if (UPDATE) {
                        const size_t at = (size_t)i * ld + ocol;
                        const T gt = (ag[q][r] + sign * kg) / n_t;               // svgd.py:124-127
                        const T hnew = alpha * H[at] + one_minus_alpha * (gt * gt);   // svgd.py:129-132
                        const T adj = gt / (fudge + sqrt_t(hnew));               // svgd.py:134-137
                        H[at] = hnew;
                        X[at] = x - eps * adj;                                   // svgd.py:139-143
                    } else {
                        kgrad_out[(size_t)i * out_ld + ocol] = kg;
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
inline int many_select_grid(int N) {
    const int want = (N + 8 * MANY_THREADS - 1) / (8 * MANY_THREADS);
    return want < 256 ? want : 256;
}

// the column phases of MEAN / GRAM and the column splits of GRAM, the same in every phase
struct ManyGram { int tc, pairs, cap, splits; size_t phases; };

inline ManyGram many_gram_geom(int n, size_t dim, size_t esize) {
    ManyGram g;
    g.tc = many_gram_tile(esize);
    g.pairs = many_pairs(n);
    g.cap = many_split_cap(n);
    const size_t first = dim < (size_t)MANY_PHASE_COLS ? dim : (size_t)MANY_PHASE_COLS;   // the widest phase
    const size_t n_tiles = (first + g.tc - 1) / g.tc;
    g.splits = (int)(n_tiles < (size_t)g.cap ? n_tiles : (size_t)g.cap);
    g.phases = (dim + MANY_PHASE_COLS - 1) / MANY_PHASE_COLS;
    return g;
}

inline int many_phase_cols(size_t dim, size_t ph) {
    const size_t left = dim - ph * MANY_PHASE_COLS;
    return (int)(left < (size_t)MANY_PHASE_COLS ? left : (size_t)MANY_PHASE_COLS);
}

// the launches of one step: all are counted, those that fit `room` are written
struct ManyPlan {
    int *out;
    int room;
    long long k;
    void add(int id, int tile, int grid, int cap) {
        if (out && 4 * k + 3 < room) { out[4 * k] = id; out[4 * k + 1] = tile; out[4 * k + 2] = grid; out[4 * k + 3] = cap; }
        ++k;
    }
};

inline long long many_plan(int n, size_t dim, size_t esize, int *out, int room) {
    const ManyGram g = many_gram_geom(n, dim, esize);
    const int np = many_np(n), N = n * n;
    ManyPlan p = {out, room, 0};
    for (size_t ph = 0; ph < g.phases; ++ph) {
        p.add(SGMCMC_SVGD_MANY_MEAN, MANY_MEAN_COLS, (many_phase_cols(dim, ph) + MANY_MEAN_COLS - 1) / MANY_MEAN_COLS, 0);
        p.add(SGMCMC_SVGD_MANY_GRAM, g.tc, g.splits * g.pairs, g.cap);
    }
    p.add(SGMCMC_SVGD_MANY_REDUCE, 0, (g.pairs * MANY_BLOCK_ELEMS + MANY_THREADS - 1) / MANY_THREADS, 0);
    p.add(SGMCMC_SVGD_MANY_DIST, 0, (N + MANY_THREADS - 1) / MANY_THREADS, 0);
    for (int q = 0; q < (int)esize; ++q) p.add(SGMCMC_SVGD_MANY_SELECT, 0, many_select_grid(N), 256);
    if (!(N & 1)) p.add(SGMCMC_SVGD_MANY_NEXT, 0, many_select_grid(N), 256);
    p.add(SGMCMC_SVGD_MANY_BANDWIDTH, 0, 1, 0);
    p.add(SGMCMC_SVGD_MANY_KMATRIX, 0, np, 0);
    p.add(SGMCMC_SVGD_MANY_UPDATE, MANY_UCOLS, (int)((dim + MANY_UCOLS - 1) / MANY_UCOLS), 0);
    return p.k;
}

int many_check(const char *who, bool nulls, size_t n, size_t dim, size_t ld) {
    if (nulls) return fail(SGMCMC_EINVAL, "%s: null pointer", who);
    if (n < 2 || n > (size_t)MANY_MAX_PARTICLES)
        return fail(SGMCMC_EINVAL, "%s: n_particles = %zu outside [2, %d]", who, n, MANY_MAX_PARTICLES);
    if (dim < 1) return fail(SGMCMC_EINVAL, "%s: dim < 1", who);
    if (ld < dim) return fail(SGMCMC_EINVAL, "%s: ld < dim", who);
    return 0;
}

int many_check_late(const char *who, size_t dim, const void *ws) {
    if (reinterpret_cast<uintptr_t>(ws) & 31) return fail(SGMCMC_EINVAL, "%s: workspace is not 32-byte aligned", who);
    if (dim > ((size_t)1 << 34)) return fail(SGMCMC_EINVAL, "%s: dim above 2^34", who);
    return 0;
}

template <typename T>
int many_kernel_matrix(const T *X, int n, size_t dim, size_t ld, unsigned char *ws, hipStream_t st) {
    const ManyWs w = many_ws(n, sizeof(T));
    const ManyGram gg = many_gram_geom(n, dim, sizeof(T));
    const int np = many_np(n), nb64 = many_nb64(n), pairs = gg.pairs, splits = gg.splits, N = n * n;
    T *hdr = reinterpret_cast<T *>(ws + w.hdr), *D = reinterpret_cast<T *>(ws + w.D), *K = reinterpret_cast<T *>(ws + w.K);
    T *ksum = reinterpret_cast<T *>(ws + w.ksum), *parts = reinterpret_cast<T *>(ws + w.parts);
    T *means = reinterpret_cast<T *>(ws + w.means);
    unsigned int *sel = reinterpret_cast<unsigned int *>(ws + w.sel);
    int rc;
    for (size_t ph = 0; ph < gg.phases; ++ph) {
        const size_t c0 = ph * MANY_PHASE_COLS;
        const int pcols = many_phase_cols(dim, ph);
        hipLaunchKernelGGL((many_mean_kernel<T>), dim3((pcols + MANY_MEAN_COLS - 1) / MANY_MEAN_COLS), dim3(MANY_THREADS), 0,
                           st, X, ld, n, c0, pcols, means);
        if ((rc = launched("svgd_many_mean_kernel"))) return rc;
        hipLaunchKernelGGL((many_gram_kernel<T>), dim3(splits * pairs), dim3(MANY_THREADS), 0, st, X, ld, n, c0, pcols,
                           (const T *)means, (int)(ph > 0), nb64, pairs, splits, parts);
        if ((rc = launched("svgd_many_gram_kernel"))) return rc;
    }
    hipLaunchKernelGGL((many_reduce_kernel<T>), dim3((pairs * MANY_BLOCK_ELEMS + MANY_THREADS - 1) / MANY_THREADS),
                       dim3(MANY_THREADS), 0, st, parts, n, np, nb64, pairs, splits, K);
    if ((rc = launched("svgd_many_reduce_kernel"))) return rc;
    hipLaunchKernelGGL((many_dist_kernel<T>), dim3((N + MANY_THREADS - 1) / MANY_THREADS), dim3(MANY_THREADS), 0, st, K, n, np,
                       D, sel);
    if ((rc = launched("svgd_many_dist_kernel"))) return rc;
    const int mid = N / 2, rank = (N & 1) ? mid : mid - 1, sgrid = many_select_grid(N);
    for (int p = 0; p < (int)sizeof(T); ++p) {
        hipLaunchKernelGGL((many_select_kernel<T>), dim3(sgrid), dim3(MANY_THREADS), 0, st, D, N, rank, p, sel);
        if ((rc = launched("svgd_many_select_kernel"))) return rc;
    }
    if (!(N & 1)) {
        hipLaunchKernelGGL((many_next_kernel<T>), dim3(sgrid), dim3(MANY_THREADS), 0, st, D, N, rank, sel);
        if ((rc = launched("svgd_many_next_kernel"))) return rc;
    }
    hipLaunchKernelGGL((many_bandwidth_kernel<T>), dim3(1), dim3(MANY_THREADS), 0, st, n, sel, hdr);
    if ((rc = launched("svgd_many_bandwidth_kernel"))) return rc;
    hipLaunchKernelGGL((many_kmatrix_kernel<T>), dim3(np), dim3(MANY_THREADS), 0, st, D, n, np, hdr, K, ksum);
    return launched("svgd_many_kmatrix_kernel");
}

template <typename T, bool UPDATE>
int many_apply(T *X, const T *G, T *H, T *kgrad_out, size_t out_ld, int n, size_t dim, size_t ld, T eps, double alpha,
               T fudge, T sign, unsigned char *ws, hipStream_t st) {
    const ManyWs w = many_ws(n, sizeof(T));
    const int np = many_np(n);
    const size_t lds_bytes = ((size_t)np + MANY_JCHUNK) * MANY_UCOLS * sizeof(T);
    const void *fn = reinterpret_cast<const void *>(&many_update_kernel<T, UPDATE>);
    if (lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(svgd_many_update_kernel)");
    }
    const unsigned grid = (unsigned)((dim + MANY_UCOLS - 1) / MANY_UCOLS);
    hipLaunchKernelGGL((many_update_kernel<T, UPDATE>), dim3(grid), dim3(MANY_UTHREADS), lds_bytes, st, X, G, H, kgrad_out,
                       dim, ld, out_ld, n, reinterpret_cast<const T *>(ws + w.hdr), reinterpret_cast<const T *>(ws + w.K),
                       reinterpret_cast<const T *>(ws + w.ksum), eps, (T)alpha, (T)(1.0 - alpha), fudge, sign);
    return launched("svgd_many_update_kernel");
}

template <typename T>
int many_step_impl(T *X, const T *G, T *H, size_t n, size_t dim, size_t ld, T eps, double alpha, T fudge,
                   int repulsion_sign, void *ws, sgmcmc_stream_t stream) {
    const char *who = "svgd_many_step";
    int rc = many_check(who, !X || !G || !H || !ws, n, dim, ld);
    if (rc) return rc;
    if (repulsion_sign != 1 && repulsion_sign != -1)
        return fail(SGMCMC_EINVAL, "%s: repulsion_sign must be +1 (reference) or -1", who);
    if ((rc = many_check_late(who, dim, ws))) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned char *w = static_cast<unsigned char *>(ws);
    if ((rc = many_kernel_matrix<T>(X, (int)n, dim, ld, w, st))) return rc;
    return many_apply<T, true>(X, G, H, nullptr, 0, (int)n, dim, ld, eps, alpha, fudge, (T)repulsion_sign, w, st);
}

template <typename T>
int many_kernel_impl(const T *X, size_t n, size_t dim, size_t ld, void *ws, T *kernel_out, T *kgrad_out, size_t kgrad_ld,
                     T *bandwidth_out, sgmcmc_stream_t stream) {
    const char *who = "svgd_many_kernel";
    int rc = many_check(who, !X || !ws, n, dim, ld);
    if (rc) return rc;
    if (kgrad_out && kgrad_ld < dim) return fail(SGMCMC_EINVAL, "%s: kgrad_ld < dim", who);
    if ((rc = many_check_late(who, dim, ws))) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned char *w = static_cast<unsigned char *>(ws);
    if ((rc = many_kernel_matrix<T>(X, (int)n, dim, ld, w, st))) return rc;
    const ManyWs lay = many_ws((int)n, sizeof(T));
    if (kernel_out) {
        const int total = (int)(n * n);
        hipLaunchKernelGGL((many_copy_kernel<T>), dim3((total + 255) / 256), dim3(256), 0, st,
                           reinterpret_cast<const T *>(w + lay.K), (int)n, many_np((int)n), kernel_out);
        if ((rc = launched("svgd_many_copy_kernel"))) return rc;
    }
    if (bandwidth_out) {
        hipError_t e = hipMemcpyAsync(bandwidth_out, w + lay.hdr, 3 * sizeof(T), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(bandwidth)");
    }
    if (kgrad_out)
        return many_apply<T, false>(const_cast<T *>(X), nullptr, nullptr, kgrad_out, kgrad_ld, (int)n, dim, ld, (T)0, 0.0,
                                    (T)0, (T)1, w, st);
    return 0;
}

}  // namespace

extern "C" {

int sgmcmc_svgd_many_abi_version(void) { return SGMCMC_SVGD_MANY_ABI_VERSION; }

int sgmcmc_svgd_many_max_particles(void) { return MANY_MAX_PARTICLES; }

size_t sgmcmc_svgd_many_workspace_bytes(size_t n_particles, size_t elem_bytes) {
    if (n_particles < 2 || n_particles > (size_t)MANY_MAX_PARTICLES || (elem_bytes != 4 && elem_bytes != 8)) return 0;
    return many_ws((int)n_particles, elem_bytes).total;
}

int sgmcmc_svgd_many_plan(size_t n_particles, size_t dim, size_t elem_bytes, int *out, int n_out) {
    const char *who = "svgd_many_plan";
    const int rc = many_check(who, false, n_particles, dim, dim);
    if (rc) return rc;
    if (elem_bytes != 4 && elem_bytes != 8) return fail(SGMCMC_EINVAL, "%s: elem_bytes must be 4 or 8", who);
    if (dim > ((size_t)1 << 34)) return fail(SGMCMC_EINVAL, "%s: dim above 2^34", who);
    const long long k = many_plan((int)n_particles, dim, elem_bytes, out, out ? n_out : 0);
    return k > 0x7fffffffLL ? 0x7fffffff : (int)k;
}

int sgmcmc_svgd_many_step_f32(float *particles, const float *grad, float *hist_grad, size_t n_particles, size_t dim,
                              size_t ld, float eps, double alpha, float fudge_factor, int repulsion_sign, void *workspace,
                              sgmcmc_stream_t stream) {
    return many_step_impl<float>(particles, grad, hist_grad, n_particles, dim, ld, eps, alpha, fudge_factor,
                                 repulsion_sign, workspace, stream);
}

int sgmcmc_svgd_many_step_f64(double *particles, const double *grad, double *hist_grad, size_t n_particles, size_t dim,
                              size_t ld, double eps, double alpha, double fudge_factor, int repulsion_sign, void *workspace,
                              sgmcmc_stream_t stream) {
    return many_step_impl<double>(particles, grad, hist_grad, n_particles, dim, ld, eps, alpha, fudge_factor,
                                  repulsion_sign, workspace, stream);
}

int sgmcmc_svgd_many_kernel_f32(const float *particles, size_t n_particles, size_t dim, size_t ld, void *workspace,
                                float *kernel_out, float *kernel_grad_out, size_t kernel_grad_ld, float *bandwidth_out,
                                sgmcmc_stream_t stream) {
    return many_kernel_impl<float>(particles, n_particles, dim, ld, workspace, kernel_out, kernel_grad_out,
                                   kernel_grad_ld, bandwidth_out, stream);
}

int sgmcmc_svgd_many_kernel_f64(const double *particles, size_t n_particles, size_t dim, size_t ld, void *workspace,
                                double *kernel_out, double *kernel_grad_out, size_t kernel_grad_ld, double *bandwidth_out,
                                sgmcmc_stream_t stream) {
    return many_kernel_impl<double>(particles, n_particles, dim, ld, workspace, kernel_out, kernel_grad_out,
                                    kernel_grad_ld, bandwidth_out, stream);
}

}  // extern "C"
