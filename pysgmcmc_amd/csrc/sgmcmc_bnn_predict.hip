// sgmcmc_bnn_predict.hip -- K11, the posterior predictive of device-resident samples of a SMALL tanh-MLP BNN: kernels and
// host side of sgmcmc_bnn_predict_{f32,f64}, sgmcmc_bnn_predict_row_tile and sgmcmc_predict_abi_version
// (include/sgmcmc_hip_predict.h, the posterior-predictive add-on outside the section 8(b) boundary). The reference evaluates
// the kept networks one by one and reduces on the host (pysgmcmc/models/bayesian_neural_network.py:560-630).
//
// Forward launch: blockIdx.x is the sample, blockIdx.y a group of row tiles. A workgroup copies ONE sample's parameters from
// its trace row into the LDS (16-byte accesses when the row is 16-byte aligned, element by element otherwise: n_params is odd
// for many nets) and walks its tiles of test rows: the X tile and two ping-pong activation buffers live in the LDS as well,
// so an activation never touches global memory and the only global traffic is the row, the X tile and one output per (sample,
// row). The layer loops are the whole-step kernel's forward loops (sgmcmc_bnn_fused.hip): every output unit owns its
// k-ordered fma chain; two adjacent outputs per lane with pair LDS accesses where the width and the offsets are even, the
// scalar loop otherwise -- same bits either way. means[s][r] therefore depends on theta_s and x_r and on nothing else: not on
// the row tile, the grid, the alignment, or how many samples or rows the call holds. Plain dot products in k order, no MFMA
// (a matrix-core form would change the summation order).
//
// Ensemble launch, behind it on the same stream: lane = test row, so every access is a coalesced row segment of `means`; one
// lane sums its column over s ascending in f64, twice (mean, then squared deviations), so equal `means` give equal bits
// whatever the launch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sgmcmc_hip_predict.h"

#pragma clang fp contract(off)

#include "sgmcmc_host.hpp"

using namespace sgmcmc_host;

namespace {

constexpr int PREDICT_MAX_LAYERS = 8;
constexpr int PREDICT_THREADS = 256;                       // 4 waves; at the default net 4 workgroups share a CU's LDS
constexpr int PREDICT_MAX_TILE = 32;                       // test rows per tile
constexpr int PREDICT_ENS_THREADS = 64;
constexpr size_t PREDICT_LDS_MAX = (size_t)160 * 1024;     // LDS of one CU (gfx950)
constexpr size_t PREDICT_LDS_SHARE = (size_t)40 * 1024;    // a workgroup's share when four are resident
constexpr size_t PREDICT_GRID_TARGET = 4096;               // workgroups a launch aims for before tiles are walked in a loop
constexpr size_t PREDICT_GRID_Y_MAX = 65535;

__device__ __forceinline__ float tanh_t(float x) { return tanhf(x); }
__device__ __forceinline__ double tanh_t(double x) { return tanh(x); }
__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

// pairs of consecutive elements as ONE LDS access (ds_read_b64 / b128), as in the whole-step kernel
template <typename T> struct Pair;
template <> struct Pair<float> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct Pair<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <typename T>
__device__ __forceinline__ typename Pair<T>::type ld2(const T *p) { return *reinterpret_cast<const typename Pair<T>::type *>(p); }
template <typename T>
__device__ __forceinline__ void st2(T *p, typename Pair<T>::type v) { *reinterpret_cast<typename Pair<T>::type *>(p) = v; }

template <typename T>
struct PredictChains {
    const T *p[SGMCMC_PREDICT_MAX_CHAINS];                 // by value in the kernel arguments: no device-side pointer table
};

// The net and where a workgroup keeps it: element offsets into the LDS, every one a multiple of 4 (16 bytes in f32, 32 in
// f64), the parameter copy at 0. Host arithmetic shared by the entry and by sgmcmc_bnn_predict_row_tile.
struct PredictNet {
    int n_layers;                                          // number of weight layers L
    int sizes[PREDICT_MAX_LAYERS + 1];                     // sizes[0] = inputs, sizes[L] = 1
    int off_w[PREDICT_MAX_LAYERS + 1], off_b[PREDICT_MAX_LAYERS + 1];   // parameter offsets of layer l (1-based)
    int n_params;
    int tile;                                              // test rows per tile
    int lds_x, lds_a[2];                                   // X tile; activations of layer l in lds_a[l & 1]
    size_t lds_bytes;
};

inline size_t round4(size_t v) { return (v + 3) & ~(size_t)3; }

int predict_plan(const char *what, const int *layer_sizes, int n_layers, size_t esize, PredictNet &net)
{
    if (!layer_sizes) return fail(SGMCMC_EINVAL, "%s: layer_sizes is NULL", what);
    if (n_layers < 1 || n_layers > PREDICT_MAX_LAYERS) return fail(SGMCMC_EINVAL, "%s: 1..8 layers", what);
    for (int l = 0; l <= n_layers; ++l) {
        if (layer_sizes[l] < 1) return fail(SGMCMC_EINVAL, "%s: bad layer size", what);
        net.sizes[l] = layer_sizes[l];
    }
    if (layer_sizes[n_layers] != 1) return fail(SGMCMC_EINVAL, "%s: the last layer must have one unit", what);
    net.n_layers = n_layers;
    const size_t cap = PREDICT_LDS_MAX / esize;            // no sum below grows past it: nothing wraps
    size_t off = 0, widest = 0;
    for (int l = 1; l <= n_layers; ++l) {                  // parameter order: W1, b1, ..., WL, bL, log_var
        net.off_w[l] = (int)off; off += (size_t)net.sizes[l - 1] * (size_t)net.sizes[l];
        if (off > cap) return fail(SGMCMC_EINVAL, "%s: the parameters alone need more than 160 KiB of LDS", what);
        net.off_b[l] = (int)off; off += (size_t)net.sizes[l];
        if (off + 1 > cap) return fail(SGMCMC_EINVAL, "%s: the parameters alone need more than 160 KiB of LDS", what);
        if (l < n_layers && (size_t)net.sizes[l] > widest) widest = (size_t)net.sizes[l];
    }
    net.n_params = (int)(off + 1);
    const size_t w = round4(off + 1), d0 = (size_t)net.sizes[0];
    auto bytes = [&](size_t tile) { return (w + round4(tile * d0) + 2 * round4(tile * widest)) * esize; };
    size_t budget = 2 * w * esize;
    if (budget < PREDICT_LDS_SHARE) budget = PREDICT_LDS_SHARE;
    if (budget > PREDICT_LDS_MAX) budget = PREDICT_LDS_MAX;
    size_t tile = PREDICT_MAX_TILE;
    while (tile > 1 && bytes(tile) > budget) tile /= 2;
    if (bytes(tile) > PREDICT_LDS_MAX)
        return fail(SGMCMC_EINVAL, "%s: the parameters and ONE test row need %zu B of LDS (> 160 KiB)", what, bytes(tile));
    net.tile = (int)tile;
    net.lds_x = (int)w;
    net.lds_a[0] = (int)(w + round4(tile * d0));
    net.lds_a[1] = net.lds_a[0] + (int)round4(tile * widest);
    net.lds_bytes = bytes(tile);
    return 0;
}

template <typename T>
struct PredictArgs {
    PredictNet net;
    size_t n, ld;                                          // rows per chain matrix, elements between rows
    const T *X;
    size_t n_rows, n_tiles;
    T *means, *noise_var;
};

template <typename T>
__global__ void __launch_bounds__(PREDICT_THREADS) bnn_predict_kernel(const PredictChains<T> ch, const PredictArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char predict_lds_raw[];
    T *wl = reinterpret_cast<T *>(predict_lds_raw);        // this sample's parameters
    T *xs = wl + a.net.lds_x;
    const int tid = threadIdx.x, nt = blockDim.x;
    const size_t s = blockIdx.x;
    const size_t c = s / a.n;
    const T *row = ch.p[c] + (s - c * a.n) * a.ld;
    const int np = a.net.n_params;
    // ---- the sample's parameters into LDS: what lies behind n_params in a padded row is never read
    if ((reinterpret_cast<uintptr_t>(row) & 15u) == 0) {
        struct alignas(16) Q { unsigned v[4]; };
        constexpr int PER = 16 / (int)sizeof(T);
        const int nq = np / PER;
        const Q *__restrict__ src = reinterpret_cast<const Q *>(row);
        Q *dst = reinterpret_cast<Q *>(wl);
        for (int q = tid; q < nq; q += nt) dst[q] = src[q];
        for (int k = nq * PER + tid; k < np; k += nt) wl[k] = row[k];
    } else {
#pragma unroll 4
        for (int k = tid; k < np; k += nt) wl[k] = row[k];
    }
    if (a.noise_var != nullptr && blockIdx.y == 0 && tid == 0) a.noise_var[s] = (T)exp((double)row[np - 1]);
    const int L = a.net.n_layers, D0 = a.net.sizes[0], tile = a.net.tile;
    T *out = a.means + s * a.n_rows;
    for (size_t t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        const size_t r0 = t * (size_t)tile;
        const int B = (int)(a.n_rows - r0 < (size_t)tile ? a.n_rows - r0 : (size_t)tile);
        const T *__restrict__ xg = a.X + r0 * (size_t)D0;
        for (int k = tid; k < B * D0; k += nt) xs[k] = xg[k];
        __syncthreads();                                   // the first tile's also ends the parameter copy
        for (int l = 1; l <= L; ++l) {
            const int nin = a.net.sizes[l - 1], nout = a.net.sizes[l];
            const T *W = wl + a.net.off_w[l], *bias = wl + a.net.off_b[l];
            const T *hin = l == 1 ? xs : wl + a.net.lds_a[(l - 1) & 1];
            if (l == L) {
                // the one output unit: its k-ordered chain, then straight to means (coalesced over the tile's rows)
                for (int b = tid; b < B; b += nt) {
                    T acc = bias[0];
#pragma unroll 8
                    for (int k = 0; k < nin; ++k) acc = fma_t(hin[b * nin + k], W[k], acc);
                    out[r0 + b] = acc;
                }
            } else {
                T *hout = wl + a.net.lds_a[l & 1];
                // two adjacent outputs per lane where the layout allows pair accesses (even width, even offsets; the LDS
                // regions start on multiples of 4 elements): every output keeps its own k-ordered fma chain
                const bool pairs = (nout % 2 == 0) && ((a.net.off_w[l] | a.net.off_b[l]) % 2 == 0);
                if (pairs) {
                    const int half = nout / 2;
                    for (int idx = tid; idx < B * half; idx += nt) {
                        const int b = idx / half, j = 2 * (idx - b * half);
                        typename Pair<T>::type acc = ld2(bias + j);
#pragma unroll 8
                        for (int k = 0; k < nin; ++k) {
                            const T h = hin[b * nin + k];
                            const typename Pair<T>::type w = ld2(W + k * nout + j);
                            acc.x = fma_t(h, w.x, acc.x);
                            acc.y = fma_t(h, w.y, acc.y);
                        }
                        acc.x = tanh_t(acc.x); acc.y = tanh_t(acc.y);
                        st2(hout + b * nout + j, acc);
                    }
                } else {
                    for (int idx = tid; idx < B * nout; idx += nt) {
                        const int b = idx / nout, j = idx - b * nout;
                        T acc = bias[j];
#pragma unroll 8
                        for (int k = 0; k < nin; ++k) acc = fma_t(hin[b * nin + k], W[k * nout + j], acc);
                        hout[idx] = tanh_t(acc);
                    }
                }
            }
            __syncthreads();                               // the last layer's frees the X tile for the next one
        }
    }
}

// ens_mean[r] = mean_s means[s][r], ens_var[r] = mean_s (means[s][r] - ens_mean[r])^2: one lane per row, s ascending, f64
template <typename T>
__global__ void __launch_bounds__(PREDICT_ENS_THREADS) bnn_predict_ensemble_kernel(const T *__restrict__ means, size_t S,
                                                                                   size_t n_rows, double *__restrict__ ens_mean,
                                                                                   double *__restrict__ ens_var)
{
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const T *col = means + r;
    double sum = 0.0;
#pragma unroll 8
    for (size_t s = 0; s < S; ++s) sum += (double)col[s * n_rows];
    const double mean = sum / (double)S;
    double q = 0.0;
#pragma unroll 8
    for (size_t s = 0; s < S; ++s) {
        const double d = (double)col[s * n_rows] - mean;
        q += d * d;
    }
    ens_mean[r] = mean;
    ens_var[r] = q / (double)S;
}

template <typename T>
int bnn_predict(const T *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers, const T *X,
                size_t n_rows, T *means, T *noise_var, double *ens_mean, double *ens_var, hipStream_t st)
{
    const char *what = "bnn_predict";
    if (n_rows == 0 || n == 0) return 0;
    if (m < 1 || m > SGMCMC_PREDICT_MAX_CHAINS)
        return fail(SGMCMC_EINVAL, "%s: m = %d chains, must be 1 .. %d", what, m, SGMCMC_PREDICT_MAX_CHAINS);
    if (!chains || !layer_sizes || !X || !means) return fail(SGMCMC_EINVAL, "%s: NULL argument", what);
    if ((ens_mean == nullptr) != (ens_var == nullptr))
        return fail(SGMCMC_EINVAL, "%s: ens_mean and ens_var go together", what);
    PredictArgs<T> a{};
    if (int rc = predict_plan(what, layer_sizes, n_layers, sizeof(T), a.net)) return rc;
    if (ld < (size_t)a.net.n_params)
        return fail(SGMCMC_EINVAL, "%s: ld = %zu is smaller than n_params = %d", what, ld, a.net.n_params);
    PredictChains<T> ch;
    for (int c = 0; c < SGMCMC_PREDICT_MAX_CHAINS; ++c) {
        ch.p[c] = c < m ? chains[c] : nullptr;
        if (c < m && !ch.p[c]) return fail(SGMCMC_EINVAL, "%s: chains[%d] is NULL", what, c);
    }
    if (n > (size_t)INT32_MAX / (size_t)m)
        return fail(SGMCMC_EINVAL, "%s: m * n = %d * %zu samples, must be < 2^31", what, m, n);
    const size_t S = (size_t)m * n;
    if (ens_mean && (n_rows + PREDICT_ENS_THREADS - 1) / PREDICT_ENS_THREADS > (size_t)INT32_MAX)
        return fail(SGMCMC_EINVAL, "%s: n_rows = %zu is too large for one launch", what, n_rows);
    a.n = n; a.ld = ld; a.X = X; a.n_rows = n_rows; a.means = means; a.noise_var = noise_var;
    a.n_tiles = (n_rows + (size_t)a.net.tile - 1) / (size_t)a.net.tile;
    // enough workgroups to fill the chip; beyond that a workgroup keeps its parameters and walks several tiles
    size_t gy = (PREDICT_GRID_TARGET + S - 1) / S;
    if (gy > a.n_tiles) gy = a.n_tiles;
    if (gy > PREDICT_GRID_Y_MAX) gy = PREDICT_GRID_Y_MAX;
    auto kernel = &bnn_predict_kernel<T>;
    if (a.net.lds_bytes > 64 * 1024) {
        hipError_t e0 = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)a.net.lds_bytes);
        if (e0 != hipSuccess) return hip_fail(e0, "hipFuncSetAttribute(bnn_predict_kernel)");
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)S, (unsigned)gy), dim3(PREDICT_THREADS), a.net.lds_bytes, st, ch, a);
    if (int rc = launched("bnn_predict_kernel")) return rc;
    if (!ens_mean) return 0;
    const unsigned blocks = (unsigned)((n_rows + PREDICT_ENS_THREADS - 1) / PREDICT_ENS_THREADS);
    hipLaunchKernelGGL(bnn_predict_ensemble_kernel<T>, dim3(blocks), dim3(PREDICT_ENS_THREADS), 0, st,
                       static_cast<const T *>(means), S, n_rows, ens_mean, ens_var);
    return launched("bnn_predict_ensemble_kernel");
}

}  // namespace

extern "C" {

int sgmcmc_predict_abi_version(void) { return SGMCMC_PREDICT_ABI_VERSION; }

int sgmcmc_bnn_predict_f32(const float *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers,
                           const float *X, size_t n_rows, float *means, float *noise_var, double *ens_mean, double *ens_var,
                           sgmcmc_stream_t stream)
{
    return bnn_predict<float>(chains, m, n, ld, layer_sizes, n_layers, X, n_rows, means, noise_var, ens_mean, ens_var,
                              static_cast<hipStream_t>(stream));
}
int sgmcmc_bnn_predict_f64(const double *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers,
                           const double *X, size_t n_rows, double *means, double *noise_var, double *ens_mean,
                           double *ens_var, sgmcmc_stream_t stream)
{
    return bnn_predict<double>(chains, m, n, ld, layer_sizes, n_layers, X, n_rows, means, noise_var, ens_mean, ens_var,
                               static_cast<hipStream_t>(stream));
}

int sgmcmc_bnn_predict_row_tile(const int *layer_sizes, int n_layers, size_t element_size)
{
    if (element_size != 4 && element_size != 8)
        return fail(SGMCMC_EINVAL, "bnn_predict_row_tile: element_size must be 4 or 8, not %zu", element_size);
    PredictNet net{};
    if (int rc = predict_plan("bnn_predict_row_tile", layer_sizes, n_layers, element_size, net)) return rc;
    return net.tile;
}

}  // extern "C"
