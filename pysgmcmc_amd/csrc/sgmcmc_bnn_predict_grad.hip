// sgmcmc_bnn_predict_grad.hip -- K14, the input gradients of the posterior predictive of device-resident samples of a SMALL
// tanh-MLP BNN: kernels and host side of sgmcmc_bnn_predict_grad_{f32,f64}, sgmcmc_bnn_predict_grad_row_tile and
// sgmcmc_predict_grad_abi_version (include/sgmcmc_hip_predict_grad.h, the predictive-gradient add-on outside the section 8(b)
// boundary). A Bayesian-optimisation loop climbs an acquisition function of the predictive mean and variance; the model
// interface the reference follows (pysgmcmc/models/base_model.py) names the derivatives it needs `predictive_gradients`.
//
// Forward + backward launch: blockIdx.x is the sample, blockIdx.y a group of row tiles, as in K11 (sgmcmc_bnn_predict.hip).
// A workgroup copies ONE sample's parameters into the LDS and walks its tiles of test rows. The forward loops are K11's,
// restated here -- every output unit owns its k-ordered fma chain, pair LDS accesses where the layout allows them -- so
// means[s][r] has K11's bits; the difference is that EVERY hidden layer's activations stay in the LDS (K11 ping-pongs two
// buffers). The backward sweep then walks the layers downwards through the transposed weights: lane (b, k) owns
// delta_{l-1}[b][k] and reads ROW k of W_l, which is contiguous in j (two elements per LDS access where the width and the
// offset are even; the same statements in the same order either way), against delta_l[b][:], which the lanes of one test
// row share. Lanes that differ in k read row starts n_l elements apart: at n_l = 50 that is a stride of 50 dwords in f32,
// 16 distinct banks per 32-lane group, a 2-way conflict on an access whose other operand is a broadcast; the job is bound
// by the latency of the fma chains, not by the LDS. Deltas ping-pong between two buffers; nothing but X, the parameter row,
// means and grads touches global memory, and grads is written coalesced over (row, d). No MFMA: a matrix-core form would
// change the summation order.
//
// Ensemble launches, behind it on the same stream: K11's reduction of means (one lane per test row), then one lane per
// (row, d) element summing over s ascending in f64. Equal means and grads give equal bits whatever the launch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sgmcmc_hip_predict_grad.h"

#pragma clang fp contract(off)

#include "sgmcmc_host.hpp"

using namespace sgmcmc_host;

namespace {

constexpr int PGRAD_MAX_LAYERS = 8;
constexpr int PGRAD_THREADS = 256;                         // 4 waves: up to 256 VGPRs per lane, far from the 512-lane cliff
constexpr int PGRAD_MAX_TILE = 32;                         // test rows per tile
constexpr int PGRAD_ENS_THREADS = 64;
constexpr int PGRAD_DENS_THREADS = 256;
constexpr size_t PGRAD_LDS_MAX = (size_t)160 * 1024;       // LDS of one CU (gfx950)
constexpr size_t PGRAD_LDS_SHARE = (size_t)40 * 1024;      // a workgroup's share when four are resident
constexpr size_t PGRAD_GRID_TARGET = 4096;                 // workgroups a launch aims for before tiles are walked in a loop
constexpr size_t PGRAD_GRID_Y_MAX = 65535;
constexpr size_t PGRAD_PARAMS_SATURATED = (size_t)1 << 40; // n_params is not counted beyond this: no sum wraps

__device__ __forceinline__ float tanh_t(float x) { return tanhf(x); }
__device__ __forceinline__ double tanh_t(double x) { return tanh(x); }
__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

// pairs of consecutive elements as ONE LDS access (ds_read_b64 / b128), as in K11
template <typename T> struct Pair;
template <> struct Pair<float> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct Pair<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <typename T>
__device__ __forceinline__ typename Pair<T>::type ld2(const T *p) { return *reinterpret_cast<const typename Pair<T>::type *>(p); }
template <typename T>
__device__ __forceinline__ void st2(T *p, typename Pair<T>::type v) { *reinterpret_cast<typename Pair<T>::type *>(p) = v; }

template <typename T>
struct PGradChains {
    const T *p[SGMCMC_PREDICT_GRAD_MAX_CHAINS];            // by value in the kernel arguments: no device-side pointer table
};

// The net and where a workgroup keeps it: element offsets into the LDS, every one a multiple of 4, the parameter copy at 0.
struct PGradNet {
    int n_layers;                                          // number of weight layers L
    int sizes[PGRAD_MAX_LAYERS + 1];                       // sizes[0] = inputs, sizes[L] = 1
    int off_w[PGRAD_MAX_LAYERS + 1], off_b[PGRAD_MAX_LAYERS + 1];   // parameter offsets of layer l (1-based)
    int n_params;
    int tile;                                              // test rows per tile
    int lds_x;                                             // X tile
    int lds_h[PGRAD_MAX_LAYERS];                           // activations of hidden layer l = 1 .. L-1
    int lds_d[2];                                          // delta of hidden layer l in lds_d[l & 1]
    size_t lds_bytes;
};

inline size_t round4(size_t v) { return (v + 3) & ~(size_t)3; }

// K11's net rules in K11's wording, and n_params (saturated at 2^40, so that nothing wraps for sizes near INT_MAX)
int pgrad_net_rules(const char *what, const int *layer_sizes, int n_layers, PGradNet &net, size_t &n_params)
{
    if (!layer_sizes) return fail(SGMCMC_EINVAL, "%s: layer_sizes is NULL", what);
    if (n_layers < 1 || n_layers > PGRAD_MAX_LAYERS) return fail(SGMCMC_EINVAL, "%s: 1..8 layers", what);
    for (int l = 0; l <= n_layers; ++l) {
        if (layer_sizes[l] < 1) return fail(SGMCMC_EINVAL, "%s: bad layer size", what);
        net.sizes[l] = layer_sizes[l];
    }
    if (layer_sizes[n_layers] != 1) return fail(SGMCMC_EINVAL, "%s: the last layer must have one unit", what);
    net.n_layers = n_layers;
    size_t off = 0;
    for (int l = 1; l <= n_layers && off < PGRAD_PARAMS_SATURATED; ++l)
        off += (size_t)net.sizes[l - 1] * (size_t)net.sizes[l] + (size_t)net.sizes[l];
    n_params = off < PGRAD_PARAMS_SATURATED ? off + 1 : PGRAD_PARAMS_SATURATED;
    return 0;
}

// The LDS plan of a net that passed pgrad_net_rules: the tile and the offsets. Footprint: parameter copy + X tile + every
// hidden layer's activations for the tile + two delta buffers of the widest hidden layer.
int pgrad_plan(const char *what, size_t n_params, size_t esize, PGradNet &net)
{
    const size_t cap = PGRAD_LDS_MAX / esize;
    if (n_params > cap) return fail(SGMCMC_EINVAL, "%s: the parameters alone need more than 160 KiB of LDS", what);
    const int L = net.n_layers;
    size_t off = 0, widest = 0;                            // every size is <= n_params <= cap from here on
    for (int l = 1; l <= L; ++l) {                         // parameter order: W1, b1, ..., WL, bL, log_var
        net.off_w[l] = (int)off; off += (size_t)net.sizes[l - 1] * (size_t)net.sizes[l];
        net.off_b[l] = (int)off; off += (size_t)net.sizes[l];
        if (l < L && (size_t)net.sizes[l] > widest) widest = (size_t)net.sizes[l];
    }
    net.n_params = (int)n_params;
    const size_t w = round4(n_params), d0 = (size_t)net.sizes[0];
    auto elems = [&](size_t tile) {
        size_t e = w + round4(tile * d0) + 2 * round4(tile * widest);
        for (int l = 1; l < L; ++l) e += round4(tile * (size_t)net.sizes[l]);
        return e;
    };
    size_t budget = 2 * w * esize;
    if (budget < PGRAD_LDS_SHARE) budget = PGRAD_LDS_SHARE;
    if (budget > PGRAD_LDS_MAX) budget = PGRAD_LDS_MAX;
    size_t tile = PGRAD_MAX_TILE;
    while (tile > 1 && elems(tile) * esize > budget) tile /= 2;
    if (elems(tile) * esize > PGRAD_LDS_MAX)
        return fail(SGMCMC_EINVAL, "%s: the parameters, the activations and the deltas of ONE test row need %zu B of LDS "
                    "(> 160 KiB)", what, elems(tile) * esize);
    net.tile = (int)tile;
    size_t at = w;
    net.lds_x = (int)at; at += round4(tile * d0);
    for (int l = 1; l < L; ++l) { net.lds_h[l] = (int)at; at += round4(tile * (size_t)net.sizes[l]); }
    net.lds_d[0] = (int)at; at += round4(tile * widest);
    net.lds_d[1] = (int)at; at += round4(tile * widest);
    net.lds_bytes = at * esize;
    return 0;
}

template <typename T>
struct PGradArgs {
    PGradNet net;
    size_t n, ld;                                          // rows per chain matrix, elements between rows
    const T *X;
    size_t n_rows, n_tiles;
    T *means, *grads;
};

// acc = 0; for j ascending: acc = fma(w[j], d[j], acc) -- two elements per LDS access where both rows start on even elements
template <typename T>
__device__ __forceinline__ T row_dot(const T *__restrict__ w, const T *__restrict__ d, int n, bool pairs)
{
    T acc = (T)0;
    if (pairs) {
#pragma unroll 4
        for (int j = 0; j < n; j += 2) {
            const typename Pair<T>::type wv = ld2(w + j), dv = ld2(d + j);
            acc = fma_t(wv.x, dv.x, acc);
            acc = fma_t(wv.y, dv.y, acc);
        }
    } else {
#pragma unroll 8
        for (int j = 0; j < n; ++j) acc = fma_t(w[j], d[j], acc);
    }
    return acc;
}

template <typename T>
__global__ void __launch_bounds__(PGRAD_THREADS) bnn_predict_grad_kernel(const PGradChains<T> ch, const PGradArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char pgrad_lds_raw[];
    T *wl = reinterpret_cast<T *>(pgrad_lds_raw);          // this sample's parameters
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
    const int L = a.net.n_layers, D0 = a.net.sizes[0], tile = a.net.tile;
    T *out = a.means + s * a.n_rows;
    T *gout = a.grads + s * a.n_rows * (size_t)D0;
    for (size_t t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        const size_t r0 = t * (size_t)tile;
        const int B = (int)(a.n_rows - r0 < (size_t)tile ? a.n_rows - r0 : (size_t)tile);
        const T *__restrict__ xg = a.X + r0 * (size_t)D0;
        for (int k = tid; k < B * D0; k += nt) xs[k] = xg[k];
        __syncthreads();                                   // the first tile's also ends the parameter copy
        // ---- forward: K11's loops, every hidden layer's activations kept
        for (int l = 1; l <= L; ++l) {
            const int nin = a.net.sizes[l - 1], nout = a.net.sizes[l];
            const T *W = wl + a.net.off_w[l], *bias = wl + a.net.off_b[l];
            const T *hin = l == 1 ? xs : wl + a.net.lds_h[l - 1];
            if (l == L) {
                // the one output unit: its k-ordered chain, then straight to means (coalesced over the tile's rows)
                for (int b = tid; b < B; b += nt) {
                    T acc = bias[0];
#pragma unroll 8
                    for (int k = 0; k < nin; ++k) acc = fma_t(hin[b * nin + k], W[k], acc);
                    out[r0 + b] = acc;
                }
            } else {
                T *hout = wl + a.net.lds_h[l];
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
            __syncthreads();
        }
        // ---- backward: d means / d X through the transposed weights; lane (b, k) owns one delta, idx = b * width + k
        T *g = gout + r0 * (size_t)D0;
        if (L == 1) {
            const T *W1 = wl + a.net.off_w[1];             // n_1 = 1: W_1[d][0] is element d
            for (int idx = tid; idx < B * D0; idx += nt) g[idx] = W1[idx % D0];
            continue;                                      // the forward pass's last barrier freed the X tile
        }
        {
            const int nk = a.net.sizes[L - 1];
            const T *WL = wl + a.net.off_w[L], *h = wl + a.net.lds_h[L - 1];
            T *dout = wl + a.net.lds_d[(L - 1) & 1];
            for (int idx = tid; idx < B * nk; idx += nt) {
                const T hv = h[idx];
                const T hh = hv * hv;
                const T one_m = (T)1 - hh;
                dout[idx] = WL[idx % nk] * one_m;
            }
            __syncthreads();
        }
        for (int l = L - 1; l >= 2; --l) {
            const int nk = a.net.sizes[l - 1], nj = a.net.sizes[l];
            const T *W = wl + a.net.off_w[l], *h = wl + a.net.lds_h[l - 1];
            const T *din = wl + a.net.lds_d[l & 1];
            T *dout = wl + a.net.lds_d[(l - 1) & 1];
            const bool pairs = (nj % 2 == 0) && (a.net.off_w[l] % 2 == 0);
            for (int idx = tid; idx < B * nk; idx += nt) {
                const int b = idx / nk, k = idx - b * nk;
                const T acc = row_dot(W + k * nj, din + b * nj, nj, pairs);
                const T hv = h[idx];
                const T hh = hv * hv;
                const T one_m = (T)1 - hh;
                dout[idx] = acc * one_m;
            }
            __syncthreads();
        }
        {
            const int nj = a.net.sizes[1];
            const T *W = wl + a.net.off_w[1], *din = wl + a.net.lds_d[1];
            const bool pairs = (nj % 2 == 0) && (a.net.off_w[1] % 2 == 0);
            for (int idx = tid; idx < B * D0; idx += nt) {
                const int b = idx / D0, d = idx - b * D0;
                g[idx] = row_dot(W + d * nj, din + b * nj, nj, pairs);
            }
            // no barrier: before anything this stage reads (delta_1, W_1) is written again, the next tile passes the
            // barriers of its X copy and of its forward layers
        }
    }
}

// ens_mean[r] = mean_s means[s][r], ens_var[r] = mean_s (means[s][r] - ens_mean[r])^2: K11's statements in K11's order
template <typename T>
__global__ void __launch_bounds__(PGRAD_ENS_THREADS) bnn_predict_grad_ensemble_kernel(const T *__restrict__ means, size_t S,
                                                                                      size_t n_rows,
                                                                                      double *__restrict__ ens_mean,
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

// dmean[r][d] = (sum_s grads[s][r][d]) / S, dvar[r][d] = (2 sum_s (means[s][r] - ens_mean[r]) grads[s][r][d]) / S: one lane
// per element e = r * D0 + d (coalesced over grads' rows), s ascending, f64
template <typename T>
__global__ void __launch_bounds__(PGRAD_DENS_THREADS) bnn_predict_grad_dens_kernel(const T *__restrict__ means,
                                                                                   const T *__restrict__ grads, size_t S,
                                                                                   size_t n_rows, size_t D0,
                                                                                   const double *__restrict__ ens_mean,
                                                                                   double *__restrict__ dmean,
                                                                                   double *__restrict__ dvar)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t ne = n_rows * D0;
    if (e >= ne) return;
    const size_t r = e / D0;
    const double mean = ens_mean[r];
    const T *gcol = grads + e, *mcol = means + r;
    double G = 0.0, C = 0.0;
#pragma unroll 4
    for (size_t s = 0; s < S; ++s) {
        const double gv = (double)gcol[s * ne];
        const double dev = (double)mcol[s * n_rows] - mean;
        const double prod = dev * gv;
        G += gv;
        C += prod;
    }
    dmean[e] = G / (double)S;
    const double twice = 2.0 * C;
    dvar[e] = twice / (double)S;
}

template <typename T>
int bnn_predict_grad(const T *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers, const T *X,
                     size_t n_rows, T *means, T *grads, double *ens_mean, double *ens_var, double *dmean, double *dvar,
                     hipStream_t st)
{
    const char *what = "bnn_predict_grad";
    if (n_rows == 0 || n == 0) return 0;
    if (m < 1 || m > SGMCMC_PREDICT_GRAD_MAX_CHAINS)
        return fail(SGMCMC_EINVAL, "%s: m = %d chains, must be 1 .. %d", what, m, SGMCMC_PREDICT_GRAD_MAX_CHAINS);
    const struct { const void *p; const char *name; } required[] = {
        {chains, "chains"}, {layer_sizes, "layer_sizes"}, {X, "X"}, {means, "means"}, {grads, "grads"}};
    for (const auto &arg : required)
        if (!arg.p) return fail(SGMCMC_EINVAL, "%s: %s is NULL", what, arg.name);
    const int n_ens = (ens_mean != nullptr) + (ens_var != nullptr) + (dmean != nullptr) + (dvar != nullptr);
    if (n_ens != 0 && n_ens != 4)
        return fail(SGMCMC_EINVAL, "%s: ens_mean, ens_var, dmean and dvar go together (all four, or none)", what);
    PGradArgs<T> a{};
    size_t n_params = 0;
    if (int rc = pgrad_net_rules(what, layer_sizes, n_layers, a.net, n_params)) return rc;
    PGradChains<T> ch;
    for (int c = 0; c < SGMCMC_PREDICT_GRAD_MAX_CHAINS; ++c) {
        ch.p[c] = c < m ? chains[c] : nullptr;
        if (c < m && !ch.p[c]) return fail(SGMCMC_EINVAL, "%s: chains[%d] is NULL", what, c);
    }
    if (ld < n_params) return fail(SGMCMC_EINVAL, "%s: ld = %zu is smaller than n_params = %zu", what, ld, n_params);
    if (n > (size_t)INT32_MAX / (size_t)m)
        return fail(SGMCMC_EINVAL, "%s: m * n = %d * %zu samples, must be < 2^31", what, m, n);
    const size_t S = (size_t)m * n, D0 = (size_t)a.net.sizes[0];
    if (n_rows > SIZE_MAX - PGRAD_ENS_THREADS || (n_rows + PGRAD_ENS_THREADS - 1) / PGRAD_ENS_THREADS > (size_t)INT32_MAX)
        return fail(SGMCMC_EINVAL, "%s: n_rows = %zu is too large for one launch", what, n_rows);
    if (n_rows > ((size_t)INT32_MAX * PGRAD_DENS_THREADS) / D0)
        return fail(SGMCMC_EINVAL, "%s: n_rows * D0 = %zu * %zu elements is too large for one launch", what, n_rows, D0);
    if (int rc = pgrad_plan(what, n_params, sizeof(T), a.net)) return rc;
    a.n = n; a.ld = ld; a.X = X; a.n_rows = n_rows; a.means = means; a.grads = grads;
    a.n_tiles = (n_rows + (size_t)a.net.tile - 1) / (size_t)a.net.tile;
    // enough workgroups to fill the chip; beyond that a workgroup keeps its parameters and walks several tiles
    size_t gy = (PGRAD_GRID_TARGET + S - 1) / S;
    if (gy > a.n_tiles) gy = a.n_tiles;
    if (gy > PGRAD_GRID_Y_MAX) gy = PGRAD_GRID_Y_MAX;
    auto kernel = &bnn_predict_grad_kernel<T>;
    if (a.net.lds_bytes > 64 * 1024) {
        hipError_t e0 = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)a.net.lds_bytes);
        if (e0 != hipSuccess) return hip_fail(e0, "hipFuncSetAttribute(bnn_predict_grad_kernel)");
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)S, (unsigned)gy), dim3(PGRAD_THREADS), a.net.lds_bytes, st, ch, a);
    if (int rc = launched("bnn_predict_grad_kernel")) return rc;
    if (!ens_mean) return 0;
    const unsigned blocks = (unsigned)((n_rows + PGRAD_ENS_THREADS - 1) / PGRAD_ENS_THREADS);
    hipLaunchKernelGGL(bnn_predict_grad_ensemble_kernel<T>, dim3(blocks), dim3(PGRAD_ENS_THREADS), 0, st,
                       static_cast<const T *>(means), S, n_rows, ens_mean, ens_var);
    if (int rc = launched("bnn_predict_grad_ensemble_kernel")) return rc;
    const unsigned dblocks = (unsigned)((n_rows * D0 + PGRAD_DENS_THREADS - 1) / PGRAD_DENS_THREADS);
    hipLaunchKernelGGL(bnn_predict_grad_dens_kernel<T>, dim3(dblocks), dim3(PGRAD_DENS_THREADS), 0, st,
                       static_cast<const T *>(means), static_cast<const T *>(grads), S, n_rows, D0,
                       static_cast<const double *>(ens_mean), dmean, dvar);
    return launched("bnn_predict_grad_dens_kernel");
}

}  // namespace

extern "C" {

int sgmcmc_predict_grad_abi_version(void) { return SGMCMC_PREDICT_GRAD_ABI_VERSION; }

int sgmcmc_bnn_predict_grad_f32(const float *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers,
                                const float *X, size_t n_rows, float *means, float *grads, double *ens_mean, double *ens_var,
                                double *dmean, double *dvar, sgmcmc_stream_t stream)
{
    return bnn_predict_grad<float>(chains, m, n, ld, layer_sizes, n_layers, X, n_rows, means, grads, ens_mean, ens_var, dmean,
                                   dvar, static_cast<hipStream_t>(stream));
}
int sgmcmc_bnn_predict_grad_f64(const double *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers,
                                const double *X, size_t n_rows, double *means, double *grads, double *ens_mean,
                                double *ens_var, double *dmean, double *dvar, sgmcmc_stream_t stream)
{
    return bnn_predict_grad<double>(chains, m, n, ld, layer_sizes, n_layers, X, n_rows, means, grads, ens_mean, ens_var, dmean,
                                    dvar, static_cast<hipStream_t>(stream));
}

int sgmcmc_bnn_predict_grad_row_tile(const int *layer_sizes, int n_layers, size_t element_size)
{
    const char *what = "bnn_predict_grad_row_tile";
    if (element_size != 4 && element_size != 8)
        return fail(SGMCMC_EINVAL, "%s: element_size must be 4 or 8, not %zu", what, element_size);
    PGradNet net{};
    size_t n_params = 0;
    if (int rc = pgrad_net_rules(what, layer_sizes, n_layers, net, n_params)) return rc;
    if (int rc = pgrad_plan(what, n_params, element_size, net)) return rc;
    return net.tile;
}

}  // extern "C"
