// sgmcmc_bnn_small_net.hpp -- the core the kernels on a kept ensemble of a SMALL tanh-MLP BNN are written against: K11
// (sgmcmc_bnn_predict.hip), K13 (sgmcmc_bnn_score.hip) and K14 (sgmcmc_bnn_predict_grad.hip). Defined here ONCE: the device
// primitives, the by-value table of chain pointers, the net rules with their texts, the parameter offsets, the search for
// the row tile, the copy of a trace row into the LDS, the forward layer loop, the ensemble-moments kernel, the grid rule and
// the launch with its LDS opt-in. The add-on headers promise that `means` has the same bits and that `ens_mean` / `ens_var`
// are the same statements in the same order whichever entry wrote them: with one definition that holds by construction.
// Internal: nothing under include/ names it. Everything lives in an anonymous namespace (one copy per translation unit).
//
// The forward loop is the whole-step kernel's (sgmcmc_bnn_fused.hip): every output unit owns its k-ordered fma chain; two
// adjacent outputs per lane with pair LDS accesses where the width and the offsets are even, the scalar loop otherwise --
// same bits either way. means[s][r] therefore depends on theta_s and x_r and on nothing else: not on the row tile, the grid,
// the alignment, how many samples or rows the call holds, or where a kernel keeps its hidden layers. Plain dot products in k
// order, no MFMA (a matrix-core form would change the summation order).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sgmcmc_hip_predict.h"
#include "sgmcmc_hip_predict_grad.h"
#include "sgmcmc_hip_score.h"

#pragma clang fp contract(off)

#include "sgmcmc_host.hpp"

namespace {

using namespace sgmcmc_host;

constexpr int SMALL_NET_MAX_LAYERS = 8;
constexpr int SMALL_NET_THREADS = 256;                     // 4 waves; at the default net 4 workgroups share a CU's LDS
constexpr int SMALL_NET_MAX_TILE = 32;                     // test rows per tile
constexpr int SMALL_NET_ENS_THREADS = 64;
constexpr int SMALL_NET_MAX_CHAINS = SGMCMC_PREDICT_MAX_CHAINS;
constexpr size_t SMALL_NET_LDS_MAX = (size_t)160 * 1024;   // LDS of one CU (gfx950)
constexpr size_t SMALL_NET_LDS_SHARE = (size_t)40 * 1024;  // a workgroup's share when four are resident
constexpr size_t SMALL_NET_GRID_TARGET = 4096;             // workgroups a launch aims for before tiles are walked in a loop
constexpr size_t SMALL_NET_GRID_Y_MAX = 65535;
constexpr size_t SMALL_NET_PARAMS_SATURATED = (size_t)1 << 40;  // n_params is not counted beyond this: no sum wraps
static_assert(SGMCMC_PREDICT_MAX_CHAINS == SGMCMC_SCORE_MAX_CHAINS && SGMCMC_PREDICT_MAX_CHAINS == SGMCMC_PREDICT_GRAD_MAX_CHAINS,
              "the three add-ons share one table of chain pointers");

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
struct SmallNetChains {
    const T *p[SMALL_NET_MAX_CHAINS];                      // by value in the kernel arguments: no device-side pointer table
    // the trace row of sample s = c * n + i: row i of chain c, rows ld elements apart
    __device__ __forceinline__ const T *row(size_t s, size_t n, size_t ld) const
    {
        const size_t c = s / n;
        return p[c] + (s - c * n) * ld;
    }
};

// the host's table into the kernel's: entries behind m are NULL, one among the first m is refused
template <typename T>
inline int small_net_chains(const char *what, const T *const *chains, int m, SmallNetChains<T> &ch)
{
    for (int c = 0; c < SMALL_NET_MAX_CHAINS; ++c) {
        ch.p[c] = c < m ? chains[c] : nullptr;
        if (c < m && !ch.p[c]) return fail(SGMCMC_EINVAL, "%s: chains[%d] is NULL", what, c);
    }
    return 0;
}

// The net every kernel shares. A kernel's own struct derives from it and adds its tile and its LDS regions: element offsets
// into the LDS, every one a multiple of 4 (16 bytes in f32, 32 in f64), the parameter copy at 0.
struct SmallNet {
    int n_layers;                                          // number of weight layers L
    int sizes[SMALL_NET_MAX_LAYERS + 1];                   // sizes[0] = inputs, sizes[L] = 1
    int off_w[SMALL_NET_MAX_LAYERS + 1], off_b[SMALL_NET_MAX_LAYERS + 1];   // parameter offsets of layer l (1-based)
    int n_params;
};

inline size_t round4(size_t v) { return (v + 3) & ~(size_t)3; }

// The net rules, refused under the caller's `what`; fills n_layers and sizes. n_params is saturated at 2^40, so that nothing
// wraps for sizes near INT_MAX.
inline int small_net_rules(const char *what, const int *layer_sizes, int n_layers, SmallNet &net, size_t &n_params)
{
    if (!layer_sizes) return fail(SGMCMC_EINVAL, "%s: layer_sizes is NULL", what);
    if (n_layers < 1 || n_layers > SMALL_NET_MAX_LAYERS) return fail(SGMCMC_EINVAL, "%s: 1..8 layers", what);
    for (int l = 0; l <= n_layers; ++l) {
        if (layer_sizes[l] < 1) return fail(SGMCMC_EINVAL, "%s: bad layer size", what);
        net.sizes[l] = layer_sizes[l];
    }
    if (layer_sizes[n_layers] != 1) return fail(SGMCMC_EINVAL, "%s: the last layer must have one unit", what);
    net.n_layers = n_layers;
    size_t off = 0;
    for (int l = 1; l <= n_layers && off < SMALL_NET_PARAMS_SATURATED; ++l)
        off += (size_t)net.sizes[l - 1] * (size_t)net.sizes[l] + (size_t)net.sizes[l];
    n_params = off < SMALL_NET_PARAMS_SATURATED ? off + 1 : SMALL_NET_PARAMS_SATURATED;
    return 0;
}

// The parameter offsets of a net that passed small_net_rules; parameters that do not fit the LDS on their own are refused.
inline int small_net_offsets(const char *what, size_t n_params, size_t esize, SmallNet &net)
{
    if (n_params > SMALL_NET_LDS_MAX / esize)
        return fail(SGMCMC_EINVAL, "%s: the parameters alone need more than 160 KiB of LDS", what);
    size_t off = 0;                                        // every size is <= n_params <= 160 KiB / esize from here on
    for (int l = 1; l <= net.n_layers; ++l) {              // parameter order: W1, b1, ..., WL, bL, log_var
        net.off_w[l] = (int)off; off += (size_t)net.sizes[l - 1] * (size_t)net.sizes[l];
        net.off_b[l] = (int)off; off += (size_t)net.sizes[l];
    }
    net.n_params = (int)n_params;
    return 0;
}

inline size_t small_net_widest_hidden(const SmallNet &net)
{
    size_t widest = 0;
    for (int l = 1; l < net.n_layers; ++l)
        if ((size_t)net.sizes[l] > widest) widest = (size_t)net.sizes[l];
    return widest;
}

// The row tile: the largest power of two <= 32 whose footprint of elems(tile) elements stays within max(40 KiB, twice the
// parameter copy), at most 160 KiB; 1 where nothing fits, which the caller refuses in its own words.
template <typename Elems>
inline size_t small_net_tile(size_t n_params, size_t esize, Elems elems)
{
    size_t budget = 2 * round4(n_params) * esize;
    if (budget < SMALL_NET_LDS_SHARE) budget = SMALL_NET_LDS_SHARE;
    if (budget > SMALL_NET_LDS_MAX) budget = SMALL_NET_LDS_MAX;
    size_t tile = SMALL_NET_MAX_TILE;
    while (tile > 1 && elems(tile) * esize > budget) tile /= 2;
    return tile;
}

// ---- the sample's parameters into LDS: what lies behind n_params in a padded row is never read. 16-byte accesses when the
// row is 16-byte aligned, element by element otherwise (n_params is odd for many nets). The first tile's barrier ends it.
template <typename T>
__device__ __forceinline__ void load_params_to_lds(T *wl, const T *row, int np, int tid, int nt)
{
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
}

// The forward pass of B test rows whose X tile is at xs (behind a barrier): hidden layer l goes to wl + hidden_at(l), the
// one output of row b to out[b]. Ends with the last layer's barrier.
template <typename T, typename HiddenAt>
__device__ __forceinline__ void forward_tile(const SmallNet &net, T *wl, const T *xs, int B, T *out, int tid, int nt,
                                             HiddenAt hidden_at)
{
    const int L = net.n_layers;
    for (int l = 1; l <= L; ++l) {
        const int nin = net.sizes[l - 1], nout = net.sizes[l];
        const T *W = wl + net.off_w[l], *bias = wl + net.off_b[l];
        const T *hin = l == 1 ? xs : wl + hidden_at(l - 1);
        if (l == L) {
            // the one output unit: its k-ordered chain, then straight to means (coalesced over the tile's rows)
            for (int b = tid; b < B; b += nt) {
                T acc = bias[0];
#pragma unroll 8
                for (int k = 0; k < nin; ++k) acc = fma_t(hin[b * nin + k], W[k], acc);
                out[b] = acc;
            }
        } else {
            T *hout = wl + hidden_at(l);
            // two adjacent outputs per lane where the layout allows pair accesses (even width, even offsets; the LDS
            // regions start on multiples of 4 elements): every output keeps its own k-ordered fma chain
            const bool pairs = (nout % 2 == 0) && ((net.off_w[l] | net.off_b[l]) % 2 == 0);
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
        __syncthreads();                                   // the last layer's frees the X tile for the next one
    }
}

// ens_mean[r] = mean_s means[s][r], ens_var[r] = mean_s (means[s][r] - ens_mean[r])^2: lane = test row, so every access is a
// coalesced row segment of `means`; one lane sums its column over s ascending in f64, twice (mean, then squared deviations),
// so equal `means` give equal bits whatever the launch.
template <typename T>
__global__ void __launch_bounds__(SMALL_NET_ENS_THREADS) bnn_ensemble_kernel(const T *__restrict__ means, size_t S, size_t n_rows,
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

// the caller has checked that ceil(n_rows / 64) fits a grid
template <typename T>
inline int launch_ensemble(const T *means, size_t S, size_t n_rows, double *ens_mean, double *ens_var, hipStream_t st)
{
    const unsigned blocks = (unsigned)((n_rows + SMALL_NET_ENS_THREADS - 1) / SMALL_NET_ENS_THREADS);
    hipLaunchKernelGGL(bnn_ensemble_kernel<T>, dim3(blocks), dim3(SMALL_NET_ENS_THREADS), 0, st, means, S, n_rows, ens_mean,
                       ens_var);
    return launched("bnn_ensemble_kernel");
}

// grid.y = min(n_tiles, ceil(4096 / S), 65535): enough workgroups to fill the chip; beyond that a workgroup keeps its
// parameters and walks several tiles
inline unsigned small_net_grid_y(size_t S, size_t n_tiles)
{
    size_t gy = (SMALL_NET_GRID_TARGET + S - 1) / S;
    if (gy > n_tiles) gy = n_tiles;
    if (gy > SMALL_NET_GRID_Y_MAX) gy = SMALL_NET_GRID_Y_MAX;
    return (unsigned)gy;
}

// one workgroup per (sample, group of row tiles), with the opt-in a kernel needs above 64 KiB of dynamic LDS
template <typename Chains, typename Args>
inline int launch_tiles(void (*kernel)(const Chains, const Args), const char *name, size_t S, size_t n_tiles, size_t lds_bytes,
                        hipStream_t st, const Chains &ch, const Args &a)
{
    if (lds_bytes > 64 * 1024) {
        hipError_t e0 = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)lds_bytes);
        if (e0 != hipSuccess) return fail((int)e0, "hipFuncSetAttribute(%s): %s", name, hipGetErrorString(e0));
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)S, small_net_grid_y(S, n_tiles)), dim3(SMALL_NET_THREADS), lds_bytes, st, ch, a);
    return launched(name);
}

}  // namespace
