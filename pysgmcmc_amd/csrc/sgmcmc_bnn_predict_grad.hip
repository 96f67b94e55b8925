// sgmcmc_bnn_predict_grad.hip -- K14, the input gradients of the posterior predictive of device-resident samples of a SMALL
// tanh-MLP BNN: kernels and host side of sgmcmc_bnn_predict_grad_{f32,f64}, sgmcmc_bnn_predict_grad_row_tile and
// sgmcmc_predict_grad_abi_version (include/sgmcmc_hip_predict_grad.h, the predictive-gradient add-on outside the section 8(b)
// boundary). A Bayesian-optimisation loop climbs an acquisition function of the predictive mean and variance; the model
// interface the reference follows (pysgmcmc/models/base_model.py) names the derivatives it needs `predictive_gradients`.
//
// Forward + backward launch: blockIdx.x is the sample, blockIdx.y a group of row tiles, as in K11 (sgmcmc_bnn_predict.hip).
// A workgroup copies ONE sample's parameters into the LDS and walks its tiles of test rows. The row copy and the forward
// layer loop are the small-net core's (sgmcmc_bnn_small_net.hpp), the ones K11 runs, so means[s][r] has K11's bits; the
// difference is that EVERY hidden layer's activations stay in the LDS (K11 ping-pongs two buffers). The backward sweep then
// walks the layers downwards through the transposed weights: lane (b, k) owns
// delta_{l-1}[b][k] and reads ROW k of W_l, which is contiguous in j (two elements per LDS access where the width and the
// offset are even; the same statements in the same order either way), against delta_l[b][:], which the lanes of one test
// row share. Lanes that differ in k read row starts n_l elements apart: at n_l = 50 that is a stride of 50 dwords in f32,
// 16 distinct banks per 32-lane group, a 2-way conflict on an access whose other operand is a broadcast; the job is bound
// by the latency of the fma chains, not by the LDS. Deltas ping-pong between two buffers; nothing but X, the parameter row,
// means and grads touches global memory, and grads is written coalesced over (row, d). No MFMA: a matrix-core form would
// change the summation order.
//
// Ensemble launches, behind it on the same stream: the core's reduction of means (one lane per test row), the kernel K11
// launches, then one lane per (row, d) element summing over s ascending in f64. Equal means and grads give equal bits
// whatever the launch.
#include "sgmcmc_bnn_small_net.hpp"

namespace {

constexpr int PGRAD_DENS_THREADS = 256;

// The net and where a workgroup keeps it.
struct PGradNet : SmallNet {
    int tile;                                              // test rows per tile
    int lds_x;                                             // X tile
    int lds_h[SMALL_NET_MAX_LAYERS];                       // activations of hidden layer l = 1 .. L-1
    int lds_d[2];                                          // delta of hidden layer l in lds_d[l & 1]
    size_t lds_bytes;
};

// The LDS plan of a net that passed small_net_rules: the offsets, the tile and the regions. Footprint: parameter copy + X
// tile + every hidden layer's activations for the tile + two delta buffers of the widest hidden layer.
int pgrad_plan(const char *what, size_t n_params, size_t esize, PGradNet &net)
{
    if (int rc = small_net_offsets(what, n_params, esize, net)) return rc;
    const int L = net.n_layers;
    const size_t w = round4(n_params), d0 = (size_t)net.sizes[0], widest = small_net_widest_hidden(net);
    auto elems = [&](size_t tile) {
        size_t e = w + round4(tile * d0) + 2 * round4(tile * widest);
        for (int l = 1; l < L; ++l) e += round4(tile * (size_t)net.sizes[l]);
        return e;
    };
    const size_t tile = small_net_tile(n_params, esize, elems);
    if (elems(tile) * esize > SMALL_NET_LDS_MAX)
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
__global__ void __launch_bounds__(SMALL_NET_THREADS) bnn_predict_grad_kernel(const SmallNetChains<T> ch, const PGradArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char pgrad_lds_raw[];
    T *wl = reinterpret_cast<T *>(pgrad_lds_raw);          // this sample's parameters
    T *xs = wl + a.net.lds_x;
    const int tid = threadIdx.x, nt = blockDim.x;
    const size_t s = blockIdx.x;
    load_params_to_lds(wl, ch.row(s, a.n, a.ld), a.net.n_params, tid, nt);
    const int L = a.net.n_layers, D0 = a.net.sizes[0], tile = a.net.tile;
    T *out = a.means + s * a.n_rows;
    T *gout = a.grads + s * a.n_rows * (size_t)D0;
    for (size_t t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        const size_t r0 = t * (size_t)tile;
        const int B = (int)(a.n_rows - r0 < (size_t)tile ? a.n_rows - r0 : (size_t)tile);
        const T *__restrict__ xg = a.X + r0 * (size_t)D0;
        for (int k = tid; k < B * D0; k += nt) xs[k] = xg[k];
        __syncthreads();                                   // the first tile's also ends the parameter copy
        // ---- forward: every hidden layer's activations kept
        forward_tile(a.net, wl, xs, B, out + r0, tid, nt, [&](int l) { return a.net.lds_h[l]; });
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
    if (int rc = small_net_rules(what, layer_sizes, n_layers, a.net, n_params)) return rc;
    SmallNetChains<T> ch;
    if (int rc = small_net_chains(what, chains, m, ch)) return rc;
    if (ld < n_params) return fail(SGMCMC_EINVAL, "%s: ld = %zu is smaller than n_params = %zu", what, ld, n_params);
    if (n > (size_t)INT32_MAX / (size_t)m)
        return fail(SGMCMC_EINVAL, "%s: m * n = %d * %zu samples, must be < 2^31", what, m, n);
    const size_t S = (size_t)m * n, D0 = (size_t)a.net.sizes[0];
    if (n_rows > SIZE_MAX - SMALL_NET_ENS_THREADS
        || (n_rows + SMALL_NET_ENS_THREADS - 1) / SMALL_NET_ENS_THREADS > (size_t)INT32_MAX)
        return fail(SGMCMC_EINVAL, "%s: n_rows = %zu is too large for one launch", what, n_rows);
    if (n_rows > ((size_t)INT32_MAX * PGRAD_DENS_THREADS) / D0)
        return fail(SGMCMC_EINVAL, "%s: n_rows * D0 = %zu * %zu elements is too large for one launch", what, n_rows, D0);
    if (int rc = pgrad_plan(what, n_params, sizeof(T), a.net)) return rc;
    a.n = n; a.ld = ld; a.X = X; a.n_rows = n_rows; a.means = means; a.grads = grads;
    a.n_tiles = (n_rows + (size_t)a.net.tile - 1) / (size_t)a.net.tile;
    if (int rc = launch_tiles(&bnn_predict_grad_kernel<T>, "bnn_predict_grad_kernel", S, a.n_tiles, a.net.lds_bytes, st, ch, a))
        return rc;
    if (!ens_mean) return 0;
    if (int rc = launch_ensemble<T>(means, S, n_rows, ens_mean, ens_var, st)) return rc;
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
    if (int rc = small_net_rules(what, layer_sizes, n_layers, net, n_params)) return rc;
    if (int rc = pgrad_plan(what, n_params, element_size, net)) return rc;
    return net.tile;
}

}  // extern "C"
