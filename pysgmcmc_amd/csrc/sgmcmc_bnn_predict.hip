// sgmcmc_bnn_predict.hip -- K11, the posterior predictive of device-resident samples of a SMALL tanh-MLP BNN: kernels and
// host side of sgmcmc_bnn_predict_{f32,f64}, sgmcmc_bnn_predict_row_tile and sgmcmc_predict_abi_version
// (include/sgmcmc_hip_predict.h, the posterior-predictive add-on outside the section 8(b) boundary). The reference evaluates
// the kept networks one by one and reduces on the host (pysgmcmc/models/bayesian_neural_network.py:560-630).
//
// Forward launch: blockIdx.x is the sample, blockIdx.y a group of row tiles. A workgroup copies ONE sample's parameters from
// its trace row into the LDS and walks its tiles of test rows: the X tile and two ping-pong activation buffers live in the
// LDS as well, so an activation never touches global memory and the only global traffic is the row, the X tile and one output
// per (sample, row). The row copy, the layer loop and the ensemble launch behind it on the same stream are the small-net
// core's (sgmcmc_bnn_small_net.hpp), which K13 and K14 share; what is K11's own is the two-buffer LDS layout, its footprint
// and the noise_var store.
#include "sgmcmc_bnn_small_net.hpp"

namespace {

// The net and where a workgroup keeps it. Host arithmetic shared by the entry and by sgmcmc_bnn_predict_row_tile.
struct PredictNet : SmallNet {
    int tile;                                              // test rows per tile
    int lds_x, lds_a[2];                                   // X tile; activations of layer l in lds_a[l & 1]
    size_t lds_bytes;
};

int predict_plan(const char *what, const int *layer_sizes, int n_layers, size_t esize, PredictNet &net)
{
    size_t n_params = 0;
    if (int rc = small_net_rules(what, layer_sizes, n_layers, net, n_params)) return rc;
    if (int rc = small_net_offsets(what, n_params, esize, net)) return rc;
    const size_t w = round4(n_params), d0 = (size_t)net.sizes[0], widest = small_net_widest_hidden(net);
    auto elems = [&](size_t tile) { return w + round4(tile * d0) + 2 * round4(tile * widest); };
    const size_t tile = small_net_tile(n_params, esize, elems);
    if (elems(tile) * esize > SMALL_NET_LDS_MAX)
        return fail(SGMCMC_EINVAL, "%s: the parameters and ONE test row need %zu B of LDS (> 160 KiB)", what,
                    elems(tile) * esize);
    net.tile = (int)tile;
    net.lds_x = (int)w;
    net.lds_a[0] = (int)(w + round4(tile * d0));
    net.lds_a[1] = net.lds_a[0] + (int)round4(tile * widest);
    net.lds_bytes = elems(tile) * esize;
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
__global__ void __launch_bounds__(SMALL_NET_THREADS) bnn_predict_kernel(const SmallNetChains<T> ch, const PredictArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char predict_lds_raw[];
    T *wl = reinterpret_cast<T *>(predict_lds_raw);        // this sample's parameters
    T *xs = wl + a.net.lds_x;
    const int tid = threadIdx.x, nt = blockDim.x;
    const size_t s = blockIdx.x;
    const T *row = ch.row(s, a.n, a.ld);
    const int np = a.net.n_params;
    load_params_to_lds(wl, row, np, tid, nt);
    if (a.noise_var != nullptr && blockIdx.y == 0 && tid == 0) a.noise_var[s] = (T)exp((double)row[np - 1]);
    const int D0 = a.net.sizes[0], tile = a.net.tile;
    T *out = a.means + s * a.n_rows;
    for (size_t t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        const size_t r0 = t * (size_t)tile;
        const int B = (int)(a.n_rows - r0 < (size_t)tile ? a.n_rows - r0 : (size_t)tile);
        const T *__restrict__ xg = a.X + r0 * (size_t)D0;
        for (int k = tid; k < B * D0; k += nt) xs[k] = xg[k];
        __syncthreads();                                   // the first tile's also ends the parameter copy
        forward_tile(a.net, wl, xs, B, out + r0, tid, nt, [&](int l) { return a.net.lds_a[l & 1]; });
    }
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
    SmallNetChains<T> ch;
    if (int rc = small_net_chains(what, chains, m, ch)) return rc;
    if (n > (size_t)INT32_MAX / (size_t)m)
        return fail(SGMCMC_EINVAL, "%s: m * n = %d * %zu samples, must be < 2^31", what, m, n);
    const size_t S = (size_t)m * n;
    if (ens_mean && (n_rows + SMALL_NET_ENS_THREADS - 1) / SMALL_NET_ENS_THREADS > (size_t)INT32_MAX)
        return fail(SGMCMC_EINVAL, "%s: n_rows = %zu is too large for one launch", what, n_rows);
    a.n = n; a.ld = ld; a.X = X; a.n_rows = n_rows; a.means = means; a.noise_var = noise_var;
    a.n_tiles = (n_rows + (size_t)a.net.tile - 1) / (size_t)a.net.tile;
    if (int rc = launch_tiles(&bnn_predict_kernel<T>, "bnn_predict_kernel", S, a.n_tiles, a.net.lds_bytes, st, ch, a)) return rc;
    return ens_mean ? launch_ensemble<T>(means, S, n_rows, ens_mean, ens_var, st) : 0;
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
