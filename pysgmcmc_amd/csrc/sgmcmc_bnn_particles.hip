// sgmcmc_bnn_particles.hip -- K15, the cost and the parameter gradient of every particle of a SMALL tanh-MLP BNN on one
// minibatch: kernel and host side of sgmcmc_bnn_particles_cost_grad_{f32,f64}, sgmcmc_bnn_particles_lds_bytes and
// sgmcmc_particles_abi_version (include/sgmcmc_hip_particles.h, the particle-gradient add-on outside the section 8(b)
// boundary). Stein variational gradient descent keeps its particles as the rows of an (n, P) device matrix and needs
// d cost / d theta of every row each step; this is the whole-step kernel's (sgmcmc_bnn_fused.hip) forward pass, loss head and
// backward sweep without its sampler state, its update and its step loop.
//
// blockIdx.x is the particle: ONE workgroup of 512 lanes copies the particle's parameters and the minibatch into the LDS,
// runs the small-net core's forward layer loop (sgmcmc_bnn_small_net.hpp: the whole-step kernel's loop, bit for bit) with
// every layer's activations kept, the loss head in double, and the backward sweep whose statements are the whole-step
// kernel's: gW[k][j] one b-ascending fma chain from 0, gb[j] a b-ascending plain sum, delta_{l-1}[b][k] one j-ascending fma
// chain from 0 times (1 - h * h). Pairs of adjacent outputs per lane with 8/16-byte LDS accesses where widths and offsets are
// even, the scalar loops otherwise; every output keeps its own chain, so the bits depend on neither. The gradient goes to
// global memory element by element (a row may start at any element), with the weight-prior term coef * theta added on the way
// when the caller asks for the full gradient. Nothing else is written to global memory; no atomics, no MFMA.
//
// LDS: 160 bytes for the block sums, then, in elements, the parameter copy (rounded up to 4) and the regions X, h_1 .. h_L,
// delta_1 .. delta_L, y packed without padding: the regions of an even number of elements first, so that each of them
// starts on an even element (a region of an odd number of elements has an odd width and is only ever read element by
// element). That stays within the whole-step kernel's footprint rule, which is what the launch asks for.
#include "sgmcmc_bnn_small_net.hpp"

#include "sgmcmc_hip_particles.h"

namespace {

constexpr int PARTICLES_THREADS = 512;                     // 8 waves, 2 per SIMD: the whole-step kernel's workgroup

// The net and where a workgroup keeps it: element offsets from the parameter copy.
struct ParticlesNet : SmallNet {
    int batch;
    int lds_h[SMALL_NET_MAX_LAYERS + 1];                   // h_0 = the minibatch's X, h_l the output of layer l (h_L: the means)
    int lds_d[SMALL_NET_MAX_LAYERS + 1];                   // delta_l, l = 1 .. L
    int lds_y;
};

template <typename T>
struct ParticlesArgs {
    ParticlesNet net;
    const T *theta;
    size_t ld;
    const T *Xb, *yb;
    size_t ldx;
    double batch_size, n_examples, wdecay, wp_den, lvp_den, ln_prior_mean, ln_prior_var;
    T coef;                                                // weight-prior gradient coef * theta; 0: left out
    T *grad;
    size_t ld_grad;
    T *cost_out;
};

// The footprint rule of the whole-step kernel, in bytes; 0 when it exceeds the LDS of one CU. Every size of a net that passed
// small_net_rules and small_net_offsets is <= 160 KiB / esize, so nothing wraps.
inline size_t particles_lds_bytes(const SmallNet &net, size_t n_params, int batch, size_t esize)
{
    size_t sum = 0;
    for (int l = 0; l <= net.n_layers; ++l) sum += (size_t)net.sizes[l];
    const size_t rows = 2 * sum + 1;
    if ((size_t)batch > SMALL_NET_LDS_MAX / rows) return 0;
    const size_t bytes = 160 + (rows * (size_t)batch + n_params + 4) * esize;
    return bytes <= SMALL_NET_LDS_MAX ? bytes : 0;
}

// The regions behind the parameter copy, dense, those of an even number of elements first
inline void particles_plan(ParticlesNet &net, size_t n_params, int batch)
{
    const int L = net.n_layers;
    size_t at = round4(n_params);
    for (int odd = 0; odd < 2; ++odd) {
        auto place = [&](int &off, size_t elems) {
            if ((int)(elems & 1) == odd) { off = (int)at; at += elems; }
        };
        for (int l = 0; l <= L; ++l) place(net.lds_h[l], (size_t)batch * (size_t)net.sizes[l]);
        for (int l = 1; l <= L; ++l) place(net.lds_d[l], (size_t)batch * (size_t)net.sizes[l]);
        place(net.lds_y, (size_t)batch);
    }
    net.lds_d[0] = 0;
    net.batch = batch;
}

// block-wide sum of one double per lane; every lane returns the total. red: 17 doubles of LDS.
__device__ __forceinline__ double particles_block_sum(double v, double *red)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                       // red may still be read from the previous call
    if (lane == 0) red[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
        red[16] = t;
    }
    __syncthreads();
    return red[16];
}

template <typename T>
__global__ void __launch_bounds__(PARTICLES_THREADS) bnn_particles_kernel(const ParticlesArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char particles_lds_raw[];
    double *red = reinterpret_cast<double *>(particles_lds_raw);  // 17 doubles (+ pad to 160 B)
    T *wl = reinterpret_cast<T *>(particles_lds_raw + 160);       // this particle's parameters
    const int tid = threadIdx.x, nt = blockDim.x;
    const size_t p = blockIdx.x;
    const int L = a.net.n_layers, B = a.net.batch, D0 = a.net.sizes[0], np = a.net.n_params;
    const T *theta = a.theta + p * a.ld;
    T *grad = a.grad + p * a.ld_grad;
    T *yb = wl + a.net.lds_y;
    const T coef = a.coef;
    // one gradient element on its way out: the weight-prior term is the statement the update operators apply as grad_decay
    auto put = [&](int i, T raw) { grad[i] = (coef != T(0)) ? raw + coef * wl[i] : raw; };

    load_params_to_lds(wl, theta, np, tid, nt);
    {
        T *x0 = wl + a.net.lds_h[0];
        for (int i = tid; i < B * D0; i += nt) {
            const int b = i / D0, d = i - b * D0;
            x0[i] = a.Xb[(size_t)b * a.ldx + d];
        }
        for (int i = tid; i < B; i += nt) yb[i] = a.yb[i];
    }
    __syncthreads();
    // sum(theta^2): the weight-prior value of the cost
    double part = 0.0;
    for (int i = tid; i < np; i += nt) { double v = (double)wl[i]; part += v * v; }
    const double tsq = particles_block_sum(part, red);
    // ---- forward: every layer's activations kept
    forward_tile(a.net, wl, wl + a.net.lds_h[0], B, wl + a.net.lds_h[L], tid, nt, [&](int l) { return a.net.lds_h[l]; });
    // ---- loss head (bayesian_neural_network.py:365-388), as in the whole-step kernel
    const double s = (double)wl[np - 1];
    const double es = exp(s), inv = 1.0 / (es + 1e-16), dscale = -(inv / a.batch_size);
    {
        const T *mean = wl + a.net.lds_h[L];
        T *dL = wl + a.net.lds_d[L];
        double sse = 0.0;
        for (int i = tid; i < B; i += nt) {
            double r = (double)yb[i] - (double)mean[i];
            sse += r * r;
            dL[i] = (T)(r * dscale);
        }
        const double tot = particles_block_sum(sse, red);  // ends with a barrier: dL is visible
        if (tid == 0) {
            const double Bd = (double)B;
            double log_like = (-(tot * (0.5 * inv)) - 0.5 * s * Bd) / a.batch_size;
            double d = s - a.ln_prior_mean;
            double lvp = -(d * d) / a.lvp_den - 0.5 * a.ln_prior_var;
            double wp = (-0.5 * a.wdecay) * tsq / a.wp_den;
            a.cost_out[p] = (T)(-(log_like + lvp / a.n_examples + wp / a.n_examples));
            put(np - 1, (T)(-((tot * (0.5 * es * inv * inv) - 0.5 * Bd) / a.batch_size
                              + (-2.0 * d / a.lvp_den) / a.n_examples)));
        }
    }
    // ---- backward
    for (int l = L; l >= 1; --l) {
        const int nin = a.net.sizes[l - 1], nout = a.net.sizes[l];
        const int ow = a.net.off_w[l], ob = a.net.off_b[l];
        const T *W = wl + ow;
        const T *hin = wl + a.net.lds_h[l - 1];
        const T *dl = wl + a.net.lds_d[l];
        // gW = h_{l-1}^T delta_l. 2 x 2 outputs per lane where the layout allows pair accesses: two pair loads feed four
        // independent b-ordered fma chains (same bits as the scalar form); gb = delta_l^T 1 rides along in b order
        const bool pj = (nout % 2 == 0) && ((ow | a.net.lds_d[l]) % 2 == 0);
        const bool pk = (nin % 2 == 0) && (a.net.lds_h[l - 1] % 2 == 0);
        if (pj && pk) {
            const int hj = nout / 2, items = (nin / 2) * hj;
            for (int idx = tid; idx < items; idx += nt) {
                const int k = 2 * (idx / hj), j = 2 * (idx % hj);
                typename Pair<T>::type a0 = {T(0), T(0)}, a1 = {T(0), T(0)}, sb = {T(0), T(0)};
#pragma unroll 4
                for (int b = 0; b < B; ++b) {
                    const typename Pair<T>::type h = ld2(hin + b * nin + k), d = ld2(dl + b * nout + j);
                    a0.x = fma_t(h.x, d.x, a0.x); a0.y = fma_t(h.x, d.y, a0.y);
                    a1.x = fma_t(h.y, d.x, a1.x); a1.y = fma_t(h.y, d.y, a1.y);
                    sb.x += d.x; sb.y += d.y;
                }
                put(ow + k * nout + j, a0.x); put(ow + k * nout + j + 1, a0.y);
                put(ow + (k + 1) * nout + j, a1.x); put(ow + (k + 1) * nout + j + 1, a1.y);
                if (k == 0) { put(ob + j, sb.x); put(ob + j + 1, sb.y); }     // (the lanes of the first row pair keep it)
            }
        } else {
            for (int idx = tid; idx < nin * nout; idx += nt) {
                const int k = idx / nout, j = idx - k * nout;
                T acc = T(0);
#pragma unroll 8
                for (int b = 0; b < B; ++b) acc = fma_t(hin[b * nin + k], dl[b * nout + j], acc);
                put(ow + idx, acc);
            }
            for (int j = tid; j < nout; j += nt) {                            // gb = delta_l^T 1
                T acc = T(0);
#pragma unroll 8
                for (int b = 0; b < B; ++b) acc += dl[b * nout + j];
                put(ob + j, acc);
            }
        }
        if (l > 1) {                                                          // delta_{l-1} = (delta_l W^T) (1 - h^2)
            T *dprev = wl + a.net.lds_d[l - 1];
            if (pj && pk && a.net.lds_d[l - 1] % 2 == 0) {
                // two adjacent k per lane, j in pairs: three pair loads per four fmas; each output keeps its j-ordered chain
                const int hk = nin / 2;
                for (int idx = tid; idx < B * hk; idx += nt) {
                    const int b = idx / hk, k = 2 * (idx - b * hk);
                    T acc0 = T(0), acc1 = T(0);
#pragma unroll 4
                    for (int j = 0; j < nout; j += 2) {
                        const typename Pair<T>::type d = ld2(dl + b * nout + j);
                        const typename Pair<T>::type w0 = ld2(W + k * nout + j), w1 = ld2(W + (k + 1) * nout + j);
                        acc0 = fma_t(d.x, w0.x, acc0); acc0 = fma_t(d.y, w0.y, acc0);
                        acc1 = fma_t(d.x, w1.x, acc1); acc1 = fma_t(d.y, w1.y, acc1);
                    }
                    const typename Pair<T>::type hv = ld2(hin + b * nin + k);
                    typename Pair<T>::type out = {acc0 * (T(1) - hv.x * hv.x), acc1 * (T(1) - hv.y * hv.y)};
                    st2(dprev + b * nin + k, out);
                }
            } else {
                for (int idx = tid; idx < B * nin; idx += nt) {
                    const int b = idx / nin, k = idx - b * nin;
                    T acc = T(0);
#pragma unroll 8
                    for (int j = 0; j < nout; ++j) acc = fma_t(dl[b * nout + j], W[k * nout + j], acc);
                    const T hv = hin[idx];
                    dprev[idx] = acc * (T(1) - hv * hv);
                }
            }
            __syncthreads();
        }
    }
}

// the checks every entry shares, under the caller's `what`: the net rules, batch; fills net.sizes and n_params
inline int particles_net(const char *what, const int *layer_sizes, int n_layers, int batch, ParticlesNet &net, size_t &n_params)
{
    if (int rc = small_net_rules(what, layer_sizes, n_layers, net, n_params)) return rc;
    if (batch < 1) return fail(SGMCMC_EINVAL, "%s: batch = %d, must be >= 1", what, batch);
    return 0;
}

template <typename T>
int bnn_particles_cost_grad(const T *theta, size_t n_particles, size_t ld, const int *layer_sizes, int n_layers, const T *Xb,
                            size_t ldx, const T *yb, int batch, double batch_size, double n_examples, double wdecay,
                            double prior_mean, double prior_var, int add_prior, T *grad, size_t ld_grad, T *cost_out,
                            hipStream_t st)
{
    const char *what = "bnn_particles_cost_grad";
    if (n_particles == 0) return 0;
    const struct { const void *p; const char *name; } required[] = {
        {theta, "theta"}, {Xb, "Xb"}, {yb, "yb"}, {grad, "grad"}, {cost_out, "cost_out"}};
    for (const auto &arg : required)
        if (!arg.p) return fail(SGMCMC_EINVAL, "%s: %s is NULL", what, arg.name);
    ParticlesArgs<T> a{};
    size_t n_params = 0;
    if (int rc = particles_net(what, layer_sizes, n_layers, batch, a.net, n_params)) return rc;
    if (ld < n_params) return fail(SGMCMC_EINVAL, "%s: ld = %zu is smaller than n_params = %zu", what, ld, n_params);
    if (ld_grad < n_params)
        return fail(SGMCMC_EINVAL, "%s: ld_grad = %zu is smaller than n_params = %zu", what, ld_grad, n_params);
    if (ldx < (size_t)a.net.sizes[0])
        return fail(SGMCMC_EINVAL, "%s: ldx = %zu is smaller than the %d inputs", what, ldx, a.net.sizes[0]);
    if (int rc = small_net_offsets(what, n_params, sizeof(T), a.net)) return rc;
    const size_t lds_bytes = particles_lds_bytes(a.net, n_params, batch, sizeof(T));
    if (lds_bytes == 0)
        return fail(SGMCMC_EINVAL, "%s: the parameters, the minibatch, the activations and the deltas need more than 160 KiB "
                    "of LDS at batch %d", what, batch);
    if (n_particles > (size_t)INT32_MAX)
        return fail(SGMCMC_EINVAL, "%s: n_particles = %zu, must be < 2^31", what, n_particles);
    particles_plan(a.net, n_params, batch);
    a.theta = theta; a.ld = ld; a.Xb = Xb; a.yb = yb; a.ldx = ldx;
    a.batch_size = batch_size; a.n_examples = n_examples; a.wdecay = wdecay;
    a.wp_den = (double)n_params + (2.0 * 1e-16 + 1e-16);
    a.lvp_den = 2.0 * prior_var + (2.0 * 1e-16 + 1e-16);
    a.ln_prior_mean = std::log(prior_mean); a.ln_prior_var = std::log(prior_var);
    a.coef = add_prior ? (T)(wdecay / (a.wp_den * n_examples)) : T(0);
    a.grad = grad; a.ld_grad = ld_grad; a.cost_out = cost_out;
    auto kernel = &bnn_particles_kernel<T>;
    if (lds_bytes > 64 * 1024) {
        hipError_t e0 = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)lds_bytes);
        if (e0 != hipSuccess) return fail((int)e0, "hipFuncSetAttribute(bnn_particles_kernel): %s", hipGetErrorString(e0));
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_particles), dim3(PARTICLES_THREADS), lds_bytes, st, a);
    return launched("bnn_particles_kernel");
}

}  // namespace

extern "C" {

int sgmcmc_particles_abi_version(void) { return SGMCMC_PARTICLES_ABI_VERSION; }

size_t sgmcmc_bnn_particles_lds_bytes(const int *layer_sizes, int n_layers, int batch, size_t esize)
{
    const char *what = "bnn_particles_lds_bytes";
    if (esize != 4 && esize != 8) { fail(SGMCMC_EINVAL, "%s: esize must be 4 or 8, not %zu", what, esize); return 0; }
    ParticlesNet net{};
    size_t n_params = 0;
    if (particles_net(what, layer_sizes, n_layers, batch, net, n_params)) return 0;
    if (n_params > SMALL_NET_LDS_MAX / esize) return 0;
    return particles_lds_bytes(net, n_params, batch, esize);
}

int sgmcmc_bnn_particles_cost_grad_f32(const float *theta, size_t n_particles, size_t ld, const int *layer_sizes, int n_layers,
                                       const float *Xb, size_t ldx, const float *yb, int batch, double batch_size,
                                       double n_examples, double wdecay, double prior_mean, double prior_var, int add_prior,
                                       float *grad, size_t ld_grad, float *cost_out, sgmcmc_stream_t stream)
{
    return bnn_particles_cost_grad<float>(theta, n_particles, ld, layer_sizes, n_layers, Xb, ldx, yb, batch, batch_size,
                                          n_examples, wdecay, prior_mean, prior_var, add_prior, grad, ld_grad, cost_out,
                                          static_cast<hipStream_t>(stream));
}
int sgmcmc_bnn_particles_cost_grad_f64(const double *theta, size_t n_particles, size_t ld, const int *layer_sizes, int n_layers,
                                       const double *Xb, size_t ldx, const double *yb, int batch, double batch_size,
                                       double n_examples, double wdecay, double prior_mean, double prior_var, int add_prior,
                                       double *grad, size_t ld_grad, double *cost_out, sgmcmc_stream_t stream)
{
    return bnn_particles_cost_grad<double>(theta, n_particles, ld, layer_sizes, n_layers, Xb, ldx, yb, batch, batch_size,
                                           n_examples, wdecay, prior_mean, prior_var, add_prior, grad, ld_grad, cost_out,
                                           static_cast<hipStream_t>(stream));
}

}  // extern "C"
