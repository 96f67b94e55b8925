// sgmcmc_bnn_fused.hip -- whole SGHMC steps of a SMALL tanh-MLP BNN in one kernel.
//
// BASELINE.json configs[1] (the reference's default model: 3x50 tanh net, 5 252 parameters,
// minibatch 20) is launch-bound on any GPU: one `next(sampler)` is ~20 launches of ~3-5 us even
// when replayed from a hipGraph. This kernel runs `n_steps` COMPLETE steps -- minibatch window,
// forward, loss head (pysgmcmc/models/bayesian_neural_network.py:365-388), analytic backward into
// the gradient row, fused SGHMC update (pysgmcmc/samplers/sghmc.py:165-251, the same quad operator
// and the same Philox stream as kernel K1), sum(theta^2) for the next cost -- with ONE workgroup of
// 512 lanes per chain and `__syncthreads()` between phases. Activations, deltas and a copy of the
// parameters live in LDS (the dot-product loops never wait on global memory); the sampler state stays
// in its arena rows (L2-resident at this size) and is streamed once per step by the update phase, which
// also drops theta' straight into the LDS copy for the next step.
// Measured (MI355X, 3x50 net, batch 20): 20.0 us per step (round 5; 27.2 before) = forward 5.2 + weight / bias gradients 3.2 +
// delta products 4.5 + update 3.2 + head / sums / barriers 3.9, bound by the instruction and LDS latency of ONE workgroup on one CU,
// not by memory: 256 chains in one launch take the same time per step. What round 5 changed: 512 lanes instead of 1024 (the
// 128-register cap of a 1024-lane workgroup spilled: 24.3 -> 20.4 us), pairs of adjacent outputs per lane with 8-byte LDS
// accesses (2 x 2 register tiles for the weight gradients, the bias gradients riding in the same loop), theta' written to the
// LDS copy by the update (no reload through L2), the next step's minibatch window requested a step ahead. Every output keeps
// its k-ordered fma chain, so the results are bit-identical to the scalar loops. (Tried and dropped: the update reading theta and
// the gradient from LDS copies through flat accesses -- 20.4 us for one chain, 256 chains 32 -> 37 us per step.) blockIdx.x is
// the chain: independent chains (seed = seed_base + chain, own state rows, own window stream) run
// concurrently on other CUs at no extra cost.
//
// The update arithmetic is the shared SghmcOp (bit-identical to K1 given the same gradient); the
// matrix products are plain fp32/fp64 dot products in k order, so a fused chain tracks the
// GEMM-based path to rounding (tests: 2e-4 relative over 12 steps, like the GEMM path itself
// against the fp64 golden trajectory).
//
// Three update operators (KIND): SGHMC (K1's SghmcOp), preconditioned SGLD (K2's SgldOp) and relativistic SGHMC (K3's
// RsghmcOp: rows theta, p, grad; no preconditioner rows, no burn-in switch). The operator's five stepsize-derived scalars
// arrive by value (bnn_fused_sghmc_kernel<T, KIND>: one stepsize for the launch) or from a device table of one block per step
// (bnn_fused_sghmc_kernel<T, KIND + FUSED_TABLE>: a stepsize schedule inside the launch; include/sgmcmc_hip_fused.h). The
// table is a template parameter, so the by-value kernels carry no trace of it.
//
// Thinned device trace (KIND + FUSED_TRACE, include/sgmcmc_hip_fused_trace.h): after every `trace_every`-th step the workgroup
// copies theta' from its LDS copy into the next row of a device matrix, so a run that keeps samples needs no launch boundary
// and no host copy per kept sample. A template parameter again: the untraced kernels are the instruction streams they were.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <utility>

#include "sgmcmc_hip.h"
#include "sgmcmc_hip_fused.h"
#include "sgmcmc_hip_fused_trace.h"

#pragma clang fp contract(off)

#include "sgmcmc_device.hpp"
#include "sgmcmc_host.hpp"
#include "sgmcmc_scalars.hpp"

using namespace sgmcmc_host;

namespace {

constexpr int FUSED_MAX_LAYERS = 8;
constexpr int FUSED_TABLE = 4;             // bit of the kernel's KIND_ parameter: per-step scalars table
constexpr int FUSED_TRACE = 8;             // bit of the kernel's KIND_ parameter: every trace_every-th theta' into a device trace
constexpr int FUSED_THREADS = 512;       // 8 waves: 2 per SIMD, 256 registers each (1024 lanes spilled registers: 24.3 vs 20.4 us per step)

__device__ __forceinline__ float tanh_t(float x) { return tanhf(x); }
__device__ __forceinline__ double tanh_t(double x) { return tanh(x); }
// dot products accumulate with fused multiply-add (a matrix product has no reference rounding order;
// GEMM libraries fuse too); the UPDATE arithmetic below stays one rounding per reference op
__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

// pairs of consecutive elements as ONE LDS access (ds_read_b64 / b128): half the LDS instructions of the dot-product loops
template <typename T> struct Pair;
template <> struct Pair<float> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct Pair<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <typename T>
__device__ __forceinline__ typename Pair<T>::type ld2(const T *p) { return *reinterpret_cast<const typename Pair<T>::type *>(p); }
template <typename T>
__device__ __forceinline__ void st2(T *p, typename Pair<T>::type v) { *reinterpret_cast<typename Pair<T>::type *>(p) = v; }

template <typename T>
struct FusedArgs {
    T *theta, *V, *grad, *tau, *g, *vh, *minv;          // chain c at + c * chain_stride (V: the relativistic kind's p)
    size_t n_params, chain_stride;
    int n_layers;                                        // number of weight layers L
    int sizes[FUSED_MAX_LAYERS + 1];                     // sizes[0] = inputs, sizes[L] = 1
    size_t off_w[FUSED_MAX_LAYERS + 1], off_b[FUSED_MAX_LAYERS + 1];   // parameter offsets of layer l (1-based)
    size_t act_off[FUSED_MAX_LAYERS + 1], del_off[FUSED_MAX_LAYERS + 1];  // LDS element offsets
    size_t lds_y;                                        // LDS element offset of the target window
    size_t lds_w;                                        // LDS element offset of the parameter copy
    const T *X, *y;
    size_t n_data;
    const int *starts;                                   // [n_chains][n_steps]
    int batch;
    double batch_size, n_examples, wp_den, lvp_den, ln_prior_mean, ln_prior_var, wdecay;
    T eps_e2, c1, c3, e4, mdecay, grad_decay;            // host-derived scalars of K1
    T sgld_eps, sgld_A, sgld_a_eff, sgld_two_eps, sgld_den;   // host-derived scalars of K2 (SGLD chains)
    uint64_t first_step, n_steps, burn_in_steps, seed_base;
    const T *xi;                                         // nullable: [n_steps][n_params], chain 0
    T *cost_out;                                         // [n_chains][n_steps]
    T rs_eps, rs_mass, rs_D, rs_m2c2, rs_nscale, rs_inv; // host-derived scalars of K3 (relativistic chains); rs_inv = 1 / m2c2
    int rs_pow2;                                         // m2c2 is a power of two: RsghmcOp's POW2 form (by-value launches only)
    const T *scalars_steps;                              // table kernels: [n_steps][5], the operator's scalars_dev block of step t
    // trace kernels: local step t is kept iff (trace_phase + t + 1) % trace_every == 0; the j-th kept step of the launch writes
    // theta' to trace + chain * trace_chain_stride + (trace_row + j) * n_params
    T *trace;
    size_t trace_chain_stride;
    uint64_t trace_row, trace_every, trace_phase;
};

// block-wide sum of one double per lane; every lane returns the total. red: 17 doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double *red)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = wave_sum_dpp_lane63(v);
    __syncthreads();                                      // red may still be read from the previous call
    if (lane == 63) red[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
        red[16] = t;
    }
    __syncthreads();
    return red[16];
}

// wl: the LDS copy of the parameters the next step's forward pass reads -- theta' goes there straight from the registers, so the
// next step does not wait for a round trip through L2 to get it back
template <typename Op>
__device__ __forceinline__ double run_update(Op &op, size_t n_params, typename Op::real *wl)
{
    const size_t nq_full = n_params / 4;
    const int tail = (int)(n_params % 4);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t q = threadIdx.x; q < nq_full; q += blockDim.x) {
        typename Op::Regs R;
        op.template load_vec<false>(q, R);
        op.compute(q, R);
        op.template store_vec<false>(q, R);
#pragma unroll
        for (int j = 0; j < 4; ++j) wl[4 * q + j] = R.th[j];
        op.template accumulate<true>(R, 4, acc);
    }
    if (tail && threadIdx.x == blockDim.x - 1) {
        typename Op::Regs R;
        op.load_part_(nq_full, tail, R);
        op.compute(nq_full, R);
        op.store_part_(nq_full, tail, R);
        for (int j = 0; j < tail; ++j) wl[4 * nq_full + j] = R.th[j];
        op.template accumulate<true>(R, tail, acc);
    }
    return acc[0];                                        // this lane's share of sum(theta'^2)
}

// TABLE: the operator reads its five scalars from `srow` (this step's row of FusedArgs::scalars_steps) in prepare(), as a
// graph-replayed per-step launch reads them from StepOpts.scalars_dev
template <bool TABLE, typename Op>
__device__ __forceinline__ double run_update_with(Op &op, const typename Op::real *srow, size_t n_params, typename Op::real *wl)
{
    if constexpr (TABLE) { op.scalars_dev = srow; op.prepare(); }
    return run_update(op, n_params, wl);
}

// KIND 0: SGHMC (K1's operator, sghmc.py:165-251); KIND 1: preconditioned SGLD (K2's operator, sgld.py:149-211)
template <typename T, int KIND, bool TABLE, bool ADAPT, bool INJECT>
__device__ __forceinline__ double update_phase(const FusedArgs<T> &a, T *theta, T *V, const T *grad, T *tau, T *g, T *vh,
                                               T *minv, const T *xi, const T *srow, uint64_t seed, uint64_t step, T *wl)
{
    NoiseKey nk;
    nk.k0 = (uint32_t)seed; nk.k1 = (uint32_t)(seed >> 32);
    nk.s0 = (uint32_t)step; nk.s1 = (uint32_t)(step >> 32);
    nk.step_dev = nullptr;
    if (KIND == 0) {
        SghmcOp<T, ADAPT, INJECT> op{theta, V, grad, tau, g, vh, minv, nullptr, xi,
                                     a.eps_e2, a.c1, a.c3, a.e4, a.mdecay, a.grad_decay, nk, nullptr};
        return run_update_with<TABLE>(op, srow, a.n_params, wl);
    } else {
        SgldOp<T, ADAPT, INJECT> op{theta, grad, tau, g, vh, minv, nullptr, xi, a.sgld_eps, a.sgld_A, a.sgld_a_eff,
                                    a.sgld_two_eps, a.sgld_den, a.grad_decay, nk, nullptr};
        return run_update_with<TABLE>(op, srow, a.n_params, wl);
    }
}

// KIND 2: relativistic SGHMC (K3's operator, relativistic_sghmc.py:120-140). K8 leaves d cost / d theta in the gradient row; the
// operator negates it, as in the per-step launch.
template <typename T, bool TABLE, bool POW2, bool INJECT>
__device__ __forceinline__ double update_phase_rsghmc(const FusedArgs<T> &a, T *theta, T *p, const T *grad, const T *xi,
                                                      const T *srow, uint64_t seed, uint64_t step, T *wl)
{
    NoiseKey nk;
    nk.k0 = (uint32_t)seed; nk.k1 = (uint32_t)(seed >> 32);
    nk.s0 = (uint32_t)step; nk.s1 = (uint32_t)(step >> 32);
    nk.step_dev = nullptr;
    RsghmcOp<T, POW2, INJECT> op{theta, p, grad, xi, a.rs_eps, a.rs_mass, a.rs_D, a.rs_m2c2, a.rs_nscale, a.grad_decay, nk,
                                 nullptr, nullptr, a.rs_inv};
    return run_update_with<TABLE>(op, srow, a.n_params, wl);
}

// KIND_: the update operator (0 SGHMC, 1 SGLD, 2 relativistic SGHMC), + FUSED_TABLE when the operator's scalars come from
// FusedArgs::scalars_steps (row t at step t: a stepsize schedule inside the launch) instead of by value. A template
// parameter, not a branch: bnn_fused_sghmc_kernel<T, 0> and <T, 1> are the by-value kernels they always were.
// + FUSED_TRACE: the kept steps' theta' go to FusedArgs::trace as well.
template <typename T, int KIND_>
__global__ void __launch_bounds__(FUSED_THREADS) bnn_fused_sghmc_kernel(const FusedArgs<T> a)
{
    constexpr int KIND = KIND_ & 3;
    constexpr bool TABLE = (KIND_ & FUSED_TABLE) != 0;
    constexpr bool TRACE = (KIND_ & FUSED_TRACE) != 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double *red = reinterpret_cast<double *>(smem_raw);           // 17 doubles (+ pad to 160 B)
    T *lds = reinterpret_cast<T *>(smem_raw + 160);
    const int chain = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const size_t cs = (size_t)chain * a.chain_stride;
    T *theta = a.theta + cs, *V = KIND != 1 ? a.V + cs : nullptr, *grad = a.grad + cs;
    T *tau = KIND != 2 ? a.tau + cs : nullptr, *g = KIND != 2 ? a.g + cs : nullptr;
    T *vh = KIND != 2 ? a.vh + cs : nullptr, *minv = KIND != 2 ? a.minv + cs : nullptr;
    const int L = a.n_layers, B = a.batch;
    const uint64_t seed = a.seed_base + (uint64_t)chain;
    T *yb = lds + a.lds_y;
    T *wl = lds + a.lds_w;                                // this step's parameters

    // sum(theta^2) of the starting point (weight-prior value of the first cost)
    double part = 0.0;
    for (size_t i = tid; i < a.n_params; i += nt) { double v = (double)theta[i]; part += v * v; }
    double tsq = block_sum(part, red);

    // The next step's minibatch window is requested a whole step ahead (its start index, then one window element per lane, into
    // registers): the dependent pair of global loads is off the step's critical path. Windows larger than the workgroup are
    // loaded in place as before.
    const int D0 = a.sizes[0];
    const bool prefetch = (size_t)B * D0 <= (size_t)nt;
    T x_next = T(0), y_next = T(0);
    auto fetch_window = [&](uint64_t tt) {
        const size_t st = (size_t)a.starts[(size_t)chain * a.n_steps + tt];
        if (tid < B * D0) x_next = a.X[st * D0 + tid];
        if (tid < B) y_next = a.y[st + tid];
    };
    if (prefetch) fetch_window(0);
    // steps left until the next kept one (a countdown instead of a 64-bit remainder per step), and where its row goes
    uint64_t keep_in = TRACE ? a.trace_every - a.trace_phase : 0;
    T *trow = TRACE ? a.trace + (size_t)chain * a.trace_chain_stride + (size_t)a.trace_row * a.n_params : nullptr;
    for (uint64_t t = 0; t < a.n_steps; ++t) {
        const uint64_t step = a.first_step + t;
        // ---- parameters into LDS (first step of the launch: later ones find theta' there, written by the update phase);
        // minibatch window [start, start + B) (pysgmcmc/data_batches.py:118-123)
        {
            if (t == 0) {
#pragma unroll 4
                for (size_t i = tid; i < a.n_params; i += nt) wl[i] = theta[i];
            }
            T *x0 = lds + a.act_off[0];
            if (prefetch) {
                if (tid < B * D0) x0[tid] = x_next;
                if (tid < B) yb[tid] = y_next;
                if (t + 1 < a.n_steps) fetch_window(t + 1);
            } else {
                const size_t start = (size_t)a.starts[(size_t)chain * a.n_steps + t];
                for (int i = tid; i < B * D0; i += nt) x0[i] = a.X[start * D0 + i];
                for (int i = tid; i < B; i += nt) yb[i] = a.y[start + i];
            }
        }
        __syncthreads();
        // ---- forward
        for (int l = 1; l <= L; ++l) {
            const int nin = a.sizes[l - 1], nout = a.sizes[l];
            const T *W = wl + a.off_w[l], *bias = wl + a.off_b[l];
            const T *hin = lds + a.act_off[l - 1];
            T *hout = lds + a.act_off[l];
            // two adjacent outputs per lane where the layout allows pair accesses (even width, even offsets): the weight row and
            // the bias come as pairs; every output keeps its own k-ordered fma chain (same bits as the scalar form)
            const bool pairs = (nout % 2 == 0) && ((a.off_w[l] | a.off_b[l] | a.act_off[l] | a.lds_w) % 2 == 0);
            if (pairs) {
                const int half = nout / 2;
                for (int idx = tid; idx < B * half; idx += nt) {
                    const int b = idx / half, j = 2 * (idx - b * half);
                    typename Pair<T>::type acc = ld2(bias + j);
#pragma unroll 8
                    for (int k = 0; k < nin; ++k) {
                        const T h = hin[b * nin + k];
                        const typename Pair<T>::type w = ld2(W + (size_t)k * nout + j);
                        acc.x = fma_t(h, w.x, acc.x);
                        acc.y = fma_t(h, w.y, acc.y);
                    }
                    if (l < L) { acc.x = tanh_t(acc.x); acc.y = tanh_t(acc.y); }
                    st2(hout + b * nout + j, acc);
                }
            } else {
                for (int idx = tid; idx < B * nout; idx += nt) {
                    const int b = idx / nout, j = idx - b * nout;
                    T acc = bias[j];
#pragma unroll 8
                    for (int k = 0; k < nin; ++k) acc = fma_t(hin[b * nin + k], W[(size_t)k * nout + j], acc);
                    hout[idx] = (l < L) ? tanh_t(acc) : acc;
                }
            }
            __syncthreads();
        }
        // ---- loss head (bayesian_neural_network.py:365-388)
        const double s = (double)wl[a.n_params - 1];
        const double es = exp(s), inv = 1.0 / (es + 1e-16), dscale = -(inv / a.batch_size);
        {
            const T *mean = lds + a.act_off[L];
            T *dL = lds + a.del_off[L];
            double sse = 0.0;
            for (int i = tid; i < B; i += nt) {
                double r = (double)yb[i] - (double)mean[i];
                sse += r * r;
                dL[i] = (T)(r * dscale);
            }
            const double tot = block_sum(sse, red);       // ends with a barrier: dL is visible
            if (tid == 0) {
                const double Bd = (double)B;
                double log_like = (-(tot * (0.5 * inv)) - 0.5 * s * Bd) / a.batch_size;
                double d = s - a.ln_prior_mean;
                double lvp = -(d * d) / a.lvp_den - 0.5 * a.ln_prior_var;
                double wp = (-0.5 * a.wdecay) * tsq / a.wp_den;
                a.cost_out[(size_t)chain * a.n_steps + t] = (T)(-(log_like + lvp / a.n_examples + wp / a.n_examples));
                // d NLL / d log_var; its weight-prior term is added by the update (grad_decay)
                grad[a.n_params - 1] = (T)(-((tot * (0.5 * es * inv * inv) - 0.5 * Bd) / a.batch_size
                                             + (-2.0 * d / a.lvp_den) / a.n_examples));
            }
        }
        // ---- backward
        for (int l = L; l >= 1; --l) {
            const int nin = a.sizes[l - 1], nout = a.sizes[l];
            const T *W = wl + a.off_w[l];
            const T *hin = lds + a.act_off[l - 1];
            const T *dl = lds + a.del_off[l];
            T *gW = grad + a.off_w[l], *gb = grad + a.off_b[l];
            // gW = h_{l-1}^T delta_l. 2 x 2 outputs per lane where the layout allows pair accesses: two pair loads feed four
            // independent b-ordered fma chains (same bits as the scalar form, a quarter of its LDS instructions)
            const bool pj = (nout % 2 == 0) && ((a.off_w[l] | a.del_off[l]) % 2 == 0);
            const bool pk = (nin % 2 == 0) && (a.act_off[l - 1] % 2 == 0);
            if (pj && pk && a.off_b[l] % 2 == 0) {
                const int hj = nout / 2, items = (nin / 2) * hj;
                for (int idx = tid; idx < items; idx += nt) {
                    const int k = 2 * (idx / hj), j = 2 * (idx % hj);
                    typename Pair<T>::type a0 = {T(0), T(0)}, a1 = {T(0), T(0)}, sb = {T(0), T(0)};
#pragma unroll 4
                    for (int b = 0; b < B; ++b) {
                        const typename Pair<T>::type h = ld2(hin + b * nin + k), d = ld2(dl + b * nout + j);
                        a0.x = fma_t(h.x, d.x, a0.x); a0.y = fma_t(h.x, d.y, a0.y);
                        a1.x = fma_t(h.y, d.x, a1.x); a1.y = fma_t(h.y, d.y, a1.y);
                        sb.x += d.x; sb.y += d.y;                 // gb = delta_l^T 1 rides along (b order, as the loop below)
                    }
                    st2(gW + (size_t)k * nout + j, a0);
                    st2(gW + (size_t)(k + 1) * nout + j, a1);
                    if (k == 0) st2(gb + j, sb);                  // (the lanes of the first row pair keep it)
                }
            } else {
                for (int idx = tid; idx < nin * nout; idx += nt) {
                    const int k = idx / nout, j = idx - k * nout;
                    T acc = T(0);
#pragma unroll 8
                    for (int b = 0; b < B; ++b) acc = fma_t(hin[b * nin + k], dl[b * nout + j], acc);
                    gW[idx] = acc;
                }
            }
            if (!(pj && pk && a.off_b[l] % 2 == 0)) {
                for (int j = tid; j < nout; j += nt) {                    // gb = delta_l^T 1
                    T acc = T(0);
#pragma unroll 8
                    for (int b = 0; b < B; ++b) acc += dl[b * nout + j];
                    gb[j] = acc;
                }
            }
            if (l > 1) {                                                  // delta_{l-1} = (delta_l W^T) (1 - h^2)
                T *dprev = lds + a.del_off[l - 1];
                if (pj && pk && a.del_off[l - 1] % 2 == 0) {
                    // two adjacent k per lane, j in pairs: three pair loads per four fmas; each output keeps its j-ordered chain
                    const int hk = nin / 2;
                    for (int idx = tid; idx < B * hk; idx += nt) {
                        const int b = idx / hk, k = 2 * (idx - b * hk);
                        T acc0 = T(0), acc1 = T(0);
#pragma unroll 4
                        for (int j = 0; j < nout; j += 2) {
                            const typename Pair<T>::type d = ld2(dl + b * nout + j);
                            const typename Pair<T>::type w0 = ld2(W + (size_t)k * nout + j), w1 = ld2(W + (size_t)(k + 1) * nout + j);
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
                        for (int j = 0; j < nout; ++j) acc = fma_t(dl[b * nout + j], W[(size_t)k * nout + j], acc);
                        const T hv = hin[idx];
                        dprev[idx] = acc * (T(1) - hv * hv);
                    }
                }
            }
            __syncthreads();
        }
        // ---- fused update (K1's, K2's or K3's operator) + sum(theta'^2)
        const bool adapt = step < a.burn_in_steps || a.burn_in_steps == 0;
        const T *xi = (a.xi != nullptr && chain == 0) ? a.xi + (size_t)t * a.n_params : nullptr;
        const T *srow = TABLE ? a.scalars_steps + 5 * t : nullptr;
        double share;
        if constexpr (KIND == 2) {
            if (!TABLE && a.rs_pow2) {
                share = xi ? update_phase_rsghmc<T, TABLE, true, true>(a, theta, V, grad, xi, srow, seed, step, wl)
                           : update_phase_rsghmc<T, TABLE, true, false>(a, theta, V, grad, xi, srow, seed, step, wl);
            } else {
                share = xi ? update_phase_rsghmc<T, TABLE, false, true>(a, theta, V, grad, xi, srow, seed, step, wl)
                           : update_phase_rsghmc<T, TABLE, false, false>(a, theta, V, grad, xi, srow, seed, step, wl);
            }
        } else if (adapt) {
            share = xi ? update_phase<T, KIND, TABLE, true, true>(a, theta, V, grad, tau, g, vh, minv, xi, srow, seed, step, wl)
                       : update_phase<T, KIND, TABLE, true, false>(a, theta, V, grad, tau, g, vh, minv, xi, srow, seed, step, wl);
        } else {
            share = xi ? update_phase<T, KIND, TABLE, false, true>(a, theta, V, grad, tau, g, vh, minv, xi, srow, seed, step, wl)
                       : update_phase<T, KIND, TABLE, false, false>(a, theta, V, grad, tau, g, vh, minv, xi, srow, seed, step, wl);
        }
        __threadfence_block();
        tsq = block_sum(share, red);                      // barriers inside: the new theta is visible to the block
        if constexpr (TRACE) {
            // wl holds theta' (the bits the update stored to the arena) and is not written again before the next update,
            // many barriers away: plain element stores, coalesced over the lanes, no alignment demand on a row (n_params is odd
            // for many nets)
            if (--keep_in == 0) {
                for (size_t i = tid; i < a.n_params; i += nt) trow[i] = wl[i];
                trow += a.n_params;
                keep_in = a.trace_every;
            }
        }
    }
}

template <typename T, int KIND, bool TABLE, bool TRACE>
int launch_fused(const FusedArgs<T> &a, int n_chains, size_t lds_bytes, hipStream_t st)
{
    auto kernel = &bnn_fused_sghmc_kernel<T, KIND | (TABLE ? FUSED_TABLE : 0) | (TRACE ? FUSED_TRACE : 0)>;
    if (lds_bytes > 64 * 1024) {
        hipError_t e0 = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)lds_bytes);
        if (e0 != hipSuccess) return hip_fail(e0, "hipFuncSetAttribute(bnn_fused_sghmc_kernel)");
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_chains), dim3(FUSED_THREADS), lds_bytes, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, "launch bnn_fused_sghmc_kernel");
}

// The 15 arguments every entry point shares, in the headers' order, as F(type, name): ONE list for the struct the entry
// points pack them into, for their parameter lists and for the pack itself.
#define FUSED_NET(F, T)                                                                                                    \
    F(size_t, n_params) F(size_t, chain_stride) F(int, n_chains) F(const int *, layer_sizes) F(int, n_layers)              \
    F(const T *, X) F(const T *, y) F(size_t, n_data) F(const int *, window_starts) F(int, batch) F(double, batch_size)    \
    F(double, n_examples) F(double, wdecay) F(double, prior_mean) F(double, prior_var)
#define FUSED_NET_FIELD(type, name) type name;
#define FUSED_NET_PARAM(type, name) type name,
#define FUSED_NET_ARG(type, name) name,
#define FUSED_NET_PARAMS(T) FUSED_NET(FUSED_NET_PARAM, T)   /* ends with its comma: every entry point has parameters after it */
#define FUSED_NET_PACK(T) FusedNet<T>{FUSED_NET(FUSED_NET_ARG, T)}

template <typename T>
struct FusedNet { FUSED_NET(FUSED_NET_FIELD, T) };

// What the entry points of a KIND take and call themselves. Rows: SGHMC theta, V, grad, tau, g, v_hat, minv; SGLD the same
// without V; relativistic theta, p, grad. Scalars: in the order of sgmcmc_<kind>_scalars_* (SGHMC eps, scale_grad, mdecay;
// SGLD eps, A, scale_grad; relativistic eps, mass, c, D, b_hat). Names: by value, with a required table.
constexpr int FUSED_N_ROWS[3] = {7, 6, 3};
constexpr int FUSED_N_SCALARS[3] = {3, 3, 5};
constexpr const char *FUSED_NAME[3][2] = {{"bnn_fused_sghmc_steps", "bnn_fused_sghmc_sched_steps"},
                                          {"bnn_fused_sgld_steps", "bnn_fused_sgld_sched_steps"},
                                          {"bnn_fused_rsghmc_steps", "bnn_fused_rsghmc_steps"}};

// Where a traced launch keeps its samples (include/sgmcmc_hip_fused_trace.h)
template <typename T>
struct FusedTrace {
    T *trace;
    size_t chain_stride;
    uint64_t capacity, row, every, phase;
};

// The one host path from every entry point to the launch. `by_value`: the scalars the operator's five by-value scalars are
// derived from (sgmcmc_scalars.hpp). `scalars_steps`: DEVICE table [n_steps][5] that replaces those five step by step, or
// NULL; `need_table`: the entry point has no by-value stepsize, so NULL is an error and `by_value` is not read. `trace`: NULL, or
// the thinned device trace of the launch, checked after everything else under the name `what_traced`.
template <typename T, int KIND>
int bnn_fused_entry(T *const (&rows)[FUSED_N_ROWS[KIND]], const FusedNet<T> &n, const T (&by_value)[FUSED_N_SCALARS[KIND]],
                    const T *scalars_steps, bool need_table, uint64_t first_step, uint64_t n_steps, uint64_t burn_in_steps,
                    uint64_t seed_base, const T *xi, T *cost_out, sgmcmc_stream_t stream, const FusedTrace<T> *trace = nullptr,
                    const char *what_traced = nullptr)
{
    const char *what = trace ? what_traced : FUSED_NAME[KIND][need_table];
    if (n_steps == 0 || n.n_chains == 0) return 0;
    bool null_row = false;
    for (T *p : rows) null_row |= !p;
    if (null_row || !n.layer_sizes || !n.X || !n.y || !n.window_starts || !cost_out)
        return fail(SGMCMC_EINVAL, "%s: NULL argument", what);
    if (need_table && !scalars_steps) return fail(SGMCMC_EINVAL, "%s: scalars_steps is NULL", what);
    if (n.n_layers < 1 || n.n_layers > FUSED_MAX_LAYERS) return fail(SGMCMC_EINVAL, "%s: 1..8 layers", what);
    if (n.layer_sizes[n.n_layers] != 1) return fail(SGMCMC_EINVAL, "%s: the last layer must have one unit", what);
    if (n.batch < 1 || (size_t)n.batch > n.n_data) return fail(SGMCMC_EINVAL, "%s: bad batch", what);
    if (xi && (n.n_params % 4) != 0) return fail(SGMCMC_EINVAL, "%s: injected xi needs n_params %% 4 == 0", what);
    if (n.n_chains > 1 && (n.chain_stride < n.n_params || (n.chain_stride % 4) != 0))
        return fail(SGMCMC_EINVAL, "%s: chain_stride must be >= n_params and a multiple of 4", what);
    for (T *p : rows)
        if (reinterpret_cast<uintptr_t>(p) & 15u) return fail(SGMCMC_EINVAL, "%s: rows must be 16-B aligned", what);
    FusedArgs<T> a{};                                     // the rows a KIND does not have stay NULL
    if constexpr (KIND == 0) {
        a.theta = rows[0]; a.V = rows[1]; a.grad = rows[2]; a.tau = rows[3]; a.g = rows[4]; a.vh = rows[5]; a.minv = rows[6];
    } else if constexpr (KIND == 1) {
        a.theta = rows[0]; a.grad = rows[1]; a.tau = rows[2]; a.g = rows[3]; a.vh = rows[4]; a.minv = rows[5];
    } else {
        a.theta = rows[0]; a.V = rows[1]; a.grad = rows[2];
    }
    a.n_params = n.n_params; a.chain_stride = n.chain_stride; a.n_layers = n.n_layers;
    size_t off = 0, lds_elems = 0;
    for (int l = 0; l <= n.n_layers; ++l) {
        if (n.layer_sizes[l] < 1) return fail(SGMCMC_EINVAL, "%s: bad layer size", what);
        a.sizes[l] = n.layer_sizes[l];
    }
    for (int l = 1; l <= n.n_layers; ++l) {                // parameter order: W1, b1, ..., WL, bL, log_var
        a.off_w[l] = off; off += (size_t)a.sizes[l - 1] * a.sizes[l];
        a.off_b[l] = off; off += (size_t)a.sizes[l];
    }
    if (off + 1 != n.n_params) return fail(SGMCMC_EINVAL, "%s: n_params does not match the layer sizes", what);
    for (int l = 0; l <= n.n_layers; ++l) { a.act_off[l] = lds_elems; lds_elems += (size_t)n.batch * a.sizes[l]; }
    a.del_off[0] = 0;
    for (int l = 1; l <= n.n_layers; ++l) { a.del_off[l] = lds_elems; lds_elems += (size_t)n.batch * a.sizes[l]; }
    a.lds_y = lds_elems; lds_elems += (size_t)n.batch;
    lds_elems = (lds_elems + 3) & ~(size_t)3;
    a.lds_w = lds_elems; lds_elems += n.n_params;
    const size_t lds_bytes = 160 + lds_elems * sizeof(T);
    if (lds_bytes > 160 * 1024) return fail(SGMCMC_EINVAL, "%s: activations need %zu B of LDS (> 160 KiB); "
                                            "use the GEMM path", what, lds_bytes);
    a.X = n.X; a.y = n.y; a.n_data = n.n_data; a.starts = n.window_starts; a.batch = n.batch;
    a.batch_size = n.batch_size; a.n_examples = n.n_examples; a.wdecay = n.wdecay;
    a.wp_den = (double)n.n_params + (2.0 * 1e-16 + 1e-16);
    a.lvp_den = 2.0 * n.prior_var + (2.0 * 1e-16 + 1e-16);
    a.ln_prior_mean = std::log(n.prior_mean); a.ln_prior_var = std::log(n.prior_var);
    const T *v = by_value;
    T sc[5] = {T(0), T(0), T(0), T(0), T(0)};
    if constexpr (KIND == 0) {
        if (!need_table) sghmc_scalars<T>(v[0], v[1], v[2], sc);
        a.eps_e2 = sc[0]; a.c1 = sc[1]; a.c3 = sc[2]; a.e4 = sc[3]; a.mdecay = sc[4];
    } else if constexpr (KIND == 1) {
        if (!need_table) sgld_scalars<T>(v[0], v[1], v[2], sc);
        a.sgld_eps = sc[0]; a.sgld_A = sc[1]; a.sgld_a_eff = sc[2]; a.sgld_two_eps = sc[3]; a.sgld_den = sc[4];
    } else {
        rsghmc_scalars<T>(v[0], v[1], v[2], v[3], v[4], sc);
        a.rs_eps = sc[0]; a.rs_mass = sc[1]; a.rs_D = sc[2]; a.rs_m2c2 = sc[3]; a.rs_nscale = sc[4];
        // POW2 as in sgmcmc_rsghmc.hip; not with a table, whose rows carry their own m2c2
        a.rs_pow2 = (rsghmc_m2c2_is_pow2<T>(sc[3], a.rs_inv) && !scalars_steps) ? 1 : 0;
    }
    a.grad_decay = (T)(n.wdecay / (a.wp_den * n.n_examples));   // weight-prior gradient, folded into the update
    a.first_step = first_step; a.n_steps = n_steps; a.burn_in_steps = burn_in_steps; a.seed_base = seed_base;
    a.xi = xi; a.cost_out = cost_out; a.scalars_steps = scalars_steps;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (trace) {
        typedef unsigned __int128 u128;                    // the bounds below must not wrap, whatever the caller passed
        if (!trace->trace) return fail(SGMCMC_EINVAL, "%s: trace is NULL", what);
        if (trace->every == 0) return fail(SGMCMC_EINVAL, "%s: trace_every must be >= 1", what);
        if (trace->phase >= trace->every) return fail(SGMCMC_EINVAL, "%s: trace_phase must be < trace_every", what);
        if ((u128)trace->row + ((u128)trace->phase + n_steps) / trace->every > (u128)trace->capacity)
            return fail(SGMCMC_EINVAL, "%s: the launch keeps more rows than trace_capacity holds from trace_row on", what);
        if (n.n_chains > 1 && (u128)trace->chain_stride < (u128)trace->capacity * n.n_params)
            return fail(SGMCMC_EINVAL, "%s: trace_chain_stride must be >= trace_capacity * n_params", what);
        a.trace = trace->trace; a.trace_chain_stride = trace->chain_stride;
        a.trace_row = trace->row; a.trace_every = trace->every; a.trace_phase = trace->phase;
        return scalars_steps ? launch_fused<T, KIND, true, true>(a, n.n_chains, lds_bytes, st)
                             : launch_fused<T, KIND, false, true>(a, n.n_chains, lds_bytes, st);
    }
    return scalars_steps ? launch_fused<T, KIND, true, false>(a, n.n_chains, lds_bytes, st)
                         : launch_fused<T, KIND, false, false>(a, n.n_chains, lds_bytes, st);
}

// include/sgmcmc_hip_fused_trace.h: the kind, its rows and its by-value scalars arrive as values, so ONE entry per dtype reaches
// the three instantiations of the host path above. A table replaces the by-value stepsize as in the `sched` entries.
template <typename T, int KIND, size_t... R, size_t... S>
int bnn_fused_trace_kind(std::index_sequence<R...>, std::index_sequence<S...>, T *const *rows, const FusedNet<T> &n,
                         const T *scalars, const T *scalars_steps, uint64_t first_step, uint64_t n_steps,
                         uint64_t burn_in_steps, uint64_t seed_base, const T *xi, T *cost_out, const FusedTrace<T> &tr,
                         sgmcmc_stream_t stream)
{
    // SGLD's entry takes eps, scale_grad, A; its operator's derivation eps, A, scale_grad
    constexpr size_t order[3][5] = {{0, 1, 2, 0, 0}, {0, 2, 1, 0, 0}, {0, 1, 2, 3, 4}};
    return bnn_fused_entry<T, KIND>({rows[R]...}, n, {scalars[order[KIND][S]]...}, scalars_steps,
                                    KIND != 2 && scalars_steps != nullptr, first_step, n_steps, KIND == 2 ? 0 : burn_in_steps,
                                    seed_base, xi, cost_out, stream, &tr, "bnn_fused_trace_steps");
}

template <typename T>
int bnn_fused_trace_entry(int kind, T *const *rows, int n_rows, const FusedNet<T> &n, const T *scalars, int n_scalars,
                          const T *scalars_steps, uint64_t first_step, uint64_t n_steps, uint64_t burn_in_steps,
                          uint64_t seed_base, const T *xi, T *cost_out, const FusedTrace<T> &tr, sgmcmc_stream_t stream)
{
    const char *what = "bnn_fused_trace_steps";
    if (n_steps == 0 || n.n_chains == 0) return 0;
    if (kind < 0 || kind > 2) return fail(SGMCMC_EINVAL, "%s: kind must be 0 (SGHMC), 1 (SGLD) or 2 (relativistic), not %d", what, kind);
    if (n_rows != FUSED_N_ROWS[kind]) return fail(SGMCMC_EINVAL, "%s: kind %d has %d rows, not %d", what, kind, FUSED_N_ROWS[kind], n_rows);
    if (n_scalars != FUSED_N_SCALARS[kind])
        return fail(SGMCMC_EINVAL, "%s: kind %d has %d scalars, not %d", what, kind, FUSED_N_SCALARS[kind], n_scalars);
    if (!rows || !scalars) return fail(SGMCMC_EINVAL, "%s: NULL argument", what);
#define TRACE_KIND(K)                                                                                                      \
    bnn_fused_trace_kind<T, K>(std::make_index_sequence<FUSED_N_ROWS[K]>{}, std::make_index_sequence<FUSED_N_SCALARS[K]>{},  \
                               rows, n, scalars, scalars_steps, first_step, n_steps, burn_in_steps, seed_base, xi, cost_out, \
                               tr, stream)
    return kind == 0 ? TRACE_KIND(0) : kind == 1 ? TRACE_KIND(1) : TRACE_KIND(2);
#undef TRACE_KIND
}

// HOST table [n_steps][5] of an operator's scalars for the stepsizes eps[0 .. n_steps): `derive(eps, row)` is the shared derivation
template <typename T, typename F>
int scalars_steps_fill(const char *what, const T *eps, size_t n_steps, T *block, F derive)
{
    if (n_steps == 0) return 0;
    if (!eps || !block) return fail(SGMCMC_EINVAL, "%s: eps_host and block_host must be non-NULL", what);
    for (size_t t = 0; t < n_steps; ++t) {
        T s[5];
        derive(eps[t], s);
        for (int k = 0; k < 5; ++k) block[5 * t + k] = s[k];
    }
    return 0;
}

}  // namespace

// Each entry point packs its arguments and names its kind. The f32 and f64 twins of a signature are stamped from one text,
// the ENTRY(SFX, T) defined just above each FUSED_TWINS.
#define FUSED_TWINS ENTRY(f32, float) ENTRY(f64, double)

extern "C" {

// ---- include/sgmcmc_hip.h, [whole-step]: one by-value stepsize per launch

#define ENTRY(SFX, T)                                                                                                      \
    int sgmcmc_bnn_fused_sghmc_steps_##SFX(T *theta, T *V, T *grad, T *tau, T *g, T *v_hat, T *minv, FUSED_NET_PARAMS(T)   \
                                           T eps, T scale_grad, T mdecay, uint64_t first_step, uint64_t n_steps,           \
                                           uint64_t burn_in_steps, uint64_t seed_base, const T *xi, T *cost_out,           \
                                           sgmcmc_stream_t stream)                                                         \
    {                                                                                                                      \
        return bnn_fused_entry<T, 0>({theta, V, grad, tau, g, v_hat, minv}, FUSED_NET_PACK(T), {eps, scale_grad, mdecay},  \
                                     nullptr, false, first_step, n_steps, burn_in_steps, seed_base, xi, cost_out, stream); \
    }
FUSED_TWINS
#undef ENTRY

#define ENTRY(SFX, T)                                                                                                      \
    int sgmcmc_bnn_fused_sgld_steps_##SFX(T *theta, T *grad, T *tau, T *g, T *v_hat, T *minv, FUSED_NET_PARAMS(T) T eps,   \
                                          T scale_grad, T A, uint64_t first_step, uint64_t n_steps,                        \
                                          uint64_t burn_in_steps, uint64_t seed_base, const T *xi, T *cost_out,            \
                                          sgmcmc_stream_t stream)                                                          \
    {                                                                                                                      \
        return bnn_fused_entry<T, 1>({theta, grad, tau, g, v_hat, minv}, FUSED_NET_PACK(T), {eps, A, scale_grad}, nullptr, \
                                     false, first_step, n_steps, burn_in_steps, seed_base, xi, cost_out, stream);          \
    }
FUSED_TWINS
#undef ENTRY

// ---- include/sgmcmc_hip_fused.h

int sgmcmc_fused_abi_version(void) { return SGMCMC_FUSED_ABI_VERSION; }

int sgmcmc_sghmc_scalars_steps_f32(const float *eps_host, size_t n_steps, float scale_grad, float mdecay, float *block_host)
{
    return scalars_steps_fill<float>("sghmc_scalars_steps", eps_host, n_steps, block_host,
                                     [=](float e, float (&s)[5]) { sghmc_scalars<float>(e, scale_grad, mdecay, s); });
}
int sgmcmc_sghmc_scalars_steps_f64(const double *eps_host, size_t n_steps, double scale_grad, double mdecay, double *block_host)
{
    return scalars_steps_fill<double>("sghmc_scalars_steps", eps_host, n_steps, block_host,
                                      [=](double e, double (&s)[5]) { sghmc_scalars<double>(e, scale_grad, mdecay, s); });
}
int sgmcmc_sgld_scalars_steps_f32(const float *eps_host, size_t n_steps, float A, float scale_grad, float *block_host)
{
    return scalars_steps_fill<float>("sgld_scalars_steps", eps_host, n_steps, block_host,
                                     [=](float e, float (&s)[5]) { sgld_scalars<float>(e, A, scale_grad, s); });
}
int sgmcmc_sgld_scalars_steps_f64(const double *eps_host, size_t n_steps, double A, double scale_grad, double *block_host)
{
    return scalars_steps_fill<double>("sgld_scalars_steps", eps_host, n_steps, block_host,
                                      [=](double e, double (&s)[5]) { sgld_scalars<double>(e, A, scale_grad, s); });
}
int sgmcmc_rsghmc_scalars_steps_f32(const float *eps_host, size_t n_steps, float mass, float c, float D, float b_hat,
                                    float *block_host)
{
    return scalars_steps_fill<float>("rsghmc_scalars_steps", eps_host, n_steps, block_host,
                                     [=](float e, float (&s)[5]) { rsghmc_scalars<float>(e, mass, c, D, b_hat, s); });
}
int sgmcmc_rsghmc_scalars_steps_f64(const double *eps_host, size_t n_steps, double mass, double c, double D, double b_hat,
                                    double *block_host)
{
    return scalars_steps_fill<double>("rsghmc_scalars_steps", eps_host, n_steps, block_host,
                                      [=](double e, double (&s)[5]) { rsghmc_scalars<double>(e, mass, c, D, b_hat, s); });
}

// `scale_grad` and `mdecay` / `A` keep their places and are not read: the table's rows carry what is derived from them
#define ENTRY(SFX, T)                                                                                                      \
    int sgmcmc_bnn_fused_sghmc_sched_steps_##SFX(T *theta, T *V, T *grad, T *tau, T *g, T *v_hat, T *minv,                 \
                                                 FUSED_NET_PARAMS(T) const T *scalars_steps, T scale_grad, T mdecay,       \
                                                 uint64_t first_step, uint64_t n_steps, uint64_t burn_in_steps,            \
                                                 uint64_t seed_base, const T *xi, T *cost_out, sgmcmc_stream_t stream)     \
    {                                                                                                                      \
        return bnn_fused_entry<T, 0>({theta, V, grad, tau, g, v_hat, minv}, FUSED_NET_PACK(T), {T(0), scale_grad, mdecay}, \
                                     scalars_steps, true, first_step, n_steps, burn_in_steps, seed_base, xi, cost_out,     \
                                     stream);                                                                              \
    }
FUSED_TWINS
#undef ENTRY

#define ENTRY(SFX, T)                                                                                                      \
    int sgmcmc_bnn_fused_sgld_sched_steps_##SFX(T *theta, T *grad, T *tau, T *g, T *v_hat, T *minv, FUSED_NET_PARAMS(T)    \
                                                const T *scalars_steps, T scale_grad, T A, uint64_t first_step,            \
                                                uint64_t n_steps, uint64_t burn_in_steps, uint64_t seed_base,              \
                                                const T *xi, T *cost_out, sgmcmc_stream_t stream)                          \
    {                                                                                                                      \
        return bnn_fused_entry<T, 1>({theta, grad, tau, g, v_hat, minv}, FUSED_NET_PACK(T), {T(0), A, scale_grad},         \
                                     scalars_steps, true, first_step, n_steps, burn_in_steps, seed_base, xi, cost_out,     \
                                     stream);                                                                              \
    }
FUSED_TWINS
#undef ENTRY

#define ENTRY(SFX, T)                                                                                                      \
    int sgmcmc_bnn_fused_rsghmc_steps_##SFX(T *theta, T *p, T *grad, FUSED_NET_PARAMS(T) T eps, T mass, T c, T D, T b_hat, \
                                            const T *scalars_steps, uint64_t first_step, uint64_t n_steps,                 \
                                            uint64_t seed_base, const T *xi, T *cost_out, sgmcmc_stream_t stream)          \
    {                                                                                                                      \
        return bnn_fused_entry<T, 2>({theta, p, grad}, FUSED_NET_PACK(T), {eps, mass, c, D, b_hat}, scalars_steps, false,  \
                                     first_step, n_steps, 0, seed_base, xi, cost_out, stream);                             \
    }
FUSED_TWINS
#undef ENTRY

// ---- include/sgmcmc_hip_fused_trace.h

int sgmcmc_fused_trace_abi_version(void) { return SGMCMC_FUSED_TRACE_ABI_VERSION; }

#define ENTRY(SFX, T)                                                                                                      \
    int sgmcmc_bnn_fused_trace_steps_##SFX(int kind, T *const *rows, int n_rows, FUSED_NET_PARAMS(T) const T *scalars,     \
                                           int n_scalars, const T *scalars_steps, uint64_t first_step, uint64_t n_steps,   \
                                           uint64_t burn_in_steps, uint64_t seed_base, const T *xi, T *cost_out, T *trace, \
                                           size_t trace_chain_stride, uint64_t trace_capacity, uint64_t trace_row,         \
                                           uint64_t trace_every, uint64_t trace_phase, sgmcmc_stream_t stream)             \
    {                                                                                                                      \
        return bnn_fused_trace_entry<T>(kind, rows, n_rows, FUSED_NET_PACK(T), scalars, n_scalars, scalars_steps,          \
                                        first_step, n_steps, burn_in_steps, seed_base, xi, cost_out,                       \
                                        FusedTrace<T>{trace, trace_chain_stride, trace_capacity, trace_row, trace_every,   \
                                                      trace_phase}, stream);                                               \
    }
FUSED_TWINS
#undef ENTRY

}  // extern "C"
