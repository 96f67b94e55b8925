// sgmcmc_bnn_cost.hip -- the small kernels of the BNN cost path (pysgmcmc/models/bayesian_neural_network.py:365-388) and
// their C entries ([bnn cost] group of include/sgmcmc_hip.h): the loss head, alone (bnn_head) and folded into the backward
// of the single-output last layer (head_last_layer_backward); that backward on its own (last_layer_backward); the tanh
// backward with and without the bias gradient of the layer below (tanh_backward_colsum, tanh_backward); bias + tanh of a
// hidden layer (bias_tanh) and of the last hidden layer fused with the output unit's dot product (tanh_rowdot).
// With them a whole BNN step is ~26 launches instead of ~90 tiny framework ops. Single-block / plain elementwise /
// 16-column blocks: launch-bound by design. The hidden layers' products are sgmcmc_bnn_gemm.hip and sgmcmc_bnn_gw.hip.
//
// One IEEE rounding per operation (fp contract off); every reduction has a fixed association (wave shuffles, then the
// waves through LDS in wave order): no atomics, the same bits on every launch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sgmcmc_hip.h"

#pragma clang fp contract(off)

#include "sgmcmc_host.hpp"
#include "sgmcmc_stats_ws.hpp"

using namespace sgmcmc_host;

namespace {

// --------------------------------------------------------------------------
// the loss head
// --------------------------------------------------------------------------

struct BnnHeadConsts {
    double batch_size, n_examples, wp_den, lvp_den, ln_prior_mean, ln_prior_var, wdecay;
    int fold_prior_grad;     // 1: the update kernel adds the weight-prior gradient (grad_decay), omit it here
    int add_last_bias;       // 1: mean[] lacks the last layer's bias; add *last_bias
};

// flags: bit 0 = fold_prior_grad, bit 1 = add_last_bias
BnnHeadConsts head_consts(double batch_size, double n_examples, double n_params, double wdecay, double prior_mean,
                          double prior_var, int flags)
{
    BnnHeadConsts k;
    k.batch_size = batch_size; k.n_examples = n_examples; k.wdecay = wdecay;
    k.wp_den = n_params + (2.0 * 1e-16 + 1e-16);                 /* safe_divide, n_params > 0 */
    k.lvp_den = 2.0 * prior_var + (2.0 * 1e-16 + 1e-16);
    k.ln_prior_mean = std::log(prior_mean); k.ln_prior_var = std::log(prior_var);
    k.fold_prior_grad = (flags & 1) ? 1 : 0;
    k.add_last_bias = (flags & 2) ? 1 : 0;
    return k;
}

// The head's scalar arithmetic, in double whatever T is. Every lane holds what a residual and its d cost / d mean need
// (the constructor); ONE thread computes the scalar outputs, in two parts so that a kernel can run what does not depend on
// the residuals (prior) in front of its barriers and the rest (write) behind them.
struct LossHead {
    double s, bias_add, es, inv, dscale;
    double d = 0.0, lvp = 0.0, prior_coef = 0.0;                 // prior()

    // s_ptr: the scalar log-variance parameter (output_bias). add_last_bias: `mean` holds h W (no bias yet); the
    // single-output layer's bias is added to every mean
    template <typename T>
    __device__ __forceinline__ LossHead(const T *s_ptr, const T *last_bias, const BnnHeadConsts &k)
    {
        s = (double)*s_ptr;
        bias_add = (k.add_last_bias && last_bias != nullptr) ? (double)*last_bias : 0.0;
        es = exp(s);
        inv = 1.0 / (es + 1e-16);                                // :369
        dscale = -(inv / k.batch_size);
    }
    template <typename T>
    __device__ __forceinline__ double residual(T y, T mean) const { return (double)y - ((double)mean + bias_add); }
    template <typename T>
    __device__ __forceinline__ T dmean(double r) const { return (T)(r * dscale); }      // d cost / d mean_i

    __device__ __forceinline__ void prior(const BnnHeadConsts &k)
    {
        d = s - k.ln_prior_mean;
        lvp = -(d * d) / k.lvp_den - 0.5 * k.ln_prior_var;                                  // :102-107
        prior_coef = k.fold_prior_grad ? 0.0 : k.wdecay / (k.wp_den * k.n_examples);
    }
    // sse, sumr: sum of the B squared residuals and of the residuals; tsq: sum over ALL parameters of theta^2. Writes the
    // cost, d cost/d log_var (into the gradient arena slot of output_bias), mse and, if asked for, the last bias's gradient
    template <typename T>
    __device__ __forceinline__ void write(const BnnHeadConsts &k, double sse, double sumr, double tsq, size_t B,
                                          const T *last_bias, T *cost_out, T *grad_s_out, T *grad_bias_out,
                                          T *mse_out) const
    {
        const double Bd = (double)B;
        double log_like = (-(sse * (0.5 * inv)) - 0.5 * s * Bd) / k.batch_size;            // :371-377
        double wp = (-0.5 * k.wdecay) * tsq / k.wp_den;                                     // :131-141
        double cost = -(log_like + lvp / k.n_examples + wp / k.n_examples);                 // :380-388
        double ds = -((sse * (0.5 * es * inv * inv) - 0.5 * Bd) / k.batch_size
                      + (-2.0 * d / k.lvp_den) / k.n_examples) + prior_coef * s;
        *cost_out = (T)cost;
        *grad_s_out = (T)ds;
        *mse_out = (T)(sse / Bd);
        // bias gradient of the single-output last layer: sum_i delta_i (+ prior term unless folded)
        if (grad_bias_out != nullptr) *grad_bias_out = (T)(sumr * dscale + prior_coef * (double)*last_bias);
    }
};

// This lane's share of the B residuals: sse += sum r_i^2, sumr += sum r_i (DELTA: delta[i] = d cost / d mean_i on the way).
template <bool DELTA, typename T>
__device__ __forceinline__ void head_residuals(const LossHead &hd, const T *mean, const T *__restrict__ y, size_t B,
                                               T *__restrict__ delta, double &sse, double &sumr)
{
    for (size_t i = threadIdx.x; i < B; i += blockDim.x) {
        double r = hd.residual(y[i], mean[i]);
        sse += r * r;                                            // :370
        sumr += r;
        if (DELTA) delta[i] = hd.dmean<T>(r);
    }
}
// The head's block-wide sums of N doubles per lane, in a fixed order: put takes them through the wave's shuffles into one
// LDS slot per wave; after the caller's barrier, get adds the slots of the block's waves in wave order.
template <int N>
__device__ __forceinline__ void head_sums_put(double (&v)[N], double (*lds)[16])
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] += __shfl_down(v[j], off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) lds[j][threadIdx.x >> 6] = v[j];
    }
}
template <int N>
__device__ __forceinline__ void head_sums_get(double (*lds)[16], int n_waves, double (&tot)[N])
{
    for (int w = 0; w < n_waves; ++w) {
#pragma unroll
        for (int j = 0; j < N; ++j) tot[j] += lds[j][w];
    }
}

// mean[B], y[B]: network mean output and targets; theta_sumsq: sum(theta^2) as a double on the device, or (stats_ws) the
// statistics workspace of the previous step kernel. Writes delta[B] = d cost/d mean and the head's scalar outputs.
template <typename T>
__global__ void __launch_bounds__(1024) bnn_head_kernel(const T *__restrict__ mean, const T *__restrict__ y,
                                                       const T *__restrict__ s_ptr, const double *__restrict__ theta_sumsq,
                                                       const double *__restrict__ stats_ws, const T *__restrict__ last_bias,
                                                       size_t B, BnnHeadConsts k, T *__restrict__ delta,
                                                       T *__restrict__ cost_out, T *__restrict__ grad_s_out,
                                                       T *__restrict__ grad_bias_out, T *__restrict__ mse_out)
{
    __shared__ double lds[3][16];
    LossHead hd(s_ptr, last_bias, k);
    double v[3] = {0.0, 0.0, 0.0};                               // sse, sumr, this lane's share of sum(theta^2)
    head_residuals<true>(hd, mean, y, B, delta, v[0], v[1]);
    // sum(theta^2) from the workspace: statistic 0 of its records, summed here in a fixed order -- saves the separate K7
    // launch on the step's critical path
    if (stats_ws != nullptr) {
        const unsigned nparts = stats_ws_records(stats_ws);
        unsigned i = threadIdx.x;
        const unsigned bd = blockDim.x;
        for (; i + 3u * bd < nparts; i += 4u * bd) {           // 4 loads in flight, fixed add order
            double x0 = stats_ws_stat(stats_ws, i), x1 = stats_ws_stat(stats_ws, i + bd);
            double x2 = stats_ws_stat(stats_ws, i + 2u * bd), x3 = stats_ws_stat(stats_ws, i + 3u * bd);
            v[2] += x0; v[2] += x1; v[2] += x2; v[2] += x3;
        }
        for (; i < nparts; i += bd) v[2] += stats_ws_stat(stats_ws, i);
    }
    head_sums_put(v, lds);
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot[3] = {0.0, 0.0, 0.0};
        head_sums_get(lds, (int)(blockDim.x >> 6), tot);
        if (stats_ws == nullptr) tot[2] = *theta_sumsq;
        hd.prior(k);
        hd.write(k, tot[0], tot[1], tot[2], B, last_bias, cost_out, grad_s_out, grad_bias_out, mse_out);
    }
}

// --------------------------------------------------------------------------
// the 16-column block of the backward kernels
// --------------------------------------------------------------------------

// One block of 1024 lanes owns CS_COLS = 16 columns (64-byte row segments) of a row-major [rows][cols] matrix: lane & 15 =
// column, the other 64 "row lanes" (4 per wave x 16 waves) stride over the rows, so a 256 x 2048 matrix is 128 blocks (one per
// two CUs) instead of the 32 a 64-column block gives, and every lane has its 4 rows' loads in flight at once.
constexpr int CS_COLS = 16;

struct ColLane {
    int lane, wave;
    size_t c, rl;            // this lane's column (may lie past the matrix) and its row lane 0 .. 63
};
__device__ __forceinline__ ColLane col_lane()
{
    ColLane L;
    L.lane = threadIdx.x & 63; L.wave = threadIdx.x >> 6;
    L.c = (size_t)blockIdx.x * CS_COLS + (L.lane & (CS_COLS - 1));
    L.rl = (size_t)L.wave * 4 + (L.lane >> 4);
    return L;
}

// Column sums of N accumulators per lane: put combines the 4 row lanes of a wave by two shuffles and leaves one LDS slot per
// wave and column; after the caller's barrier, write adds the 16 waves in wave order (deterministic, no atomics) and stores
// out[j][c] = total_j (+ beta * add[j][c]).
template <typename T, int N>
__device__ __forceinline__ void col_sums_put(const ColLane &L, T (&acc)[N], T (*lds)[16][CS_COLS])
{
#pragma unroll
    for (int j = 0; j < N; ++j) { acc[j] += __shfl_xor(acc[j], 16, 64); acc[j] += __shfl_xor(acc[j], 32, 64); }
    if (L.lane < CS_COLS) {
#pragma unroll
        for (int j = 0; j < N; ++j) lds[j][L.wave][L.lane] = acc[j];
    }
}
template <typename T, int N>
__device__ __forceinline__ void col_sums_write(const ColLane &L, size_t c, size_t cols, T (*lds)[16][CS_COLS], T beta,
                                               const T *const (&add)[N], T *const (&out)[N])
{
    if (L.wave == 0 && L.lane < CS_COLS && c < cols) {
        T tot[N];
#pragma unroll
        for (int j = 0; j < N; ++j) tot[j] = T(0);
#pragma unroll
        for (int w = 0; w < 16; ++w) {
#pragma unroll
            for (int j = 0; j < N; ++j) tot[j] += lds[j][w][L.lane];
        }
#pragma unroll
        for (int j = 0; j < N; ++j) out[j][c] = (beta != T(0)) ? tot[j] + beta * add[j][c] : tot[j];
    }
}

// Rank-1 back-propagation through the single-output last layer and the tanh below it, one element:
// delta_prev = (dvec[r] w[c]) (1 - h[r][c]^2), which also enters the bias gradient; h dvec[r] enters the weight gradient.
template <typename T>
__device__ __forceinline__ void rank1_element(T dr, T wc, T hv, T &delta_prev, T (&acc)[2])
{
    const T d = (dr * wc) * (T(1) - hv * hv);
    delta_prev = d;
    acc[0] += d;
    acc[1] += hv * dr;
}
// ... and one lane's rows r, r + 64, ... of column c: four rows per trip (their loads in flight together), then the tail.
// dvec(r) = d cost / d mean_r.
template <typename T, typename D>
__device__ __forceinline__ void rank1_rows(size_t r, size_t rows, size_t cols, size_t c, T wc, const T *__restrict__ h,
                                           T *__restrict__ delta_prev, D dvec, T (&acc)[2])
{
    for (; r + 192 < rows; r += 256) {
        T hv[4], dr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { hv[u] = h[(r + 64 * u) * cols + c]; dr[u] = dvec(r + 64 * u); }
#pragma unroll
        for (int u = 0; u < 4; ++u) rank1_element(dr[u], wc, hv[u], delta_prev[(r + 64 * u) * cols + c], acc);
    }
    for (; r < rows; r += 64) {
        const size_t i = r * cols + c;
        const T hv = h[i], dr = dvec(r);
        rank1_element(dr, wc, hv, delta_prev[i], acc);
    }
}

// delta *= (1 - h^2), the tanh backward (h = tanh(a) kept from the forward pass)
template <typename T>
__global__ void __launch_bounds__(256) tanh_backward_kernel(T *__restrict__ delta, const T *__restrict__ h, size_t n)
{
    const size_t G = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += G) {
        T hv = h[i];
        delta[i] = delta[i] * (T(1) - hv * hv);
    }
}

// Fused tanh backward + bias gradient of the layer below: delta[r][c] *= 1 - h[r][c]^2 and
// colsum[c] = sum_r delta[r][c] (+ beta * bias[c]). Row-major [rows][cols].
template <typename T>
__global__ void __launch_bounds__(1024) tanh_backward_colsum_kernel(T *__restrict__ delta, const T *__restrict__ h,
                                                                     size_t rows, size_t cols, const T *__restrict__ bias,
                                                                     T beta, T *__restrict__ colsum)
{
    __shared__ T lds[1][16][CS_COLS];
    const ColLane L = col_lane();
    const size_t c = L.c;
    T acc[1] = {T(0)};
    if (c < cols) {
        size_t r = L.rl;
        for (; r + 192 < rows; r += 256) {                    // 4 rows per trip: 8 loads in flight per lane
            T hv[4], dv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const size_t i = (r + 64 * u) * cols + c; hv[u] = h[i]; dv[u] = delta[i]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                T d = dv[u] * (T(1) - hv[u] * hv[u]);
                delta[(r + 64 * u) * cols + c] = d;
                acc[0] += d;
            }
        }
        for (; r < rows; r += 64) {
            const size_t i = r * cols + c;
            T hv = h[i];
            T d = delta[i] * (T(1) - hv * hv);
            delta[i] = d;
            acc[0] += d;
        }
    }
    col_sums_put(L, acc, lds);
    __syncthreads();
    col_sums_write<T, 1>(L, c, cols, lds, beta, {bias}, {colsum});
}

// Backward of a single-output last layer fused with the tanh backward of the layer below:
//   delta_prev[r][c] = dvec[r] * w[c] * (1 - h[r][c]^2)     (rank-1 back-propagation + tanh')
//   colsum[c]        = sum_r delta_prev[r][c] (+ beta * bias_prev[c])   bias gradient of the layer below
//   gw[c]            = sum_r h[r][c] * dvec[r] (+ beta * w[c])          weight gradient of the last layer
template <typename T>
__global__ void __launch_bounds__(1024) last_layer_backward_kernel(const T *__restrict__ dvec, const T *__restrict__ w,
                                                                    const T *__restrict__ h, size_t rows, size_t cols,
                                                                    const T *__restrict__ bias_prev, T beta,
                                                                    T *__restrict__ delta_prev, T *__restrict__ colsum,
                                                                    T *__restrict__ gw)
{
    __shared__ T lds[2][16][CS_COLS];
    const ColLane L = col_lane();
    const size_t c = L.c;
    T acc[2] = {T(0), T(0)};
    if (c < cols) rank1_rows(L.rl, rows, cols, c, w[c], h, delta_prev, [&](size_t r) -> T { return dvec[r]; }, acc);
    col_sums_put(L, acc, lds);
    __syncthreads();
    col_sums_write<T, 2>(L, c, cols, lds, beta, {bias_prev, w}, {colsum, gw});
}

// The loss head (bnn_head_kernel) folded into the backward of a single-output last layer: dvec[r] = d cost / d mean_r is a
// function of the residual and the scalar log-variance only, so every workgroup forms it on the fly; one extra
// workgroup (the last of the grid, no columns of its own) reduces the residuals and writes the head's scalar outputs (cost,
// d cost/d log_var, mse, last bias gradient).
// sum(theta^2) arrives as the n_tsq slices tanh_rowdot_kernel left in tsq_parts. One launch less per step.
constexpr int HEAD_MAX_PART_ROWS = 1024;                     // batch rows when the mean arrives as partial dot products
template <typename T>
__global__ void __launch_bounds__(1024) head_last_layer_backward_kernel(
    const T *__restrict__ mean_parts, int n_mean_parts, const T *__restrict__ y, const T *__restrict__ s_ptr, const double *__restrict__ tsq_parts,
    int n_tsq, const T *__restrict__ last_bias, BnnHeadConsts k, T *__restrict__ cost_out, T *__restrict__ grad_s_out,
    T *__restrict__ grad_bias_out, T *__restrict__ mse_out, const T *__restrict__ w, const T *__restrict__ h, size_t rows,
    size_t cols, const T *__restrict__ bias_prev, T beta, T *__restrict__ delta_prev, T *__restrict__ colsum,
    T *__restrict__ gw)
{
    __shared__ T lds[2][16][CS_COLS];
    __shared__ double lds_h[2][16];
    __shared__ T mean_lds[HEAD_MAX_PART_ROWS];
    const ColLane L = col_lane();
    // The LAST workgroup of the grid owns no columns: it does the head's own reductions and the scalar outputs (one thread's
    // ~1.5 us of dependent double-precision divisions at the end) next to the column workgroups instead of at the tail of one
    // of them (measured at 256 x 2048, round 4).
    const bool head_wg = blockIdx.x == gridDim.x - 1;
    const size_t c = head_wg ? cols : L.c;
    const size_t rl = L.rl;
    // Everything this lane will want from memory is requested FIRST -- its partial dot products, the activations and targets of
    // its first four rows, the scalars -- and the double-precision scalar chain (exp, reciprocal: ~1 us of dependent
    // instructions that used to start after the barrier) runs while those loads fly.
    // -- the output unit's pre-bias mean: a plain vector, or n_mean_parts partial dot products per row (what
    // sgmcmc_bnn_dense_tanh_f32 leaves: one per 64-column tile), added here in a fixed order by every workgroup: four adjacent
    // lanes per row, each adds a contiguous quarter of the parts (its loads issued together, not one dependent round trip per
    // part), then the quarters are added in lane order
    constexpr int PRE = 8;                                       // parts per lane requested ahead (32 parts: all of them)
    const int per = (n_mean_parts + 3) / 4;
    const size_t pr = threadIdx.x >> 2;                          // first trip: row and quarter of this lane
    const int pq = (int)(threadIdx.x & 3), plo = pq * per, phi = (plo + per < n_mean_parts) ? plo + per : n_mean_parts;
    const bool pre_parts = n_mean_parts > 1 && threadIdx.x < 4 * rows && per <= PRE;
    T pv[PRE];
    if (pre_parts) {
#pragma unroll
        for (int u = 0; u < PRE; ++u) pv[u] = (plo + u < phi) ? mean_parts[(size_t)(plo + u) * rows + pr] : T(0);
    }
    const bool pre_rows = c < cols && rl + 192 < rows;           // the first trip of the main loop
    T hv0[4], yv0[4];
    if (pre_rows) {
#pragma unroll
        for (int u = 0; u < 4; ++u) { hv0[u] = h[(rl + 64 * u) * cols + c]; yv0[u] = y[rl + 64 * u]; }
    }
    const T wc = (c < cols) ? w[c] : T(0);
    LossHead hd(s_ptr, last_bias, k);
    // (head workgroup, thread 0) whatever of the scalar outputs does not depend on the residuals: before the barriers, not after
    double tq = 0.0;
    if (head_wg && threadIdx.x == 0) {
        for (int j = 0; j < n_tsq; ++j) tq += tsq_parts[j];
        hd.prior(k);
    }
    const T *__restrict__ mean = mean_parts;
    if (n_mean_parts > 1) {
        for (size_t i = threadIdx.x; i < 4 * rows; i += blockDim.x) {   // rows <= 1024: whole waves enter each trip
            const size_t r = i >> 2;
            const int q = (int)(i & 3), lo = q * per, hi = (lo + per < n_mean_parts) ? lo + per : n_mean_parts;
            T m = T(0);
            int p = lo;
            if (pre_parts && i == threadIdx.x) {
                // the same left-to-right sum as the loop below
#pragma unroll
                for (int u = 0; u < PRE; ++u)
                    if (lo + u < hi) m += pv[u];
            } else {
                for (; p + 4 <= hi; p += 4) {
                    const T v0 = mean_parts[(size_t)p * rows + r], v1 = mean_parts[(size_t)(p + 1) * rows + r];
                    const T v2 = mean_parts[(size_t)(p + 2) * rows + r], v3 = mean_parts[(size_t)(p + 3) * rows + r];
                    m = (((m + v0) + v1) + v2) + v3;
                }
                for (; p < hi; ++p) m += mean_parts[(size_t)p * rows + r];
            }
            const T m1 = __shfl_down(m, 1, 64), m2 = __shfl_down(m, 2, 64), m3 = __shfl_down(m, 3, 64);
            if (q == 0) mean_lds[r] = ((m + m1) + m2) + m3;
        }
        __syncthreads();
        mean = mean_lds;
    }
    auto dvec_y = [&](T yr, size_t r) -> T { return hd.dmean<T>(hd.residual(yr, mean[r])); };
    T acc[2] = {T(0), T(0)};
    if (c < cols) {
        size_t r = rl;
        if (pre_rows) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                rank1_element(dvec_y(yv0[u], r + 64 * u), wc, hv0[u], delta_prev[(r + 64 * u) * cols + c], acc);
            r += 256;
        }
        rank1_rows(r, rows, cols, c, wc, h, delta_prev, [&](size_t rr) -> T { return dvec_y(y[rr], rr); }, acc);
    }
    col_sums_put(L, acc, lds);
    if (head_wg) {
        double v[2] = {0.0, 0.0};
        head_residuals<false>(hd, mean, y, rows, (T *)nullptr, v[0], v[1]);
        head_sums_put(v, lds_h);
    }
    __syncthreads();
    col_sums_write<T, 2>(L, c, cols, lds, beta, {bias_prev, w}, {colsum, gw});
    if (head_wg && threadIdx.x == 0) {
        double tot[2] = {0.0, 0.0};
        head_sums_get(lds_h, 16, tot);
        hd.write(k, tot[0], tot[1], tq, rows, last_bias, cost_out, grad_s_out, grad_bias_out, mse_out);
    }
}

// --------------------------------------------------------------------------
// bias + tanh, forward
// --------------------------------------------------------------------------

__device__ __forceinline__ float tanh_dev(float x) { return tanhf(x); }
__device__ __forceinline__ double tanh_dev(double x) { return tanh(x); }

// a[r][c] = tanh(a[r][c] + bias[c]) in place: the hidden layers' activation with the bias add that the forward GEMM then
// does not need as an epilogue (the library's plain product is 1.4-2.1 us faster than its bias-epilogue one at batch 256,
// round 3). One quad per lane per trip, 16-byte accesses when the pitch allows.
template <typename T>
__global__ void __launch_bounds__(256) bias_tanh_kernel(T *__restrict__ a, const T *__restrict__ bias, unsigned rows, unsigned cols)
{
    // 32-bit indices (the host checks rows * cols <= 2^32 - 2^24, so i + G cannot wrap): a 64-bit modulo per quad would cost
    // more than the tanh
    const unsigned G = gridDim.x * blockDim.x, gid = blockIdx.x * blockDim.x + threadIdx.x;
    const bool vec = (cols % 4 == 0) && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(bias)) % (4 * sizeof(T)) == 0);
    if (vec) {
        struct alignas(4 * sizeof(T)) Q { T v[4]; };
        Q *aq = reinterpret_cast<Q *>(a);
        const Q *bq = reinterpret_cast<const Q *>(bias);
        const unsigned qpr = cols / 4, nq = rows * qpr;
        for (unsigned q = gid; q < nq; q += G) {
            Q x = aq[q];
            const Q b = bq[q % qpr];
#pragma unroll
            for (int j = 0; j < 4; ++j) x.v[j] = tanh_dev(x.v[j] + b.v[j]);
            aq[q] = x;
        }
    } else {
        const unsigned n = rows * cols;
        for (unsigned i = gid; i < n; i += G) a[i] = tanh_dev(a[i] + bias[i % cols]);
    }
}

// Forward of the last hidden layer fused with the single-output layer above it:
//   h[r][c] = tanh(a[r][c] (+ bias[c])) in place,  out[r] = sum_c h[r][c] * w[c]   (the output unit's pre-bias mean)
// one 256-lane workgroup per row, fixed summation tree (deterministic). Replaces a tanh launch and a GEMV launch.
// 4 consecutive elements per lane per trip (16-byte accesses when the row pitch allows; all loads of a lane issued
// before the first tanh).
// Optional side job (stats_ws != NULL): workgroups 0 .. min(TSQ_SLICES, rows) - 1 also add up one contiguous slice each of
// the sum(theta^2) partials the previous step kernel left in its statistics workspace and write it to tsq_parts[slice];
// the fused head (head_last_layer_backward_kernel) adds the slices in order. Saves the loss head's own pass over the
// ~10 k partials, and with it the separate head launch (each dependent launch of the step costs ~5 us).
template <typename T>
__global__ void __launch_bounds__(256) tanh_rowdot_kernel(T *__restrict__ a, const T *__restrict__ w, size_t cols,
                                                          T *__restrict__ out, const double *__restrict__ stats_ws,
                                                          double *__restrict__ tsq_parts, const T *__restrict__ bias)
{
    __shared__ T lds[4];
    __shared__ double lds_d[4];
    const unsigned n_slices = gridDim.x < (unsigned)TSQ_SLICES ? gridDim.x : (unsigned)TSQ_SLICES;
    double tsq = 0.0;
    if (stats_ws != nullptr && blockIdx.x < n_slices) {
        const StatsSlice sl = stats_ws_slice(stats_ws_records(stats_ws), n_slices, blockIdx.x);
        for (unsigned i = sl.lo + threadIdx.x; i < sl.hi; i += 256) tsq += stats_ws_stat(stats_ws, i);
    }
    T *row = a + (size_t)blockIdx.x * cols;
    T acc = T(0);
    const bool vec = (cols % 4 == 0) && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(w) |
                                          reinterpret_cast<uintptr_t>(bias)) % (4 * sizeof(T)) == 0);
    if (vec) {
        struct alignas(4 * sizeof(T)) Q { T v[4]; };
        Q *rq = reinterpret_cast<Q *>(row);
        const Q *wq = reinterpret_cast<const Q *>(w);
        const Q *bq = reinterpret_cast<const Q *>(bias);
        const Q zero = {{T(0), T(0), T(0), T(0)}};
        const size_t nq = cols / 4;
        size_t q = threadIdx.x;
        for (; q + 256 < nq; q += 512) {                      // two quads per lane in flight
            Q x0 = rq[q], x1 = rq[q + 256], w0 = wq[q], w1 = wq[q + 256];
            const Q b0 = bias ? bq[q] : zero, b1 = bias ? bq[q + 256] : zero;
#pragma unroll
            for (int j = 0; j < 4; ++j) { x0.v[j] = tanh_dev(x0.v[j] + b0.v[j]); x1.v[j] = tanh_dev(x1.v[j] + b1.v[j]); }
            rq[q] = x0; rq[q + 256] = x1;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += x0.v[j] * w0.v[j];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += x1.v[j] * w1.v[j];
        }
        for (; q < nq; q += 256) {
            Q x0 = rq[q], w0 = wq[q];
            const Q b0 = bias ? bq[q] : zero;
#pragma unroll
            for (int j = 0; j < 4; ++j) x0.v[j] = tanh_dev(x0.v[j] + b0.v[j]);
            rq[q] = x0;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += x0.v[j] * w0.v[j];
        }
    } else {
        for (size_t c = threadIdx.x; c < cols; c += 256) {
            const T h = tanh_dev(row[c] + (bias ? bias[c] : T(0)));
            row[c] = h;
            acc += h * w[c];
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (stats_ws != nullptr && blockIdx.x < n_slices) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) tsq += __shfl_down(tsq, off, 64);
        if ((threadIdx.x & 63) == 0) lds_d[threadIdx.x >> 6] = tsq;
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        out[blockIdx.x] = ((lds[0] + lds[1]) + lds[2]) + lds[3];
        if (stats_ws != nullptr && blockIdx.x < n_slices) tsq_parts[blockIdx.x] = ((lds_d[0] + lds_d[1]) + lds_d[2]) + lds_d[3];
    }
}

inline unsigned col_blocks(size_t cols) { return (unsigned)((cols + CS_COLS - 1) / CS_COLS); }

}  // namespace

// --------------------------------------------------------------------------
// C ABI
// --------------------------------------------------------------------------

extern "C" {

#define SGMCMC_BNN_COST(SFX, T)                                                                                      \
    int sgmcmc_bnn_head_##SFX(const T *mean, const T *y, const T *log_var, const double *theta_sumsq,                \
                              const void *stats_ws, const T *last_bias, size_t B, double batch_size,                 \
                              double n_examples, double n_params, double wdecay, double prior_mean, double prior_var, \
                              int fold_prior_grad, T *delta, T *cost_out, T *grad_log_var_out,                       \
                              T *grad_last_bias_out, T *mse_out, sgmcmc_stream_t stream)                             \
    {                                                                                                                \
        if (!mean || !y || !log_var || (!theta_sumsq && !stats_ws) || !delta || !cost_out || !grad_log_var_out ||    \
            !mse_out || B == 0 || (grad_last_bias_out && !last_bias))                                                \
            return fail(SGMCMC_EINVAL, "bnn_head: NULL argument or B == 0");                                         \
        const BnnHeadConsts k = head_consts(batch_size, n_examples, n_params, wdecay, prior_mean, prior_var,         \
                                            fold_prior_grad);                                                        \
        hipLaunchKernelGGL((bnn_head_kernel<T>), dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), mean, y,  \
                           log_var, theta_sumsq, static_cast<const double *>(stats_ws), last_bias, B, k, delta,      \
                           cost_out, grad_log_var_out, grad_last_bias_out, mse_out);                                 \
        return launched("bnn_head");                                                                                 \
    }                                                                                                                \
    int sgmcmc_bnn_head_last_layer_backward_##SFX(                                                                   \
        const T *mean, size_t n_mean_parts, const T *y, const T *log_var, const double *tsq_parts, const T *last_bias, \
        size_t rows, size_t cols, double batch_size, double n_examples, double n_params, double wdecay,              \
        double prior_mean, double prior_var, int fold_prior_grad, const T *w, const T *h, const T *bias_prev, T beta, \
        T *cost_out, T *grad_log_var_out, T *grad_last_bias_out, T *mse_out, T *delta_prev, T *colsum, T *gw,        \
        sgmcmc_stream_t stream)                                                                                      \
    {                                                                                                                \
        if (!mean || !y || !log_var || !tsq_parts || !w || !h || !cost_out || !grad_log_var_out || !mse_out ||       \
            !delta_prev || !colsum || !gw || rows == 0 || cols == 0 || (grad_last_bias_out && !last_bias) ||         \
            (beta != T(0) && !bias_prev))                                                                            \
            return fail(SGMCMC_EINVAL, "bnn_head_last_layer_backward: NULL argument or empty matrix");               \
        if (n_mean_parts == 0 || n_mean_parts > 4096 || (n_mean_parts > 1 && rows > (size_t)HEAD_MAX_PART_ROWS))     \
            return fail(SGMCMC_EINVAL,                                                                               \
                        "bnn_head_last_layer_backward: n_mean_parts must be 1 .. 4096 (and rows <= 1024 when > 1)"); \
        const BnnHeadConsts k = head_consts(batch_size, n_examples, n_params, wdecay, prior_mean, prior_var,         \
                                            fold_prior_grad);                                                        \
        /* slices of sum(theta^2) the forward launch left: min(16, its workgroups) -- one workgroup per row          \
           (tanh_rowdot), or per 32 x 64 output tile (bnn_dense_tanh, which callers use only with >= 16 tiles) */     \
        const int n_tsq = (int)((n_mean_parts > 1 || rows >= (size_t)TSQ_SLICES) ? (size_t)TSQ_SLICES : rows);       \
        hipLaunchKernelGGL((head_last_layer_backward_kernel<T>), dim3(col_blocks(cols) + 1u), dim3(1024), 0,         \
                           static_cast<hipStream_t>(stream), mean, (int)n_mean_parts, y, log_var, tsq_parts, n_tsq,  \
                           last_bias, k, cost_out, grad_log_var_out, grad_last_bias_out, mse_out, w, h, rows, cols,  \
                           bias_prev, beta, delta_prev, colsum, gw);                                                 \
        return launched("head_last_layer_backward");                                                                 \
    }                                                                                                                \
    int sgmcmc_bnn_last_layer_backward_##SFX(const T *dvec, const T *w, const T *h, size_t rows, size_t cols,        \
                                             const T *bias_prev, T beta, T *delta_prev, T *colsum, T *gw,            \
                                             sgmcmc_stream_t stream)                                                 \
    {                                                                                                                \
        if (rows == 0 || cols == 0) return 0;                                                                        \
        if (!dvec || !w || !h || !delta_prev || !colsum || !gw || (beta != T(0) && !bias_prev))                      \
            return fail(SGMCMC_EINVAL, "last_layer_backward: NULL argument");                                        \
        hipLaunchKernelGGL((last_layer_backward_kernel<T>), dim3(col_blocks(cols)), dim3(1024), 0,                   \
                           static_cast<hipStream_t>(stream), dvec, w, h, rows, cols, bias_prev, beta, delta_prev,    \
                           colsum, gw);                                                                              \
        return launched("last_layer_backward");                                                                      \
    }                                                                                                                \
    int sgmcmc_tanh_backward_colsum_##SFX(T *delta, const T *h, size_t rows, size_t cols, const T *bias, T beta,     \
                                          T *colsum, sgmcmc_stream_t stream)                                         \
    {                                                                                                                \
        if (rows == 0 || cols == 0) return 0;                                                                        \
        if (!delta || !h || !colsum || (beta != T(0) && !bias))                                                      \
            return fail(SGMCMC_EINVAL, "tanh_backward_colsum: NULL argument");                                       \
        hipLaunchKernelGGL((tanh_backward_colsum_kernel<T>), dim3(col_blocks(cols)), dim3(1024), 0,                  \
                           static_cast<hipStream_t>(stream), delta, h, rows, cols, bias, beta, colsum);              \
        return launched("tanh_backward_colsum");                                                                     \
    }                                                                                                                \
    int sgmcmc_tanh_backward_##SFX(T *delta, const T *h, size_t n, sgmcmc_stream_t stream)                           \
    {                                                                                                                \
        if (n == 0) return 0;                                                                                        \
        if (!delta || !h) return fail(SGMCMC_EINVAL, "tanh_backward: NULL argument");                                \
        hipLaunchKernelGGL((tanh_backward_kernel<T>), dim3(small_grid(n)), dim3(256), 0,                             \
                           static_cast<hipStream_t>(stream), delta, h, n);                                           \
        return launched("tanh_backward");                                                                            \
    }                                                                                                                \
    int sgmcmc_bias_tanh_rowdot_##SFX(T *a, const T *bias, const T *w, size_t rows, size_t cols, T *out,             \
                                      const void *stats_ws, double *tsq_parts, sgmcmc_stream_t stream)               \
    {                                                                                                                \
        if (rows == 0 || cols == 0) return 0;                                                                        \
        if (!a || !w || !out) return fail(SGMCMC_EINVAL, "tanh_rowdot: NULL argument");                             \
        if ((stats_ws == nullptr) != (tsq_parts == nullptr))                                                         \
            return fail(SGMCMC_EINVAL, "tanh_rowdot: stats_ws and tsq_parts go together");                           \
        if (rows > 0x7fffffffull) return fail(SGMCMC_EINVAL, "tanh_rowdot: too many rows");                          \
        hipLaunchKernelGGL((tanh_rowdot_kernel<T>), dim3((unsigned)rows), dim3(256), 0, static_cast<hipStream_t>(stream), \
                           a, w, cols, out, static_cast<const double *>(stats_ws), tsq_parts, bias);                 \
        return launched("tanh_rowdot");                                                                              \
    }                                                                                                                \
    int sgmcmc_bias_tanh_##SFX(T *a, const T *bias, size_t rows, size_t cols, sgmcmc_stream_t stream)                \
    {                                                                                                                \
        if (rows == 0 || cols == 0) return 0;                                                                        \
        if (!a || !bias) return fail(SGMCMC_EINVAL, "bias_tanh: NULL argument");                                     \
        /* the scalar path steps a 32-bit index by up to 2^24 lanes: beyond 2^32 - 2^24 elements it would wrap */    \
        if (rows > (0x100000000ull - 0x1000000ull) / cols)                                                           \
            return fail(SGMCMC_EINVAL, "bias_tanh: more than 2^32 - 2^24 elements");                                 \
        const size_t lanes = (rows * cols + 3) / 4, blocks = (lanes + 255) / 256;                                    \
        hipLaunchKernelGGL((bias_tanh_kernel<T>), dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,   \
                           static_cast<hipStream_t>(stream), a, bias, (unsigned)rows, (unsigned)cols);               \
        return launched("bias_tanh");                                                                                \
    }
SGMCMC_BNN_COST(f32, float)
SGMCMC_BNN_COST(f64, double)
#undef SGMCMC_BNN_COST

}  // extern "C"
