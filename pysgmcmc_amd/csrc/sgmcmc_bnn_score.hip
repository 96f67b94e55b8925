// sgmcmc_bnn_score.hip -- K13, the held-out score of device-resident samples of a SMALL tanh-MLP BNN: kernels and host side
// of sgmcmc_bnn_score_{f32,f64} and sgmcmc_score_abi_version (include/sgmcmc_hip_score.h, the held-out-score add-on outside
// the section 8(b) boundary). The reference leaves model diagnostics open (pysgmcmc/diagnostics/model_diagnostics.py); the
// density is the one its BNN trains on (pysgmcmc/models/bayesian_neural_network.py:368).
//
// The forward pass is K11's: the entry calls sgmcmc_bnn_predict_* with no optional output, so `means` has K11's bits. A net
// K11 refuses is refused with its text, by the rules both share (sgmcmc_bnn_small_net.hpp), under K11's name. Behind the
// forward launch on the same stream, every reduction in f64 in the header's order:
//   row kernel     lane = test row, 64-lane workgroups, so every access to means / loglik is a coalesced row segment. The
//                  per-sample constants a_s, b_s go through the LDS in blocks of 64 samples (lane j forms those of sample
//                  s0 + j), which puts barriers inside the sample loop: lanes behind n_rows stay in the loop and only skip
//                  their loads and stores. Two passes over s ascending; pass 2 forms l again with pass 1's statements. A lane
//                  loads its column's next 16 means before it uses the first: one lane per row is latency-bound otherwise.
//   sample kernel  one 256-lane workgroup per sample: lane j adds rows j, j + 256, ... ascending, then a fixed pairwise tree.
//   summary kernel one 256-lane workgroup, the same order, three sums.
// No atomics anywhere: equal inputs give equal bits whatever the launch.
#include "sgmcmc_bnn_small_net.hpp"

namespace {

constexpr int SCORE_ROW_THREADS = 64;                      // one wave: rows per workgroup AND samples per LDS block
constexpr int SCORE_ROW_AHEAD = 16;                        // loads of means a lane keeps in flight
constexpr int SCORE_SUM_THREADS = 256;
constexpr double SCORE_LOG_2PI = 1.8378770664093453;

// a_s and b_s of sample s (the header's statements)
template <typename T>
__device__ __forceinline__ void score_constants(const SmallNetChains<T> &ch, size_t n, size_t ld, int n_params, size_t s,
                                                double &a, double &b)
{
    const double lv = (double)ch.row(s, n, ld)[n_params - 1];
    a = -0.5 * (SCORE_LOG_2PI + lv);
    b = 0.5 / (exp(lv) + 1e-16);
}

__device__ __forceinline__ double score_loglik(double y, double f, double a, double b)
{
    const double d = y - f;
    return a - (d * d) * b;
}

// means[s .. s + SCORE_ROW_AHEAD)[r] of one row's column, of which `left` >= 1 are wanted (the others repeat the last one):
// every load is issued before the first is used, so a lane waits for memory once per SCORE_ROW_AHEAD samples and not once
// per sample. The sums that follow stay ONE chain in s order.
template <typename T>
__device__ __forceinline__ void score_load_ahead(const T *__restrict__ col, size_t n_rows, size_t s, int left,
                                                 T (&f)[SCORE_ROW_AHEAD])
{
#pragma unroll
    for (int k = 0; k < SCORE_ROW_AHEAD; ++k) f[k] = col[(s + (size_t)(k < left ? k : left - 1)) * n_rows];
}

// adds the 256 partials of `part` in place by the fixed pairwise tree; the total ends in part[0]
__device__ __forceinline__ void score_tree(double *part, int tid)
{
    __syncthreads();
    for (int h = SCORE_SUM_THREADS / 2; h >= 1; h /= 2) {
        if (tid < h) part[tid] += part[tid + h];
        __syncthreads();
    }
}

template <typename T>
__global__ void __launch_bounds__(SCORE_ROW_THREADS) bnn_score_row_kernel(const SmallNetChains<T> ch, size_t n, size_t ld,
                                                                          int n_params, size_t S, const T *__restrict__ means,
                                                                          const T *__restrict__ y, size_t n_rows,
                                                                          double *__restrict__ row_lppd,
                                                                          double *__restrict__ row_pwaic,
                                                                          double *__restrict__ ens_mean,
                                                                          double *__restrict__ ens_var,
                                                                          double *__restrict__ loglik)
{
    __shared__ double sa[SCORE_ROW_THREADS], sb[SCORE_ROW_THREADS];
    const int tid = threadIdx.x;
    const size_t r = (size_t)blockIdx.x * SCORE_ROW_THREADS + tid;
    const bool active = r < n_rows;                        // an idle lane stays in the loops: they hold barriers
    const double yr = active ? (double)y[r] : 0.0;
    const T *col = means + (active ? r : 0);
    // ---- pass 1: sum f, max l, sum l
    double sum_f = 0.0, sum_l = 0.0, M = -INFINITY;
    for (size_t s0 = 0; s0 < S; s0 += SCORE_ROW_THREADS) {
        __syncthreads();                                   // the block before is read by every lane
        if (s0 + tid < S) score_constants(ch, n, ld, n_params, s0 + tid, sa[tid], sb[tid]);
        __syncthreads();
        if (active) {
            const int nb = (int)(S - s0 < (size_t)SCORE_ROW_THREADS ? S - s0 : (size_t)SCORE_ROW_THREADS);
            for (int j0 = 0; j0 < nb; j0 += SCORE_ROW_AHEAD) {
                T fa[SCORE_ROW_AHEAD];
                score_load_ahead(col, n_rows, s0 + j0, nb - j0, fa);
#pragma unroll
                for (int k = 0; k < SCORE_ROW_AHEAD; ++k) {
                    const int j = j0 + k;
                    if (j < nb) {
                        const double f = (double)fa[k];
                        const double l = score_loglik(yr, f, sa[j], sb[j]);
                        sum_f += f;
                        M = fmax(M, l);
                        sum_l += l;
                        if (loglik != nullptr) loglik[(s0 + j) * n_rows + r] = l;
                    }
                }
            }
        }
    }
    const double mean = sum_f / (double)S;
    const double lbar = sum_l / (double)S;
    // ---- pass 2: squared deviations of f and of l, sum exp(l - M)
    double q = 0.0, Z = 0.0, w = 0.0;
    for (size_t s0 = 0; s0 < S; s0 += SCORE_ROW_THREADS) {
        __syncthreads();
        if (s0 + tid < S) score_constants(ch, n, ld, n_params, s0 + tid, sa[tid], sb[tid]);
        __syncthreads();
        if (active) {
            const int nb = (int)(S - s0 < (size_t)SCORE_ROW_THREADS ? S - s0 : (size_t)SCORE_ROW_THREADS);
            for (int j0 = 0; j0 < nb; j0 += SCORE_ROW_AHEAD) {
                T fa[SCORE_ROW_AHEAD];
                score_load_ahead(col, n_rows, s0 + j0, nb - j0, fa);
#pragma unroll
                for (int k = 0; k < SCORE_ROW_AHEAD; ++k) {
                    const int j = j0 + k;
                    if (j < nb) {
                        const double f = (double)fa[k];
                        const double l = score_loglik(yr, f, sa[j], sb[j]);
                        const double df = f - mean;
                        q += df * df;
                        Z += exp(l - M);
                        const double dl = l - lbar;
                        w += dl * dl;
                    }
                }
            }
        }
    }
    if (!active) return;
    ens_mean[r] = mean;
    ens_var[r] = q / (double)S;
    row_lppd[r] = (M + log(Z)) - log((double)S);
    row_pwaic[r] = S > 1 ? w / (double)(S - 1) : 0.0;
}

// sample_loglik[s] = sum_r l[s][r]
template <typename T>
__global__ void __launch_bounds__(SCORE_SUM_THREADS) bnn_score_sample_kernel(const SmallNetChains<T> ch, size_t n, size_t ld,
                                                                            int n_params, const T *__restrict__ means,
                                                                            const T *__restrict__ y, size_t n_rows,
                                                                            double *__restrict__ sample_loglik)
{
    __shared__ double part[SCORE_SUM_THREADS];
    __shared__ double ab[2];
    const int tid = threadIdx.x;
    const size_t s = blockIdx.x;
    if (tid == 0) score_constants(ch, n, ld, n_params, s, ab[0], ab[1]);
    __syncthreads();
    const double a = ab[0], b = ab[1];
    const T *row = means + s * n_rows;
    double acc = 0.0;
    for (size_t r = tid; r < n_rows; r += SCORE_SUM_THREADS) acc += score_loglik((double)y[r], (double)row[r], a, b);
    part[tid] = acc;
    score_tree(part, tid);
    if (tid == 0) sample_loglik[s] = part[0];
}

// summary = { sum row_lppd, sum row_pwaic, sum (ens_mean - y)^2 }
template <typename T>
__global__ void __launch_bounds__(SCORE_SUM_THREADS) bnn_score_summary_kernel(const double *__restrict__ row_lppd,
                                                                             const double *__restrict__ row_pwaic,
                                                                             const double *__restrict__ ens_mean,
                                                                             const T *__restrict__ y, size_t n_rows,
                                                                             double *__restrict__ summary)
{
    __shared__ double part[3][SCORE_SUM_THREADS];
    const int tid = threadIdx.x;
    double lppd = 0.0, pwaic = 0.0, sq = 0.0;
    for (size_t r = tid; r < n_rows; r += SCORE_SUM_THREADS) {
        lppd += row_lppd[r];
        pwaic += row_pwaic[r];
        const double e = ens_mean[r] - (double)y[r];
        sq += e * e;
    }
    part[0][tid] = lppd; part[1][tid] = pwaic; part[2][tid] = sq;
    for (int k = 0; k < 3; ++k) score_tree(part[k], tid);
    if (tid < 3) summary[tid] = part[tid][0];
}

inline int score_forward(const float *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers,
                         const float *X, size_t n_rows, float *means, hipStream_t st)
{
    return sgmcmc_bnn_predict_f32(chains, m, n, ld, layer_sizes, n_layers, X, n_rows, means, nullptr, nullptr, nullptr, st);
}
inline int score_forward(const double *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers,
                         const double *X, size_t n_rows, double *means, hipStream_t st)
{
    return sgmcmc_bnn_predict_f64(chains, m, n, ld, layer_sizes, n_layers, X, n_rows, means, nullptr, nullptr, nullptr, st);
}

template <typename T>
int bnn_score(const T *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers, const T *X,
              const T *y, size_t n_rows, T *means, double *row_lppd, double *row_pwaic, double *ens_mean, double *ens_var,
              double *loglik, double *sample_loglik, double *summary, hipStream_t st)
{
    const char *what = "bnn_score";
    if (n_rows == 0 || n == 0) return 0;
    if (m < 1 || m > SGMCMC_SCORE_MAX_CHAINS)
        return fail(SGMCMC_EINVAL, "%s: m = %d chains, must be 1 .. %d", what, m, SGMCMC_SCORE_MAX_CHAINS);
    const struct { const void *p; const char *name; } required[] = {
        {chains, "chains"}, {layer_sizes, "layer_sizes"}, {X, "X"}, {y, "y"}, {means, "means"}, {row_lppd, "row_lppd"},
        {row_pwaic, "row_pwaic"}, {ens_mean, "ens_mean"}, {ens_var, "ens_var"}};
    for (const auto &arg : required)
        if (!arg.p) return fail(SGMCMC_EINVAL, "%s: %s is NULL", what, arg.name);
    SmallNetChains<T> ch;
    if (int rc = small_net_chains(what, chains, m, ch)) return rc;
    // a net K11 refuses on its sizes or on its parameters alone: the shared rules under K11's name, so K11's text
    SmallNet net{};
    size_t n_params = 0;
    if (int rc = small_net_rules("bnn_predict", layer_sizes, n_layers, net, n_params)) return rc;
    if (int rc = small_net_offsets("bnn_predict", n_params, sizeof(T), net)) return rc;
    if (ld < n_params) return fail(SGMCMC_EINVAL, "%s: ld = %zu is smaller than n_params = %zu", what, ld, n_params);
    if (n > (size_t)INT32_MAX / (size_t)m)
        return fail(SGMCMC_EINVAL, "%s: m * n = %d * %zu samples, must be < 2^31", what, m, n);
    const size_t S = (size_t)m * n;
    const size_t blocks = (n_rows + SCORE_ROW_THREADS - 1) / SCORE_ROW_THREADS;
    if (n_rows > SIZE_MAX - SCORE_ROW_THREADS || blocks > (size_t)INT32_MAX)
        return fail(SGMCMC_EINVAL, "%s: n_rows = %zu is too large for one launch", what, n_rows);
    // 1. the forward pass: K11's launch, K11's bits (and its refusal of a net that does not fit the LDS, before it launches)
    if (int rc = score_forward(chains, m, n, ld, layer_sizes, n_layers, X, n_rows, means, st)) return rc;
    // 2. the rows
    hipLaunchKernelGGL(bnn_score_row_kernel<T>, dim3((unsigned)blocks), dim3(SCORE_ROW_THREADS), 0, st, ch, n, ld,
                       (int)n_params, S, static_cast<const T *>(means), y, n_rows, row_lppd, row_pwaic, ens_mean, ens_var,
                       loglik);
    if (int rc = launched("bnn_score_row_kernel")) return rc;
    // 3. the samples
    if (sample_loglik) {
        hipLaunchKernelGGL(bnn_score_sample_kernel<T>, dim3((unsigned)S), dim3(SCORE_SUM_THREADS), 0, st, ch, n, ld,
                           (int)n_params, static_cast<const T *>(means), y, n_rows, sample_loglik);
        if (int rc = launched("bnn_score_sample_kernel")) return rc;
    }
    // 4. the totals
    if (summary) {
        hipLaunchKernelGGL(bnn_score_summary_kernel<T>, dim3(1), dim3(SCORE_SUM_THREADS), 0, st,
                           static_cast<const double *>(row_lppd), static_cast<const double *>(row_pwaic),
                           static_cast<const double *>(ens_mean), y, n_rows, summary);
        if (int rc = launched("bnn_score_summary_kernel")) return rc;
    }
    return 0;
}

}  // namespace

extern "C" {

int sgmcmc_score_abi_version(void) { return SGMCMC_SCORE_ABI_VERSION; }

int sgmcmc_bnn_score_f32(const float *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers,
                         const float *X, const float *y, size_t n_rows, float *means, double *row_lppd, double *row_pwaic,
                         double *ens_mean, double *ens_var, double *loglik, double *sample_loglik, double *summary,
                         sgmcmc_stream_t stream)
{
    return bnn_score<float>(chains, m, n, ld, layer_sizes, n_layers, X, y, n_rows, means, row_lppd, row_pwaic, ens_mean,
                            ens_var, loglik, sample_loglik, summary, static_cast<hipStream_t>(stream));
}
int sgmcmc_bnn_score_f64(const double *const *chains, int m, size_t n, size_t ld, const int *layer_sizes, int n_layers,
                         const double *X, const double *y, size_t n_rows, double *means, double *row_lppd,
                         double *row_pwaic, double *ens_mean, double *ens_var, double *loglik, double *sample_loglik,
                         double *summary, sgmcmc_stream_t stream)
{
    return bnn_score<double>(chains, m, n, ld, layer_sizes, n_layers, X, y, n_rows, means, row_lppd, row_pwaic, ens_mean,
                             ens_var, loglik, sample_loglik, summary, static_cast<hipStream_t>(stream));
}

}  // extern "C"
