// sgmcmc_kernels.hip -- the [boundary] group of the C ABI in include/sgmcmc_hip.h apart from the sampler steps: ABI version
// and the thread-local error text (sgmcmc_host::fail / hip_fail are defined here for every translation unit of the
// library), events, device count, the step statistics' workspace sizes and final pass (K7), the Philox fills (K5: normals
// through the shared streaming kernel of sgmcmc_stream.hpp, raw words), the Welford moments (K4), the summary reduction
// (K6), R-hat pack / finish, the device-side step counter and the minibatch window gather.
//
// The fused update kernels K1-K3 live in sgmcmc_sghmc.hip, sgmcmc_sgld.hip and sgmcmc_rsghmc.hip (kernel shape and
// operators: sgmcmc_stream.hpp, sgmcmc_device.hpp), the BNN cost path's kernels in sgmcmc_bnn_cost.hip.
//
// One IEEE rounding per reference op (-ffp-contract=off, correctly rounded '/' and sqrt), so results equal the CPU oracle
// bit for bit. K6 and K7 are the reductions: wave shuffles -> LDS -> (per-block partials ->) fixed-order final pass.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "sgmcmc_stats_ws.hpp"
#include "sgmcmc_stream.hpp"

namespace {

// Final pass: ONE block of 1024 lanes = 256 records x 4 statistics per trip. Lane t handles statistic t & 3 of records
// t >> 2, (t >> 2) + 256, ... (the 32-byte records are read as fully coalesced 8-byte elements, 8 loads in flight),
// then a fixed shuffle/LDS tree combines the 256 lanes of each statistic. Fixed association => deterministic.
__global__ void __launch_bounds__(1024) stats_final_kernel(const double *__restrict__ part, double *__restrict__ out4)
{
    __shared__ double lds[16][4];
    const unsigned nparts = stats_ws_records(part);
    const int k = threadIdx.x & 3, t = threadIdx.x >> 2;
    const int wave = threadIdx.x >> 6;
    double v = 0.0;
    unsigned i = t;
    for (; i + 7u * 256u < nparts; i += 8u * 256u) {
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = stats_ws_stat(part, i + (unsigned)u * 256u, k);
#pragma unroll
        for (int u = 0; u < 8; ++u) v += x[u];
    }
    for (; i < nparts; i += 256u) v += stats_ws_stat(part, i, k);
    // lanes with equal (lane & 3) hold the same statistic: xor-shuffles over the other 4 lane bits
#pragma unroll
    for (int off = 32; off >= 4; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) < 4) lds[wave][k] = v;
    __syncthreads();
    if (threadIdx.x < 4) {
        double tot = 0.0;
#pragma unroll
        for (int w = 0; w < 16; ++w) tot += lds[w][threadIdx.x];
        out4[threadIdx.x] = tot;
    }
}

// --------------------------------------------------------------------------
// K6 summary: wave shuffles -> LDS -> per-block partials -> fixed-order final
// --------------------------------------------------------------------------

constexpr int SUMMARY_BLOCKS = 1024;
constexpr int SUMMARY_THREADS = 256;

struct Summary { double s, ss, mn, mx; };

// min / max that propagate NaN whichever side holds it (a bare `a < b ? a : b` drops a NaN in b), so the summary's min
// and max are NaN exactly when some element is, in any reduction order; on numbers they pick what the bare form picks
__device__ __forceinline__ double min_nan(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double max_nan(double a, double b) { return (a > b || a != a) ? a : b; }

__device__ __forceinline__ Summary summary_combine(Summary a, Summary b)
{
    Summary o;
    o.s = a.s + b.s; o.ss = a.ss + b.ss;
    o.mn = min_nan(a.mn, b.mn);
    o.mx = max_nan(a.mx, b.mx);
    return o;
}
__device__ __forceinline__ Summary summary_wave_reduce(Summary v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Summary o;
        o.s = __shfl_down(v.s, off, 64);
        o.ss = __shfl_down(v.ss, off, 64);
        o.mn = __shfl_down(v.mn, off, 64);
        o.mx = __shfl_down(v.mx, off, 64);
        v = summary_combine(v, o);
    }
    return v;
}
__device__ __forceinline__ Summary summary_block_reduce(Summary v)
{
    __shared__ Summary lds[SUMMARY_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = summary_wave_reduce(v);
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    if (wave == 0) {
        const int nw = blockDim.x >> 6;
        Summary w = lds[lane < nw ? lane : 0];
        if (lane >= nw) { w.s = 0; w.ss = 0; w.mn = INFINITY; w.mx = -INFINITY; }
        v = summary_wave_reduce(w);
    }
    return v;
}

template <typename T>
__global__ void __launch_bounds__(SUMMARY_THREADS) summary_partial(const T *__restrict__ x, size_t n, Summary *__restrict__ part)
{
    Summary acc = {0.0, 0.0, INFINITY, -INFINITY};
    const size_t G = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += G) {
        double v = (double)x[i];
        acc.s += v; acc.ss += v * v;
        acc.mn = min_nan(v, acc.mn);
        acc.mx = max_nan(v, acc.mx);
    }
    acc = summary_block_reduce(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
__global__ void __launch_bounds__(SUMMARY_THREADS) summary_final(const Summary *__restrict__ part, int nparts, double *__restrict__ out4)
{
    Summary acc = {0.0, 0.0, INFINITY, -INFINITY};
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) acc = summary_combine(acc, part[i]);
    acc = summary_block_reduce(acc);
    if (threadIdx.x == 0) { out4[0] = acc.s; out4[1] = acc.ss; out4[2] = acc.mn; out4[3] = acc.mx; }
}

// --------------------------------------------------------------------------
// R-hat pack / finish and raw Philox words (small elementwise kernels)
// --------------------------------------------------------------------------

// One IEEE rounding per operation in T (fp contract off): the C oracle's rhat_pack / rhat_finish give the same bits.
// Sharded layout: the padded index range [0, n_shards * shard_len) is cut into n_shards chunks, chunk s holds
// [mean | mean^2 | var] of parameters [s * shard_len, (s + 1) * shard_len) -- what reduce_scatter hands to rank s.
// n_shards = 1, shard_len = n is the plain [mean | mean^2 | var] layout of an all-reduce. Padding is written as 0.
template <typename T>
__global__ void __launch_bounds__(256) rhat_pack_kernel(const T *__restrict__ mean, const T *__restrict__ m2,
                                                        size_t n, T inv_cm1, size_t shard_len, size_t total,
                                                        T *__restrict__ out3)
{
    const size_t G = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += G) {
        const size_t s = i / shard_len, j = i - s * shard_len;
        T mu = T(0), var = T(0);
        if (i < n) { mu = mean[i]; var = m2[i] * inv_cm1; }
        T *o = out3 + s * 3 * shard_len + j;
        o[0] = mu;
        o[shard_len] = mu * mu;
        o[2 * shard_len] = var;
    }
}
// sum3 = [S_mean | S_sq | S_var] with row pitch ld; n = valid elements of this (shard of the) buffer
template <typename T>
__global__ void __launch_bounds__(256) rhat_finish_kernel(const T *__restrict__ sum3, size_t n, size_t ld, T m, T cnt,
                                                          T *__restrict__ rhat)
{
    const size_t G = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += G) {
        T s_mean = sum3[i], s_sq = sum3[ld + i], s_var = sum3[2 * ld + i];
        T W = s_var / m;
        T B = cnt * ((s_sq - (s_mean * s_mean) / m) / (m - T(1)));
        T Vhat = W * ((cnt - T(1)) / cnt) + B / cnt;
        rhat[i] = sqrt(Vhat / W);
    }
}
__global__ void __launch_bounds__(256) philox_bits_kernel(uint32_t *__restrict__ out, size_t n, NoiseKey nk)
{
    nk.resolve();
    const size_t G = (size_t)gridDim.x * blockDim.x;
    const size_t nq = (n + 3) / 4;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += G) {
        uint32_t x[4];
        philox_quad(nk, q, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) if (4 * q + j < n) out[4 * q + j] = x[j];
    }
}

// --------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------

}  // namespace

// error reporting shared by the translation units of the library (sgmcmc_host.hpp)
namespace sgmcmc_host {
thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
int hip_fail(hipError_t e, const char *what)
{
    return fail((int)e, "%s: %s", what, hipGetErrorString(e));
}
}  // namespace sgmcmc_host
using namespace sgmcmc_host;

namespace {

__global__ void counter_add_kernel(uint64_t *ctr, uint64_t inc) { *ctr += inc; }

// minibatch window [start, start + B) of the resident dataset into the static feed buffers
// (pysgmcmc/data_batches.py:118-123): x rows are contiguous, so the window is ONE contiguous range of X
template <typename T>
__global__ void window_gather_kernel(const T *__restrict__ X, const T *__restrict__ y, size_t start, size_t B, size_t D,
                                     T *__restrict__ xb, size_t ldx, T *__restrict__ yb)
{
    const size_t nx = B * D;
    const T *__restrict__ src = X + start * D;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, G = (size_t)gridDim.x * blockDim.x;
    // 16-byte copies when source window and destination are 16-byte aligned (4 elements of f32, 2 of f64 per access)
    constexpr size_t V = 16 / sizeof(T);
    struct alignas(16) Q { T v[V]; };
    if (ldx == D) {
        const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(xb)) & 15u) == 0;
        const size_t nq = vec ? nx / V : 0;
        for (size_t q = gid; q < nq; q += G) reinterpret_cast<Q *>(xb)[q] = reinterpret_cast<const Q *>(src)[q];
        for (size_t i = nq * V + gid; i < nx; i += G) xb[i] = src[i];
    } else {
        // pitched destination (row stride ldx > D; the columns beyond D are the caller's): row by row
        const bool vec = D % V == 0 && ldx % V == 0 &&
                         ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(xb)) & 15u) == 0;
        if (vec) {
            const size_t qpr = D / V, lq = ldx / V;
            for (size_t q = gid; q < B * qpr; q += G) {
                const size_t r = q / qpr, c = q - r * qpr;
                reinterpret_cast<Q *>(xb)[r * lq + c] = reinterpret_cast<const Q *>(src)[q];
            }
        } else {
            for (size_t i = gid; i < nx; i += G) {
                const size_t r = i / D, c = i - r * D;
                xb[r * ldx + c] = src[i];
            }
        }
    }
    for (size_t i = gid; i < B; i += G) yb[i] = y[start + i];
}

template <typename T>
int summary(const T *x, size_t n, double *out4, void *ws, hipStream_t st)
{
    // n = 0 reads nothing (an empty tensor may hand over NULL) and leaves the identities {0, 0, +inf, -inf}
    if ((!x && n) || !out4 || !ws) return fail(SGMCMC_EINVAL, "summary: NULL argument");
    size_t want = (n + SUMMARY_THREADS - 1) / SUMMARY_THREADS;
    int blocks = (int)(want < (size_t)SUMMARY_BLOCKS ? (want ? want : 1) : SUMMARY_BLOCKS);
    Summary *part = static_cast<Summary *>(ws);
    hipLaunchKernelGGL((summary_partial<T>), dim3(blocks), dim3(SUMMARY_THREADS), 0, st, x, n, part);
    hipLaunchKernelGGL(summary_final, dim3(1), dim3(SUMMARY_THREADS), 0, st, part, blocks, out4);
    return launched("summary");
}

}  // namespace

// --------------------------------------------------------------------------
// C ABI
// --------------------------------------------------------------------------

extern "C" {

int sgmcmc_abi_version(void) { return SGMCMC_ABI_VERSION; }
const char *sgmcmc_last_error(void) { return g_err; }

int sgmcmc_event_create(void **event_out)
{
    if (!event_out) return fail(SGMCMC_EINVAL, "event_create: event_out is NULL");
    hipEvent_t ev = nullptr;
    hipError_t e = hipEventCreate(&ev);
    if (e != hipSuccess) return hip_fail(e, "hipEventCreate");
    *event_out = ev;
    return 0;
}
int sgmcmc_event_destroy(void *event)
{
    if (!event) return 0;
    hipError_t e = hipEventDestroy(static_cast<hipEvent_t>(event));
    return e == hipSuccess ? 0 : hip_fail(e, "hipEventDestroy");
}
int sgmcmc_event_elapsed_ms(void *start_event, void *stop_event, float *ms_out)
{
    if (!start_event || !stop_event || !ms_out) return fail(SGMCMC_EINVAL, "event_elapsed_ms: NULL argument");
    hipError_t e = hipEventElapsedTime(ms_out, static_cast<hipEvent_t>(start_event), static_cast<hipEvent_t>(stop_event));
    return e == hipSuccess ? 0 : hip_fail(e, "hipEventElapsedTime");
}

int sgmcmc_event_synchronize(void *event)
{
    if (!event) return fail(SGMCMC_EINVAL, "event_synchronize: NULL argument");
    hipError_t e = hipEventSynchronize(static_cast<hipEvent_t>(event));
    return e == hipSuccess ? 0 : hip_fail(e, "hipEventSynchronize");
}

int sgmcmc_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(SGMCMC_ENODEV, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    return n;
}

// header + one record per block of the smallest block size (64 lanes)
size_t sgmcmc_step_stats_workspace_bytes(size_t n) { return (max_grid_for(n) + 1) * 4 * sizeof(double); }
size_t sgmcmc_step_stats_records_sized(size_t n, size_t elem_bytes, const sgmcmc_launch_t *launch_in)
{
    LaunchCfg cfg;
    if (!launch_in || resolve_launch(launch_in, cfg) != 0) return 0;
    if (cfg.block_threads <= 0) { fail(SGMCMC_EINVAL, "step_stats_records: launch.block_threads must be explicit"); return 0; }
    if (elem_bytes != 4 && elem_bytes != 8) { fail(SGMCMC_EINVAL, "step_stats_records: elem_bytes must be 4 (f32) or 8 (f64)"); return 0; }
    // launch(): f64 operators stream one quad per lane whatever quads_per_thread asks for
    const size_t want = want_blocks(n, cfg.block_threads, elem_bytes == 8 ? 1 : cfg.qpt);
    return want < (size_t)cfg.max_blocks ? want : (size_t)cfg.max_blocks;
}
size_t sgmcmc_step_stats_records(size_t n, const sgmcmc_launch_t *launch_in) { return sgmcmc_step_stats_records_sized(n, 4, launch_in); }
int sgmcmc_step_stats_finish(const void *stats_ws, double *stats_out, sgmcmc_stream_t stream)
{
    if (!stats_ws || !stats_out) return fail(SGMCMC_EINVAL, "step_stats_finish: NULL argument");
    hipLaunchKernelGGL(stats_final_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream),
                       static_cast<const double *>(stats_ws), stats_out);
    return launched("stats_final");
}

int sgmcmc_philox_normal_f32(float *out, size_t n, uint64_t seed, uint64_t step, const uint64_t *step_dev,
                             const sgmcmc_launch_t *launch_cfg, sgmcmc_stream_t stream)
{
    if (n == 0) return 0;
    if (!out) return fail(SGMCMC_EINVAL, "philox_normal: out is NULL");
    NormalFillOp<float> op{out, make_key(seed, step, step_dev)};
    return launch(op, n, aligned16(out), sizeof(*out), launch_cfg, static_cast<hipStream_t>(stream));
}
int sgmcmc_philox_normal_f64(double *out, size_t n, uint64_t seed, uint64_t step, const uint64_t *step_dev,
                             const sgmcmc_launch_t *launch_cfg, sgmcmc_stream_t stream)
{
    if (n == 0) return 0;
    if (!out) return fail(SGMCMC_EINVAL, "philox_normal: out is NULL");
    NormalFillOp<double> op{out, make_key(seed, step, step_dev)};
    return launch(op, n, aligned16(out), sizeof(*out), launch_cfg, static_cast<hipStream_t>(stream));
}
int sgmcmc_philox_bits_u32(uint32_t *out, size_t n, uint64_t seed, uint64_t step, const uint64_t *step_dev, sgmcmc_stream_t stream)
{
    if (n == 0) return 0;
    if (!out) return fail(SGMCMC_EINVAL, "philox_bits: out is NULL");
    hipLaunchKernelGGL(philox_bits_kernel, dim3(small_grid((n + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       out, n, make_key(seed, step, step_dev));
    return launched("philox_bits");
}

int sgmcmc_moments_update_f32(const float *theta, float *mean, float *m2, size_t n, uint64_t count,
                              const sgmcmc_launch_t *launch_cfg, sgmcmc_stream_t stream)
{
    if (n == 0) return 0;
    if (!theta || !mean || !m2 || count == 0) return fail(SGMCMC_EINVAL, "moments_update: NULL argument or count == 0");
    MomentsOp<float> op{theta, mean, m2, 1.0f / (float)count};
    return launch(op, n, aligned16(theta) && aligned16(mean) && aligned16(m2), 5 * sizeof(*theta), launch_cfg, static_cast<hipStream_t>(stream));
}
int sgmcmc_moments_update_f64(const double *theta, double *mean, double *m2, size_t n, uint64_t count,
                              const sgmcmc_launch_t *launch_cfg, sgmcmc_stream_t stream)
{
    if (n == 0) return 0;
    if (!theta || !mean || !m2 || count == 0) return fail(SGMCMC_EINVAL, "moments_update: NULL argument or count == 0");
    MomentsOp<double> op{theta, mean, m2, 1.0 / (double)count};
    return launch(op, n, aligned16(theta) && aligned16(mean) && aligned16(m2), 5 * sizeof(*theta), launch_cfg, static_cast<hipStream_t>(stream));
}

#define SGMCMC_RHAT(SFX, T)                                                                                           \
    int sgmcmc_rhat_pack_##SFX(const T *mean, const T *m2, size_t n, uint64_t count, size_t n_shards, size_t shard_len, \
                               T *out3, sgmcmc_stream_t stream)                                                       \
    {                                                                                                                 \
        if (n == 0) return 0;                                                                                         \
        if (!mean || !m2 || !out3 || count < 2) return fail(SGMCMC_EINVAL, "rhat_pack: NULL argument or count < 2"); \
        if (n_shards == 0 || shard_len == 0 || n_shards * shard_len < n || (n_shards - 1) * shard_len >= n)           \
            return fail(SGMCMC_EINVAL, "rhat_pack: n_shards * shard_len must cover n with no empty shard");          \
        const size_t total = n_shards * shard_len;                                                                    \
        hipLaunchKernelGGL((rhat_pack_kernel<T>), dim3(small_grid(total)), dim3(256), 0, static_cast<hipStream_t>(stream), \
                           mean, m2, n, T(1) / (T)(count - 1), shard_len, total, out3);                               \
        return launched("rhat_pack");                                                                                 \
    }                                                                                                                 \
    int sgmcmc_rhat_finish_##SFX(const T *sum3, size_t n, size_t ld, int m_chains, uint64_t count, T *rhat,          \
                                 double *summary_out4, void *summary_ws, sgmcmc_stream_t stream)                      \
    {                                                                                                                 \
        if (n == 0) return 0;                                                                                         \
        if (!sum3 || !rhat || m_chains < 2 || count < 2 || ld < n)                                                    \
            return fail(SGMCMC_EINVAL, "rhat_finish: NULL argument, m_chains < 2, count < 2 or ld < n");              \
        if ((summary_out4 == nullptr) != (summary_ws == nullptr))                                                     \
            return fail(SGMCMC_EINVAL, "rhat_finish: summary_out4 and summary_ws go together");                       \
        hipLaunchKernelGGL((rhat_finish_kernel<T>), dim3(small_grid(n)), dim3(256), 0, static_cast<hipStream_t>(stream), \
                           sum3, n, ld, (T)m_chains, (T)count, rhat);                                                 \
        if (const int rc = launched("rhat_finish")) return rc;                                                        \
        /* device-side summary {sum, sum of squares, min, max} of R-hat: no host synchronisation on the path */      \
        return summary_out4 ? summary<T>(rhat, n, summary_out4, summary_ws, static_cast<hipStream_t>(stream)) : 0;   \
    }
SGMCMC_RHAT(f32, float)
SGMCMC_RHAT(f64, double)
#undef SGMCMC_RHAT

int sgmcmc_counter_add_u64(uint64_t *counter, uint64_t inc, sgmcmc_stream_t stream)
{
    if (!counter) return fail(SGMCMC_EINVAL, "counter_add: counter is NULL");
    hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), counter, inc);
    return launched("counter_add");
}

#define SGMCMC_WINDOW_GATHER(SFX, T)                                                                                  \
    int sgmcmc_window_gather_##SFX(const T *X, const T *y, size_t n_data, size_t start, size_t batch, size_t dim,   \
                                   T *x_out, size_t x_out_ld, T *y_out, sgmcmc_stream_t stream)                      \
    {                                                                                                                \
        if (!X || !y || !x_out || !y_out) return fail(SGMCMC_EINVAL, "window_gather: NULL argument");               \
        if (batch == 0 || start + batch > n_data) return fail(SGMCMC_EINVAL, "window_gather: window outside the data"); \
        if (x_out_ld < dim) return fail(SGMCMC_EINVAL, "window_gather: x_out_ld < dim");                             \
        const size_t total = (batch * dim) / (16 / sizeof(T)) + batch;    /* 16-byte copies: see the kernel */            \
        const size_t blocks = (total + 255) / 256;                                                                   \
        hipLaunchKernelGGL((window_gather_kernel<T>), dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, \
                           static_cast<hipStream_t>(stream), X, y, start, batch, dim, x_out, x_out_ld, y_out);       \
        return launched("window_gather");                                                                            \
    }
SGMCMC_WINDOW_GATHER(f32, float)
SGMCMC_WINDOW_GATHER(f64, double)
#undef SGMCMC_WINDOW_GATHER

size_t sgmcmc_summary_workspace_bytes(void) { return sizeof(Summary) * SUMMARY_BLOCKS; }
int sgmcmc_summary_f32(const float *x, size_t n, double *out4, void *workspace, sgmcmc_stream_t stream)
{
    return summary<float>(x, n, out4, workspace, static_cast<hipStream_t>(stream));
}
int sgmcmc_summary_f64(const double *x, size_t n, double *out4, void *workspace, sgmcmc_stream_t stream)
{
    return summary<double>(x, n, out4, workspace, static_cast<hipStream_t>(stream));
}

}  // extern "C"
