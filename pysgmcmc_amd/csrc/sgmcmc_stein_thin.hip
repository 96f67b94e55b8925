// sgmcmc_stein_thin.hip -- K17: greedy Stein thinning of 2 .. 4096 samples from their Stein kernel matrix, behind
// include/sgmcmc_hip_thin.h. m dependent picks, each an argmin over n objectives and the addition of one matrix row.
//
// One launch, grid = batch, one workgroup per problem: the picks of a problem depend on each other, so a second workgroup
// could only help through a hand-off inside the launch, and n <= 4096 columns fit one workgroup's registers anyway. The
// workgroup has 64, 256 or 1024 threads (thin_geom); column j belongs to thread j mod block, slot j / block of that thread,
// so acc_j and h_j are CPT <= 4 registers each (CPT a template argument: every slot index is a constant) and the read of row
// j* is one coalesced element-wide load per slot. Per pick:
//   1. every thread ranks its own columns, the wave's 64 candidates are reduced by a butterfly of cross-lane moves and
//      lane 0 puts the wave's winner into the LDS                                                  -- barrier
//   2. lane l of EVERY wave takes the winner of wave l (lanes past the wave count a sentinel) and the same butterfly leaves
//      the workgroup's winner in every lane: that is the broadcast                                 -- barrier (the LDS is free)
//   3. thread 0 writes the index and the path value; every thread adds its columns of row j*.
// The order on (value, index) pairs is strict and total (a NaN is ranked as +infinity), so the winner does not depend on the
// shape of the reduction. Nothing else is waited on: no atomics, no flags, no scratch.
#include <hip/hip_runtime.h>

#include <cmath>

#include "sgmcmc_hip_thin.h"

#pragma clang fp contract(off)

#include "sgmcmc_host.hpp"

using namespace sgmcmc_host;

namespace {

constexpr int THIN_MAX_SAMPLES = 4096;
constexpr size_t THIN_MAX_PICKS = 65536, THIN_MAX_BATCH = 65535;
constexpr int THIN_WAVE = 64;
constexpr int THIN_MAX_BLOCK = 1024, THIN_MAX_WAVES = THIN_MAX_BLOCK / THIN_WAVE;
constexpr int THIN_NONE = 0x7fffffff;               // index of the sentinel: loses against every candidate

struct ThinBest {
    double v;
    int j;
};

// strict total order on pairs without a NaN: the smaller value, among equal values the smaller index
__device__ __forceinline__ bool thin_before(double va, int ja, double vb, int jb) { return va < vb || (va == vb && ja < jb); }

// the best pair of the wave, in every lane
__device__ __forceinline__ ThinBest thin_wave_best(ThinBest b) {
#pragma unroll
    for (int off = THIN_WAVE / 2; off >= 1; off >>= 1) {
        const double v = __shfl_xor(b.v, off, THIN_WAVE);
        const int j = __shfl_xor(b.j, off, THIN_WAVE);
        if (thin_before(v, j, b.v, b.j)) { b.v = v; b.j = j; }
    }
    return b;
}

template <typename T, int CPT>
__global__ void __launch_bounds__(THIN_MAX_BLOCK)
stein_thin_kernel(const T *__restrict__ matrix, size_t ld, int n, int m, size_t batch_stride, int distinct,
                  int *__restrict__ indices_out, double *__restrict__ path_out) {
    __shared__ double s_v[THIN_MAX_WAVES];
    __shared__ int s_j[THIN_MAX_WAVES];
    const int tid = threadIdx.x, block = blockDim.x, lane = tid & (THIN_WAVE - 1), wave = tid / THIN_WAVE;
    const int n_waves = block / THIN_WAVE;
    const T *K = matrix + (size_t)blockIdx.x * batch_stride;
    int *indices = indices_out + (size_t)blockIdx.x * (size_t)m;
    double *path = path_out ? path_out + (size_t)blockIdx.x * (size_t)m : nullptr;

    double h[CPT], acc[CPT];
    unsigned picked = 0;                            // bit c: the column of slot c has been picked (DISTINCT)
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
        const int j = tid + c * block;
        h[c] = j < n ? 0.5 * (double)K[(size_t)j * ld + (size_t)j] : 0.0;
        acc[c] = 0.0;
    }
    double S = 0.0;
    for (int t = 1; t <= m; ++t) {
        ThinBest b = {INFINITY, THIN_NONE};
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
            const int j = tid + c * block;
            double obj = acc[c] + h[c];
            obj = obj == obj ? obj : (double)INFINITY;
            if (j < n && !((picked >> c) & 1u) && thin_before(obj, j, b.v, b.j)) { b.v = obj; b.j = j; }
        }
        b = thin_wave_best(b);
        if (lane == 0) { s_v[wave] = b.v; s_j[wave] = b.j; }
        __syncthreads();
        if (lane < n_waves) { b.v = s_v[lane]; b.j = s_j[lane]; }
        else { b.v = INFINITY; b.j = THIN_NONE; }
        __syncthreads();
        b = thin_wave_best(b);
        // a candidate is always left (m <= n with DISTINCT), none of the values compared is a NaN and every candidate beats
        // the sentinel: 0 <= js < n whatever the matrix holds
        const int js = b.j;
        S = S + 2.0 * b.v;
        if (tid == 0) {
            indices[t - 1] = js;
            if (path) path[t - 1] = S / ((double)t * (double)t);
        }
        const T *row = K + (size_t)js * ld;
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
            const int j = tid + c * block;
            if (j < n) acc[c] = acc[c] + (double)row[j];
            if (distinct && j == js) picked |= 1u << c;
        }
    }
}

struct ThinGeom {
    int block, cpt, waves;
};

inline ThinGeom thin_geom(int n) {
    ThinGeom g;
    g.block = n <= 64 ? 64 : n <= 256 ? 256 : THIN_MAX_BLOCK;     // above 1024 columns a thread holds several
    g.cpt = (n + g.block - 1) / g.block;
    g.waves = g.block / THIN_WAVE;
    return g;
}

int thin_check_sizes(const char *who, size_t n, size_t m, size_t batch) {
    if (n < 2 || n > (size_t)THIN_MAX_SAMPLES) return fail(SGMCMC_EINVAL, "%s: n = %zu outside [2, %d]", who, n, THIN_MAX_SAMPLES);
    if (m < 1 || m > THIN_MAX_PICKS) return fail(SGMCMC_EINVAL, "%s: m = %zu outside [1, %zu]", who, m, THIN_MAX_PICKS);
    if (batch < 1 || batch > THIN_MAX_BATCH)
        return fail(SGMCMC_EINVAL, "%s: batch = %zu outside [1, %zu]", who, batch, THIN_MAX_BATCH);
    return 0;
}

template <typename T>
int thin_impl(const T *matrix, size_t ld_m, size_t n, size_t m, size_t batch, size_t batch_stride, int flags, int *indices_out,
              double *path_out, sgmcmc_stream_t stream) {
    const char *who = "stein_thin";
    if (!matrix || !indices_out) return fail(SGMCMC_EINVAL, "%s: null pointer", who);
    const int rc = thin_check_sizes(who, n, m, batch);
    if (rc) return rc;
    if (ld_m < n) return fail(SGMCMC_EINVAL, "%s: ld_m < n", who);
    if (batch > 1 && batch_stride == 0) return fail(SGMCMC_EINVAL, "%s: batch > 1 needs batch_stride > 0", who);
    if (flags & ~SGMCMC_THIN_DISTINCT) return fail(SGMCMC_EINVAL, "%s: unknown flag bits 0x%x", who, flags & ~SGMCMC_THIN_DISTINCT);
    if ((flags & SGMCMC_THIN_DISTINCT) && m > n) return fail(SGMCMC_EINVAL, "%s: DISTINCT needs m <= n, got m = %zu, n = %zu", who, m, n);

    const ThinGeom g = thin_geom((int)n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int distinct = flags & SGMCMC_THIN_DISTINCT;
#define THIN_LAUNCH(CPT)                                                                                                       \
    hipLaunchKernelGGL((stein_thin_kernel<T, CPT>), dim3((unsigned)batch), dim3(g.block), 0, st, matrix, ld_m, (int)n, (int)m, \
                       batch_stride, distinct, indices_out, path_out)
    switch (g.cpt) {
    case 1: THIN_LAUNCH(1); break;
    case 2: THIN_LAUNCH(2); break;
    case 3: THIN_LAUNCH(3); break;
    default: THIN_LAUNCH(4); break;
    }
#undef THIN_LAUNCH
    return launched("stein_thin_kernel");
}

}  // namespace

extern "C" {

int sgmcmc_stein_thin_abi_version(void) { return SGMCMC_THIN_ABI_VERSION; }

int sgmcmc_stein_thin_max_samples(void) { return THIN_MAX_SAMPLES; }

int sgmcmc_stein_thin_plan(size_t n, size_t m, size_t batch, int *out, int n_out) {
    const int rc = thin_check_sizes("stein_thin_plan", n, m, batch);
    if (rc) return rc;
    const ThinGeom g = thin_geom((int)n);
    const int v[4] = {g.block, g.cpt, (int)batch, g.waves};
    for (int k = 0; out && k < 4 && k < n_out; ++k) out[k] = v[k];
    return 1;
}

int sgmcmc_stein_thin_f32(const float *matrix, size_t ld_m, size_t n, size_t m, size_t batch, size_t batch_stride, int flags,
                          int *indices_out, double *path_out, sgmcmc_stream_t stream) {
    return thin_impl<float>(matrix, ld_m, n, m, batch, batch_stride, flags, indices_out, path_out, stream);
}

int sgmcmc_stein_thin_f64(const double *matrix, size_t ld_m, size_t n, size_t m, size_t batch, size_t batch_stride, int flags,
                          int *indices_out, double *path_out, sgmcmc_stream_t stream) {
    return thin_impl<double>(matrix, ld_m, n, m, batch, batch_stride, flags, indices_out, path_out, stream);
}

}  // extern "C"
