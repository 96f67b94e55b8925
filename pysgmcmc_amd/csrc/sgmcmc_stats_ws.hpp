// sgmcmc_stats_ws.hpp -- device-side reader of the statistics workspace a step kernel leaves (stats_block_write in
// sgmcmc_stream.hpp writes it): float64 elements, a 32-byte header whose element 0 is the record count as a 64-bit
// unsigned integer, then block-major 32-byte records -- statistic s of record i is element 4 + 4 i + s. Statistic 0 is the
// block's share of sum(theta^2), which the BNN cost path adds up on the side of its own launches, cut into at most
// TSQ_SLICES contiguous slices that the loss head then adds in order.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int TSQ_SLICES = 16;

__device__ __forceinline__ unsigned stats_ws_records(const double *ws)
{
    return (unsigned)reinterpret_cast<const unsigned long long *>(ws)[0];
}
__device__ __forceinline__ double stats_ws_stat(const double *ws, unsigned record, int stat = 0)
{
    return (ws + 4 + stat)[4 * (size_t)record];
}

// slice b of n_slices: the records [lo, hi), ceil(nparts / n_slices) each (the last ones shorter or empty)
struct StatsSlice { unsigned lo, hi; };
__device__ __forceinline__ StatsSlice stats_ws_slice(unsigned nparts, unsigned n_slices, unsigned b)
{
    const unsigned len = (nparts + n_slices - 1) / n_slices;
    const unsigned lo = b * len;
    return {lo, (lo + len < nparts) ? lo + len : nparts};
}

}  // namespace
