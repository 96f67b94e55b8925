// sgmcmc_host.hpp -- host-side error reporting (and two launch helpers) shared by the translation units of
// libsgmcmc_hip.so. fail / hip_fail are defined next to sgmcmc_last_error() in sgmcmc_kernels.hip; fail() formats the
// thread-local message returned by sgmcmc_last_error() and returns `code`.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdio>

namespace sgmcmc_host {
extern thread_local char g_err[512];
int fail(int code, const char *fmt, ...);
int hip_fail(hipError_t e, const char *what);

// right after a kernel launch: 0, or the launch's error reported as "launch <name>: <HIP's text>"
inline int launched(const char *name)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    char what[96];
    snprintf(what, sizeof(what), "launch %s", name);
    return hip_fail(e, what);
}

// grid of 256-lane blocks for a grid-stride loop over n elements: one lane per element, 1 .. 2^20 blocks
inline unsigned small_grid(size_t n)
{
    size_t want = (n + 255) / 256;
    size_t cap = (size_t)1 << 20;
    return (unsigned)(want < cap ? (want ? want : 1) : cap);
}

// Compute units of the current device, queried once per device and kept. 0: no device / the query failed.
inline int current_device_cus()
{
    constexpr int MAX_DEV = 64;
    static std::atomic<int> cached[MAX_DEV];                // zero-initialised: 0 = not asked yet
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return 0;
    int cus = cached[dev].load(std::memory_order_relaxed);
    if (cus > 0) return cus;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 0;
    cached[dev].store(cus, std::memory_order_relaxed);
    return cus;
}
}  // namespace sgmcmc_host
