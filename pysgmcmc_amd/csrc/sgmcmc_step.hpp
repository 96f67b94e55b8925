// sgmcmc_step.hpp -- the ONE host-side driver behind sgmcmc_{sghmc,sgld,rsghmc}_step_* and the store behind
// sgmcmc_*_scalars_*. Included by the three per-sampler translation units only. Each describes its operator to step_driver
// (SghmcStep / SgldStep / RsghmcStep there): `who` in front of every error text; refused() = the text behind it when a
// required pointer (first) or an array of adapt=1 is missing; scalars(s) = its five derived scalars; aligned() = its own
// arrays allow 16-byte accesses; first(s, sdev) = the first of its two template flags (the second is INJECT = xi given);
// elems(F, INJ) = elements streamed per parameter; op<F, INJ>(a) = the operator struct, filled field for field.
#pragma once
#include <cmath>

#include "sgmcmc_scalars.hpp"
#include "sgmcmc_stream.hpp"

namespace {

// what every step operator takes besides its own arrays
template <typename T>
struct StepArgs { const T *xi, *sdev; T grad_decay; NoiseKey nk; double *sp; bool skip_minv; T s[5]; };

// f(bool_constant<a>, bool_constant<b>): the four instantiations of a two-flag operator
template <typename F>
int dispatch2(bool a, bool b, F &&f)
{
    using Y = std::true_type;
    using N = std::false_type;
    return a ? (b ? f(Y{}, Y{}) : f(Y{}, N{})) : (b ? f(N{}, Y{}) : f(N{}, N{}));
}

template <typename D, typename T = typename D::real>
int step_driver(D d, size_t n, T grad_decay, const T *xi, uint64_t seed, uint64_t step, const uint64_t *step_dev, void *stats_ws,
                const sgmcmc_step_opts_t *opts, const sgmcmc_launch_t *lc, sgmcmc_stream_t stream)
{
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) return 0;
    if (const char *why = d.refused()) return fail(SGMCMC_EINVAL, "%s: %s", D::who, why);
    StepExtras<T> se;
    uint64_t first = 0;
    if (int rc = resolve_step_opts<T>(opts, n, stats_ws, se, first, D::who)) return rc;
    StepArgs<T> a{xi, opts ? static_cast<const T *>(opts->scalars_dev) : nullptr, grad_decay, make_key(seed, step, step_dev, first),
                  static_cast<double *>(stats_ws), d.adapt && opts && (opts->flags & SGMCMC_STEP_SKIP_MINV_STORE), {}};
    d.scalars(a.s);
    const bool vec_ok = d.aligned() && aligned16(xi) && aligned16(se.ex.mom_mean) && aligned16(se.ex.mom_m2);
    bool mom_done = false, copy_done = false;
    se.copy_done = &copy_done;
    int rc = dispatch2(d.first(a.s, a.sdev), xi != nullptr, [&](auto F, auto INJ) {
        constexpr bool f = decltype(F)::value, inj = decltype(INJ)::value;
        auto op = d.template op<f, inj>(a);
        return launch<decltype(op), !inj>(op, n, vec_ok, sizeof(T) * D::elems(f, inj), lc, se, &mom_done, st);
    });
    if (rc == 0 && se.want_moments && !mom_done) {        // no fused form for this path: the separate K4 pass, same arithmetic
        MomentsOp<T> mop{d.theta, se.ex.mom_mean, se.ex.mom_m2, se.ex.mom_inv};
        sgmcmc_launch_t lc_mom = lc ? *lc : sgmcmc_launch_t{};      // same geometry, but NOT the caller's timestamp events: they
        lc_mom.start_event = lc_mom.stop_event = nullptr;           // belong to the step kernel above
        rc = launch(mop, n, aligned16(d.theta) && aligned16(se.ex.mom_mean) && aligned16(se.ex.mom_m2), 5 * sizeof(T), lc ? &lc_mom : nullptr, st);
    }
    if (rc == 0) rc = finish_side_copy<T>(se, copy_done, st);      // opts.gather_* on a path without a fused form
    return rc;
}

template <typename T>
__global__ void store_scalars5(T *dst, T a, T b, T c, T d, T e) { dst[0] = a; dst[1] = b; dst[2] = c; dst[3] = d; dst[4] = e; }

// sgmcmc_*_scalars_*: the derived scalars `s` into the device block `dst` (sgmcmc_step_opts_t.scalars_dev)
template <typename T>
int scalars_store(const T (&s)[5], void *dst, const char *who, sgmcmc_stream_t stream)
{
    if (!dst) return fail(SGMCMC_EINVAL, "%s: scalars_dev is NULL", who);
    hipLaunchKernelGGL((store_scalars5<T>), dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), static_cast<T *>(dst), s[0], s[1], s[2], s[3], s[4]);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, "launch store_scalars");
}

}  // namespace
