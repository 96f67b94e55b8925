// sgmcmc_sgld.hip -- K2, the fused preconditioned SGLD step (pysgmcmc/samplers/sgld.py:149-211): host side of
// sgmcmc_sgld_step_{f32,f64} and sgmcmc_sgld_scalars_*. Arithmetic: SgldOp (sgmcmc_device.hpp); host sequence:
// step_driver (sgmcmc_step.hpp).
#include "sgmcmc_step.hpp"

namespace {

template <typename T>
struct SgldStep {
    typedef T real;
    static constexpr const char *who = "sgld_step";
    T *theta; const T *grad; T *tau, *g, *v_hat, *minv, *r;
    T eps, A, scale_grad;
    int adapt;
    const char *refused() const
    {
        if (!theta || !grad || !minv) return "theta, grad and minv must be non-NULL";
        return adapt && (!tau || !g || !v_hat) ? "adapt=1 needs tau, g and v_hat" : nullptr;
    }
    void scalars(T (&s)[5]) const { sgld_scalars<T>(eps, A, scale_grad, s); }
    bool aligned() const
    {
        return aligned16(theta) && aligned16(grad) && aligned16(minv) &&
               (!adapt || (aligned16(tau) && aligned16(g) && aligned16(v_hat) && aligned16(r)));
    }
    bool first(const T (&)[5], const T *) const { return adapt; }
    static constexpr size_t elems(bool AD, bool INJ) { return (AD ? 10 : 4) + (INJ ? 1 : 0); }
    template <bool AD, bool INJ>
    SgldOp<T, AD, INJ> op(const StepArgs<T> &a) const
    {
        return {theta, grad, tau, g, v_hat, minv, r, a.xi, a.s[0], a.s[1], a.s[2], a.s[3], a.s[4], a.grad_decay, a.nk, a.sp,
                a.skip_minv, a.sdev};
    }
};

}  // namespace

extern "C" {

#define SGMCMC_SGLD(SFX, T)                                                                                             \
    int sgmcmc_sgld_step_##SFX(T *theta, const T *grad, T *tau, T *g, T *v_hat, T *minv, T *r, size_t n, T eps, T A,    \
                               T scale_grad, T grad_decay, int adapt, const T *xi, uint64_t seed, uint64_t step,        \
                               const uint64_t *step_dev, void *stats_ws, const sgmcmc_step_opts_t *opts,                \
                               const sgmcmc_launch_t *launch, sgmcmc_stream_t stream)                                   \
    {                                                                                                                   \
        return step_driver(SgldStep<T>{theta, grad, tau, g, v_hat, minv, r, eps, A, scale_grad, adapt}, n, grad_decay,  \
                           xi, seed, step, step_dev, stats_ws, opts, launch, stream);                                   \
    }                                                                                                                   \
    int sgmcmc_sgld_scalars_##SFX(T eps, T A, T scale_grad, void *scalars_dev, sgmcmc_stream_t stream)                  \
    { T s[5]; sgld_scalars<T>(eps, A, scale_grad, s); return scalars_store<T>(s, scalars_dev, "sgld_scalars", stream); }
SGMCMC_SGLD(f32, float)
SGMCMC_SGLD(f64, double)
#undef SGMCMC_SGLD

}  // extern "C"
