// sgmcmc_sghmc.hip -- K1, the fused SGHMC step (pysgmcmc/samplers/sghmc.py:165-251 + the burn-in switch
// pysgmcmc/samplers/base_classes.py:432-456): host side of sgmcmc_sghmc_step_{f32,f64} and sgmcmc_sghmc_scalars_*.
// The arithmetic is SghmcOp (sgmcmc_device.hpp), the kernel shape stream_quads_vec (sgmcmc_stream.hpp), the host
// sequence step_driver (sgmcmc_step.hpp).
#include "sgmcmc_step.hpp"

namespace {

template <typename T>
struct SghmcStep {
    typedef T real;
    static constexpr const char *who = "sghmc_step";
    T *theta, *V; const T *grad; T *tau, *g, *v_hat, *minv, *r;
    T eps, scale_grad, mdecay;
    int adapt;
    const char *refused() const
    {
        if (!theta || !V || !grad || !minv) return "theta, V, grad and minv must be non-NULL";
        return adapt && (!tau || !g || !v_hat) ? "adapt=1 needs tau, g and v_hat" : nullptr;
    }
    void scalars(T (&s)[5]) const { sghmc_scalars<T>(eps, scale_grad, mdecay, s); }
    bool aligned() const
    {
        return aligned16(theta) && aligned16(V) && aligned16(grad) && aligned16(minv) &&
               (!adapt || (aligned16(tau) && aligned16(g) && aligned16(v_hat) && aligned16(r)));
    }
    bool first(const T (&)[5], const T *) const { return adapt; }
    static constexpr size_t elems(bool AD, bool INJ) { return (AD ? 12 : 6) + (INJ ? 1 : 0); }
    template <bool AD, bool INJ>
    SghmcOp<T, AD, INJ> op(const StepArgs<T> &a) const
    {
        return {theta, V, grad, tau, g, v_hat, minv, r, a.xi, a.s[0], a.s[1], a.s[2], a.s[3], a.s[4], a.grad_decay, a.nk, a.sp,
                a.skip_minv, a.sdev};
    }
};

}  // namespace

extern "C" {

#define SGMCMC_SGHMC(SFX, T)                                                                                                     \
    int sgmcmc_sghmc_step_##SFX(T *theta, T *V, const T *grad, T *tau, T *g, T *v_hat, T *minv, T *r, size_t n, T eps,           \
                                T scale_grad, T mdecay, T grad_decay, int adapt, const T *xi, uint64_t seed, uint64_t step,      \
                                const uint64_t *step_dev, void *stats_ws, const sgmcmc_step_opts_t *opts,                        \
                                const sgmcmc_launch_t *launch, sgmcmc_stream_t stream)                                           \
    {                                                                                                                            \
        return step_driver(SghmcStep<T>{theta, V, grad, tau, g, v_hat, minv, r, eps, scale_grad, mdecay, adapt}, n, grad_decay,  \
                           xi, seed, step, step_dev, stats_ws, opts, launch, stream);                                            \
    }                                                                                                                            \
    int sgmcmc_sghmc_scalars_##SFX(T eps, T scale_grad, T mdecay, void *scalars_dev, sgmcmc_stream_t stream)                     \
    { T s[5]; sghmc_scalars<T>(eps, scale_grad, mdecay, s); return scalars_store<T>(s, scalars_dev, "sghmc_scalars", stream); }
SGMCMC_SGHMC(f32, float)
SGMCMC_SGHMC(f64, double)
#undef SGMCMC_SGHMC

}  // extern "C"
