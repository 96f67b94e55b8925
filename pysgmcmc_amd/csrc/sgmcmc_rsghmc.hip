// sgmcmc_rsghmc.hip -- K3, the fused relativistic SGHMC step (pysgmcmc/samplers/relativistic_sghmc.py:120-140): host
// side of sgmcmc_rsghmc_step_{f32,f64} and sgmcmc_rsghmc_scalars_*. Arithmetic: RsghmcOp (sgmcmc_device.hpp); host
// sequence: step_driver (sgmcmc_step.hpp).
#include "sgmcmc_step.hpp"

namespace {

template <typename T>
struct RsghmcStep {
    typedef T real;
    static constexpr const char *who = "rsghmc_step";
    static constexpr int adapt = 0;
    T *theta, *p; const T *grad;
    T eps, mass, c, D, b_hat;
    T inv;                            // 1 / (m^2 c^2) of the by-value scalars, set by first()
    const char *refused() const { return !theta || !p || !grad ? "theta, p and grad_cost must be non-NULL" : nullptr; }
    void scalars(T (&s)[5]) const { rsghmc_scalars<T>(eps, mass, c, D, b_hat, s); }
    bool aligned() const { return aligned16(theta) && aligned16(p) && aligned16(grad); }
    // m^2 c^2 a power of two (the default m = c = 1): the divisions by it are exact multiplications (RsghmcOp POW2). Not with
    // device-resident scalars: the block may be refreshed with another mass / c after this launch was captured.
    bool first(const T (&s)[5], const T *sdev) { return rsghmc_m2c2_is_pow2<T>(s[3], inv) && sdev == nullptr; }
    static constexpr size_t elems(bool, bool INJ) { return INJ ? 6 : 5; }
    template <bool P2, bool INJ>
    RsghmcOp<T, P2, INJ> op(const StepArgs<T> &a) const
    {
        return {theta, p, grad, a.xi, a.s[0], a.s[1], a.s[2], a.s[3], a.s[4], a.grad_decay, a.nk, a.sp, a.sdev, inv};
    }
};

}  // namespace

extern "C" {

#define SGMCMC_RSGHMC(SFX, T)                                                                                           \
    int sgmcmc_rsghmc_step_##SFX(T *theta, T *p, const T *grad_cost, size_t n, T eps, T mass, T c, T D, T b_hat,        \
                                 T grad_decay, const T *xi, uint64_t seed, uint64_t step, const uint64_t *step_dev,     \
                                 void *stats_ws, const sgmcmc_step_opts_t *opts, const sgmcmc_launch_t *launch,         \
                                 sgmcmc_stream_t stream)                                                                \
    {                                                                                                                   \
        return step_driver(RsghmcStep<T>{theta, p, grad_cost, eps, mass, c, D, b_hat, T(0)}, n, grad_decay, xi, seed,   \
                           step, step_dev, stats_ws, opts, launch, stream);                                             \
    }                                                                                                                   \
    int sgmcmc_rsghmc_scalars_##SFX(T eps, T mass, T c, T D, T b_hat, void *scalars_dev, sgmcmc_stream_t stream)        \
    { T s[5]; rsghmc_scalars<T>(eps, mass, c, D, b_hat, s); return scalars_store<T>(s, scalars_dev, "rsghmc_scalars", stream); }
SGMCMC_RSGHMC(f32, float)
SGMCMC_RSGHMC(f64, double)
#undef SGMCMC_RSGHMC

}  // extern "C"
