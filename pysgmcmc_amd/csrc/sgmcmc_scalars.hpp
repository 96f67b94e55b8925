// sgmcmc_scalars.hpp -- the stepsize-derived scalars of the three update operators, derived on the HOST in the step's
// dtype with the op order of the reference graph. ONE derivation for every way they reach a kernel: by value (the per-step
// entry points and the whole-step kernel), through a device block (sgmcmc_*_scalars_*, StepOpts.scalars_dev) and through
// the whole-step kernel's per-step table (sgmcmc_*_scalars_steps_*), so all of them give the same bits. Anonymous namespace:
// one copy per translation unit, like sgmcmc_device.hpp. Build with -ffp-contract=off.
#pragma once
#include <cmath>

#pragma clang fp contract(off)

namespace {

// scalars of the reference graph, in the dtype, same op order (sghmc.py:111-117,211-217,235): {e2, c1, c3, e4, mdecay}
template <typename T>
void sghmc_scalars(T eps, T scale_grad, T mdecay, T (&s)[5])
{
    T eps_s = eps / std::sqrt(scale_grad);
    s[0] = std::pow(eps, T(2));
    s[1] = (T(2) * std::pow(eps_s, T(2))) * mdecay;
    s[2] = T(2) * std::pow(eps_s, T(3));
    s[3] = std::pow(eps_s, T(4));
    s[4] = mdecay;
}

// {eps, A, a_eff, two_eps, sg_den}, sgld.py:106-108,186-191,201-204
template <typename T>
void sgld_scalars(T eps, T A, T scale_grad, T (&s)[5])
{
    T sgn = (scale_grad > T(0)) ? T(1) : ((scale_grad < T(0)) ? T(-1) : T(0));
    s[0] = eps;
    s[1] = A;
    s[2] = A - T(0);
    s[3] = T(2) * eps;
    s[4] = scale_grad + ((T(2) * sgn) * T(1e-16) + T(1e-16));
}

// {eps, mass, D, m2c2, nscale}, relativistic_sghmc.py:105-106,117-125
template <typename T>
void rsghmc_scalars(T eps, T mass, T c, T D, T b_hat, T (&s)[5])
{
    s[0] = eps;
    s[1] = mass;
    s[2] = D;
    s[3] = (mass * mass) * (c * c);
    s[4] = std::sqrt(eps * ((T(2) * D) - (eps * b_hat)));
}

// m^2 c^2 a power of two (the default m = c = 1): the divisions by it are exact multiplications by `inv` (RsghmcOp POW2)
template <typename T>
bool rsghmc_m2c2_is_pow2(T m2c2, T &inv)
{
    int e2 = 0;
    inv = T(1) / m2c2;
    return m2c2 > T(0) && std::isfinite(m2c2) && std::frexp(m2c2, &e2) == T(0.5) && std::isnormal(inv) && std::isnormal(m2c2);
}

}  // namespace
