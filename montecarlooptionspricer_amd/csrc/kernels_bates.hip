// Bates and Merton paths for gfx950, as stated in include/mcgpu.h (mcg_paths_bates*): the Heston path kernel
// (heston_device.hpp) with the jump rule of bates_device.hpp composed onto either variance scheme, and the launcher that
// derives the rule's constants.
#include "bates_device.hpp"

namespace mcg {

void bates_constants(double lambda, double mu_j, double sigma_j, double dt, uint32_t (&T)[JUMP_CAP], double& comp) {
    const double L = lambda * dt;
    const double kbar = std::exp(mu_j + sigma_j * sigma_j / 2.0) - 1.0;
    comp = -lambda * kbar * dt;
    double t = std::exp(-L), cdf = t;
    for (int k = 0; k < JUMP_CAP; ++k) {
        if (k > 0) {
            t = t * L / k;
            cdf = cdf + t;
        }
        T[k] = (uint32_t)std::floor(std::min(cdf, 1.0) * 0x1p32 - 0.5);  // in [0, 2^32 - 1]: no word exceeds the last
    }
}

template <class Base>
static int launch_with_jumps(mcg_ctx* ctx, mcg_paths* P, mcg_paths* V, uint64_t seed, double S0, double r, double v0, double kappa,
                             double theta, double sigma_v, double rho, double lambda, double mu_j, double sigma_j, double dt,
                             bool want_payoff, double K, int is_call) {
    typename WithJumps<Base>::Consts c;
    c.base = Base::constants(r, kappa, theta, sigma_v, rho, dt);
    bates_constants(lambda, mu_j, sigma_j, dt, c.rare.T, c.comp);  // the jump constants (include/mcgpu.h), in binary64
    c.rare.mu_j = mu_j;
    c.rare.sigma_j = sigma_j;
    c.T0 = c.rare.T[0];
    c.T1 = c.rare.T[1];
    return launch_heston_scheme<WithJumps<Base>>(ctx, P, V, seed, S0, v0, c, want_payoff, K, is_call);
}

int launch_bates(mcg_ctx* ctx, mcg_paths* P, mcg_paths* V, uint64_t seed, double S0, double r, double v0, double kappa,
                 double theta, double sigma_v, double rho, double lambda, double mu_j, double sigma_j, double dt, bool qe,
                 bool want_payoff, double K, int is_call) {
    return (qe ? launch_with_jumps<HestonQe> : launch_with_jumps<HestonEuler>)(ctx, P, V, seed, S0, r, v0, kappa, theta, sigma_v, rho,
                                                                               lambda, mu_j, sigma_j, dt, want_payoff, K, is_call);
}

}  // namespace mcg
