// Heston path generation by Andersen's quadratic-exponential (QE) scheme for gfx950, as stated in include/mcgpu.h
// (mcg_paths_heston_qe*): the launcher of the step rule HestonQe (heston_schemes.hpp).  The kernel around it -- draws and
// rows -- is heston_device.hpp's, shared with the Euler generator (kernels_heston.hip); stores, block walk and payoff
// partials are those of every generator (paths_device.hpp).
//
// What the scheme adds per path-step: two divisions (2/psi and m/(1 + b^2): v_rcp_f64 and two Newton steps each), two more
// square roots, and -- only in a wave where some lane has psi > psi_c -- the uniform of Philox stream 3, one more
// reciprocal and a logarithm.  Both variance branches are evaluated for the whole wave and selected per lane; what is
// skipped is skipped for the wave (a scalar branch), and since Philox is counter-based the stream-3 block of a four-step
// group is computed at the first step that needs it, or never: no bit of any path depends on which waves skipped.
#include "heston_schemes.hpp"

namespace mcg {

int launch_heston_qe(mcg_ctx* ctx, mcg_paths* P, mcg_paths* V, uint64_t seed, double S0, double r, double v0, double kappa,
                     double theta, double sigma_v, double rho, double dt, bool want_payoff, double K, int is_call) {
    const HestonQe::Consts c = HestonQe::constants(r, kappa, theta, sigma_v, rho, dt);
    return launch_heston_scheme<HestonQe>(ctx, P, V, seed, S0, v0, c, want_payoff, K, is_call);
}

}  // namespace mcg
