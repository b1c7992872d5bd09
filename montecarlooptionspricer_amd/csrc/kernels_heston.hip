// Heston path generation for gfx950 by the full-truncation log-Euler scheme stated in include/mcgpu.h: the launcher of the step
// rule HestonEuler (heston_schemes.hpp).  The kernel around it -- two adjacent paths per lane with S and v in registers,
// two Philox streams per path, the price row and, optionally, the variance row stored per step -- is heston_device.hpp's,
// shared with the QE generator; its row store, block walk and payoff partials are those of every generator (paths_device.hpp).
//
// Roofline: HBM write, 8*(n_steps+1) bytes per path and matrix, reads ~0.  Per path-step the kernel pays half a Philox
// block and one Box-Muller pair more than the GBM generator, a square root, and an exponential whose argument the host
// cannot bound (fm::scaled_exp: the range reduction is skipped for a wave whose 128 exponents are all small).
#include "heston_schemes.hpp"

namespace mcg {

int launch_heston(mcg_ctx* ctx, mcg_paths* P, mcg_paths* V, uint64_t seed, double S0, double r, double v0, double kappa,
                  double theta, double sigma_v, double rho, double dt, bool want_payoff, double K, int is_call) {
    const HestonEuler::Consts c = HestonEuler::constants(r, kappa, theta, sigma_v, rho, dt);
    return launch_heston_scheme<HestonEuler>(ctx, P, V, seed, S0, v0, c, want_payoff, K, is_call);
}

}  // namespace mcg
