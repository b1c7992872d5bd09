// Heston path generation for gfx950 by the full-truncation log-Euler scheme stated in include/mcgpu.h: the step rule, and
// the launcher that derives its constants.  The kernel around it -- two adjacent paths per lane with S and v in registers,
// two Philox streams per path, step-major 16-byte nontemporal stores of the price row and, optionally, of the variance row,
// the terminal payoff partials of the fused form -- is heston_device.hpp's, shared with the QE generator.
//
// Roofline: HBM write, 8*(n_steps+1) bytes per path and matrix, reads ~0.  Per path-step the kernel pays half a Philox
// block and one Box-Muller pair more than the GBM generator, a square root, and an exponential whose argument the host
// cannot bound (fm::scaled_exp: the range reduction is skipped for a wave whose 128 exponents are all small).
#include "heston_device.hpp"

namespace mcg {

// The full-truncation log-Euler step: stateless.
struct HestonEuler {
    static constexpr int PPL = HESTON_PPL;
    struct Consts {
        double r_dt;       // r dt
        double half_dt;    // -dt / 2
        double dt;
        double kappa_dt;   // kappa dt
        double theta;
        double sigma_v;
        double rho, rho_c; // rho, sqrt(1 - rho^2)
    };
    __device__ __forceinline__ void new_block() {}
    __device__ __forceinline__ void step(const HestonArgs<Consts>& a, int64_t, uint32_t, int, const fm::Tables*, const double (&z1)[PPL],
                                         const double (&z2)[PPL], double (&S)[PPL], double (&v)[PPL]) {
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
            const double vp = __builtin_fmax(v[p], 0.0);
            const double s = sqrt_nonneg(vp * a.c.dt);
            const double w = __builtin_fma(a.c.rho, z2[p], a.c.rho_c * z1[p]);
            const double e = __builtin_fma(s, w, __builtin_fma(a.c.half_dt, vp, a.c.r_dt));
            S[p] = fm::scaled_exp(S[p], e);
            v[p] = __builtin_fma(a.c.sigma_v * s, z2[p], __builtin_fma(a.c.kappa_dt, a.c.theta - vp, v[p]));
        }
    }
};

int launch_heston(mcg_ctx* ctx, mcg_paths* P, mcg_paths* V, uint64_t seed, double S0, double r, double v0, double kappa,
                  double theta, double sigma_v, double rho, double dt, bool want_payoff, double K, int is_call) {
    HestonEuler::Consts c;
    c.r_dt = r * dt;
    c.half_dt = -0.5 * dt;
    c.dt = dt;
    c.kappa_dt = kappa * dt;
    c.theta = theta;
    c.sigma_v = sigma_v;
    c.rho = rho;
    c.rho_c = std::sqrt(std::max(0.0, 1.0 - rho * rho));
    return launch_heston_scheme<HestonEuler>(ctx, P, V, seed, S0, v0, c, want_payoff, K, is_call);
}

}  // namespace mcg
