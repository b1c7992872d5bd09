// Heston path generation by Andersen's quadratic-exponential (QE) scheme for gfx950, as stated in include/mcgpu.h
// (mcg_paths_heston_qe*): the step rule, and the launcher that derives its constants.  The kernel around it -- draws,
// rows, stores, payoff partials -- is heston_device.hpp's, shared with the Euler generator (kernels_heston.hip).
//
// What the scheme adds per path-step: two divisions (2/psi and m/(1 + b^2): v_rcp_f64 and two Newton steps each), two more
// square roots, and -- only in a wave where some lane has psi > psi_c -- the uniform of Philox stream 3, one more
// reciprocal and a logarithm.  Both variance branches are evaluated for the whole wave and selected per lane; what is
// skipped is skipped for the wave (a scalar branch), and since Philox is counter-based the stream-3 block of a four-step
// group is computed at the first step that needs it, or never: no bit of any path depends on which waves skipped.
#include "heston_device.hpp"

namespace mcg {

constexpr uint32_t STREAM_QE_UNIFORM = 3u;  // (2 belongs to the branching-process kernels)
constexpr double QE_PSI_C = 1.5;

// 1/d for a positive normal d: v_rcp_f64 (~2^-26) and two Newton steps.
__device__ __forceinline__ double qe_rcp(double d) {
    double x = __builtin_amdgcn_rcp(d);
    x = __builtin_fma(x, __builtin_fma(-d, x, 1.0), x);
    x = __builtin_fma(x, __builtin_fma(-d, x, 1.0), x);
    return x;
}
// n/d from that reciprocal and one correction of the quotient (<= 1 ulp; no scaling: the operands are far from the
// ends of the exponent range).
__device__ __forceinline__ double qe_div(double n, double d) {
    const double x = qe_rcp(d);
    const double q = n * x;
    return __builtin_fma(__builtin_fma(-d, q, n), x, q);
}

// The QE step.  Its state: the stream-3 words of the current Philox block, once some step of the block has needed them.
struct HestonQe {
    static constexpr int PPL = HESTON_PPL;
    struct Consts {
        double theta;
        double E;          // exp(-kappa dt)
        double c1, c2;     // s^2 = v c1 + c2
        double drift;      // r dt + K0
        double K1, K2, K3; // (K4 = K3)
    };
    bool have_u = false;   // (wave-uniform) the block's stream-3 words are in wu
    Philox4 wu[PPL];
    __device__ __forceinline__ void new_block() { have_u = false; }
    __device__ __forceinline__ void step(const HestonArgs<Consts>& a, const int64_t i, const uint32_t block, const int elem,
                                         const fm::Tables* tab, const double (&z1)[PPL], const double (&z2)[PPL], double (&S)[PPL],
                                         double (&v)[PPL]) {
        double m[PPL], s2[PPL], m2[PPL], vn[PPL];
        bool quad[PPL];
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
            m[p] = __builtin_fma(v[p] - a.c.theta, a.c.E, a.c.theta);
            s2[p] = __builtin_fma(v[p], a.c.c1, a.c.c2);
            m2[p] = m[p] * m[p];
            quad[p] = s2[p] <= QE_PSI_C * m2[p];  // psi <= psi_c (and m = 0, where s2 = 0)
            // the quadratic branch; a lane outside it (q < 4/3, or 0/0) gets a NaN that the select below drops
            const double q = qe_div(m2[p] + m2[p], s2[p]);  // 2 / psi
            const double q1 = q - 1.0;
            const double b2 = q1 + fm::sqrt_pos(q * q1);
            const double t = fm::sqrt_pos(b2) + z2[p];
            vn[p] = qe_div(m[p], 1.0 + b2) * (t * t);
        }
        // the exponential branch, for the wave in which some lane takes it
        if (__builtin_amdgcn_ballot_w64(!(quad[0] && quad[1])) != 0ull) {
            asm volatile("" ::);  // keep this a real (scalar) branch
            if (!have_u) {
#pragma unroll
                for (int p = 0; p < PPL; ++p)  // (the per-path part is set up again here rather than held in registers)
                    wu[p] = philox4x32_10_lane(philox_lane_setup(a.path_begin + (uint64_t)(i + p), STREAM_QE_UNIFORM, a.k1), block,
                                               a.k0, a.k1);
                have_u = true;
            }
#pragma unroll
            for (int p = 0; p < PPL; ++p) {
                const uint32_t w = elem == 0 ? wu[p].w0 : elem == 1 ? wu[p].w1 : elem == 2 ? wu[p].w2 : wu[p].w3;
                const double u = __builtin_fma((double)w, 0x1p-32, 0x1p-33);  // exact
                const double d = s2[p] + m2[p];                // p = (s2 - m2) / d,  1 - p = 2 m2 / d
                const double rm = qe_rcp(m[p]);
                const double ibeta = 0.5 * d * rm;             // 1 / beta = m / (1 - p)
                const double y = (1.0 - u) * ibeta * rm;       // (1 - u) / (1 - p), below 1 where u > p
                const double lg = __builtin_fmax(0.5 * fm::neg2log(y, tab->log), 0.0);
                double ve = u * d <= s2[p] - m2[p] ? 0.0 : lg * ibeta;  // u <= p: the mass at zero
                asm volatile("" : "+v"(ve));  // (a select per lane: hipcc otherwise sinks half of the logarithm into a divergent branch)
                vn[p] = quad[p] ? vn[p] : ve;
            }
        }
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
            vn[p] = m[p] > 0.0 ? vn[p] : 0.0;
            const double s = sqrt_nonneg(__builtin_fma(a.c.K3, vn[p], a.c.K3 * v[p]));
            const double e = __builtin_fma(s, z1[p], __builtin_fma(a.c.K2, vn[p], __builtin_fma(a.c.K1, v[p], a.c.drift)));
            S[p] = fm::scaled_exp(S[p], e);
            v[p] = vn[p];
        }
    }
};

int launch_heston_qe(mcg_ctx* ctx, mcg_paths* P, mcg_paths* V, uint64_t seed, double S0, double r, double v0, double kappa,
                     double theta, double sigma_v, double rho, double dt, bool want_payoff, double K, int is_call) {
    // the scheme's constants (include/mcgpu.h), in binary64
    const double E = std::exp(-kappa * dt);
    const double g = kappa * rho / sigma_v - 0.5;
    HestonQe::Consts c;
    c.theta = theta;
    c.E = E;
    c.c1 = kappa > 0.0 ? sigma_v * sigma_v * E * (1.0 - E) / kappa : sigma_v * sigma_v * dt;
    c.c2 = kappa > 0.0 ? theta * sigma_v * sigma_v * (1.0 - E) * (1.0 - E) / (2.0 * kappa) : 0.0;
    c.drift = r * dt + -rho * kappa * theta * dt / sigma_v;
    c.K1 = dt * g / 2.0 - rho / sigma_v;
    c.K2 = dt * g / 2.0 + rho / sigma_v;
    c.K3 = dt * (1.0 - rho * rho) / 2.0;
    return launch_heston_scheme<HestonQe>(ctx, P, V, seed, S0, v0, c, want_payoff, K, is_call);
}

}  // namespace mcg
