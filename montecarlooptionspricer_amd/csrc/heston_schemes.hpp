// The step rules of the Heston path kernel (heston_device.hpp): the full-truncation log-Euler scheme and Andersen's QE
// scheme, as stated in include/mcgpu.h.  kernels_heston.hip and kernels_heston_qe.hip instantiate the kernel with them as they
// stand; bates_device.hpp composes a jump rule onto either.  For that a step finds its scheme's constants through
// consts_of (a composed scheme's HestonArgs::c holds them as its part `base`) and takes, optionally, a last argument
// `plus(p, e)` that returns the exponent the price of path p takes, given the scheme's own e; left out, it is e.
#pragma once
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "heston_device.hpp"

namespace mcg {

// The constants of scheme S in HestonArgs::c: c itself, or c.base where S is the base of a composed scheme.
template <class S, class C>
__device__ __forceinline__ const typename S::Consts& consts_of(const C& c) {
    if constexpr (std::is_same_v<C, typename S::Consts>) return c;
    else return c.base;
}

struct SameExponent {
    __device__ __forceinline__ double operator()(int, double e) const { return e; }
};

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
    static Consts constants(double r, double kappa, double theta, double sigma_v, double rho, double dt) {
        Consts c;
        c.r_dt = r * dt;
        c.half_dt = -0.5 * dt;
        c.dt = dt;
        c.kappa_dt = kappa * dt;
        c.theta = theta;
        c.sigma_v = sigma_v;
        c.rho = rho;
        c.rho_c = std::sqrt(std::max(0.0, 1.0 - rho * rho));
        return c;
    }
    template <class Args>
    __device__ __forceinline__ void new_block(const Args&, int64_t, uint32_t, const fm::Tables*) {}
    template <class Args, class Plus = SameExponent>
    __device__ __forceinline__ void step(const Args& a, int64_t, uint32_t, int, const fm::Tables*,
                                         const double (&z1)[PPL], const double (&z2)[PPL], double (&S)[PPL], double (&v)[PPL],
                                         const Plus& plus = Plus()) {
        const Consts& c = consts_of<HestonEuler>(a.c);
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
            const double vp = __builtin_fmax(v[p], 0.0);
            const double s = sqrt_nonneg(vp * c.dt);
            const double w = __builtin_fma(c.rho, z2[p], c.rho_c * z1[p]);
            const double e = __builtin_fma(s, w, __builtin_fma(c.half_dt, vp, c.r_dt));
            S[p] = fm::scaled_exp(S[p], plus(p, e));
            v[p] = __builtin_fma(c.sigma_v * s, z2[p], __builtin_fma(c.kappa_dt, c.theta - vp, v[p]));
        }
    }
};

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
    // the scheme's constants (include/mcgpu.h), in binary64
    static Consts constants(double r, double kappa, double theta, double sigma_v, double rho, double dt) {
        const double E = std::exp(-kappa * dt);
        const double g = kappa * rho / sigma_v - 0.5;
        Consts c;
        // kappa = 0: m = v exactly.  theta + (v - theta) rounds at the size of theta, and a step from v << theta then carries
        // that into ln(1 / m^2) of the exponential branch (2e-12 of S' at v = 1e-8, theta = 0.04); theta enters nothing else here.
        c.theta = kappa > 0.0 ? theta : 0.0;
        c.E = E;
        c.c1 = kappa > 0.0 ? sigma_v * sigma_v * E * (1.0 - E) / kappa : sigma_v * sigma_v * dt;
        c.c2 = kappa > 0.0 ? theta * sigma_v * sigma_v * (1.0 - E) * (1.0 - E) / (2.0 * kappa) : 0.0;
        c.drift = r * dt + -rho * kappa * theta * dt / sigma_v;
        c.K1 = dt * g / 2.0 - rho / sigma_v;
        c.K2 = dt * g / 2.0 + rho / sigma_v;
        c.K3 = dt * (1.0 - rho * rho) / 2.0;
        return c;
    }
    bool have_u = false;   // (wave-uniform) the block's stream-3 words are in wu
    Philox4 wu[PPL];
    template <class Args>
    __device__ __forceinline__ void new_block(const Args&, int64_t, uint32_t, const fm::Tables*) { have_u = false; }
    template <class Args, class Plus = SameExponent>
    __device__ __forceinline__ void step(const Args& a, const int64_t i, const uint32_t block, const int elem,
                                         const fm::Tables* tab, const double (&z1)[PPL], const double (&z2)[PPL],
                                         double (&S)[PPL], double (&v)[PPL], const Plus& plus = Plus()) {
        const Consts& c = consts_of<HestonQe>(a.c);
        double m[PPL], s2[PPL], m2[PPL], vn[PPL];
        bool quad[PPL];
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
            m[p] = __builtin_fma(v[p] - c.theta, c.E, c.theta);
            s2[p] = __builtin_fma(v[p], c.c1, c.c2);
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
            const double s = sqrt_nonneg(__builtin_fma(c.K3, vn[p], c.K3 * v[p]));
            const double e = __builtin_fma(s, z1[p], __builtin_fma(c.K2, vn[p], __builtin_fma(c.K1, v[p], c.drift)));
            S[p] = fm::scaled_exp(S[p], plus(p, e));
            v[p] = vn[p];
        }
    }
};

}  // namespace mcg
