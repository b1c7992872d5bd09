// Heston path generation by Andersen's quadratic-exponential (QE) scheme for gfx950, as stated in include/mcgpu.h
// (mcg_paths_heston_qe*).  The skeleton is that of the Euler generator (kernels_heston.hip): two adjacent paths per lane
// with S and v in registers, fm::Tables in LDS, a wave-uniform row pointer plus a fixed lane offset, one 16-byte
// nontemporal store per row and matrix.
//
// What the scheme adds per path-step: two divisions (2/psi and m/(1 + b^2): v_rcp_f64 and two Newton steps each), two more
// square roots, and -- only in a wave where some lane has psi > psi_c -- the uniform of Philox stream 3, one more
// reciprocal and a logarithm.  Both variance branches are evaluated for the whole wave and selected per lane; what is
// skipped is skipped for the wave (a scalar branch), and since Philox is counter-based the stream-3 block of a four-step
// group is computed at the first step that needs it, or never: no bit of any path depends on which waves skipped.
#include "devmath.hpp"
#include "fastmath.hpp"
#include "mcg_internal.hpp"

namespace mcg {

constexpr uint32_t STREAM_QE_UNIFORM = 3u;  // (2 belongs to the branching-process kernels)
constexpr double QE_PSI_C = 1.5;

struct HestonQeArgs {
    double* out;       // [n_steps+1][ld] prices
    double* var;       // [n_steps+1][ld] variances (VAR kernels only)
    int64_t ld;
    int64_t n_paths;
    int n_steps;
    uint64_t path_begin;
    uint32_t k0, k1;   // Philox key = seed
    double S0, v0;
    double theta;
    double E;          // exp(-kappa dt)
    double c1, c2;     // s^2 = v c1 + c2
    double drift;      // r dt + K0
    double K1, K2, K3; // (K4 = K3)
    double K;
    int is_call;
    double* partials;  // [gridDim.x][2]
    const double2* tabs;  // fm::Tables on the device
};

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
// sqrt(x) for x >= 0: fm::sqrt_pos where it holds, 0 for 0 (|rho| = 1, or v = v' = 0).
__device__ __forceinline__ double qe_sqrt_nonneg(double x) {
    const double s = fm::sqrt_pos(__builtin_fmax(x, 0x1p-1000));
    return x > 0.0 ? s : 0.0;
}

template <bool PAYOFF, bool VAR>
__global__ __launch_bounds__(256) void k_heston_qe_paths(HestonQeArgs a) {
    constexpr int PPL = 2;
    typedef double v2d __attribute__((ext_vector_type(2)));
    __shared__ fm::Tables tabs;
    fm::load_tables(&tabs, a.tabs);
    const fm::Tables* tab = &tabs;
    __syncthreads();
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PPL;  // first column of this lane
    // rows are padded to 256 columns and a workgroup covers 512: the upper two waves of the last one may lie beyond the row
    const bool in_row = i < a.ld;  // (wave-uniform)
    double S[PPL], v[PPL];
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        S[p] = a.S0;
        v[p] = a.v0;
    }
    if (in_row) {
        // The store of kernels_heston.hip, with both of its paddings: `s_nop 4` in front (the row pointer may come out of a
        // v_readlane right before it), `s_nop 1` behind (the next step's FMA overwrites the data registers).
        double* row = a.out + (int64_t)blockIdx.x * (256 * PPL);
        double* vrow = VAR ? a.var + (int64_t)blockIdx.x * (256 * PPL) : nullptr;
        const unsigned lane_bytes = threadIdx.x * (8u * PPL);
        auto store_pair = [&](double* r, const double (&x)[PPL]) {
            const v2d d = {x[0], x[1]};
            asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 nt\n\ts_nop 1" : : "v"(lane_bytes), "v"(d), "s"(r) : "memory");
        };
        store_pair(row, S);
        if (VAR) store_pair(vrow, v);
        PhiloxLane rng_s[PPL], rng_v[PPL];
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
            const uint64_t path = a.path_begin + (uint64_t)(i + p);
            rng_s[p] = philox_lane_setup(path, STREAM_PRICE, a.k1);
            rng_v[p] = philox_lane_setup(path, STREAM_VOL, a.k1);
        }
        uint32_t block = 0;    // the Philox block of the current four steps
        bool have_u = false;   // (wave-uniform) its stream-3 words are in wu
        Philox4 wu[PPL];
        // one step of both paths from their draws z1 (price driver) and z2 (volatility driver); elem = step & 3
        auto step = [&](const double (&z1)[PPL], const double (&z2)[PPL], const int elem) {
            double m[PPL], s2[PPL], m2[PPL], vn[PPL];
            bool quad[PPL];
#pragma unroll
            for (int p = 0; p < PPL; ++p) {
                m[p] = __builtin_fma(v[p] - a.theta, a.E, a.theta);
                s2[p] = __builtin_fma(v[p], a.c1, a.c2);
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
                const double s = qe_sqrt_nonneg(__builtin_fma(a.K3, vn[p], a.K3 * v[p]));
                const double e = __builtin_fma(s, z1[p], __builtin_fma(a.K2, vn[p], __builtin_fma(a.K1, v[p], a.drift)));
                S[p] = fm::scaled_exp(S[p], e);
                v[p] = vn[p];
            }
            row += a.ld;
            store_pair(row, S);
            if (VAR) {
                vrow += a.ld;
                store_pair(vrow, v);
            }
        };
        // One Philox block per stream feeds two Box-Muller pairs = four steps.  The main loop takes whole blocks; the
        // tail runs pair by pair over the last <= 3 steps.
        auto pairs = [&](const Philox4 (&ws)[PPL], const Philox4 (&wv)[PPL], bool second, double (&z1a)[PPL], double (&z1b)[PPL],
                         double (&z2a)[PPL], double (&z2b)[PPL]) {
#pragma unroll
            for (int p = 0; p < PPL; ++p) {
                fm::box_muller_pair(second ? ws[p].w2 : ws[p].w0, second ? ws[p].w3 : ws[p].w1, tab, z1a[p], z1b[p]);
                fm::box_muller_pair(second ? wv[p].w2 : wv[p].w0, second ? wv[p].w3 : wv[p].w1, tab, z2a[p], z2b[p]);
            }
        };
        auto draw = [&](Philox4 (&ws)[PPL], Philox4 (&wv)[PPL]) {
#pragma unroll
            for (int p = 0; p < PPL; ++p) {
                ws[p] = philox4x32_10_lane(rng_s[p], block, a.k0, a.k1);
                wv[p] = philox4x32_10_lane(rng_v[p], block, a.k0, a.k1);
            }
            have_u = false;
        };
        const int n_blocks = a.n_steps >> 2;
        Philox4 ws[PPL], wv[PPL];
        double z1a[PPL], z1b[PPL], z2a[PPL], z2b[PPL];
#pragma unroll 1
        for (; block < (uint32_t)n_blocks; ++block) {
            draw(ws, wv);
            pairs(ws, wv, false, z1a, z1b, z2a, z2b);
            step(z1a, z2a, 0);
            step(z1b, z2b, 1);
            pairs(ws, wv, true, z1a, z1b, z2a, z2b);
            step(z1a, z2a, 2);
            step(z1b, z2b, 3);
        }
        const int rest = a.n_steps & 3;
        if (rest) {  // wave-uniform
            draw(ws, wv);
            pairs(ws, wv, false, z1a, z1b, z2a, z2b);
            step(z1a, z2a, 0);
            if (rest >= 2) step(z1b, z2b, 1);
            if (rest == 3) {
                pairs(ws, wv, true, z1a, z1b, z2a, z2b);
                step(z1a, z2a, 2);
            }
        }
    }
    if (PAYOFF) {
        __shared__ double red[2 * 4];
        double acc[2] = {0.0, 0.0};
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
            const double pay = (in_row && i + p < a.n_paths) ? payoff_of(a.is_call != 0, S[p], a.K) : 0.0;
            acc[0] += pay;
            acc[1] += pay * pay;
        }
        block_sum<2, 4>(acc, red);
        if (threadIdx.x == 0) {
            a.partials[2 * (int64_t)blockIdx.x] = acc[0];
            a.partials[2 * (int64_t)blockIdx.x + 1] = acc[1];
        }
    }
}

int launch_heston_qe(mcg_ctx* ctx, mcg_paths* P, mcg_paths* V, uint64_t seed, double S0, double r, double v0, double kappa,
                     double theta, double sigma_v, double rho, double dt, bool want_payoff, double K, int is_call) {
    const int64_t n_blocks = (P->n_paths + 511) / 512;
    if (n_blocks > 0x7fffffffLL) return fail(MCG_ERR_INVALID, "n_paths too large for one launch");
    if ((P->ld & 255) != 0) return fail(MCG_ERR_INVALID, "path matrix rows must be padded to 256 columns");
    if (V && (V->ld != P->ld || V->n_steps != P->n_steps))
        return fail(MCG_ERR_INVALID, "the variance matrix must have the shape of the price matrix");
    if (want_payoff) {
        int rc = ensure_cap(ctx, &ctx->partials, &ctx->partials_cap, (size_t)(2 * n_blocks));
        if (rc) return rc;
    }
    // the scheme's constants (include/mcgpu.h), in binary64
    const double E = std::exp(-kappa * dt);
    const double g = kappa * rho / sigma_v - 0.5;
    HestonQeArgs a;
    a.out = P->data;
    a.var = V ? V->data : nullptr;
    a.ld = P->ld;
    a.n_paths = P->n_paths;
    a.n_steps = P->n_steps;
    a.path_begin = P->path_begin;
    a.k0 = (uint32_t)seed;
    a.k1 = (uint32_t)(seed >> 32);
    a.S0 = S0;
    a.v0 = v0;
    a.theta = theta;
    a.E = E;
    a.c1 = kappa > 0.0 ? sigma_v * sigma_v * E * (1.0 - E) / kappa : sigma_v * sigma_v * dt;
    a.c2 = kappa > 0.0 ? theta * sigma_v * sigma_v * (1.0 - E) * (1.0 - E) / (2.0 * kappa) : 0.0;
    a.drift = r * dt + -rho * kappa * theta * dt / sigma_v;
    a.K1 = dt * g / 2.0 - rho / sigma_v;
    a.K2 = dt * g / 2.0 + rho / sigma_v;
    a.K3 = dt * (1.0 - rho * rho) / 2.0;
    a.K = K;
    a.is_call = is_call;
    a.partials = ctx->partials;
    a.tabs = (const double2*)ctx->log_tab;
    {
        TimedLaunch t(ctx, MCG_K_HESTON);
        const dim3 grid((unsigned)n_blocks), block(256);
        if (want_payoff) {
            if (V) hipLaunchKernelGGL((k_heston_qe_paths<true, true>), grid, block, 0, ctx->stream, a);
            else hipLaunchKernelGGL((k_heston_qe_paths<true, false>), grid, block, 0, ctx->stream, a);
        } else {
            if (V) hipLaunchKernelGGL((k_heston_qe_paths<false, true>), grid, block, 0, ctx->stream, a);
            else hipLaunchKernelGGL((k_heston_qe_paths<false, false>), grid, block, 0, ctx->stream, a);
        }
    }
    MCG_HIP(hipGetLastError());
    if (want_payoff) {
        int rc = finish_sums(ctx, n_blocks, P->n_paths, P->sums);
        if (rc) return rc;
        P->has_sums = true;
        P->sums_K = K;
        P->sums_is_call = is_call;
    }
    return MCG_OK;
}

}  // namespace mcg
