// The Heston path kernel for gfx950, shared by its variance schemes (kernels_heston.hip: full-truncation log-Euler;
// kernels_heston_qe.hip: Andersen's QE; kernels_bates.hip: either with compound-Poisson jumps), on the generators' skeleton
// of paths_device.hpp (row store, block walk, payoff partials): two adjacent paths per lane with S and v in registers, two
// Philox streams per path (price driver and volatility driver, philox.hpp), the price row and -- optionally -- the variance
// row stored per step, and the launcher.
//
// A scheme is a struct the kernel holds one object of (heston_schemes.hpp: the two variance schemes; bates_device.hpp: either
// of them with jumps):
//   Consts                     what the host derives from the model's parameters (HestonArgs::c; eight doubles for a variance scheme)
//   new_block(a, i, block, tab)  called once per Philox block, after the draws of its four steps
//   step(a, i, block, elem, tab, z1, z2, S, v)
//                              advances S[] and v[] in place by step 4*block + elem, from the draws z1 (price driver) and
//                              z2 (volatility driver); i = first column of this lane
// Rows, row pointers and stores belong to the kernel.
#pragma once
#include "devmath.hpp"
#include "fastmath.hpp"
#include "paths_host.hpp"
#include "paths_device.hpp"

namespace mcg {

constexpr int HESTON_PPL = 2;  // paths per lane

template <class Consts>
struct HestonArgs {
    double* out;       // [n_steps+1][ld] prices
    double* var;       // [n_steps+1][ld] variances (VAR kernels only)
    int64_t ld;
    int64_t n_paths;
    int n_steps;
    uint64_t path_begin;
    uint32_t k0, k1;   // Philox key = seed
    double S0, v0;
    Consts c;          // the scheme's constants
    double K;
    int is_call;
    double* partials;  // [gridDim.x][2]
    const double2* tabs;  // fm::Tables on the device
};

// sqrt(x) for x >= 0: fm::sqrt_pos where it holds, 0 for 0 (a truncated variance; QE: |rho| = 1, or v = v' = 0).  Below
// 2^-1000 the root is that of 2^-1000 (1e-150: nothing a price step or a variance step can see).
__device__ __forceinline__ double sqrt_nonneg(double x) {
    const double s = fm::sqrt_pos(__builtin_fmax(x, 0x1p-1000));
    return x > 0.0 ? s : 0.0;
}

// HestonArgs stays the kernel's first and only argument: a scheme may read parts of a.c straight from the kernel's argument
// block, at offsetof(HestonArgs, c) from its start (bates_device.hpp: WithJumps::rare); the static_assert there and this note
// are what holds the two together.
template <class Scheme, bool PAYOFF, bool VAR>
__global__ __launch_bounds__(256) void k_heston_paths(HestonArgs<typename Scheme::Consts> a) {
    constexpr int PPL = HESTON_PPL;
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
        // a wave-uniform row pointer that advances by ld on the scalar unit, and a lane offset that never changes
        double* row = a.out + (int64_t)blockIdx.x * (256 * PPL);
        double* vrow = VAR ? a.var + (int64_t)blockIdx.x * (256 * PPL) : nullptr;
        const unsigned lane_bytes = threadIdx.x * (8u * PPL);
        store_pair16(row, lane_bytes, S[0], S[1]);
        if (VAR) store_pair16(vrow, lane_bytes, v[0], v[1]);
        PhiloxLane rng_s[PPL], rng_v[PPL];
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
            const uint64_t path = a.path_begin + (uint64_t)(i + p);
            rng_s[p] = philox_lane_setup(path, STREAM_PRICE, a.k1);
            rng_v[p] = philox_lane_setup(path, STREAM_VOL, a.k1);
        }
        Scheme scheme;
        uint32_t block = 0;  // the Philox block of the current four steps
        Philox4 ws[PPL], wv[PPL];
        double z1a[PPL], z1b[PPL], z2a[PPL], z2b[PPL];  // z1: price driver, z2: volatility driver; a, b: the steps of a pair
        auto pairs = [&](const bool second) {
            normal_pairs(ws, second, tab, z1a, z1b);
            normal_pairs(wv, second, tab, z2a, z2b);
        };
        walk_blocks(
            a.n_steps, block,
            [&](auto) {
#pragma unroll
                for (int p = 0; p < PPL; ++p) {
                    ws[p] = philox4x32_10_lane(rng_s[p], block, a.k0, a.k1);
                    wv[p] = philox4x32_10_lane(rng_v[p], block, a.k0, a.k1);
                }
                scheme.new_block(a, i, block, tab);
                pairs(false);
            },
            [&] { pairs(true); },
            [&](auto elem) {  // one step of both paths, and its rows
                scheme.step(a, i, block, elem, tab, elem & 1 ? z1b : z1a, elem & 1 ? z2b : z2a, S, v);
                row += a.ld;
                store_pair16(row, lane_bytes, S[0], S[1]);
                if (VAR) {
                    vrow += a.ld;
                    store_pair16(vrow, lane_bytes, v[0], v[1]);
                }
            },
            [] {});
    }
    if (PAYOFF) payoff_partials(in_row, i, a.n_paths, S, a.K, a.is_call, a.partials);
}

// One launch of k_heston_paths<Scheme, ...> over P (and V: the variance matrix, or null) from the scheme's constants c.
template <class Scheme>
int launch_heston_scheme(mcg_ctx* ctx, mcg_paths* P, mcg_paths* V, uint64_t seed, double S0, double v0,
                         const typename Scheme::Consts& c, bool want_payoff, double K, int is_call) {
    const int64_t n_blocks = launch_blocks(P, HESTON_PPL);
    if (n_blocks < 0) return MCG_ERR_INVALID;
    if (V && (V->ld != P->ld || V->n_steps != P->n_steps))
        return fail(MCG_ERR_INVALID, "the variance matrix must have the shape of the price matrix");
    const PathLaunch launch{ctx, n_blocks, P, want_payoff, K, is_call};
    const int rc = launch.reserve();
    if (rc) return rc;
    HestonArgs<typename Scheme::Consts> a;
    set_shape_key(a, P, seed);
    set_payoff(a, ctx, K, is_call);
    a.var = V ? V->data : nullptr;
    a.S0 = S0;
    a.v0 = v0;
    a.c = c;
    a.tabs = (const double2*)ctx->log_tab;
    return launch.run(MCG_K_HESTON, [&] {
        dispatch_flags(
            [&](auto payoff, auto var) {
                hipLaunchKernelGGL((k_heston_paths<Scheme, payoff.value, var.value>), dim3((unsigned)n_blocks), dim3(256), 0, ctx->stream, a);
            },
            want_payoff, V != nullptr);
    });
}

}  // namespace mcg
