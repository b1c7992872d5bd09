// Sobol' paths with a Brownian bridge for gfx950 (include/mcgpu.h: mcg_paths_gbm_sobol*, mcg_paths_localvol_sobol*).
//
// k_sobol_paths<PAYOFF, MODEL, BRIDGE> stands on the generators' skeleton of paths_device.hpp (row store, payoff partials,
// launch_blocks): two adjacent paths per lane with S (and, for local volatility, the running log-moneyness X) in registers,
// fm::scaled_exp for the price, rows in time order behind a moving row pointer.
//
// What is new:
//   the draw   dimension d of the lane's two Sobol' points: the XOR of the direction numbers V'[d][b] over the set bits of the
//              path id's Gray code, then the shift, then Phi^-1 (devmath.hpp: sobol_normal).  A dimension is wave-uniform, so
//              its 32 direction numbers and its shift come through scalar loads; a launch whose ids stay below 2^(8k) reads
//              the first 8k of them only (the terms of the higher bits are zero: the same bits for any path_begin).
//   the walk   BRIDGE: paths_device.hpp's walk_bridge over the program the host flattened from mcg_sobol_bridge's schedule;
//              the live bridge values sit in LDS, 16 bytes per lane and tree level, private to the lane: no barrier.
//              Otherwise dimension t is step t.
//   the table  MODEL 2 (a surface with a time axis) gathers from the table in global memory (L2); MODEL 1 (one slice) stages
//              its slice in LDS once, as k_localvol_paths does.
// No Philox, no Box-Muller, hence no fm::Tables in LDS.
//
// Roofline: HBM write, 8 B per path-step, but the kernel is VALU-bound: per path-step up to 32 masked XORs and a Phi^-1
// (two 7th-degree rationals, or a logarithm, a root and one) on top of the step itself.
#include <cstring>

#include "devmath.hpp"
#include "fastmath.hpp"
#include "localvol_device.hpp"
#include "paths_host.hpp"
#include "paths_device.hpp"

namespace mcg {

int sobol_check(const mcg_sobol* s);  // host/sobol.cpp

constexpr int SB_PPL = 2;  // paths per lane
enum : int { SB_GBM = 0, SB_LV_ONE_SLICE = 1, SB_LV_SURFACE = 2 };
typedef const uint32_t __attribute__((address_space(4))) * sobol_words;  // wave-uniform reads: scalar loads

struct SobolArgs {
    LocalVolArgs p;       // shape, S0, the payoff and (local volatility) what localvol_step reads; no Philox key, no tables
    double gm, gs;        // GBM: (r - sigma^2 / 2) dt, sigma sqrt(dt)
    const uint32_t* v;    // [n_steps][32] direction numbers, scrambled or not
    const uint32_t* shift;  // [n_steps]
    const BridgeOp* prog;   // [n_ops] (BRIDGE)
    int n_ops;
    int n_bits;           // the path ids of this launch are below 2^n_bits
};

// The normals of dimension d of the two points whose Gray codes are g.
__device__ __forceinline__ void sobol_pair(sobol_words v, sobol_words shift, const int d, const int n_bits, const uint32_t (&g)[SB_PPL],
                                           double (&z)[SB_PPL]) {
    sobol_words vd = v + d * 32;
    uint32_t x[SB_PPL];
#pragma unroll
    for (int p = 0; p < SB_PPL; ++p) x[p] = shift[d];
#pragma unroll
    for (int group = 0; group < 4; ++group) {
        if (8 * group < n_bits) {  // (wave-uniform)
#pragma unroll
            for (int b = 8 * group; b < 8 * group + 8; ++b) {
                const uint32_t w = vd[b];
#pragma unroll
                for (int p = 0; p < SB_PPL; ++p) x[p] ^= w & (0u - ((g[p] >> b) & 1u));
            }
        }
    }
#pragma unroll
    for (int p = 0; p < SB_PPL; ++p) z[p] = sobol_normal(x[p]);
}

template <bool PAYOFF, int MODEL, bool BRIDGE>
__global__ __launch_bounds__(256) void k_sobol_paths(SobolArgs a) {
    constexpr int PPL = SB_PPL;
    __shared__ double2 bridge[BRIDGE ? BRIDGE_SLOTS * 256 : 1];
    __shared__ double2 slice[MODEL == SB_LV_ONE_SLICE ? LOCALVOL_MAX_NX - 1 : 1];
    if (MODEL == SB_LV_ONE_SLICE) {
        if ((int)threadIdx.x < a.p.nx1) slice[threadIdx.x] = a.p.surf[threadIdx.x];
        __syncthreads();
    }
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PPL;  // first column of this lane
    // rows are padded to 256 columns and a workgroup covers 512: the upper two waves of the last one may lie beyond the row
    const bool in_row = i < a.p.ld;  // (wave-uniform)
    double S[PPL], X[PPL];
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        S[p] = a.p.S0;
        X[p] = 0.0;
    }
    if (in_row) {
        double* row = a.p.out + (int64_t)blockIdx.x * (256 * PPL);
        const unsigned lane_bytes = threadIdx.x * (8u * PPL);
        store_pair16(row, lane_bytes, S[0], S[1]);
        uint32_t g[PPL];
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
            const uint32_t id = (uint32_t)(a.p.path_begin + (uint64_t)(i + p));
            g[p] = id ^ (id >> 1);
        }
        const sobol_words v = (sobol_words)a.v, shift = (sobol_words)a.shift;
        auto draw = [&](const int d, double (&z)[PPL]) { sobol_pair(v, shift, d, a.n_bits, g, z); };
        auto step = [&](const int t, const double (&dz)[PPL]) {
            if constexpr (MODEL == SB_GBM) {
#pragma unroll
                for (int p = 0; p < PPL; ++p) S[p] = fm::scaled_exp(S[p], __builtin_fma(a.gs, dz[p], a.gm));
            } else {
                const double2* sl = MODEL == SB_LV_ONE_SLICE ? slice : a.p.surf + (size_t)t * a.p.nx1;
#pragma unroll
                for (int p = 0; p < PPL; ++p) localvol_step(a.p, sl, dz[p], S[p], X[p]);
            }
            row += a.p.ld;
            store_pair16(row, lane_bytes, S[0], S[1]);
        };
        if (BRIDGE) {
            walk_bridge(a.n_ops, (bridge_program)a.prog, bridge + threadIdx.x, draw, step);
        } else {
#pragma unroll 1
            for (int t = 0; t < a.p.n_steps; ++t) {
                double z[PPL];
                draw(t, z);
                step(t, z);
            }
        }
    }
    if (PAYOFF) payoff_partials(in_row, i, a.p.n_paths, S, a.p.K, a.p.is_call, a.p.partials);
}

// mcg_sobol_bridge's schedule (bridge = 1) as the program of walk_bridge: the nodes in the order of the depth-first walk, each
// with the slots of its parents and of itself and the unit intervals it closes.  m = (l + r) / 2 rounds down, so the left
// interval is never the longer one: where the right one is a unit interval the left one is too, and both steps follow their
// node at once, in time order.
static int bridge_program_of(int n, std::vector<BridgeOp>& prog) {
    std::vector<mcg_bridge_node> sched((size_t)n);
    int rc = mcg_sobol_bridge(n, 1, sched.data());
    if (rc) return rc;
    std::vector<int> dim_of((size_t)n + 1, -1);
    for (int d = 0; d < n; ++d) dim_of[(size_t)sched[(size_t)d].t] = d;
    prog.clear();
    prog.reserve((size_t)n);
    bool ok = true;
    int steps = 0;  // unit intervals closed: each one is a row stored
    auto emit = [&](int t, int sl, int sr, int so, bool left_unit, bool right_unit) {
        if (so >= BRIDGE_SLOTS || dim_of[(size_t)t] < 0) {
            ok = false;
            return;
        }
        const mcg_bridge_node& e = sched[(size_t)dim_of[(size_t)t]];
        BridgeOp op;
        op.wl = e.wl;
        op.wr = e.wr;
        op.sd = e.sd;
        op.dim_t = (uint32_t)dim_of[(size_t)t] | ((uint32_t)t << 16);
        const uint32_t closes = (left_unit ? 1u : 0u) | (right_unit ? 2u : 0u);
        op.slots = (uint32_t)sl | ((uint32_t)sr << 4) | ((uint32_t)so << 8) | (closes << 12);
        steps += (int)left_unit + (int)right_unit;
        prog.push_back(op);
    };
    // the endpoint: both parents are B(0) with weight 0; with n = 1 it closes [0, 1] itself
    emit(n, 0, 0, 1, n == 1, false);
    struct Frame {
        int l, r, sl, sr, depth;
    };
    std::vector<Frame> stack;
    stack.push_back({0, n, 0, 1, 0});
    while (!stack.empty()) {
        const Frame f = stack.back();
        stack.pop_back();
        if (f.r - f.l < 2) continue;
        const int m = (f.l + f.r) / 2, so = f.depth + 2;
        emit(m, f.sl, f.sr, so, m - f.l == 1, f.r - m == 1);
        stack.push_back({m, f.r, so, f.sr, f.depth + 1});  // (popped second: the right child)
        stack.push_back({f.l, m, f.sl, so, f.depth + 1});
    }
    if (!ok || (int)prog.size() != n || steps != n) return fail(MCG_ERR_INVALID, "sobol: no bridge program for %d steps", n);
    return MCG_OK;
}

// One launch of k_sobol_paths over P.  lv: the local-volatility model (scalars, n_x, table of n_slices slices on the host), or
// null for GBM with (gm, gs).  Direction numbers, shifts, program and table go into the ctx's cached buffer on the ctx's stream
// ahead of the launch.
int launch_sobol(mcg_ctx* ctx, mcg_paths* P, const mcg_sobol* sobol, double S0, double gm, double gs, const LocalVolScalars* lv,
                 int n_x, const double* table, int n_slices, bool want_payoff, double K, int is_call) {
    const int64_t n_blocks = launch_blocks(P, SB_PPL);
    if (n_blocks < 0) return MCG_ERR_INVALID;
    const int n = P->n_steps;
    if (n < 1 || n > MCG_SOBOL_MAX_DIMS || P->path_begin + (uint64_t)P->n_paths > (1ull << 32))
        return fail(MCG_ERR_INVALID, "sobol: %d steps of paths from %llu do not fit the point set", n, (unsigned long long)P->path_begin);
    if (lv && (n_x < 2 || n_x > LOCALVOL_MAX_NX || (n_slices != 1 && n_slices != n)))
        return fail(MCG_ERR_INVALID, "local vol: a table of %d slices x %d nodes does not fit %d steps", n_slices, n_x, n);
    std::vector<BridgeOp> prog;
    if (sobol->bridge) {
        const int rc = bridge_program_of(n, prog);
        if (rc) return rc;
    }
    // the upload, in doubles: table | program | direction numbers | shifts
    const size_t table_doubles = lv ? (size_t)n_slices * (size_t)(n_x - 1) * 2 : 0;
    const size_t prog_doubles = prog.size() * (sizeof(BridgeOp) / sizeof(double));
    const size_t v_doubles = (size_t)n * 16, shift_doubles = ((size_t)n + 1) / 2;
    std::vector<double> host(table_doubles + prog_doubles + v_doubles + shift_doubles, 0.0);
    double* h_prog = host.data() + table_doubles;
    double* h_v = h_prog + prog_doubles;
    double* h_shift = h_v + v_doubles;
    if (table_doubles) std::copy(table, table + table_doubles, host.data());
    if (!prog.empty()) memcpy(h_prog, prog.data(), prog.size() * sizeof(BridgeOp));
    int rc = mcg_sobol_table(sobol, n, (uint32_t*)h_v, (uint32_t*)h_shift);
    if (rc) return rc;
    const PathLaunch launch{ctx, n_blocks, P, want_payoff, K, is_call};
    rc = launch.reserve();
    if (rc) return rc;
    HostPiece up[] = {{host.data(), host.size() * sizeof(double)}};
    rc = upload_params(ctx, up);
    if (rc) return rc;
    MCG_HIP(hipStreamSynchronize(ctx->stream));  // `host` dies at return (upload_params)
    const uint64_t last = P->path_begin + (uint64_t)P->n_paths - 1;  // (n_paths > 0: the callers launch nothing otherwise)
    int n_bits = 0;
    while (n_bits < 32 && (last >> n_bits) != 0) ++n_bits;
    SobolArgs a{};
    set_shape_key(a.p, P, 0);  // (no Philox key)
    set_payoff(a.p, ctx, K, is_call);
    a.p.nx1 = lv ? n_x - 1 : 1;
    a.p.S0 = S0;
    if (lv) {
        a.p.inv_dx = lv->inv_dx;
        a.p.u0 = lv->u0;
        a.p.m = lv->m;
        a.p.u_max = (double)(n_x - 1);
    }
    a.p.surf = (const double2*)up[0].at;
    a.gm = gm;
    a.gs = gs;
    a.prog = (const BridgeOp*)(up[0].at + table_doubles);
    a.v = (const uint32_t*)(up[0].at + table_doubles + prog_doubles);
    a.shift = (const uint32_t*)(up[0].at + table_doubles + prog_doubles + v_doubles);
    a.n_ops = (int)prog.size();
    a.n_bits = n_bits;
    const int model = !lv ? SB_GBM : n_slices == 1 ? SB_LV_ONE_SLICE : SB_LV_SURFACE;
    return launch.run(MCG_K_SOBOL, [&] {
        const dim3 grid((unsigned)n_blocks), block(256);
        dispatch_flags(
            [&](auto payoff, auto bridge) {
                constexpr bool PAY = payoff.value, BR = bridge.value;
                if (model == SB_GBM) hipLaunchKernelGGL((k_sobol_paths<PAY, SB_GBM, BR>), grid, block, 0, ctx->stream, a);
                else if (model == SB_LV_ONE_SLICE) hipLaunchKernelGGL((k_sobol_paths<PAY, SB_LV_ONE_SLICE, BR>), grid, block, 0, ctx->stream, a);
                else hipLaunchKernelGGL((k_sobol_paths<PAY, SB_LV_SURFACE, BR>), grid, block, 0, ctx->stream, a);
            },
            want_payoff, sobol->bridge != 0);
    });
}

}  // namespace mcg
