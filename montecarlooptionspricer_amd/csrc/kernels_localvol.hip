// Local-volatility paths for gfx950 (include/mcgpu.h: mcg_paths_localvol, mcg_paths_localvol_payoff).
//
// k_localvol_paths<PAYOFF, ONE_SLICE> stands on the generators' skeleton of paths_device.hpp (row store, block walk, normals,
// payoff partials): two adjacent paths per lane with S and the running log-moneyness X in registers, one Philox block of the
// price stream per four steps, fm::scaled_exp for the price.
//
// What is new is the surface lookup: one 16-byte gather {a_j, d_j} per path-step at a per-lane index, from LDS.
//   ONE_SLICE  (a surface without a time axis) the slice, <= 127 entries, is staged once behind the tables.
//   otherwise  the workgroup stages the slices of the NEXT Philox block (<= 4 * 127 entries) into one of two buffers while it
//              steps through the other: the loads are issued at the top of a block and land in LDS at its end, one barrier
//              per block.  The last block stages only the slices that exist.
// Every wave of a workgroup walks through all blocks, so that the barriers match; the waves of the last workgroup that lie
// beyond the row keep their stores to themselves.
//
// Roofline: HBM write, 8 B per path-step; the table (n_steps * (n_x - 1) * 16 B, 0.5 MB at 252 x 128) is read once per
// workgroup and stays in L2.
#include "devmath.hpp"
#include "fastmath.hpp"
#include "localvol_device.hpp"
#include "paths_host.hpp"
#include "paths_device.hpp"

namespace mcg {

constexpr int LV_PPL = 2;                          // paths per lane
constexpr int LV_SLICE_MAX = LOCALVOL_MAX_NX - 1;  // entries of a slice
constexpr int LV_STAGE = 4 * LV_SLICE_MAX;         // entries of one staging buffer: the slices of a Philox block
constexpr int LV_STAGE_PER_LANE = (LV_STAGE + 255) / 256;
// Timing study (tools/build_variant.sh ... -DMCG_LV_GLOBAL_GATHER): the multi-slice kernel gathers straight from the table in
// global memory (L2) instead of staging slices into LDS; DESIGN.md has its time.  The product stages.
#ifdef MCG_LV_GLOBAL_GATHER
constexpr bool LV_STAGED = false;
#else
constexpr bool LV_STAGED = true;
#endif

template <bool PAYOFF, bool ONE_SLICE>
__global__ __launch_bounds__(256) void k_localvol_paths(LocalVolArgs a) {
    constexpr int PPL = LV_PPL;
    constexpr bool STAGED = LV_STAGED;
    __shared__ fm::Tables tabs;
    __shared__ double2 slices[ONE_SLICE ? LV_SLICE_MAX : STAGED ? 2 * LV_STAGE : 1];
    fm::load_tables(&tabs, a.tabs);
    const fm::Tables* tab = &tabs;
    const int nx1 = a.nx1;
    // entries of the staging buffer of `block`: four slices, fewer in the tail
    auto stage_count = [&](const uint32_t block) { return min(4, a.n_steps - (int)(block << 2)) * nx1; };
    if (ONE_SLICE) {
        if ((int)threadIdx.x < nx1) slices[threadIdx.x] = a.surf[threadIdx.x];
    } else if (STAGED) {
        const int cnt = stage_count(0);
#pragma unroll
        for (int k = 0; k < LV_STAGE_PER_LANE; ++k) {
            const int e = (int)threadIdx.x + 256 * k;
            if (e < cnt) slices[e] = a.surf[e];
        }
    }
    __syncthreads();
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PPL;  // first column of this lane
    // rows are padded to 256 columns and a workgroup covers 512: the upper two waves of the last one may lie beyond the row
    const bool in_row = i < a.ld;  // (wave-uniform)
    double S[PPL], X[PPL];
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        S[p] = a.S0;
        X[p] = 0.0;
    }
    if (in_row || !ONE_SLICE) {
        double* row = a.out + (int64_t)blockIdx.x * (256 * PPL);
        const unsigned lane_bytes = threadIdx.x * (8u * PPL);
        auto store_row = [&]() {
            if (in_row) store_pair16(row, lane_bytes, S[0], S[1]);
        };
        store_row();
        PhiloxLane rng[PPL];
#pragma unroll
        for (int p = 0; p < PPL; ++p) rng[p] = philox_lane_setup(a.path_begin + (uint64_t)(i + p), STREAM_PRICE, a.k1);
        uint32_t block = 0;  // the Philox block of the current four steps
        const double2* cur = slices;
        // Staging of the slices of block + 1 (multi-slice kernels): fetch() issues the global loads, land() writes them into the
        // buffer the workgroup is not stepping through.  The barrier at the top of the next block orders land() against
        // that block's reads, and this block's reads against the land() of the block after.
        double2 held[LV_STAGE_PER_LANE];
        auto fetch = [&]() {
            const int cnt = stage_count(block + 1);  // <= 0 behind the last block
            const double2* src = a.surf + (size_t)(block + 1) * 4 * nx1;
#pragma unroll
            for (int k = 0; k < LV_STAGE_PER_LANE; ++k) {
                const int e = (int)threadIdx.x + 256 * k;
                double2 v = make_double2(0.0, 0.0);  // (every element assigned: a half-written array would live in a private segment)
                if (e < cnt) v = src[e];
                held[k] = v;
            }
        };
        auto land = [&]() {
            const int cnt = stage_count(block + 1);
            double2* dst = slices + ((block + 1) & 1u) * LV_STAGE;
#pragma unroll
            for (int k = 0; k < LV_STAGE_PER_LANE; ++k) {
                const int e = (int)threadIdx.x + 256 * k;
                if (e < cnt) dst[e] = held[k];
            }
        };
        // The barrier between two blocks.  The wait in front of it is written out: the land() of the block before reaches this
        // barrier over the loop's back edge, and hipcc put no wait for its LDS writes there (it does in front of the tail's).
        auto stage_barrier = [&]() {
            if (STAGED) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __syncthreads();
            }
        };
        Philox4 w[PPL];
        double za[PPL], zb[PPL];
        walk_blocks(
            a.n_steps, block,
            [&](auto whole) {  // the tail fetches nothing: no block follows it
                if (!ONE_SLICE) {
                    if (block) stage_barrier();
                    cur = STAGED ? slices + (block & 1u) * LV_STAGE : a.surf + (size_t)block * 4 * nx1;
                    if (STAGED && whole) fetch();
                }
#pragma unroll
                for (int p = 0; p < PPL; ++p) w[p] = philox4x32_10_lane(rng[p], block, a.k0, a.k1);
                normal_pairs(w, false, tab, za, zb);
            },
            [&] { normal_pairs(w, true, tab, za, zb); },
            [&](auto elem) {
                const double2* sl = ONE_SLICE ? cur : cur + elem * nx1;
#pragma unroll
                for (int p = 0; p < PPL; ++p) localvol_step(a, sl, (elem & 1 ? zb : za)[p], S[p], X[p]);
                row += a.ld;
                store_row();
            },
            [&] {
                if (!ONE_SLICE && STAGED) land();
            });
    }
    if (PAYOFF) payoff_partials(in_row, i, a.n_paths, S, a.K, a.is_call, a.partials);
}

// One launch of k_localvol_paths over P.  table: n_slices * (n_x - 1) entries {a, d} on the host (mcg_localvol_table), n_slices
// = 1 or P->n_steps; it goes into the ctx's cached buffer on the ctx's stream ahead of the launch.
int launch_localvol(mcg_ctx* ctx, mcg_paths* P, uint64_t seed, double S0, const LocalVolScalars& c, int n_x, const double* table,
                    int n_slices, bool want_payoff, double K, int is_call) {
    const int64_t n_blocks = launch_blocks(P, LV_PPL);
    if (n_blocks < 0) return MCG_ERR_INVALID;
    if (n_x < 2 || n_x > LOCALVOL_MAX_NX || (n_slices != 1 && n_slices != P->n_steps))
        return fail(MCG_ERR_INVALID, "local vol: a table of %d slices x %d nodes does not fit %d steps", n_slices, n_x, P->n_steps);
    const PathLaunch launch{ctx, n_blocks, P, want_payoff, K, is_call};
    int rc = launch.reserve();
    if (rc) return rc;
    HostPiece up[] = {{table, (size_t)n_slices * (size_t)(n_x - 1) * sizeof(double2)}};
    rc = upload_params(ctx, up);
    if (rc) return rc;
    MCG_HIP(hipStreamSynchronize(ctx->stream));  // the caller's table may die at return (upload_params)
    LocalVolArgs a;
    set_shape_key(a, P, seed);
    set_payoff(a, ctx, K, is_call);
    a.nx1 = n_x - 1;
    a.S0 = S0;
    a.inv_dx = c.inv_dx;
    a.u0 = c.u0;
    a.m = c.m;
    a.u_max = (double)(n_x - 1);
    a.surf = (const double2*)up[0].at;
    a.tabs = (const double2*)ctx->log_tab;
    return launch.run(MCG_K_LOCALVOL, [&] {
        dispatch_flags(
            [&](auto payoff, auto one_slice) {
                hipLaunchKernelGGL((k_localvol_paths<payoff.value, one_slice.value>), dim3((unsigned)n_blocks), dim3(256), 0, ctx->stream, a);
            },
            want_payoff, n_slices == 1);
    });
}

}  // namespace mcg
