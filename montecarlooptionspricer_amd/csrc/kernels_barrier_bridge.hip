// Continuous-barrier prices from Brownian-bridge survival probabilities (mcg_barrier_survival, mcg_price_barriers_bridge;
// the contract is stated in include/mcgpu.h).  ONE streaming pass over the matrix (k_bridge_survival: 8 B per path and date
// read, 16 B on the matrix route; one fp64 logarithm per element shared by up to BRIDGE_L_MAX levels kept in registers)
// reduces every path to its survival probability P for each level of a group; the group's contracts are then evaluated on
// row n_steps and P (k_bridge_book: the layout of k_exotic_book, per-block {sum, sum^2} through block_sum) and, after the
// last group, reduced by k_book_reduce in a fixed order (the entry of a per-path kernel, the book's frame and the reduction
// are exotic_device.hpp's).  No float atomics: repeated calls are bit-identical, a path's P
// for a level depends on that path's column and that level only, and a contract's sums do not depend on the rest of the book.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "../host/barrier_bridge.hpp"
#include "devmath.hpp"
#include "exotic_device.hpp"
#include "paths_host.hpp"

namespace mcg {

constexpr int BB_ROWS = MCG_BRIDGE_ROWS;  // rows per unrolled group: their loads are issued before the first logarithm
// x <= BB_SKIP: exp(x) < 2^-54, so 1 - exp(x) rounds to 1.0 and the factor changes no bit of the product
constexpr double BB_SKIP = -38.0;

// The levels of one pass, by value in the kernel's arguments (scalar registers): slot l < n_live is written, the slots
// behind repeat the last live one (the kernel is instantiated for 1, 2, 4 and BRIDGE_L_MAX slots).
struct BridgeLevels {
    double B[BRIDGE_L_MAX];  // the barrier: the safe test compares the stored doubles with it
    double h[BRIDGE_L_MAX];  // ln B, computed on the host in binary64
    unsigned up_mask;        // bit l: slot l is an up level
    int n_live;
};

struct BridgeArgs {
    const double* data;  // the matrix, ld doubles a row
    const double* var;   // VAR: the variance matrix, ld_var doubles a row
    int64_t ld, ld_var, n_paths;
    int first_row, n_steps;
    double w;            // !VAR: (sigma sigma) dt
    double dt;           // VAR: w_j = max(v_j, 0) dt
    double* out;         // [n_live][n_paths]
    BridgeLevels lv;
};

// One row's share of the survival products of W adjacent paths: s the row's values, c = -2 / w and wz (w is not positive:
// factor 1) of the interval that ends in this row.  Per level one subtraction, two multiplies and -- unless every lane of
// the wave is at or below BB_SKIP -- one exponential.
template <int NL, int W>
__device__ __forceinline__ void bridge_row(const BridgeLevels& lv, const double (&s)[W], const double (&c)[W], const bool (&wz)[W],
                                           double (&mn)[W], double (&mx)[W], double (&dprev)[W][NL], double (&prod)[W][NL]) {
    double l[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        l[w] = log(s[w]);
        mn[w] = fmin(mn[w], s[w]);
        mx[w] = fmax(mx[w], s[w]);
    }
#pragma unroll
    for (int q = 0; q < NL; ++q) {
        double x[W];
        bool live = false;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const double d = l[w] - lv.h[q];
            const double m = fmax(dprev[w][q] * d, 0.0);
            x[w] = wz[w] ? -std::numeric_limits<double>::infinity() : m * c[w];
            dprev[w][q] = d;
            live = live || x[w] > BB_SKIP;
        }
        if (__builtin_amdgcn_ballot_w64(live) != 0ull) {  // (wave-uniform)
#pragma unroll
            for (int w = 0; w < W; ++w) prod[w][q] *= 1.0 - exp(x[w]);
        }
    }
}

// c = -2 / w and whether w is not positive, from a variance-matrix value
__device__ __forceinline__ void bridge_weight(double v, double dt, double& c, bool& wz) {
    const double w = fmax(v, 0.0) * dt;
    wz = !(w > 0.0);
    c = -2.0 / w;
}

// Survival of W adjacent paths from column p0 on, for the NL slots of a.lv: the safe test through the running minimum and
// maximum of the monitored rows (down: min > B, up: max < B -- the complement of exotic_payoff's hit rule), the product
// over the intervals row by row in ascending order.
template <bool VAR, int NL, int W>
__device__ __forceinline__ void bridge_scan(const BridgeArgs& a, int64_t p0) {
    const double* col = a.data + (int64_t)a.first_row * a.ld + p0;
    const double* vcol = VAR ? a.var + (int64_t)a.first_row * a.ld_var + p0 : nullptr;
    const int n_int = a.n_steps - a.first_row;  // intervals: interval i (1-based) ends in row first_row + i, its variance is row first_row + i - 1's
    double prod[W][NL], dprev[W][NL], mn[W], mx[W], cs[W];
    bool wzs[W];
    {
        double s[W];
        xs_load<W>(col, s);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const double l0 = log(s[w]);
            mn[w] = mx[w] = s[w];
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                prod[w][q] = 1.0;
                dprev[w][q] = l0 - a.lv.h[q];
            }
            wzs[w] = !(a.w > 0.0);
            cs[w] = -2.0 / a.w;
        }
    }
    int i = 1;
    for (; i + BB_ROWS <= n_int + 1; i += BB_ROWS) {
        double s[BB_ROWS][W], v[BB_ROWS][W];
#pragma unroll
        for (int k = 0; k < BB_ROWS; ++k) {
            xs_load<W>(col + (int64_t)(i + k) * a.ld, s[k]);
            if constexpr (VAR) xs_load<W>(vcol + (int64_t)(i + k - 1) * a.ld_var, v[k]);
        }
#pragma unroll
        for (int k = 0; k < BB_ROWS; ++k) {
            if constexpr (VAR) {
                double c[W];
                bool wz[W];
#pragma unroll
                for (int w = 0; w < W; ++w) bridge_weight(v[k][w], a.dt, c[w], wz[w]);
                bridge_row<NL, W>(a.lv, s[k], c, wz, mn, mx, dprev, prod);
            } else {
                bridge_row<NL, W>(a.lv, s[k], cs, wzs, mn, mx, dprev, prod);
            }
        }
    }
    for (; i <= n_int; ++i) {  // at most BB_ROWS - 1 rows
        double s[W], v[W];
        xs_load<W>(col + (int64_t)i * a.ld, s);
        if constexpr (VAR) {
            xs_load<W>(vcol + (int64_t)(i - 1) * a.ld_var, v);
            double c[W];
            bool wz[W];
#pragma unroll
            for (int w = 0; w < W; ++w) bridge_weight(v[w], a.dt, c[w], wz[w]);
            bridge_row<NL, W>(a.lv, s, c, wz, mn, mx, dprev, prod);
        } else {
            bridge_row<NL, W>(a.lv, s, cs, wzs, mn, mx, dprev, prod);
        }
    }
#pragma unroll
    for (int w = 0; w < W; ++w) {
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            const bool safe = ((a.lv.up_mask >> q) & 1u) ? mx[w] < a.lv.B[q] : mn[w] > a.lv.B[q];
            if (q < a.lv.n_live) a.out[(int64_t)q * a.n_paths + p0 + w] = safe ? prod[w][q] : 0.0;
        }
    }
}

// One lane per W adjacent paths (lane_paths); W = 2 needs 16-byte aligned rows in both matrices.
template <bool VAR, int NL, int W>
__global__ __launch_bounds__(256) void k_bridge_survival(const BridgeArgs a) {
    lane_paths<W>(a.n_paths, [&](int64_t p0, int64_t, auto w) { bridge_scan<VAR, NL, w.value>(a, p0); });
}

// k_exotic_book's layout over the contracts [c_lo, c_hi) of one level group, in the order of BridgePlan::order: blockIdx.y
// counts the chunks of XB_CH contracts from c_lo's chunk on, blockIdx.x strides over the paths (book_partials).  A chunk
// that two groups share is visited by both launches; each writes the fields of its own contracts only (and the one that
// holds the last contract zeroes the fields behind it), so k_book_reduce finds every field written once.
__global__ __launch_bounds__(256) void k_bridge_book(const double* st_row, const double* surv, int64_t n, const mcg_exotic* book,
                                                     const int* slot, int c_lo, int c_hi, int n_contracts, int n_blocks,
                                                     double* partials) {
    __shared__ double red[XB_NF * 4];
    const int chunk = c_lo / XB_CH + blockIdx.y;
    const int c0 = chunk * XB_CH;
    book_partials<XB_NF>(
        n, red, partials + ((int64_t)chunk * n_blocks + blockIdx.x) * XB_NF,
        [&](int64_t i, double (&e)[XB_NF]) {
            const double st = st_row[i];
#pragma unroll
            for (int q = 0; q < XB_CH; ++q) {
                const int c = c0 + q;
                if (c >= c_lo && c < c_hi) {
                    const double x = bridge_payoff(book[c], st, surv[(int64_t)slot[c] * n + i]);
                    e[XB_NS * q] += x;
                    e[XB_NS * q + 1] = fma(x, x, e[XB_NS * q + 1]);
                }
            }
        },
        [&](int q) {
            const int c = c0 + q / XB_NS;
            return (c >= c_lo && c < c_hi) || (c >= n_contracts && c_hi == n_contracts);
        });
}

// The levels [at, at + n_live) of (barriers, is_up) as one pass's argument
static BridgeLevels bridge_levels(const double* barriers, const int* is_up, int at, int n_live) {
    BridgeLevels lv{};
    lv.n_live = n_live;
    for (int q = 0; q < BRIDGE_L_MAX; ++q) {
        const int l = at + std::min(q, n_live - 1);
        lv.B[q] = barriers[l];
        lv.h[q] = std::log(barriers[l]);
        if (is_up[l]) lv.up_mask |= 1u << q;
    }
    return lv;
}

// k_bridge_survival for the slots of lv over rows first_row .. n_steps of P into d_out[n_live][n_paths]; one launch under
// MCG_K_EXOTIC.  V null: the scalar route with w = (sigma sigma) dt.
static int launch_bridge_survival(mcg_ctx* ctx, const mcg_paths* P, const mcg_paths* V, double sigma, double dt, int first_row,
                                  const BridgeLevels& lv, double* d_out) {
    const StreamGrid g = stream_grid(P, V);
    if (g.n_blocks < 0) return MCG_ERR_INVALID;
    BridgeArgs a{};
    a.data = P->data;
    a.var = V ? V->data : nullptr;
    a.ld = P->ld;
    a.ld_var = V ? V->ld : 0;
    a.n_paths = P->n_paths;
    a.first_row = first_row;
    a.n_steps = P->n_steps;
    a.w = (sigma * sigma) * dt;
    a.dt = dt;
    a.out = d_out;
    a.lv = lv;
    const int nl = lv.n_live <= 1 ? 1 : lv.n_live <= 2 ? 2 : lv.n_live <= 4 ? 4 : BRIDGE_L_MAX;
    return PathLaunch{ctx, g.n_blocks}.run(MCG_K_EXOTIC, [&] {
        dispatch_flags(
            [&](auto var, auto w, auto hi, auto lo) {
                constexpr int NL = hi.value ? (lo.value ? BRIDGE_L_MAX : 4) : (lo.value ? 2 : 1);
                hipLaunchKernelGGL((k_bridge_survival<var.value, NL, w.value ? 2 : 1>), dim3((unsigned)g.n_blocks), dim3(256), 0, ctx->stream, a);
            },
            V != nullptr, g.wide, nl >= 4, nl == 2 || nl == BRIDGE_L_MAX);
    });
}

int run_barrier_survival(mcg_ctx* ctx, const mcg_paths* P, const mcg_paths* V, double sigma, double dt, int first_row,
                         const double* barriers, const int* is_up, int n_levels, double* host_out) {
    const int64_t n = P->n_paths;
    const size_t bytes = (size_t)BRIDGE_L_MAX * n * sizeof(double);
    void* ws = nullptr;
    int rc = pool_alloc(ctx, bytes, &ws);
    if (rc) return rc;
    auto body = [&]() -> int {
        for (int at = 0; at < n_levels; at += BRIDGE_L_MAX) {
            const int n_live = std::min(BRIDGE_L_MAX, n_levels - at);
            const int r2 = launch_bridge_survival(ctx, P, V, sigma, dt, first_row, bridge_levels(barriers, is_up, at, n_live), (double*)ws);
            if (r2) return r2;
            // (stream order: the next group's launch overwrites the workspace behind this copy)
            MCG_HIP(hipMemcpyAsync(host_out + (size_t)at * n, ws, (size_t)n_live * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        }
        MCG_HIP(hipStreamSynchronize(ctx->stream));
        return MCG_OK;
    };
    rc = body();
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    pool_release(ctx, ws, bytes);
    return rc;
}

// Workspace (one pool buffer): [BRIDGE_L_MAX n survival probabilities][n_chunks * n_blocks * XB_NF partials][2 n_contracts + 1 sums];
// the sums stand in the order of BridgePlan::order until the host has them.
int run_barriers_bridge(mcg_ctx* ctx, const mcg_paths* P, const mcg_paths* V, double sigma, double r, double T, int first_row,
                        const mcg_exotic* book, int nc, double* price, double* std_err, double* sums) {
    const int64_t n = P->n_paths;
    const double dt = T / (double)P->n_steps;
    BridgePlan plan;
    bridge_plan(book, nc, BRIDGE_L_MAX, plan);
    std::vector<mcg_exotic> sorted((size_t)nc);
    std::vector<int> slot((size_t)nc);
    for (int s = 0; s < nc; ++s) {
        sorted[(size_t)s] = book[plan.order[(size_t)s]];
        slot[(size_t)s] = plan.level_of[(size_t)plan.order[(size_t)s]] % BRIDGE_L_MAX;
    }
    const int n_sums = 2 * nc + 1, n_chunks = (nc + XB_CH - 1) / XB_CH;
    const int n_blocks = book_blocks(ctx, n);
    const size_t n_part = (size_t)n_chunks * n_blocks * XB_NF;
    std::vector<double> h;
    const int rc = exotic_sums_frame(ctx, n, (size_t)BRIDGE_L_MAX * n + n_part + n_sums, n_sums, h, [&](double* d_surv, double* d_sums) -> int {
        double* d_part = d_surv + (size_t)BRIDGE_L_MAX * n;
        HostPiece up[] = {{sorted.data(), (size_t)nc * sizeof(mcg_exotic)}, {slot.data(), (size_t)nc * sizeof(int)}};
        int r2 = upload_params(ctx, up);
        if (r2) return r2;
        for (int g = 0; g < plan.n_groups(); ++g) {
            const int at = g * BRIDGE_L_MAX, n_live = std::min(BRIDGE_L_MAX, plan.n_levels() - at);
            r2 = launch_bridge_survival(ctx, P, V, sigma, dt, first_row, bridge_levels(plan.barrier.data(), plan.up.data(), at, n_live), d_surv);
            if (r2) return r2;
            const int c_lo = plan.group_begin[(size_t)g], c_hi = plan.group_begin[(size_t)g + 1];
            TimedLaunch t(ctx, MCG_K_EXOTIC);
            hipLaunchKernelGGL(k_bridge_book, dim3(n_blocks, (c_hi - 1) / XB_CH - c_lo / XB_CH + 1), dim3(256), 0, ctx->stream,
                               P->data + (int64_t)P->n_steps * P->ld, d_surv, n, reinterpret_cast<const mcg_exotic*>(up[0].at),
                               reinterpret_cast<const int*>(up[1].at), c_lo, c_hi, nc, n_blocks, d_part);
        }
        {
            TimedLaunch t(ctx, MCG_K_EXOTIC);
            enqueue_exotic_reduce(ctx, d_part, n_blocks, nc, (double)n, d_sums);
        }
        MCG_HIP(hipGetLastError());
        return MCG_OK;
    });
    if (rc) return rc;
    return exotic_prices_from_sums(h, nc, plan.order.data(), r, T, price, std_err, sums);
}

}  // namespace mcg
