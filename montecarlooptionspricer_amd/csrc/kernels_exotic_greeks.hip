// Greeks of the exotics book (mcg_path_tangent_stats, mcg_greeks_exotics): ONE pass over the matrix reduces every path to the
// five statistics of k_path_stats and the five more their tangents need (k_path_tangent_stats: the same stream of 8 B per
// path and date, 80 B per path written; with LOGS one fp64 logarithm per element); a book of contracts is then evaluated on
// those statistics and on rows 0 and 1 (k_exotic_greeks_book: per-block {sum, sum^2} of six estimators a contract through
// greeks_block_store, k_greeks_reduce with one workgroup per chunk: fixed order).  No float atomics: repeated calls are
// bit-identical, and a contract's sums do not depend on the rest of the book.  The estimators are stated in include/mcgpu.h.
// The scan and the entry of a per-path kernel are exotic_device.hpp's.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "devmath.hpp"
#include "exotic_device.hpp"
#include "greeks_device.hpp"
#include "paths_host.hpp"

namespace mcg {

constexpr int XT_Q = 10;              // statistics per path: 0 S_T, 1 A, 2 G, 3 min, 4 max, 5 L, 6 J, 7 j_min, 8 j_max, 9 Q
constexpr int GX_CH = 4;              // contracts one workgroup of k_exotic_greeks_book keeps in registers
constexpr int GX_E = 6;               // estimators per contract: 0 price, 1 delta, 2 gamma, 3 vega, 4 rho, 5 dual delta
constexpr int GX_NE = GX_E * GX_CH;
constexpr int GX_NF = 2 * GX_NE + 2;  // greeks_block_store's fields of one chunk

// One lane per W adjacent paths (lane_paths): path_scan with the tangent statistics.  S_T, A, G, min and max are
// bit-identical to k_path_stats<true, W>'s: the one scan computes both.
template <bool LOGS, int W>
__global__ __launch_bounds__(256) void k_path_tangent_stats(const double* data, int64_t ld, int64_t n_paths, int first_row, int n_rows,
                                                            double* out10) {
    lane_paths<W>(n_paths, [&](int64_t p0, int64_t n, auto w) {
        const double* row0 = data + p0;
        path_scan<true, true, LOGS, w.value>(row0 + (int64_t)first_row * ld, row0, ld, first_row, n_rows, n, p0, out10);
    });
}

// What the book kernel reads of the model and the grid; the host derives it once (run_greeks_exotics).  lr: sigma > 0 (the
// statistics carry L and Q); without it every term that divides by sigma is left at zero and the host reports NaN there.
struct GxModel {
    double T, dt, n_steps;
    double c_T, c_dt;      // c = r - q + sigma^2 / 2, times T and times dt
    double mu, drift_T;    // (r - q - sigma^2 / 2) dt and the same times T
    double jbar;           // (first_row + n_steps) / 2
    double inv_sigma, inv_sd, sqrt_dt;  // 1 / sigma, 1 / (sigma sqrt(dt)), sqrt(dt)
    int lr;
};

// One path's values that do not depend on the contract: its statistics, their tangents in sigma (ts) and r (tr) in the order
// S_T, A, G, m, M, and the likelihood-ratio weights of the first step and of the whole path.
struct GxPath {
    double s0, st, A, G, mn, mx;
    double ts_st, ts_A, ts_G, ts_mn, ts_mx;  // plain members, no arrays: the kind picks among them with selects, in registers
    double tr_st, tr_A, tr_G, tr_mn, tr_mx;
    double gz;                                // Z_1 / (s0^2 sigma sqrt(dt)): the fixed-strike gamma's weight, before K 1{X > K}
    double w_delta, w_gamma, w_vega, w_rho;   // what the barrier kinds multiply the payoff by
};

__device__ __forceinline__ GxPath gx_path(const GxModel& g, double s0, double s1, const double (&v)[XT_Q]) {
    GxPath p;
    p.s0 = s0;
    p.st = v[0];
    p.A = v[1];
    p.G = v[2];
    p.mn = v[3];
    p.mx = v[4];
    const double J = v[6], jm = v[7], jM = v[8];
    p.tr_st = g.T * p.st;
    p.tr_A = g.dt * J;
    p.tr_G = p.G * g.dt * g.jbar;
    p.tr_mn = g.dt * jm * p.mn;
    p.tr_mx = g.dt * jM * p.mx;
    p.ts_st = p.ts_A = p.ts_G = p.ts_mn = p.ts_mx = 0.0;
    p.gz = p.w_delta = p.w_gamma = p.w_vega = p.w_rho = 0.0;
    if (g.lr) {
        const double L = v[5], Q = v[9];
        const double l0 = log(s0), lst = log(p.st / s0);
        p.ts_st = p.st * (lst - g.c_T) * g.inv_sigma;
        p.ts_A = (L - p.A * l0 - g.c_dt * J) * g.inv_sigma;
        p.ts_G = p.G * (log(p.G / s0) - g.c_dt * g.jbar) * g.inv_sigma;
        p.ts_mn = p.mn * (log(p.mn / s0) - g.c_dt * jm) * g.inv_sigma;
        p.ts_mx = p.mx * (log(p.mx / s0) - g.c_dt * jM) * g.inv_sigma;
        const double z1 = (log(s1 / s0) - g.mu) * g.inv_sd;
        const double sum_z = (lst - g.n_steps * g.mu) * g.inv_sd;
        const double sum_z2 = (Q - 2.0 * g.mu * lst + g.n_steps * g.mu * g.mu) * (g.inv_sd * g.inv_sd);
        const double w_T = (lst - g.drift_T) * g.inv_sigma;
        const double inv_s0 = 1.0 / s0, a = z1 * g.inv_sd;  // Z_1 / (sigma sqrt(dt))
        p.gz = a * inv_s0 * inv_s0;
        p.w_delta = a * inv_s0;
        p.w_gamma = ((z1 * z1 - 1.0) * (g.inv_sd * g.inv_sd) - a) * (inv_s0 * inv_s0);
        p.w_vega = (sum_z2 - g.n_steps) * g.inv_sigma - g.sqrt_dt * sum_z;
        p.w_rho = w_T * g.inv_sigma - g.T;
    }
    return p;
}

// a or b BY VALUE: `c ? p.a : p.b` on members is a conditional lvalue, a select of addresses that keeps the struct in scratch
__device__ __forceinline__ double gx_sel(bool c, double a, double b) { return c ? a : b; }

// f' of the vanilla payoff of x against k, with the strict comparisons of k_greeks_european
__device__ __forceinline__ double gx_fp(bool call, double x, double k) {
    return call ? (x > k ? 1.0 : 0.0) : (x < k ? -1.0 : 0.0);
}

// The six undiscounted per-path estimators of one contract (include/mcgpu.h: pathwise for kinds 0-5, likelihood ratio for
// the barriers).  The price sample is exotic_payoff itself.
__device__ __forceinline__ void gx_sample(const mcg_exotic& c, const GxModel& g, const GxPath& p, double (&x)[GX_E]) {
    const bool call = c.is_call != 0;
    const double f = exotic_payoff(c, p.st, p.A, p.G, p.mn, p.mx);
    x[0] = f;
    if (c.kind >= MCG_X_BARRIER_UP_OUT) {
        const bool up = c.kind == MCG_X_BARRIER_UP_OUT || c.kind == MCG_X_BARRIER_UP_IN;
        const bool in = c.kind == MCG_X_BARRIER_UP_IN || c.kind == MCG_X_BARRIER_DOWN_IN;
        const bool hit = up ? p.mx >= c.barrier : p.mn <= c.barrier;
        x[1] = f * p.w_delta;
        x[2] = f * p.w_gamma;
        x[3] = f * p.w_vega;
        x[4] = f * p.w_rho;
        x[5] = hit == in ? -gx_fp(call, p.st, c.K) : 0.0;
        return;
    }
    // X: the statistic the contract reads, with its tangents
    // (lookback: the fixed call and the floating put read M, the fixed put and the floating call m)
    const bool arith = c.kind == MCG_X_ASIAN_ARITH_FIXED || c.kind == MCG_X_ASIAN_ARITH_FLOAT;
    const bool geo = c.kind == MCG_X_ASIAN_GEO_FIXED || c.kind == MCG_X_ASIAN_GEO_FLOAT;
    const bool use_max = (c.kind == MCG_X_LOOKBACK_FIXED) == call;
    const double X = gx_sel(arith, p.A, gx_sel(geo, p.G, gx_sel(use_max, p.mx, p.mn)));
    const double tsX = gx_sel(arith, p.ts_A, gx_sel(geo, p.ts_G, gx_sel(use_max, p.ts_mx, p.ts_mn)));
    const double trX = gx_sel(arith, p.tr_A, gx_sel(geo, p.tr_G, gx_sel(use_max, p.tr_mx, p.tr_mn)));
    const bool fixed = c.kind == MCG_X_ASIAN_ARITH_FIXED || c.kind == MCG_X_ASIAN_GEO_FIXED || c.kind == MCG_X_LOOKBACK_FIXED;
    if (fixed) {
        const double fp = gx_fp(call, X, c.K);
        x[1] = (f + c.K * fp) / p.s0;  // (f - K df/dK) / s0, df/dK = -fp
        x[2] = X > c.K ? c.K * p.gz : 0.0;
        x[3] = fp * tsX;
        x[4] = fp * trX - g.T * f;
        x[5] = -fp;
    } else {
        // f = max(+-(S_T - X), 0); the floating lookback is always in the money
        const double fp = c.kind == MCG_X_LOOKBACK_FLOAT ? (call ? 1.0 : -1.0) : gx_fp(call, p.st, X);
        x[1] = f / p.s0;
        x[2] = 0.0;
        x[3] = fp * (p.ts_st - tsX);
        x[4] = fp * (p.tr_st - trX) - g.T * f;
        x[5] = 0.0;
    }
}

// blockIdx.y: a chunk of GX_CH contracts; blockIdx.x strides over the paths (a grid that depends on the path count only).
// partials[(chunk * gridDim.x + blockIdx.x) * GX_NF + ...]: greeks_block_store's fields, estimator e of the chunk's contract
// q at GX_E q + e.  (Not on book_partials: the walk also takes the range of row 0 and ends in greeks_block_store.)
__global__ __launch_bounds__(256) void k_exotic_greeks_book(const double* stats, const double* row0, const double* row1, int64_t n,
                                                            GxModel g, const mcg_exotic* book, int n_contracts, double* partials) {
    __shared__ double red[2 * GX_NE * 4];
    const int c0 = blockIdx.y * GX_CH;
    const int live = min(GX_CH, n_contracts - c0);
    double e[2 * GX_NE];
#pragma unroll
    for (int q = 0; q < 2 * GX_NE; ++q) e[q] = 0.0;
    double lo = std::numeric_limits<double>::infinity(), hi = -std::numeric_limits<double>::infinity();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double s0 = row0[i], s1 = row1[i];
        lo = fmin(lo, s0);
        hi = fmax(hi, s0);
        double v[XT_Q];
#pragma unroll
        for (int q = 0; q < XT_Q; ++q) v[q] = stats[(int64_t)q * n + i];
        const GxPath p = gx_path(g, s0, s1, v);
#pragma unroll
        for (int q = 0; q < GX_CH; ++q) {
            if (q < live) {
                double x[GX_E];
                gx_sample(book[c0 + q], g, p, x);
#pragma unroll
                for (int f = 0; f < GX_E; ++f) {
                    e[GX_E * q + f] += x[f];
                    e[GX_NE + GX_E * q + f] = fma(x[f], x[f], e[GX_NE + GX_E * q + f]);
                }
            }
        }
    }
    greeks_block_store<GX_NE>(e, lo, hi, red, partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * GX_NF);
}

int launch_path_tangent_stats(mcg_ctx* ctx, const mcg_paths* P, int first_row, bool logs, double* d_stats) {
    const int n_rows = P->n_steps - first_row + 1;
    const StreamGrid g = stream_grid(P);
    if (g.n_blocks < 0) return MCG_ERR_INVALID;
    return PathLaunch{ctx, g.n_blocks}.run(MCG_K_EXOTIC, [&] {
        dispatch_flags(
            [&](auto l, auto w) {
                hipLaunchKernelGGL((k_path_tangent_stats<l.value, w.value ? 2 : 1>), dim3((unsigned)g.n_blocks), dim3(256), 0, ctx->stream,
                                   P->data, P->ld, P->n_paths, first_row, n_rows, d_stats);
            },
            logs, g.wide);
    });
}

int run_path_tangent_stats(mcg_ctx* ctx, const mcg_paths* P, int first_row, bool logs, double* host_out10) {
    return download_stats(
        ctx, P->n_paths, host_out10, "tangent", [&](double* d) { return launch_path_tangent_stats(ctx, P, first_row, logs, d); }, XT_Q);
}

// Workspace (one pool buffer): [10 n statistics][n_chunks * n_blocks * GX_NF partials][n_chunks * GX_NF sums]
// (sums[chunk * GX_NF + field]).
int run_greeks_exotics(mcg_ctx* ctx, const mcg_paths* P, double r, double q, double sigma, double T, int first_row,
                       const mcg_exotic* book, int nc, mcg_greeks* out) {
    const int64_t n = P->n_paths;
    const bool lr = sigma > 0.0;
    const int n_chunks = (nc + GX_CH - 1) / GX_CH, n_sums = n_chunks * GX_NF;
    const int n_blocks = book_blocks(ctx, n);
    const size_t n_part = (size_t)n_chunks * n_blocks * GX_NF;
    GxModel g{};
    g.T = T;
    g.dt = T / (double)P->n_steps;
    g.n_steps = (double)P->n_steps;
    const double c = r - q + 0.5 * sigma * sigma, half = r - q - 0.5 * sigma * sigma;
    g.c_T = c * T;
    g.c_dt = c * g.dt;
    g.mu = half * g.dt;
    g.drift_T = half * T;
    g.jbar = 0.5 * ((double)first_row + (double)P->n_steps);
    g.sqrt_dt = std::sqrt(g.dt);
    g.inv_sigma = lr ? 1.0 / sigma : 0.0;
    g.inv_sd = lr ? 1.0 / (sigma * g.sqrt_dt) : 0.0;
    g.lr = lr ? 1 : 0;
    std::vector<double> h;
    const int rc = exotic_sums_frame(ctx, n, (size_t)XT_Q * n + n_part + n_sums, n_sums, h, [&](double* d_stats, double* d_sums) -> int {
        double* d_part = d_stats + XT_Q * n;
        HostPiece up[] = {{book, (size_t)nc * sizeof(mcg_exotic)}};
        int r2 = upload_params(ctx, up);
        if (r2) return r2;
        r2 = launch_path_tangent_stats(ctx, P, first_row, lr, d_stats);
        if (r2) return r2;
        {
            TimedLaunch t(ctx, MCG_K_EXOTIC, 2);
            hipLaunchKernelGGL(k_exotic_greeks_book, dim3(n_blocks, n_chunks), dim3(256), 0, ctx->stream, d_stats, P->data, P->data + P->ld,
                               n, g, reinterpret_cast<const mcg_exotic*>(up[0].at), nc, d_part);
            enqueue_greeks_reduce(ctx, d_part, n_blocks, GX_NF, n_chunks, d_sums);
        }
        MCG_HIP(hipGetLastError());
        return MCG_OK;
    });
    if (rc) return rc;
    const double nd = (double)n, D = std::exp(-r * T), lo = h[2 * GX_NE], hi = h[2 * GX_NE + 1];
    const bool flat0 = lo == hi && lo > 0.0;  // row 0 is one positive constant
    for (int ci = 0; ci < nc; ++ci) {
        const double* s = h.data() + (size_t)(ci / GX_CH) * GX_NF + GX_E * (ci % GX_CH);
        auto fill = [&](int e, double* mean, double* se) { mean_se(s[e], s[GX_NE + e], nd, D, mean, se); };
        mcg_greeks* o = out + ci;
        greeks_all_nan(o);
        fill(0, &o->price, &o->price_se);
        fill(5, &o->dual_delta, &o->dual_delta_se);
        const int kind = book[ci].kind;
        if (kind >= MCG_X_BARRIER_UP_OUT) {
            if (lr && flat0 && first_row >= 1) {
                fill(1, &o->delta, &o->delta_se);
                fill(2, &o->gamma, &o->gamma_se);
                fill(3, &o->vega, &o->vega_se);
                fill(4, &o->rho, &o->rho_se);
            }
            continue;
        }
        const bool fixed = kind == MCG_X_ASIAN_ARITH_FIXED || kind == MCG_X_ASIAN_GEO_FIXED || kind == MCG_X_LOOKBACK_FIXED;
        if (flat0) fill(1, &o->delta, &o->delta_se);
        if (P->generated) fill(4, &o->rho, &o->rho_se);
        if (lr) fill(3, &o->vega, &o->vega_se);
        if (flat0 && (!fixed || (lr && first_row >= 1))) fill(2, &o->gamma, &o->gamma_se);
    }
    return MCG_OK;
}

}  // namespace mcg
