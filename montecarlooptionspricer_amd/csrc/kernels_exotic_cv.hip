// Control variates for the exotics book (include/mcgpu.h: mcg_price_exotics_cv, mcg_gbm_twin_stats).
//
// k_gbm_twin_stats   the five statistics of a GBM path built in registers from Philox stream 0 of (seed, path id): Philox,
//                    Box-Muller and the step X += fma(a, z, m) as the generators run them (paths_device.hpp: two adjacent
//                    paths per lane, fm::Tables in LDS, the walk over Philox blocks), one exponential per monitored step for A and three
//                    per path at the end (G, min, max; S_T is the last step's).  40 B per path written, nothing read:
//                    issue-bound on the VALU like the GBM generator's loop.
// k_exotic_book_cv   k_exotic_book with nine sums a contract instead of two: {Y, Y^2, d_a, d_a^2, Y d_a, d_b, d_b^2, Y d_b,
//                    d_a d_b}, d = control - its mean, the controls read from the paths' statistics or the twin's.  Four
//                    contracts (36 accumulators) a workgroup on blockIdx.y, on the same frame (book_partials), then
//                    k_book_reduce<CV_CH, CV_NS> in a fixed order (both exotic_device.hpp's).  No float atomics.
// The host arithmetic on the sums is host/exotics_cv.cpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "devmath.hpp"
#include "exotic_device.hpp"
#include "fastmath.hpp"
#include "paths_host.hpp"
#include "paths_device.hpp"

namespace mcg {

constexpr int CV_Q = 5;      // statistics per path: 0 S_T, 1 A, 2 G, 3 min, 4 max (k_path_stats' layout)
constexpr int CV_PPL = 2;    // paths per lane of k_gbm_twin_stats
constexpr int CV_CH = 4;     // contracts one workgroup of k_exotic_book_cv keeps in registers
constexpr int CV_NS = 9;     // sums per contract
constexpr int CV_NF = CV_CH * CV_NS;

static_assert(sizeof(mcg_exotic) == 32 && sizeof(mcg_control) == 48, "the parameter block is packed in doubles");

struct TwinArgs {
    double* out5;           // [5][n_paths]
    int64_t n_paths;
    int n_steps, first_row;
    uint64_t path_begin;
    uint32_t k0, k1;        // Philox key = seed
    double S0, a, m;        // a = sigma sqrt(dt), m = (r - q - sigma^2 / 2) dt
    const double2* tabs;    // fm::Tables on the device
};

__global__ __launch_bounds__(256) void k_gbm_twin_stats(TwinArgs t) {
    constexpr int PPL = CV_PPL;
    __shared__ fm::Tables tabs;
    fm::load_tables(&tabs, t.tabs);
    __syncthreads();
    const fm::Tables* tab = &tabs;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PPL;
    if (i >= t.n_paths) return;
    const bool row0 = t.first_row == 0;  // X_0 = 0, S_0 = S0 is monitored
    double X[PPL], sumS[PPL], sumX[PPL], mn[PPL], mx[PPL], last[PPL];
    PhiloxLane rng[PPL];
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        X[p] = 0.0;
        sumS[p] = row0 ? t.S0 : 0.0;
        sumX[p] = 0.0;
        mn[p] = row0 ? 0.0 : std::numeric_limits<double>::infinity();
        mx[p] = row0 ? 0.0 : -std::numeric_limits<double>::infinity();
        last[p] = t.S0;
        rng[p] = philox_lane_setup(t.path_begin + (uint64_t)(i + p), STREAM_PRICE, t.k1);
    }
    int row = 0;
    auto step = [&](const double (&z)[PPL]) {
        ++row;
#pragma unroll
        for (int p = 0; p < PPL; ++p) X[p] = X[p] + __builtin_fma(t.a, z[p], t.m);
        if (row >= t.first_row) {  // (wave-uniform)
            double e[PPL];
            fm::exp_full2(X[0], X[1], e[0], e[1]);
#pragma unroll
            for (int p = 0; p < PPL; ++p) {
                last[p] = t.S0 * e[p];
                sumS[p] += last[p];
                sumX[p] += X[p];
                mn[p] = __builtin_fmin(mn[p], X[p]);
                mx[p] = __builtin_fmax(mx[p], X[p]);
            }
        }
    };
    Philox4 w[PPL];
    double za[PPL], zb[PPL];
    uint32_t block = 0;
    walk_blocks(
        t.n_steps, block,
        [&](auto) {
#pragma unroll
            for (int p = 0; p < PPL; ++p) w[p] = philox4x32_10_lane(rng[p], block, t.k0, t.k1);
            normal_pairs(w, false, tab, za, zb);
        },
        [&] { normal_pairs(w, true, tab, za, zb); }, [&](auto k) { step(k & 1 ? zb : za); }, [] {});
    const double nd = (double)(t.n_steps - t.first_row + 1);
    double g[PPL], lo[PPL], hi[PPL];
    fm::exp_full2(sumX[0] / nd, sumX[1] / nd, g[0], g[1]);
    fm::exp_full2(mn[0], mn[1], lo[0], lo[1]);
    fm::exp_full2(mx[0], mx[1], hi[0], hi[1]);
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        const int64_t c = i + p;
        if (c < t.n_paths) {
            t.out5[0 * t.n_paths + c] = last[p];
            t.out5[1 * t.n_paths + c] = sumS[p] / nd;
            t.out5[2 * t.n_paths + c] = t.S0 * g[p];
            t.out5[3 * t.n_paths + c] = t.S0 * lo[p];
            t.out5[4 * t.n_paths + c] = t.S0 * hi[p];
        }
    }
}

// A control on one path's statistics (include/mcgpu.h: enum mcg_control_form).
__device__ __forceinline__ double control_value(const mcg_control& k, double st, double A, double G, double mn, double mx) {
    switch (k.form) {
        case MCG_CV_PAYOFF: return exotic_payoff(k.x, st, A, G, mn, mx);
        case MCG_CV_VANILLA: return payoff_of(k.x.is_call != 0, st, k.x.K);
        case MCG_CV_ST: return st;
        case MCG_CV_A: return A;
        default: return G;
    }
}

// blockIdx.y: a chunk of CV_CH contracts; blockIdx.x strides over the paths.  twin: the twin's statistics, or null.
// partials[(chunk * gridDim.x + blockIdx.x) * CV_NF + CV_NS * q + k]: sum k of the chunk's contract q
__global__ __launch_bounds__(256) void k_exotic_book_cv(const double* stats, const double* twin, int64_t n, int geo, int geo_twin,
                                                        const mcg_exotic* book, const mcg_control* controls, const int* ctrl,
                                                        int n_contracts, double* partials) {
    __shared__ double red[CV_NF * 4];
    const int c0 = blockIdx.y * CV_CH;
    const int live = min(CV_CH, n_contracts - c0);
    book_partials<CV_NF>(n, red, partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * CV_NF, [&](int64_t i, double (&e)[CV_NF]) {
        const double st = stats[i], A = stats[n + i], G = geo ? stats[2 * n + i] : 0.0, mn = stats[3 * n + i], mx = stats[4 * n + i];
        double tst = 0.0, tA = 0.0, tG = 0.0, tmn = 0.0, tmx = 0.0;
        if (twin) {
            tst = twin[i];
            tA = twin[n + i];
            tG = geo_twin ? twin[2 * n + i] : 0.0;
            tmn = twin[3 * n + i];
            tmx = twin[4 * n + i];
        }
        auto centred = [&](int idx) {
            if (idx < 0) return 0.0;
            const mcg_control& k = controls[idx];
            const double v = k.on_twin ? control_value(k, tst, tA, tG, tmn, tmx) : control_value(k, st, A, G, mn, mx);
            return v - k.mean;
        };
#pragma unroll
        for (int q = 0; q < CV_CH; ++q) {
            if (q < live) {
                const double y = exotic_payoff(book[c0 + q], st, A, G, mn, mx);
                const double da = centred(ctrl[2 * (c0 + q)]), db = centred(ctrl[2 * (c0 + q) + 1]);
                double* s = e + CV_NS * q;
                s[0] += y;
                s[1] = fma(y, y, s[1]);
                s[2] += da;
                s[3] = fma(da, da, s[3]);
                s[4] = fma(y, da, s[4]);
                s[5] += db;
                s[6] = fma(db, db, s[6]);
                s[7] = fma(y, db, s[7]);
                s[8] = fma(da, db, s[8]);
            }
        }
    });
}

static int launch_gbm_twin_stats(mcg_ctx* ctx, const mcg_gbm_twin* tw, int n_steps, int first_row, int64_t n_paths, double* d_stats) {
    const int64_t n_blocks = launch_blocks(n_paths, CV_PPL);
    if (n_blocks < 0) return MCG_ERR_INVALID;
    TwinArgs t;
    t.out5 = d_stats;
    t.n_paths = n_paths;
    t.n_steps = n_steps;
    t.first_row = first_row;
    t.path_begin = tw->path_begin;
    t.k0 = (uint32_t)tw->seed;
    t.k1 = (uint32_t)(tw->seed >> 32);
    t.S0 = tw->S0;
    t.a = tw->sigma * std::sqrt(tw->dt);
    t.m = (tw->r - tw->q - 0.5 * tw->sigma * tw->sigma) * tw->dt;
    t.tabs = (const double2*)ctx->log_tab;
    return PathLaunch{ctx, n_blocks}.run(
        MCG_K_EXOTIC, [&] { hipLaunchKernelGGL(k_gbm_twin_stats, dim3((unsigned)n_blocks), dim3(256), 0, ctx->stream, t); });
}

static int twin_check(const mcg_gbm_twin* tw) {
    if (!(std::isfinite(tw->S0) && std::isfinite(tw->r) && std::isfinite(tw->q) && std::isfinite(tw->sigma) && std::isfinite(tw->dt)))
        return fail(MCG_ERR_INVALID, "gbm twin: S0, r, q, sigma and dt must be finite");
    if (!(tw->S0 > 0.0) || !(tw->dt > 0.0) || tw->sigma < 0.0)
        return fail(MCG_ERR_INVALID, "gbm twin: S0 and dt must be positive, sigma >= 0 (got %g, %g, %g)", tw->S0, tw->dt, tw->sigma);
    return MCG_OK;
}

static int run_gbm_twin_stats(mcg_ctx* ctx, const mcg_gbm_twin* tw, int n_steps, int first_row, int64_t n_paths, double* host_out5) {
    return download_stats(ctx, n_paths, host_out5, "twin",
                          [&](double* d) { return launch_gbm_twin_stats(ctx, tw, n_steps, first_row, n_paths, d); });
}

// Workspace (one pool buffer): [5 n statistics][5 n twin statistics, with a twin][n_chunks * n_blocks * CV_NF partials]
// [9 n_contracts + 1 sums].  Parameters (ctx->weights): [book][controls][ctrl].
static int exotic_cv_sums(mcg_ctx* ctx, const mcg_paths* P, const mcg_paths* TP, const mcg_gbm_twin* tw, int first_row,
                          const mcg_exotic* book, int nc, const mcg_control* controls, int n_controls, const int* ctrl,
                          std::vector<double>& h) {
    const int64_t n = P->n_paths;
    const bool twin = TP || tw;
    const int n_sums = CV_NS * nc + 1, n_chunks = (nc + CV_CH - 1) / CV_CH;
    const int n_blocks = book_blocks(ctx, n);
    const size_t n_part = (size_t)n_chunks * n_blocks * CV_NF;
    const size_t n_stats = (size_t)CV_Q * n * (twin ? 2 : 1);
    const size_t book_d = (size_t)nc * sizeof(mcg_exotic) / sizeof(double), ctl_d = (size_t)n_controls * sizeof(mcg_control) / sizeof(double);
    std::vector<double> params(book_d + ctl_d + (size_t)nc);  // 2 nc ints are nc doubles
    std::memcpy(params.data(), book, (size_t)nc * sizeof(mcg_exotic));
    if (n_controls) std::memcpy(params.data() + book_d, controls, (size_t)n_controls * sizeof(mcg_control));
    std::memcpy(params.data() + book_d + ctl_d, ctrl, (size_t)nc * 2 * sizeof(int));
    return exotic_sums_frame(ctx, n, n_stats + n_part + n_sums, n_sums, h, [&](double* d_stats, double* d_sums) -> int {
        double *d_twin = twin ? d_stats + CV_Q * n : nullptr, *d_part = d_stats + n_stats;
        bool geo = std::any_of(book, book + nc, [](const mcg_exotic& c) { return reads_g(c); }), geo_twin = false;
        for (int k = 0; k < n_controls; ++k)
            if (reads_g(controls[k])) (controls[k].on_twin ? geo_twin : geo) = true;
        HostPiece up[] = {{params.data(), params.size() * sizeof(double)}};
        int rc = upload_params(ctx, up);
        if (rc) return rc;
        rc = launch_path_stats(ctx, P, first_row, geo, d_stats);
        if (rc) return rc;
        if (TP) rc = launch_path_stats(ctx, TP, first_row, geo_twin, d_twin);
        else if (tw) rc = launch_gbm_twin_stats(ctx, tw, P->n_steps, first_row, n, d_twin);
        if (rc) return rc;
        {
            TimedLaunch t(ctx, MCG_K_EXOTIC, 2);
            hipLaunchKernelGGL(k_exotic_book_cv, dim3(n_blocks, n_chunks), dim3(256), 0, ctx->stream, d_stats, d_twin, n, geo ? 1 : 0,
                               (geo_twin || tw) ? 1 : 0, reinterpret_cast<const mcg_exotic*>(up[0].at),
                               reinterpret_cast<const mcg_control*>(up[0].at + book_d), reinterpret_cast<const int*>(up[0].at + book_d + ctl_d),
                               nc, d_part);
            hipLaunchKernelGGL((k_book_reduce<CV_CH, CV_NS>), dim3(n_chunks), dim3(256), 0, ctx->stream, d_part, n_blocks, nc, (double)n, d_sums);
        }
        MCG_HIP(hipGetLastError());
        return MCG_OK;
    });
}

}  // namespace mcg

using namespace mcg;

int mcg_gbm_twin_stats(mcg_ctx* ctx, const mcg_gbm_twin* twin, int n_steps, int first_row, int64_t n_paths, double* host_out5) {
    if (!ctx || !twin || !host_out5) return fail(MCG_ERR_INVALID, "ctx/twin/host_out5 is NULL");
    int rc = twin_check(twin);
    if (rc) return rc;
    if (n_steps < 1) return fail(MCG_ERR_INVALID, "n_steps must be >= 1 (got %d)", n_steps);
    if (first_row < 0 || first_row > n_steps) return fail(MCG_ERR_INVALID, "first_row must be in [0, n_steps = %d] (got %d)", n_steps, first_row);
    if (n_paths < 1) return fail(MCG_ERR_EMPTY_PATHS, "no paths to take statistics of");
    MCG_HIP(hipSetDevice(ctx->device));
    return run_gbm_twin_stats(ctx, twin, n_steps, first_row, n_paths, host_out5);
}

int mcg_price_exotics_cv(mcg_ctx* ctx, const mcg_paths* P, const mcg_paths* twin_paths, const mcg_gbm_twin* gbm_twin, double r, double T,
                         int first_row, const mcg_exotic* book, int n_contracts, const mcg_control* controls, int n_controls,
                         const int* ctrl, double* price, double* std_err, double* beta, double* plain_price, double* plain_se,
                         double* sums) {
    int rc = exotic_args(ctx, P, first_row);
    if (rc) return rc;
    if (!book || !price || !ctrl) return fail(MCG_ERR_INVALID, "book/price/ctrl is NULL");
    if (n_contracts < 1 || n_contracts > 1024) return fail(MCG_ERR_INVALID, "n_contracts must be in [1, 1024] (got %d)", n_contracts);
    if (n_controls < 0 || n_controls > 1024) return fail(MCG_ERR_INVALID, "n_controls must be in [0, 1024] (got %d)", n_controls);
    if (n_controls > 0 && !controls) return fail(MCG_ERR_INVALID, "controls is NULL");
    for (int c = 0; c < n_contracts; ++c) {
        rc = exotic_contract_check(book[c], "contract", c);
        if (rc) return rc;
    }
    if (twin_paths && gbm_twin) return fail(MCG_ERR_INVALID, "a twin matrix and an in-register twin were both given");
    if (twin_paths) {
        if (twin_paths->ctx != ctx) return fail(MCG_ERR_INVALID, "the twin matrix belongs to a different ctx");
        if (twin_paths->n_paths != P->n_paths || twin_paths->n_steps != P->n_steps)
            return fail(MCG_ERR_INVALID, "the twin matrix is %lld x %d, the paths are %lld x %d", (long long)twin_paths->n_paths,
                        twin_paths->n_steps, (long long)P->n_paths, P->n_steps);
    }
    if (gbm_twin) {
        rc = twin_check(gbm_twin);
        if (rc) return rc;
    }
    for (int k = 0; k < n_controls; ++k) {
        const mcg_control& x = controls[k];
        if (x.form < MCG_CV_PAYOFF || x.form > MCG_CV_G) return fail(MCG_ERR_INVALID, "control %d: form must be in [0, 4] (got %d)", k, x.form);
        if (x.on_twin && !twin_paths && !gbm_twin) return fail(MCG_ERR_INVALID, "control %d is on the twin, and no twin was given", k);
        if (!std::isfinite(x.mean)) return fail(MCG_ERR_INVALID, "control %d: mean must be finite", k);
        if (x.form == MCG_CV_PAYOFF) {
            rc = exotic_contract_check(x.x, "control", k);
            if (rc) return rc;
        } else if (x.form == MCG_CV_VANILLA && !std::isfinite(x.x.K)) {
            return fail(MCG_ERR_INVALID, "control %d: K must be finite", k);
        }
    }
    for (int c = 0; c < n_contracts; ++c) {
        for (int s = 0; s < 2; ++s)
            if (ctrl[2 * c + s] < -1 || ctrl[2 * c + s] >= n_controls)
                return fail(MCG_ERR_INVALID, "contract %d: control index %d is outside [-1, %d)", c, ctrl[2 * c + s], n_controls);
        if (ctrl[2 * c + 1] >= 0 && ctrl[2 * c] < 0) return fail(MCG_ERR_INVALID, "contract %d: a second control needs a first one", c);
    }
    if (P->n_paths < 1 && !ctx->allreduce) return fail(MCG_ERR_EMPTY_PATHS, "no paths to price");
    MCG_HIP(hipSetDevice(ctx->device));
    std::vector<double> h;
    rc = exotic_cv_sums(ctx, P, twin_paths, gbm_twin, first_row, book, n_contracts, controls, n_controls, ctrl, h);
    if (rc) return rc;
    rc = mcg_exotics_cv_from_sums(h.data(), n_contracts, ctrl, r, T, price, std_err, beta, plain_price, plain_se);
    if (rc) return rc;
    if (sums) std::copy(h.begin(), h.end(), sums);
    return MCG_OK;
}
