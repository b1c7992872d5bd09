// Path-dependent European payoffs (mcg_path_stats, mcg_price_exotics): ONE pass over the monitored rows of the step-major
// matrix reduces every path to {S_T, arithmetic mean, geometric mean, min, max} (k_path_stats: a pure HBM-read stream of
// 8 B per path and date, 40 B per path written); a book of contracts is then evaluated on those statistics
// (k_exotic_book: per-block {sum, sum^2} of every contract's payoff through block_sum, k_book_reduce: fixed order).
// No float atomics: repeated calls are bit-identical, and a contract's sums do not depend on the rest of the book.
// The scan, the entry of a per-path kernel, the book's frame and the reduction are exotic_device.hpp's.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "devmath.hpp"
#include "exotic_device.hpp"
#include "paths_host.hpp"

namespace mcg {

constexpr int XS_Q = 5;      // statistics per path: 0 S_T, 1 A, 2 G, 3 min, 4 max

// One lane per W adjacent paths (lane_paths): path_scan without the tangent statistics.
template <bool GEO, int W>
__global__ __launch_bounds__(256) void k_path_stats(const double* data, int64_t ld, int64_t n_paths, int first_row, int n_rows,
                                                    double* out5) {
    const double* rows = data + (int64_t)first_row * ld;
    lane_paths<W>(n_paths, [&](int64_t p0, int64_t n, auto w) {
        path_scan<GEO, false, false, w.value>(rows + p0, data + p0, ld, first_row, n_rows, n, p0, out5);
    });
}

// blockIdx.y: a chunk of XB_CH contracts; blockIdx.x strides over the paths (book_partials).
// partials[(chunk * gridDim.x + blockIdx.x) * XB_NF + XB_NS * q + {0: sum, 1: sum of squares}] of the chunk's contract q
__global__ __launch_bounds__(256) void k_exotic_book(const double* stats, int64_t n, int geo, const mcg_exotic* book, int n_contracts,
                                                     double* partials) {
    __shared__ double red[XB_NF * 4];
    const int c0 = blockIdx.y * XB_CH;
    const int live = min(XB_CH, n_contracts - c0);
    book_partials<XB_NF>(n, red, partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * XB_NF, [&](int64_t i, double (&e)[XB_NF]) {
        const double st = stats[i], A = stats[n + i], G = geo ? stats[2 * n + i] : 0.0, mn = stats[3 * n + i], mx = stats[4 * n + i];
#pragma unroll
        for (int q = 0; q < XB_CH; ++q) {
            if (q < live) {
                const double x = exotic_payoff(book[c0 + q], st, A, G, mn, mx);
                e[XB_NS * q] += x;
                e[XB_NS * q + 1] = fma(x, x, e[XB_NS * q + 1]);
            }
        }
    });
}

void enqueue_exotic_reduce(mcg_ctx* ctx, const double* d_part, int n_blocks, int n_contracts, double n_local, double* d_sums) {
    hipLaunchKernelGGL((k_book_reduce<XB_CH, XB_NS>), dim3((n_contracts + XB_CH - 1) / XB_CH), dim3(256), 0, ctx->stream, d_part, n_blocks,
                       n_contracts, n_local, d_sums);
}

int launch_path_stats(mcg_ctx* ctx, const mcg_paths* P, int first_row, bool geo, double* d_stats) {
    const int n_rows = P->n_steps - first_row + 1;
    const StreamGrid g = stream_grid(P);
    if (g.n_blocks < 0) return MCG_ERR_INVALID;
    return PathLaunch{ctx, g.n_blocks}.run(MCG_K_EXOTIC, [&] {
        dispatch_flags(
            [&](auto geo_, auto w) {
                hipLaunchKernelGGL((k_path_stats<geo_.value, w.value ? 2 : 1>), dim3((unsigned)g.n_blocks), dim3(256), 0, ctx->stream, P->data,
                                   P->ld, P->n_paths, first_row, n_rows, d_stats);
            },
            geo, g.wide);
    });
}

int download_stats(mcg_ctx* ctx, int64_t n_paths, double* host_out5, const char* what, const std::function<int(double*)>& launch,
                   int n_stats) {
    const size_t bytes = (size_t)n_stats * n_paths * sizeof(double);
    void* ws = nullptr;
    int rc = pool_alloc(ctx, bytes, &ws);
    if (rc) return rc;
    rc = launch((double*)ws);
    if (rc == MCG_OK) {
        hipError_t e = hipMemcpyAsync(host_out5, ws, bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = fail(MCG_ERR_HIP, "download of the %s statistics failed: %s", what, hipGetErrorString(e));
    } else {
        (void)hipStreamSynchronize(ctx->stream);
    }
    pool_release(ctx, ws, bytes);
    return rc;
}

int run_path_stats(mcg_ctx* ctx, const mcg_paths* P, int first_row, double* host_out5) {
    return download_stats(ctx, P->n_paths, host_out5, "path", [&](double* d) { return launch_path_stats(ctx, P, first_row, true, d); });
}

// The all-reduce of a payload that may exceed what the node-local collective carries in one call.
int exotic_allreduce_sums(mcg_ctx* ctx, double* d, int count) {
    const int piece = ctx->shm ? SHM_ALLREDUCE_MAX : count;
    for (int at = 0; at < count; at += piece)
        if (ctx->allreduce(ctx->allreduce_user, d + at, std::min(piece, count - at), (void*)ctx->stream) != 0)
            return fail(MCG_ERR_COMM, "all-reduce of the exotic payoff sums failed");
    return MCG_OK;
}

// Workspace (one pool buffer): [5 n statistics][n_chunks * n_blocks * XB_NF partials][2 n_contracts + 1 sums].
static int exotic_sums(mcg_ctx* ctx, const mcg_paths* P, int first_row, const mcg_exotic* book, int nc, std::vector<double>& h) {
    const int64_t n = P->n_paths;
    const int n_sums = 2 * nc + 1, n_chunks = (nc + XB_CH - 1) / XB_CH;
    const int n_blocks = book_blocks(ctx, n);
    const size_t n_part = (size_t)n_chunks * n_blocks * XB_NF;
    return exotic_sums_frame(ctx, n, (size_t)XS_Q * n + n_part + n_sums, n_sums, h, [&](double* d_stats, double* d_sums) -> int {
        double* d_part = d_stats + XS_Q * n;
        const bool geo = std::any_of(book, book + nc, [](const mcg_exotic& c) { return reads_g(c); });
        HostPiece up[] = {{book, (size_t)nc * sizeof(mcg_exotic)}};
        int rc = upload_params(ctx, up);
        if (rc) return rc;
        rc = launch_path_stats(ctx, P, first_row, geo, d_stats);
        if (rc) return rc;
        {
            TimedLaunch t(ctx, MCG_K_EXOTIC, 2);
            hipLaunchKernelGGL(k_exotic_book, dim3(n_blocks, n_chunks), dim3(256), 0, ctx->stream, d_stats, n, geo ? 1 : 0,
                               reinterpret_cast<const mcg_exotic*>(up[0].at), nc, d_part);
            enqueue_exotic_reduce(ctx, d_part, n_blocks, nc, (double)n, d_sums);
        }
        MCG_HIP(hipGetLastError());
        return MCG_OK;
    });
}

int exotic_sums_frame(mcg_ctx* ctx, int64_t n, size_t ws_doubles, int n_sums, std::vector<double>& h,
                      const std::function<int(double* ws, double* d_sums)>& fill) {
    void* ws = nullptr;
    int rc = pool_alloc(ctx, ws_doubles * sizeof(double), &ws);
    if (rc) return rc;
    double* d_sums = (double*)ws + (ws_doubles - n_sums);
    auto body = [&]() -> int {
        if (n > 0) {
            const int r2 = fill((double*)ws, d_sums);
            if (r2) return r2;
        } else {
            MCG_HIP(hipMemsetAsync(d_sums, 0, n_sums * sizeof(double), ctx->stream));
        }
        if (ctx->allreduce) {
            const int r2 = exotic_allreduce_sums(ctx, d_sums, n_sums);
            if (r2) return r2;
        }
        h.resize(n_sums);
        MCG_HIP(hipMemcpyAsync(h.data(), d_sums, n_sums * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MCG_HIP(hipStreamSynchronize(ctx->stream));
        return MCG_OK;
    };
    rc = body();
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    pool_release(ctx, ws, ws_doubles * sizeof(double));
    return rc;
}

int run_exotics(mcg_ctx* ctx, const mcg_paths* P, double r, double T, int first_row, const mcg_exotic* book, int nc, double* price,
                double* std_err, double* sums) {
    std::vector<double> h;
    const int rc = exotic_sums(ctx, P, first_row, book, nc, h);
    if (rc) return rc;
    return exotic_prices_from_sums(h, nc, nullptr, r, T, price, std_err, sums);
}

int exotic_prices_from_sums(const std::vector<double>& h, int nc, const int* order, double r, double T, double* price, double* std_err,
                            double* sums) {
    const double n = h[2 * (size_t)nc];
    if (!(n >= 1.0)) return fail(MCG_ERR_EMPTY_PATHS, "no paths to price");
    const double disc = std::exp(-r * T);
    for (int s = 0; s < nc; ++s) {
        const int c = order ? order[s] : s;
        double se;
        sums_to_mean_stderr(h[2 * (size_t)s], h[2 * (size_t)s + 1], n, &price[c], &se);
        price[c] = disc * price[c];
        if (std_err) std_err[c] = disc * se;
        if (sums) {
            sums[2 * (size_t)c] = h[2 * (size_t)s];
            sums[2 * (size_t)c + 1] = h[2 * (size_t)s + 1];
        }
    }
    if (sums) sums[2 * (size_t)nc] = n;
    return MCG_OK;
}

}  // namespace mcg
