// Path-dependent European payoffs (mcg_path_stats, mcg_price_exotics): ONE pass over the monitored rows of the step-major
// matrix reduces every path to {S_T, arithmetic mean, geometric mean, min, max} (k_path_stats: a pure HBM-read stream of
// 8 B per path and date, 40 B per path written); a book of contracts is then evaluated on those statistics
// (k_exotic_book: per-block {sum, sum^2} of every contract's payoff through block_sum, k_exotic_reduce: fixed order).
// No float atomics: repeated calls are bit-identical, and a contract's sums do not depend on the rest of the book.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "devmath.hpp"
#include "exotic_device.hpp"
#include "paths_host.hpp"

namespace mcg {

constexpr int XS_Q = 5;      // statistics per path: 0 S_T, 1 A, 2 G, 3 min, 4 max

// Statistics of W adjacent paths over n_rows rows from col on.  The rows of a group of XS_ROWS are loaded first and then
// combined pairwise (sum, min, max, product of mantissas), so a group costs one dependent step per accumulator.
// Geometric mean: prod (renormalised to [1, 2) after every group) and the exponent sum carry ln of the product exactly up
// to the roundings of the n_rows multiplications; ONE log per path at the end.  A path that holds a value below the
// smallest normal double (zero, subnormal, negative) is rescanned with a log per element: exp(mean(log S)) as written.
template <bool GEO, int W>
__device__ __forceinline__ void path_stats_scan(const double* col, int64_t ld, int n_rows, int64_t n_paths, int64_t p0, double* out5) {
    double sum[W], mn[W], mx[W], last[W], prod[W];
    long long es[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        sum[w] = 0.0;
        mn[w] = std::numeric_limits<double>::infinity();
        mx[w] = -std::numeric_limits<double>::infinity();
        last[w] = 0.0;
        prod[w] = 1.0;
        es[w] = 0;
    }
    int j = 0;
    for (; j + XS_ROWS <= n_rows; j += XS_ROWS) {
        double x[XS_ROWS][W];
#pragma unroll
        for (int k = 0; k < XS_ROWS; ++k) xs_load<W>(col + (int64_t)(j + k) * ld, x[k]);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            double s[XS_ROWS], lo[XS_ROWS], hi[XS_ROWS], m[XS_ROWS];
            int e = 0;
#pragma unroll
            for (int k = 0; k < XS_ROWS; ++k) {
                s[k] = lo[k] = hi[k] = x[k][w];
                if constexpr (GEO) m[k] = xs_split(x[k][w], e);
            }
#pragma unroll
            for (int h = XS_ROWS / 2; h >= 1; h >>= 1) {
#pragma unroll
                for (int k = 0; k < h; ++k) {
                    s[k] += s[k + h];
                    lo[k] = fmin(lo[k], lo[k + h]);
                    hi[k] = fmax(hi[k], hi[k + h]);
                    if constexpr (GEO) m[k] *= m[k + h];
                }
            }
            sum[w] += s[0];
            mn[w] = fmin(mn[w], lo[0]);
            mx[w] = fmax(mx[w], hi[0]);
            last[w] = x[XS_ROWS - 1][w];
            if constexpr (GEO) {
                prod[w] = xs_split(prod[w] * m[0], e);  // < 2 * 2^8 before, [1, 2) after
                es[w] += e;
            }
        }
    }
    for (; j < n_rows; ++j) {  // at most XS_ROWS - 1 rows: prod stays below 2^8
        double x[W];
        xs_load<W>(col + (int64_t)j * ld, x);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            sum[w] += x[w];
            mn[w] = fmin(mn[w], x[w]);
            mx[w] = fmax(mx[w], x[w]);
            last[w] = x[w];
            if constexpr (GEO) {
                int e = 0;
                prod[w] *= xs_split(x[w], e);
                es[w] += e;
            }
        }
    }
    const double nd = (double)n_rows;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int64_t p = p0 + w;
        out5[0 * n_paths + p] = last[w];
        out5[1 * n_paths + p] = sum[w] / nd;
        out5[3 * n_paths + p] = mn[w];
        out5[4 * n_paths + p] = mx[w];
        if constexpr (GEO) {
            double ls = (double)es[w] * 0.6931471805599453094 + log(prod[w]);
            if (!(mn[w] >= std::numeric_limits<double>::min())) {
                ls = 0.0;
                for (int k = 0; k < n_rows; ++k) ls += log(col[(int64_t)k * ld + w]);
            }
            out5[2 * n_paths + p] = exp(ls / nd);
        }
    }
}

// One lane per W adjacent paths.  W = 2 needs 16-byte aligned rows (even ld, aligned base: what paths_new makes); the last
// path of an odd count is scanned alone by its lane.
template <bool GEO, int W>
__global__ __launch_bounds__(256) void k_path_stats(const double* data, int64_t ld, int64_t n_paths, int first_row, int n_rows,
                                                    double* out5) {
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * W;
    if (p0 >= n_paths) return;
    const double* col = data + (int64_t)first_row * ld + p0;
    if (W == 2 && p0 + 1 == n_paths) path_stats_scan<GEO, 1>(col, ld, n_rows, n_paths, p0, out5);
    else path_stats_scan<GEO, W>(col, ld, n_rows, n_paths, p0, out5);
}

// blockIdx.y: a chunk of XB_CH contracts; blockIdx.x strides over the paths (a grid that depends on the path count only:
// a contract's partial sums are the same whatever else the book holds and wherever it stands).
// partials[(chunk * gridDim.x + blockIdx.x) * XB_NF + {q: sum, XB_CH + q: sum of squares}]
__global__ __launch_bounds__(256) void k_exotic_book(const double* stats, int64_t n, int geo, const mcg_exotic* book, int n_contracts,
                                                     double* partials) {
    __shared__ double red[XB_NF * 4];
    const int c0 = blockIdx.y * XB_CH;
    const int live = min(XB_CH, n_contracts - c0);
    double e[XB_NF];
#pragma unroll
    for (int q = 0; q < XB_NF; ++q) e[q] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double st = stats[i], A = stats[n + i], G = geo ? stats[2 * n + i] : 0.0, mn = stats[3 * n + i], mx = stats[4 * n + i];
#pragma unroll
        for (int q = 0; q < XB_CH; ++q) {
            if (q < live) {
                const double x = exotic_payoff(book[c0 + q], st, A, G, mn, mx);
                e[q] += x;
                e[XB_CH + q] = fma(x, x, e[XB_CH + q]);
            }
        }
    }
    block_sum<XB_NF, 4>(e, red);
    if (threadIdx.x == 0) {
        double* out = partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * XB_NF;
#pragma unroll
        for (int q = 0; q < XB_NF; ++q) out[q] = e[q];
    }
}

// One workgroup per chunk, like k_greeks_reduce: wave w takes the fields w, w + 4, ...; lane l the blocks l, l + 64, ...,
// then the butterfly.  sums = {sum, sum^2} per contract, then the local path count.
__global__ __launch_bounds__(256) void k_exotic_reduce(const double* partials, int n_blocks, int n_contracts, double n_local, double* sums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* src = partials + (int64_t)blockIdx.x * n_blocks * XB_NF;
    for (int q = wave; q < XB_NF; q += 4) {
        double s = 0.0;
        for (int b = lane; b < n_blocks; b += 64) s += src[(int64_t)b * XB_NF + q];
        s = wave_sum(s);
        const int c = blockIdx.x * XB_CH + q % XB_CH;
        if (lane == 0 && c < n_contracts) sums[2 * c + q / XB_CH] = s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) sums[2 * n_contracts] = n_local;
}

void enqueue_exotic_reduce(mcg_ctx* ctx, const double* d_part, int n_blocks, int n_contracts, double n_local, double* d_sums) {
    hipLaunchKernelGGL(k_exotic_reduce, dim3((n_contracts + XB_CH - 1) / XB_CH), dim3(256), 0, ctx->stream, d_part, n_blocks, n_contracts,
                       n_local, d_sums);
}

int launch_path_stats(mcg_ctx* ctx, const mcg_paths* P, int first_row, bool geo, double* d_stats) {
    const int n_rows = P->n_steps - first_row + 1;
    const bool wide = (P->ld & 1) == 0 && (reinterpret_cast<uintptr_t>(P->data) & 15) == 0;
    const int64_t lanes = wide ? (P->n_paths + 1) / 2 : P->n_paths;
    const int64_t n_blocks = launch_units((lanes + 255) / 256);
    if (n_blocks < 0) return MCG_ERR_INVALID;
    return PathLaunch{ctx, n_blocks}.run(MCG_K_EXOTIC, [&] {
        dispatch_flags(
            [&](auto g, auto w) {
                hipLaunchKernelGGL((k_path_stats<g.value, w.value ? 2 : 1>), dim3((unsigned)n_blocks), dim3(256), 0, ctx->stream, P->data,
                                   P->ld, P->n_paths, first_row, n_rows, d_stats);
            },
            geo, wide);
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
    const int n_blocks = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)ctx->n_cus * 8));
    const size_t n_part = (size_t)n_chunks * n_blocks * XB_NF;
    return exotic_sums_frame(ctx, n, (size_t)XS_Q * n + n_part + n_sums, n_sums, h, [&](double* d_stats, double* d_sums) -> int {
        double* d_part = d_stats + XS_Q * n;
        bool geo = false;
        for (int c = 0; c < nc; ++c) geo = geo || book[c].kind == MCG_X_ASIAN_GEO_FIXED || book[c].kind == MCG_X_ASIAN_GEO_FLOAT;
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
    const double n = h[2 * nc];
    if (!(n >= 1.0)) return fail(MCG_ERR_EMPTY_PATHS, "no paths to price");
    const double disc = std::exp(-r * T);
    for (int c = 0; c < nc; ++c) {
        double se;
        sums_to_mean_stderr(h[2 * c], h[2 * c + 1], n, &price[c], &se);
        price[c] = disc * price[c];
        if (std_err) std_err[c] = disc * se;
    }
    if (sums) std::copy(h.begin(), h.end(), sums);
    return MCG_OK;
}

}  // namespace mcg
