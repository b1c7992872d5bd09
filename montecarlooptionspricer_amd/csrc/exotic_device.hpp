// What the consumers of the step-major matrix in the exotics family share (kernels_exotic.hip, kernels_exotic_cv.hip,
// kernels_exotic_greeks.hip, kernels_barrier_bridge.hip), each stated once:
//   xs_load, xs_split, path_scan   the streaming scan that reduces a path to its statistics (k_path_stats, k_path_tangent_stats)
//   lane_paths                     the entry of a kernel with one lane per W adjacent paths (those two and k_bridge_survival)
//   exotic_payoff                  the payoff of one mcg_exotic contract on a path's five statistics
//   bridge_payoff                  the sample of a barrier contract from S_T and a Brownian-bridge survival probability
//   book_partials                  the frame of a book kernel: per-block partial sums of NF accumulators over the paths
//   k_book_reduce                  the fixed-order reduction of a book kernel's partials into per-contract sums
// Device-only code for gfx950.
#pragma once
#include <limits>

#include "../../include/mcgpu.h"
#include "devmath.hpp"

namespace mcg {

typedef double xs_d2 __attribute__((ext_vector_type(2)));

constexpr int XS_ROWS = 8;   // rows per unrolled group: 8 x 16 B in flight per lane, 32 KiB per workgroup
// The book layout of k_exotic_book and k_bridge_book (kernels_barrier_bridge.hip): {sum, sum of squares} per contract
constexpr int XB_CH = 8;     // contracts one workgroup of a book kernel keeps in registers
constexpr int XB_NS = 2;     // sums per contract
constexpr int XB_NF = XB_NS * XB_CH;

template <int W>
__device__ __forceinline__ void xs_load(const double* p, double (&x)[W]) {
    if constexpr (W == 2) {
        const xs_d2 v = __builtin_nontemporal_load(reinterpret_cast<const xs_d2*>(p));
        x[0] = v.x;
        x[1] = v.y;
    } else {
        x[0] = __builtin_nontemporal_load(p);
    }
}

// x = m 2^k with m in [1, 2), for a positive normal x: returns m and adds k to e (three integer instructions, no log).
__device__ __forceinline__ double xs_split(double x, int& e) {
    const int hi = __double2hiint(x);
    e += ((hi >> 20) & 0x7ff) - 1023;
    return __hiloint2double((hi & 0x000fffff) | 0x3ff00000, __double2loint(x));
}

// Statistics of W adjacent paths over n_rows rows from col on; row0 is the same lane's place in row 0 of the matrix (read
// with LOGS only).  out: [5][n_paths] {S_T, A, G (with GEO), min, max}, with TAN [10][n_paths]: those and {L, J, j_min,
// j_max, Q}.  The rows of a group of XS_ROWS are loaded first and then combined pairwise (sum, min, max, product of
// mantissas, with TAN J's terms), so a group costs one dependent step per accumulator.  The first five statistics take the
// same operations in the same order whatever TAN and LOGS are: mcg_path_tangent_stats' are bit-identical to mcg_path_stats'.
// Geometric mean: prod (renormalised to [1, 2) after every group) and the exponent sum carry ln of the product exactly up
// to the roundings of the n_rows multiplications; ONE log per path at the end.  A path that holds a value below the
// smallest normal double (zero, subnormal, negative) is rescanned with a log per element: exp(mean(log S)) as written.
// TAN, per group: the first row of the group that holds the group's minimum (maximum) by comparing the rows against it from
// the last to the first, taken over only where the group's minimum is strictly below the running one -- the values of min
// and max are fmin's and fmax's as before, ties go to the lowest row.
// LOGS: one logarithm per element feeds L (x ln x) and Q (the squared difference to the row before, rows below first_row
// included: they are walked first, one row at a time).
template <bool GEO, bool TAN, bool LOGS, int W>
__device__ __forceinline__ void path_scan(const double* col, const double* row0, int64_t ld, int first_row, int n_rows, int64_t n_paths,
                                          int64_t p0, double* out) {
    static_assert(GEO || !TAN, "the tangent statistics include G");
    static_assert(TAN || !LOGS, "L and Q are tangent statistics");
    double sum[W], mn[W], mx[W], last[W], prod[W], sj[W], sl[W], qq[W], lprev[W];
    long long es[W];
    int imn[W], imx[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        sum[w] = 0.0;
        mn[w] = std::numeric_limits<double>::infinity();
        mx[w] = -std::numeric_limits<double>::infinity();
        last[w] = 0.0;
        prod[w] = 1.0;
        es[w] = 0;
        sj[w] = 0.0;
        sl[w] = 0.0;
        qq[w] = 0.0;
        lprev[w] = 0.0;
        imn[w] = 0;
        imx[w] = 0;
    }
    if constexpr (LOGS) {
        // ln of row 0, then the steps that end below first_row.  With first_row = 0 the scan's first row is row 0 again: its
        // difference to lprev is exactly zero.
        double x[W];
        xs_load<W>(row0, x);
#pragma unroll
        for (int w = 0; w < W; ++w) lprev[w] = log(x[w]);
        for (int i = 1; i < first_row; ++i) {
            xs_load<W>(row0 + (int64_t)i * ld, x);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const double l = log(x[w]), d = l - lprev[w];
                qq[w] = fma(d, d, qq[w]);
                lprev[w] = l;
            }
        }
    }
    int j = 0;
    for (; j + XS_ROWS <= n_rows; j += XS_ROWS) {
        double x[XS_ROWS][W];
#pragma unroll
        for (int k = 0; k < XS_ROWS; ++k) xs_load<W>(col + (int64_t)(j + k) * ld, x[k]);
        const double jd = (double)(first_row + j);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            double s[XS_ROWS], lo[XS_ROWS], hi[XS_ROWS], m[XS_ROWS], t[XS_ROWS];
            int e = 0;
#pragma unroll
            for (int k = 0; k < XS_ROWS; ++k) {
                s[k] = lo[k] = hi[k] = x[k][w];
                if constexpr (GEO) m[k] = xs_split(x[k][w], e);
                if constexpr (TAN) t[k] = (jd + (double)k) * x[k][w];
            }
#pragma unroll
            for (int h = XS_ROWS / 2; h >= 1; h >>= 1) {
#pragma unroll
                for (int k = 0; k < h; ++k) {
                    s[k] += s[k + h];
                    lo[k] = fmin(lo[k], lo[k + h]);
                    hi[k] = fmax(hi[k], hi[k + h]);
                    if constexpr (GEO) m[k] *= m[k + h];
                    if constexpr (TAN) t[k] += t[k + h];
                }
            }
            if constexpr (TAN) {
                int klo = XS_ROWS - 1, khi = XS_ROWS - 1;
#pragma unroll
                for (int k = XS_ROWS - 2; k >= 0; --k) {
                    klo = x[k][w] == lo[0] ? k : klo;
                    khi = x[k][w] == hi[0] ? k : khi;
                }
                imn[w] = lo[0] < mn[w] ? j + klo : imn[w];
                imx[w] = hi[0] > mx[w] ? j + khi : imx[w];
            }
            sum[w] += s[0];
            mn[w] = fmin(mn[w], lo[0]);
            mx[w] = fmax(mx[w], hi[0]);
            last[w] = x[XS_ROWS - 1][w];
            if constexpr (GEO) {
                prod[w] = xs_split(prod[w] * m[0], e);  // < 2 * 2^8 before, [1, 2) after
                es[w] += e;
            }
            if constexpr (TAN) sj[w] += t[0];
            if constexpr (LOGS) {
#pragma unroll
                for (int k = 0; k < XS_ROWS; ++k) {
                    const double l = log(x[k][w]), d = l - lprev[w];
                    qq[w] = fma(d, d, qq[w]);
                    sl[w] = fma(x[k][w], l, sl[w]);
                    lprev[w] = l;
                }
            }
        }
    }
    for (; j < n_rows; ++j) {  // at most XS_ROWS - 1 rows: prod stays below 2^8
        double x[W];
        xs_load<W>(col + (int64_t)j * ld, x);
        const double jd = (double)(first_row + j);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            if constexpr (TAN) {
                imn[w] = x[w] < mn[w] ? j : imn[w];
                imx[w] = x[w] > mx[w] ? j : imx[w];
            }
            sum[w] += x[w];
            mn[w] = fmin(mn[w], x[w]);
            mx[w] = fmax(mx[w], x[w]);
            last[w] = x[w];
            if constexpr (GEO) {
                int e = 0;
                prod[w] *= xs_split(x[w], e);
                es[w] += e;
            }
            if constexpr (TAN) sj[w] = fma(jd, x[w], sj[w]);
            if constexpr (LOGS) {
                const double l = log(x[w]), d = l - lprev[w];
                qq[w] = fma(d, d, qq[w]);
                sl[w] = fma(x[w], l, sl[w]);
                lprev[w] = l;
            }
        }
    }
    const double nd = (double)n_rows, nan = std::numeric_limits<double>::quiet_NaN();
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int64_t p = p0 + w;
        out[0 * n_paths + p] = last[w];
        out[1 * n_paths + p] = sum[w] / nd;
        out[3 * n_paths + p] = mn[w];
        out[4 * n_paths + p] = mx[w];
        if constexpr (GEO) {
            double ls = (double)es[w] * 0.6931471805599453094 + log(prod[w]);
            if (!(mn[w] >= std::numeric_limits<double>::min())) {
                ls = 0.0;
                for (int k = 0; k < n_rows; ++k) ls += log(col[(int64_t)k * ld + w]);
            }
            out[2 * n_paths + p] = exp(ls / nd);
        }
        if constexpr (TAN) {
            out[5 * n_paths + p] = LOGS ? sl[w] / nd : nan;
            out[6 * n_paths + p] = sj[w] / nd;
            out[7 * n_paths + p] = (double)(first_row + imn[w]);
            out[8 * n_paths + p] = (double)(first_row + imx[w]);
            out[9 * n_paths + p] = LOGS ? qq[w] : nan;
        }
    }
}

// The entry of a kernel with one lane per W adjacent paths (the grid of stream_grid, paths_host.hpp): scan(p0, n_paths, w)
// with w an integral_constant, W paths from p0 on -- or one, where W = 2 and the last path of an odd count stands alone.
// W = 2 needs 16-byte aligned rows (even ld, aligned base: what paths_new makes).  n_paths goes to scan as an argument so
// that a scan which indexes its output by it uses the very value tested here: the compiler then knows 0 <= p0 < n_paths in
// the scan's address arithmetic, which a copy of n_paths captured by the callable does not tell it.
template <int W, class Scan>
__device__ __forceinline__ void lane_paths(int64_t n_paths, Scan&& scan) {
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * W;
    if (p0 >= n_paths) return;
    if (W == 2 && p0 + 1 == n_paths) scan(p0, n_paths, std::integral_constant<int, 1>{});
    else scan(p0, n_paths, std::integral_constant<int, W>{});
}

// The undiscounted payoffs of include/mcgpu.h, on one path's statistics.  Strike and barrier tests are plain comparisons
// of the stored doubles.
__device__ __forceinline__ double exotic_payoff(const mcg_exotic& c, double st, double A, double G, double mn, double mx) {
    const bool call = c.is_call != 0;
    switch (c.kind) {
        case MCG_X_ASIAN_ARITH_FIXED: return payoff_of(call, A, c.K);
        case MCG_X_ASIAN_ARITH_FLOAT: return payoff_of(call, st, A);
        case MCG_X_ASIAN_GEO_FIXED: return payoff_of(call, G, c.K);
        case MCG_X_ASIAN_GEO_FLOAT: return payoff_of(call, st, G);
        case MCG_X_LOOKBACK_FIXED: return call ? fmax(0.0, mx - c.K) : fmax(0.0, c.K - mn);
        case MCG_X_LOOKBACK_FLOAT: return call ? st - mn : mx - st;
        default: {
            const bool up = c.kind == MCG_X_BARRIER_UP_OUT || c.kind == MCG_X_BARRIER_UP_IN;
            const bool in = c.kind == MCG_X_BARRIER_UP_IN || c.kind == MCG_X_BARRIER_DOWN_IN;
            const bool hit = up ? mx >= c.barrier : mn <= c.barrier;
            return hit == in ? payoff_of(call, st, c.K) : c.rebate;
        }
    }
}

// The sample of a barrier contract from a Brownian-bridge survival probability p (k_bridge_book, k_mlmc_book): the vanilla
// payoff f on S_T weighted by p, the rebate by its complement; an in contract the other way round
__device__ __forceinline__ double bridge_payoff(const mcg_exotic& c, double st, double p) {
    const double f = payoff_of(c.is_call != 0, st, c.K), q = 1.0 - p;
    const bool in = c.kind == MCG_X_BARRIER_UP_IN || c.kind == MCG_X_BARRIER_DOWN_IN;
    return in ? f * q + c.rebate * p : f * p + c.rebate * q;
}

// The frame of a book kernel (256 lanes): NF accumulators from zero, per_path(i, e) for the paths i = this lane's place in
// a grid-stride walk of blockIdx.x over n, block_sum (red: NF * 4 doubles of LDS), and thread 0 stores field q into out[q]
// where keep(q).  The grid over the paths depends on the path count only (book_blocks), and block_sum's total of a value
// does not depend on its index: a contract's partial sums are the same whatever else the book holds and wherever it stands.
template <int NF, class PerPath, class Keep>
__device__ __forceinline__ void book_partials(int64_t n, double* red, double* out, PerPath&& per_path, Keep&& keep) {
    double e[NF];
#pragma unroll
    for (int q = 0; q < NF; ++q) e[q] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) per_path(i, e);
    block_sum<NF, 4>(e, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NF; ++q)
            if (keep(q)) out[q] = e[q];
    }
}
template <int NF, class PerPath>
__device__ __forceinline__ void book_partials(int64_t n, double* red, double* out, PerPath&& per_path) {
    book_partials<NF>(n, red, out, per_path, [](int) { return true; });
}

// partials[(chunk * n_blocks + block) * CH * NS + NS * q + k], sum k of the chunk's contract q -> sums[NS * contract + k],
// then the local path count.  One workgroup per chunk of CH contracts, like k_greeks_reduce: wave w takes the fields w,
// w + 4, ...; lane l the blocks l, l + 64, ..., then the butterfly.
template <int CH, int NS>
__global__ __launch_bounds__(256) void k_book_reduce(const double* partials, int n_blocks, int n_contracts, double n_local, double* sums) {
    constexpr int NF = CH * NS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* src = partials + (int64_t)blockIdx.x * n_blocks * NF;
    for (int q = wave; q < NF; q += 4) {
        double s = 0.0;
        for (int b = lane; b < n_blocks; b += 64) s += src[(int64_t)b * NF + q];
        s = wave_sum(s);
        const int c = blockIdx.x * CH + q / NS;
        if (lane == 0 && c < n_contracts) sums[NS * c + q % NS] = s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) sums[NS * n_contracts] = n_local;
}

}  // namespace mcg
