// Greeks (mcg_greeks_european, mcg_greeks_lsm): one pass over the rows a Greek needs, per-block partial sums and sums of
// squares of the per-path estimators plus the range of row 0, then a fixed-order reduction in one block.  No float atomics:
// repeated calls are bit-identical.  The LSM tangent sweep itself is k_lsm_date<NB, true> (kernels_lsm.hip).
#include <algorithm>
#include <cmath>
#include <limits>

#include "devmath.hpp"
#include "greeks_device.hpp"
#include "mcg_internal.hpp"

namespace mcg {

// European: reads row 0 (S0) and row n_steps (S_T) once, 16 B per path.  Undiscounted per-path estimators:
//   0 payoff   1 f' S_T / S0 (delta)   2 1{S_T > K} W_T K / (S0^2 sigma T) (gamma)   3 f' S_T (W_T - sigma T) (vega)
//   4 T (f' S_T - payoff) (rho)   5 -f' (dual delta),   f' = 1{S_T > K} (call), -1{S_T < K} (put),
//   W_T = (ln(S_T / S0) - (r - sigma^2 / 2) T) / sigma  (gamma and vega only when sigma > 0; else 0).
constexpr int GK_EU = 6;
__global__ __launch_bounds__(256) void k_greeks_european(const double* row0, const double* rowT, int64_t n, double K, int is_call,
                                                         double r, double T, double sigma, double* partials) {
    __shared__ double red[2 * GK_EU * 4];
    const bool call = is_call != 0;
    const bool lr = sigma > 0.0;
    const double drift = (r - 0.5 * sigma * sigma) * T, inv_sigma = lr ? 1.0 / sigma : 0.0, sigma_t = sigma * T;
    const double gamma_scale = lr ? K / (sigma * T) : 0.0;
    double e[2 * GK_EU];
#pragma unroll
    for (int q = 0; q < 2 * GK_EU; ++q) e[q] = 0.0;
    double lo = std::numeric_limits<double>::infinity(), hi = -std::numeric_limits<double>::infinity();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double s0 = row0[i], st = rowT[i];
        lo = fmin(lo, s0);
        hi = fmax(hi, s0);
        const double pay = payoff_of(call, st, K);
        const double fp = call ? (st > K ? 1.0 : 0.0) : (st < K ? -1.0 : 0.0);
        double x[GK_EU];
        x[0] = pay;
        x[1] = fp * st / s0;
        x[2] = 0.0;
        x[3] = 0.0;
        if (lr) {
            const double w = (log(st / s0) - drift) * inv_sigma;
            x[2] = st > K ? w * gamma_scale / (s0 * s0) : 0.0;
            x[3] = fp * st * (w - sigma_t);
        }
        x[4] = T * (fp * st - pay);
        x[5] = -fp;
#pragma unroll
        for (int q = 0; q < GK_EU; ++q) {
            e[q] += x[q];
            e[GK_EU + q] = fma(x[q], x[q], e[GK_EU + q]);
        }
    }
    greeks_block_store<GK_EU>(e, lo, hi, red, partials + (int64_t)blockIdx.x * (2 * GK_EU + 2));
}

// LSM: per path V_0, dV_0 = dV_0/dK and the delta term (V_0 - K dV_0) / S0 (homogeneity of degree 1 in (S0, K)).
constexpr int GK_LSM = 3;
__global__ __launch_bounds__(256) void k_greeks_lsm(const double* V, const double* dV, const double* row0, int64_t n, double K,
                                                    double* partials) {
    __shared__ double red[2 * GK_LSM * 4];
    double e[2 * GK_LSM];
#pragma unroll
    for (int q = 0; q < 2 * GK_LSM; ++q) e[q] = 0.0;
    double lo = std::numeric_limits<double>::infinity(), hi = -std::numeric_limits<double>::infinity();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double s0 = row0[i], v = V[i], dv = dV[i];
        lo = fmin(lo, s0);
        hi = fmax(hi, s0);
        const double x[GK_LSM] = {v, dv, (v - K * dv) / s0};
#pragma unroll
        for (int q = 0; q < GK_LSM; ++q) {
            e[q] += x[q];
            e[GK_LSM + q] = fma(x[q], x[q], e[GK_LSM + q]);
        }
    }
    greeks_block_store<GK_LSM>(e, lo, hi, red, partials + (int64_t)blockIdx.x * (2 * GK_LSM + 2));
}

// partials[chunk][n_blocks][nf] -> out[chunk][nf], one workgroup per chunk (blockIdx.x; the European and LSM Greeks have
// one, the exotics book one per GX_CH contracts), in a fixed order: wave w takes the fields w, w + 4, ...; lane l the blocks
// l, l + 64, ..., then the butterfly.  The last two fields are a minimum and a maximum, the others sums.
__global__ __launch_bounds__(256) void k_greeks_reduce(const double* partials, int n_blocks, int nf, double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    partials += (int64_t)blockIdx.x * n_blocks * nf;
    out += (int64_t)blockIdx.x * nf;
    for (int q = wave; q < nf; q += 4) {
        const int kind = q == nf - 2 ? 1 : q == nf - 1 ? 2 : 0;  // 0 sum, 1 min, 2 max
        double s = kind == 0 ? 0.0 : kind == 1 ? std::numeric_limits<double>::infinity() : -std::numeric_limits<double>::infinity();
        for (int b = lane; b < n_blocks; b += 64) {
            const double x = partials[(int64_t)b * nf + q];
            s = kind == 0 ? s + x : kind == 1 ? fmin(s, x) : fmax(s, x);
        }
        if (kind == 0) {
            s = wave_sum(s);
        } else {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const double y = __shfl_xor(s, o);
                s = kind == 1 ? fmin(s, y) : fmax(s, y);
            }
        }
        if (lane == 0) out[q] = s;
    }
}

void enqueue_greeks_reduce(mcg_ctx* ctx, const double* d_part, int n_blocks, int nf, int n_chunks, double* d_out) {
    hipLaunchKernelGGL(k_greeks_reduce, dim3(n_chunks), dim3(256), 0, ctx->stream, d_part, n_blocks, nf, d_out);
}

// Reduce NE estimators' partials of n_blocks blocks and bring {sums, sums of squares, min, max of row 0} to the host.
static int greeks_reduce(mcg_ctx* ctx, int n_blocks, int ne, double* host) {
    const int nf = 2 * ne + 2;
    double* d = ctx->scalars + SC_GREEKS;
    {
        TimedLaunch t(ctx, MCG_K_PAYOFF);
        enqueue_greeks_reduce(ctx, ctx->partials, n_blocks, nf, 1, d);
    }
    MCG_HIP(hipGetLastError());
    MCG_HIP(hipMemcpyAsync(ctx->h_scalars + SC_GREEKS, d, nf * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MCG_HIP(hipStreamSynchronize(ctx->stream));
    for (int q = 0; q < nf; ++q) host[q] = ctx->h_scalars[SC_GREEKS + q];
    return MCG_OK;
}

int run_greeks_european(mcg_ctx* ctx, const mcg_paths* P, double K, double r, double T, int is_call, double sigma,
                        mcg_greeks* out) {
    const int64_t n = P->n_paths;
    const int n_blocks = book_blocks(ctx, n);
    constexpr int nf = 2 * GK_EU + 2;
    int rc = ensure_cap(ctx, &ctx->partials, &ctx->partials_cap, (size_t)n_blocks * nf);
    if (rc) return rc;
    {
        TimedLaunch t(ctx, MCG_K_PAYOFF);
        hipLaunchKernelGGL(k_greeks_european, dim3(n_blocks), dim3(256), 0, ctx->stream, P->data, P->data + (int64_t)P->n_steps * P->ld,
                           n, K, is_call, r, T, sigma, ctx->partials);
    }
    MCG_HIP(hipGetLastError());
    double h[nf];
    rc = greeks_reduce(ctx, n_blocks, GK_EU, h);
    if (rc) return rc;
    const double nd = (double)n, D = std::exp(-r * T), lo = h[2 * GK_EU], hi = h[2 * GK_EU + 1];
    greeks_all_nan(out);
    mean_se(h[0], h[GK_EU + 0], nd, D, &out->price, &out->price_se);
    mean_se(h[5], h[GK_EU + 5], nd, D, &out->dual_delta, &out->dual_delta_se);
    if (lo == hi && lo > 0.0) mean_se(h[1], h[GK_EU + 1], nd, D, &out->delta, &out->delta_se);
    if (P->generated) mean_se(h[4], h[GK_EU + 4], nd, D, &out->rho, &out->rho_se);
    if (sigma > 0.0) {
        mean_se(h[2], h[GK_EU + 2], nd, D, &out->gamma, &out->gamma_se);
        mean_se(h[3], h[GK_EU + 3], nd, D, &out->vega, &out->vega_se);
    }
    return MCG_OK;
}

int greeks_lsm_final(mcg_ctx* ctx, const mcg_paths* P, double K, const double* V, const double* dV, mcg_greeks* out) {
    const int64_t n = P->n_paths;
    const int n_blocks = book_blocks(ctx, n);
    constexpr int nf = 2 * GK_LSM + 2;
    int rc = ensure_cap(ctx, &ctx->partials, &ctx->partials_cap, (size_t)n_blocks * nf);
    if (rc) return rc;
    {
        TimedLaunch t(ctx, MCG_K_LSM_SWEEP);
        hipLaunchKernelGGL(k_greeks_lsm, dim3(n_blocks), dim3(256), 0, ctx->stream, V, dV, P->data, n, K, ctx->partials);
    }
    MCG_HIP(hipGetLastError());
    double h[nf];
    rc = greeks_reduce(ctx, n_blocks, GK_LSM, h);
    if (rc) return rc;
    const double nd = (double)n, lo = h[2 * GK_LSM], hi = h[2 * GK_LSM + 1];
    greeks_all_nan(out);
    mean_se(h[0], h[GK_LSM + 0], nd, 1.0, &out->price, &out->price_se);
    mean_se(h[1], h[GK_LSM + 1], nd, 1.0, &out->dual_delta, &out->dual_delta_se);
    if (lo == hi && lo > 0.0) {
        double unused;
        mean_se(h[2], h[GK_LSM + 2], nd, 1.0, &unused, &out->delta_se);
        out->delta = (out->price - K * out->dual_delta) / lo;  // exactly price = delta S0 + K dual_delta
    }
    return MCG_OK;
}

}  // namespace mcg
