// mcg_lsm_apply: an LSM exercise policy applied to a device-resident step-major path matrix (gfx950).
//
// ONE forward streaming pass: a lane owns a unit of two adjacent paths (16-byte loads, like k_lsm_date and k_path_stats),
// a wavefront 128 adjacent paths, a workgroup a chunk of 512, and walks the dates upwards.  At date j a live path stops
// when the date's row is an EXERCISE_RULE, its payoff exceeds 1e-14 and the row's continuation value does not exceed the
// payoff; it then carries v = payoff exp(-r dt j).  What is left at row n_steps takes the terminal payoff.
//   * Row loads do not depend on decisions: LA_DEPTH rows are always in flight per lane (a ring of registers).
//   * The wavefront's ballot of live paths is looked at after every date: once it is empty the wave stops reading its
//     chunk -- unlike every other kernel here the bytes moved depend on the data (at most LA_DEPTH rows requested in vain
//     per wave and chunk).
//   * A date's coefficient row, kind and discount are wave-uniform: read straight from the policy table in global memory
//     through scalar loads (two 64-byte loads for the sixteen coefficients), nothing staged in LDS, so the table's size
//     (dates x 20 doubles) is no limit.
//   * One kernel for every order: Horner enters an unrolled chain at the policy's order (a wave-uniform switch), so a path
//     costs order + 1 fused multiply-adds and the coefficients stay in scalar registers under static indices.  The entry
//     step is fma(0, y, c_p) = c_p exactly (y finite), after which the chain is lsm_continuation's (lsm_device.hpp).
//   * {sum v, sum v^2}: per lane over its chunks in order, block_sum per workgroup, finish_sums over the workgroups: fixed
//     order, no floating-point atomics.  The histogram of stopping dates is counted per wavefront (popcount of a ballot),
//     kept per workgroup in LDS where n_steps + 1 <= LA_HIST_LDS, and flushed with integer adds (else added to the global
//     counters directly, one add per wavefront and date that has exercises).
// The grid is a fixed number of workgroups per CU striding over the chunks: early stopping makes chunks uneven, a few
// chunks per workgroup even that out and keep the histogram's flush to grid x dates adds.
#include <algorithm>
#include <atomic>
#include <vector>

#include "devmath.hpp"
#include "lsm_device.hpp"
#include "paths_host.hpp"

namespace mcg {

constexpr int LA_DEPTH = 8;         // rows in flight per lane: 8 x 16 B, 32 KiB per workgroup (k_path_stats' figure)
constexpr int LA_HIST_LDS = 1024;   // dates (n_steps + 1) whose counters a workgroup keeps in LDS
constexpr int LA_WGS_PER_CU = 8;    // workgroups per CU at most; fewer where the occupancy query says so (run_lsm_apply)

struct LsmApplyArgs {
    const double* data;  // step-major matrix: 16-byte aligned rows (even ld)
    int64_t ld, n;
    int n_steps, order, is_call;
    double K, invK;
    const double* coef;  // (n_steps + 1) rows of MCG_LSM_POLICY_STRIDE doubles
    const double* disc;  // exp(-r dt j), j = 0 .. n_steps
    double* partials;    // {sum v, sum v^2} per workgroup
    unsigned long long* hist;  // n_steps + 1 counters, zeroed before the launch
};

// (la_d2, la_table and la_continuation, the policy's Horner rule, are lsm_device.hpp's: mcg_lsm_dual_upper evaluates the same rows)
__global__ __launch_bounds__(256) void k_lsm_apply(LsmApplyArgs a) {
    constexpr int D = LA_DEPTH;
    __shared__ unsigned sm_hist[LA_HIST_LDS];
    __shared__ double red[2 * 4];
    const bool lds_hist = a.n_steps + 1 <= LA_HIST_LDS;  // (uniform)
    if (lds_hist) {
        for (int i = threadIdx.x; i <= a.n_steps; i += 256) sm_hist[i] = 0u;
        __syncthreads();
    }
    const bool call = a.is_call != 0;
    const int lane = threadIdx.x & 63;
    const int64_t n_units = (a.n + 1) / 2;
    const int64_t n_chunks = (n_units + 255) / 256;
    const int64_t ld2 = a.ld / 2;  // a row in units
    const int order = __builtin_amdgcn_readfirstlane(a.order);
    const la_table coef = (la_table)a.coef, discounts = (la_table)a.disc;
    double f[2] = {0.0, 0.0};
    for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const int64_t u = ch * 256 + threadIdx.x;
        const bool valid = u < n_units;  // (a lane beyond the last unit loads nothing and owns no path)
        const la_d2* col = reinterpret_cast<const la_d2*>(a.data) + u;
        bool live0 = valid, live1 = valid && 2 * u + 1 < a.n;
        double v0 = 0.0, v1 = 0.0;
        la_d2 x[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            x[d] = la_d2{0.0, 0.0};
            if (valid && d <= a.n_steps) x[d] = __builtin_nontemporal_load(col + (int64_t)d * ld2);  // each row is read once
        }
        for (int j0 = 0;; j0 += D) {  // (ends at row n_steps at the latest: nothing is live after the terminal row)
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int j = j0 + d;  // wave-uniform: so are the date's kind, coefficients and discount below
                const la_d2 s = x[d];
                if (valid && j + D <= a.n_steps) x[d] = __builtin_nontemporal_load(col + (int64_t)(j + D) * ld2);
                const la_table row = coef + (int64_t)j * MCG_LSM_POLICY_STRIDE;
                const double p0 = payoff_of(call, s.x, a.K), p1 = payoff_of(call, s.y, a.K);
                bool stop0, stop1;
                if (j >= a.n_steps) {  // the terminal row: whoever is left takes its payoff (possibly 0)
                    stop0 = live0;
                    stop1 = live1;
                } else if (row[18] == (double)MCG_POL_EXERCISE_RULE) {
                    double c[16];
#pragma unroll
                    for (int t = 0; t < 16; ++t) c[t] = row[t];
                    const double center = row[17];
                    double cont0, cont1;
                    la_continuation(c, order, fma(s.x, a.invK, -1.0) - center, fma(s.y, a.invK, -1.0) - center, cont0, cont1);
                    stop0 = live0 && p0 > LSM_ITM_EPS && !(cont0 > p0);
                    stop1 = live1 && p1 > LSM_ITM_EPS && !(cont1 > p1);
                } else {
                    stop0 = stop1 = false;
                }
                const unsigned long long b0 = __builtin_amdgcn_ballot_w64(stop0), b1 = __builtin_amdgcn_ballot_w64(stop1);
                if ((b0 | b1) != 0ull) {  // (uniform)
                    const double disc = discounts[j];
                    if (stop0) v0 = p0 * disc;
                    if (stop1) v1 = p1 * disc;
                    live0 = live0 && !stop0;
                    live1 = live1 && !stop1;
                    if (lane == 0) {
                        const unsigned cnt = (unsigned)(__popcll(b0) + __popcll(b1));
                        if (lds_hist) atomicAdd(&sm_hist[j], cnt);
                        else atomicAdd(a.hist + j, (unsigned long long)cnt);
                    }
                }
                if (__builtin_amdgcn_ballot_w64(live0 || live1) == 0ull) goto chunk_done;  // the wave stops reading
            }
        }
    chunk_done:
        f[0] += v0;
        f[0] += v1;
        f[1] = fma(v0, v0, f[1]);
        f[1] = fma(v1, v1, f[1]);
    }
    block_sum<2, 4>(f, red);  // (its barrier also follows every wave's last LDS counter add)
    if (threadIdx.x == 0) {
        a.partials[2 * (int64_t)blockIdx.x] = f[0];
        a.partials[2 * (int64_t)blockIdx.x + 1] = f[1];
    }
    if (lds_hist) {
        for (int i = threadIdx.x; i <= a.n_steps; i += 256) {
            const unsigned cnt = sm_hist[i];
            if (cnt != 0u) atomicAdd(a.hist + i, (unsigned long long)cnt);
        }
    }
}

// The policy has been checked (host/lsm_policy.cpp) and has the matrix's n_steps; P holds at least one path.
// out3 = {sum v, sum v^2, n}; tau_hist: n_steps + 1 counts on the host, or null.
int run_lsm_apply(mcg_ctx* ctx, const mcg_lsm_policy_hdr* hdr, const double* coef, const mcg_paths* P, double out3[3],
                  int64_t* tau_hist) {
    const int rows = P->n_steps + 1;
    if ((P->ld & 1) != 0 || (reinterpret_cast<uintptr_t>(P->data) & 15) != 0)
        return fail(MCG_ERR_INVALID, "path matrix rows must be 16-byte aligned");
    const int64_t n_chunks = ((P->n_paths + 1) / 2 + 255) / 256;
    // one resident wave of workgroups: a second, partial round would leave most CUs idle behind the early finishers
    static std::atomic<int> occupancy{0};
    int occ = occupancy.load(std::memory_order_relaxed);
    if (occ < 1) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)k_lsm_apply, 256, 0) != hipSuccess || occ < 1) {
            (void)hipGetLastError();
            occ = 1;
        }
        occ = std::min(occ, LA_WGS_PER_CU);
        occupancy.store(occ, std::memory_order_relaxed);
    }
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(n_chunks, (int64_t)ctx->n_cus * occ));
    // the table workspace: the policy's rows, the discounts, then the counters
    const size_t n_coef = (size_t)rows * MCG_LSM_POLICY_STRIDE;
    int rc = ensure_cap(ctx, &ctx->partials, &ctx->partials_cap, 2 * (size_t)grid);
    if (rc) return rc;
    std::vector<double> table(n_coef + (size_t)rows);
    std::copy(coef, coef + n_coef, table.begin());
    lsm_policy_discounts(hdr, table.data() + n_coef);
    HostPiece up[] = {{table.data(), table.size() * sizeof(double)}};
    rc = upload_params(ctx, up, (size_t)rows);  // (finish_sums synchronises before `table` goes: upload_params)
    if (rc) return rc;
    unsigned long long* d_hist = reinterpret_cast<unsigned long long*>(up[0].at + n_coef + rows);
    MCG_HIP(hipMemsetAsync(d_hist, 0, (size_t)rows * sizeof(unsigned long long), ctx->stream));
    LsmApplyArgs a;
    a.data = P->data;
    a.ld = P->ld;
    a.n = P->n_paths;
    a.n_steps = P->n_steps;
    a.order = hdr->poly_order;
    a.is_call = hdr->is_call;
    a.K = hdr->K;
    a.invK = 1.0 / hdr->K;
    a.coef = up[0].at;
    a.disc = up[0].at + n_coef;
    a.partials = ctx->partials;
    a.hist = d_hist;
    {
        TimedLaunch t(ctx, MCG_K_LSM_APPLY);
        hipLaunchKernelGGL(k_lsm_apply, dim3(grid), dim3(256), 0, ctx->stream, a);
    }
    MCG_HIP(hipGetLastError());
    rc = finish_sums(ctx, grid, P->n_paths, out3);  // synchronises the stream
    if (rc) return rc;
    if (tau_hist) {
        static_assert(sizeof(int64_t) == sizeof(unsigned long long), "the counters are downloaded as they are");
        MCG_HIP(hipMemcpyAsync(tau_hist, d_hist, (size_t)rows * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        MCG_HIP(hipStreamSynchronize(ctx->stream));
    }
    return MCG_OK;
}

}  // namespace mcg
