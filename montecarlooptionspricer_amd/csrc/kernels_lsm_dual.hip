// mcg_lsm_dual_upper: the Andersen-Broadie dual upper bound of an LSM exercise policy by nested simulation (gfx950;
// include/mcgpu.h states the estimator, host/lsm_dual.cpp the checks and the slicing of the inner paths).
//
// k_lsm_dual_inner    grid (chunk of 512 outer paths, slice of inner paths, date j).  A lane owns two adjacent outer paths
//                     (one 16-byte load of row j) and, for every inner path k of its slice in ascending order, builds a GBM
//                     path in registers from S_j on: Philox on the inner stream (block and stream wave-uniform), Box-Muller
//                     on fm::Tables in LDS, X += fma(a, z, m) -- the twin's step (kernels_exotic_cv.hip) -- then the policy of
//                     the date reached: whether anybody may stop there from a word of 64 dates' bits in scalar registers, and only
//                     then the row through scalar loads, requested ahead of the exponential that hides them, and Horner (the
//                     kernel is compiled for orders up to 3, 7 and 15); k_lsm_apply's stop decision; the wave leaves an inner path set
//                     once none of its 128 paths is alive.  Nothing is stored per step; the slice's sum of v goes to the
//                     workspace [slice][date][outer].  Live path-steps and executed ones (steps of the wave times its outer
//                     paths) are counted in scalar integers, added per workgroup in LDS and once to the global counters.
// k_lsm_dual_combine  a lane per outer path: C_j = (the slices' sums in slice order) / n_inner, the decisions e_j on the outer
//                     path, the martingale recursion, D = max (h_j - Mt_j); writes D (and C), and the workgroup's
//                     {sum D, sum D^2} by block_sum; finish_sums adds the workgroups' in a fixed order.
// No floating-point atomics: D_i depends on outer path i alone (its prices, its global id, the policy, the model), so any split
// of the outer set into shards gives the same bits.  The outer set is worked through in batches that bound the workspace; a
// batch is a multiple of 512 paths, so neither D nor the workgroups' partial sums depend on it.
#include <algorithm>
#include <cstring>
#include <limits>
#include <vector>

#include "devmath.hpp"
#include "fastmath.hpp"
#include "lsm_device.hpp"
#include "paths_host.hpp"
#include "paths_device.hpp"

namespace mcg {

constexpr uint32_t DUAL_STREAM0 = 0x10000u;  // inner path k draws from stream DUAL_STREAM0 + k: no generator's stream
constexpr int DUAL_CHUNK = 512;              // outer paths of a workgroup of k_lsm_dual_inner
constexpr size_t DUAL_WS_DOUBLES = (size_t)1 << 24;  // the workspace of one batch: 128 MiB at most (one chunk's where that is more)

struct DualInnerArgs {
    const double* data;  // the outer matrix, step-major: 16-byte aligned rows (even ld)
    int64_t ld, n;       // n: outer paths of the matrix
    int64_t first;       // the batch's first outer path (a multiple of DUAL_CHUNK)
    int64_t ws_ld;       // outer paths of the batch, rounded up to DUAL_CHUNK
    int n_steps, order, is_call;  // order: what the launcher picks the instance by (the kernel reads coefficients 0 .. TOP)
    int n_inner, per_slice;
    uint64_t path_begin;
    uint32_t k0, k1;     // Philox key = the inner seed
    double K, invK, a, m;
    const double* coef;  // (n_steps + 1) rows of MCG_LSM_POLICY_STRIDE doubles
    const double* disc;  // exp(-r dt j)
    const unsigned long long* stops;  // bit j: row j is an EXERCISE_RULE or the last one (64 dates a word)
    double* ws;          // [slice][n_steps][ws_ld]
    unsigned long long* counters;  // {live path-steps, executed path-steps}
    const double2* tabs;
};

// A date's row as the inner loop reads it: scalars throughout (the date is wave-uniform).  TOP: the highest coefficient read,
// 3, 7 or 15 -- the kernel is compiled for these three, so that the step holds no branch on the order and the row's loads, the
// exponential and Horner are one basic block: the loads issue at its top and the exponential hides them.
template <int TOP>
struct DualRow {
    double c[TOP + 1];
    double centre, disc;
};

template <int TOP>
__device__ __forceinline__ void dual_row_load(DualRow<TOP>& r, la_table coef, la_table discounts, int l) {
    const la_table row = coef + (int64_t)l * MCG_LSM_POLICY_STRIDE;
#pragma unroll
    for (int q = 0; q <= TOP; ++q) r.c[q] = row[q];
    r.centre = row[17];
    r.disc = discounts[l];
}

// la_continuation's Horner entered at TOP instead of at the policy's order: the table the host uploads holds zeros above the
// order (run_lsm_dual), and from a = 0 the chain's steps above the order are fma(0, y, 0) = 0 and the order's own
// fma(0, y, c_p) = c_p (y finite), as la_continuation's entry step -- the same continuation value.
template <int TOP>
__device__ __forceinline__ void dual_continuation(const double (&c)[TOP + 1], double y0, double y1, double& cont0, double& cont1) {
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int q = TOP; q >= 0; --q) {
        a = fma(a, y0, c[q]);
        b = fma(b, y1, c[q]);
    }
    cont0 = a;
    cont1 = b;
}

template <int TOP>
__global__ __launch_bounds__(256) void k_lsm_dual_inner(DualInnerArgs t) {
    __shared__ fm::Tables tabs;
    __shared__ unsigned long long sm_count[2];
    fm::load_tables(&tabs, t.tabs);
    if (threadIdx.x < 2) sm_count[threadIdx.x] = 0ull;
    __syncthreads();
    const fm::Tables* tab = &tabs;
    const bool call = t.is_call != 0;
    const int j = blockIdx.z, slice = blockIdx.y, n_steps = t.n_steps;
    const la_table coef = (la_table)t.coef, discounts = (la_table)t.disc;
    const unsigned long long __attribute__((address_space(4)))* stops = (const unsigned long long __attribute__((address_space(4)))*)t.stops;
    const int64_t col = (int64_t)blockIdx.x * DUAL_CHUNK + 2 * (int64_t)threadIdx.x;  // in the batch
    const int64_t i = t.first + col;                                                 // in the matrix
    const bool valid0 = i < t.n, valid1 = i + 1 < t.n;
    la_d2 s_j = {0.0, 0.0};
    if (valid0) s_j = *reinterpret_cast<const la_d2*>(t.data + (int64_t)j * t.ld + i);  // (ld is even and >= n rounded up to 2)
    const unsigned long long m0 = __builtin_amdgcn_ballot_w64(valid0), m1 = __builtin_amdgcn_ballot_w64(valid1);
    const unsigned n_valid = (unsigned)(__popcll(m0) + __popcll(m1));  // (uniform)
    unsigned long long live_steps = 0ull, exec_steps = 0ull;          // (uniform: scalar registers)
    double acc0 = 0.0, acc1 = 0.0;
    const int k_begin = slice * t.per_slice, k_end = min(t.n_inner, k_begin + t.per_slice);
    if (n_valid != 0u) {
        const uint64_t g = t.path_begin + (uint64_t)i;
        for (int k = k_begin; k < k_end; ++k) {
            PhiloxLane rng[2];
            rng[0] = philox_lane_setup(g, DUAL_STREAM0 + (uint32_t)k, t.k1);
            rng[1] = philox_lane_setup(g + 1, DUAL_STREAM0 + (uint32_t)k, t.k1);
            double X[2] = {0.0, 0.0};
            double v0 = 0.0, v1 = 0.0;
            bool live0 = valid0, live1 = valid1;
            int l = j;
            unsigned long long bits = stops[(j + 1) >> 6];  // 64 dates' "somebody may stop here" bits (uniform)
            // one step to date l + 1 and the policy there; true once no path of the wave is alive (at date n_steps at the latest)
            auto step = [&](const double (&z)[2]) -> bool {
                ++l;
                if ((l & 63) == 0) bits = stops[l >> 6];
                live_steps += (unsigned long long)(__popcll(__builtin_amdgcn_ballot_w64(live0)) + __popcll(__builtin_amdgcn_ballot_w64(live1)));
                exec_steps += n_valid;
                X[0] = X[0] + __builtin_fma(t.a, z[0], t.m);
                X[1] = X[1] + __builtin_fma(t.a, z[1], t.m);
                if (((bits >> (l & 63)) & 1ull) == 0ull) return false;  // a CONTINUE row: nobody stops, no price needed
                // the row's scalars are requested here and read behind the exponential.  The last row's rule is evaluated in
                // vain rather than branched around: a TERMINAL row's coefficients and centre are not checked and may hold
                // anything, NaN included -- by design harmless, `last` alone decides there and cont is not looked at
                DualRow<TOP> row;
                dual_row_load<TOP>(row, coef, discounts, l);
                __builtin_amdgcn_sched_barrier(0);  // (left to itself the scheduler moves the requests down to their first use)
                double e0, e1;
                fm::exp_full2(X[0], X[1], e0, e1);
                const double s0 = s_j.x * e0, s1 = s_j.y * e1;
                const double p0 = payoff_of(call, s0, t.K), p1 = payoff_of(call, s1, t.K);
                double cont0, cont1;
                dual_continuation<TOP>(row.c, fma(s0, t.invK, -1.0) - row.centre, fma(s1, t.invK, -1.0) - row.centre, cont0, cont1);
                const bool last = l >= n_steps;
                const bool stop0 = live0 && (last || (p0 > LSM_ITM_EPS && !(cont0 > p0)));
                const bool stop1 = live1 && (last || (p1 > LSM_ITM_EPS && !(cont1 > p1)));
                v0 = stop0 ? p0 * row.disc : v0;
                v1 = stop1 ? p1 * row.disc : v1;
                live0 = live0 && !stop0;
                live1 = live1 && !stop1;
                return __builtin_amdgcn_ballot_w64(live0 || live1) == 0ull;
            };
            Philox4 w[2];
            double za[2], zb[2];
            const uint32_t block0 = (uint32_t)j << 12;
            for (uint32_t b = 0;; ++b) {  // relative step s = 4 b + element
                w[0] = philox4x32_10_lane(rng[0], block0 | b, t.k0, t.k1);
                w[1] = philox4x32_10_lane(rng[1], block0 | b, t.k0, t.k1);
                normal_pairs(w, false, tab, za, zb);
                if (step(za)) break;
                if (step(zb)) break;
                normal_pairs(w, true, tab, za, zb);
                if (step(za)) break;
                if (step(zb)) break;
            }
            acc0 += v0;
            acc1 += v1;
        }
    }
    la_d2* out = reinterpret_cast<la_d2*>(t.ws + ((int64_t)slice * n_steps + j) * t.ws_ld + col);  // (col < ws_ld: the grid covers ws_ld)
    *out = la_d2{acc0, acc1};
    if ((threadIdx.x & 63) == 0 && exec_steps != 0ull) {
        atomicAdd(&sm_count[0], live_steps);
        atomicAdd(&sm_count[1], exec_steps);
    }
    __syncthreads();
    if (threadIdx.x < 2 && sm_count[threadIdx.x] != 0ull) atomicAdd(t.counters + threadIdx.x, sm_count[threadIdx.x]);
}

struct DualCombineArgs {
    const double* data;
    int64_t ld, n, first, ws_ld;
    int n_steps, order, is_call, n_slices;
    double K, invK, n_inner;  // n_inner: as a double, the divisor of a date's sum
    double dt, maturity;
    const double* coef;
    const double* disc;
    const double* ws;
    double* d_out;   // [n]
    double* c_out;   // [n_steps][n], or null
    double* partials;  // {sum D, sum D^2} of workgroup (first / 256 + blockIdx.x)
};

__global__ __launch_bounds__(256) void k_lsm_dual_combine(DualCombineArgs t) {
    __shared__ double red[2 * 4];
    const bool call = t.is_call != 0;
    const int n_steps = t.n_steps;
    const int order = __builtin_amdgcn_readfirstlane(t.order);
    const la_table coef = (la_table)t.coef, discounts = (la_table)t.disc;
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x, i = t.first + col;
    const bool valid = i < t.n;
    double D = 0.0;
    if (valid) {
        D = -std::numeric_limits<double>::infinity();
        double Mt = 0.0, c_prev = 0.0;
        for (int j = 0; j <= n_steps; ++j) {  // (uniform)
            const la_table row = coef + (int64_t)j * MCG_LSM_POLICY_STRIDE;
            const double s = t.data[(int64_t)j * t.ld + i];
            const double p = payoff_of(call, s, t.K);
            const double h = p * discounts[j];
            const bool last = j >= n_steps;
            double c_j = 0.0;
            bool e = true;
            if (!last) {
                double sum = 0.0;
                for (int q = 0; q < t.n_slices; ++q) sum += t.ws[((int64_t)q * n_steps + j) * t.ws_ld + col];
                c_j = sum / t.n_inner;
                if (t.c_out) t.c_out[(int64_t)j * t.n + i] = c_j;
                e = false;
                if (row[18] == (double)MCG_POL_EXERCISE_RULE) {
                    double c[16];
#pragma unroll
                    for (int q = 0; q < 16; ++q) c[q] = row[q];
                    const double y = fma(s, t.invK, -1.0) - row[17];
                    double cont, unused;
                    la_continuation(c, order, y, y, cont, unused);
                    e = p > LSM_ITM_EPS && !(cont > p);
                }
            }
            if (j > 0) {
                const double L = last ? h : (e ? h : c_j);
                Mt = Mt + L - c_prev;
            }
            if (last || !((double)j * t.dt > t.maturity)) D = fmax(D, h - Mt);
            c_prev = c_j;
        }
        t.d_out[i] = D;
    }
    double f[2] = {valid ? D : 0.0, valid ? D * D : 0.0};
    block_sum<2, 4>(f, red);
    if (threadIdx.x == 0) {
        const int64_t b = t.first / 256 + blockIdx.x;
        t.partials[2 * b] = f[0];
        t.partials[2 * b + 1] = f[1];
    }
}

int lsm_dual_check(const mcg_lsm_policy_hdr* hdr, const double* coef, const mcg_lsm_dual_model* model);
void lsm_dual_slices(int n_inner, int n_steps, int* per_slice, int* n_slices);

// The arguments have been checked; P holds at least one path.  out3 = {sum D, sum D^2, n}; counts = {live, executed} path-steps.
static int run_lsm_dual(mcg_ctx* ctx, const mcg_lsm_policy_hdr* hdr, const double* coef, const mcg_paths* P,
                        const mcg_lsm_dual_model* model, double out3[3], double* cont_out, double* d_out, unsigned long long counts[2]) {
    const int n_steps = P->n_steps, rows = n_steps + 1;
    const int64_t n = P->n_paths;
    if ((P->ld & 1) != 0 || (reinterpret_cast<uintptr_t>(P->data) & 15) != 0 || P->ld < ((n + 1) & ~(int64_t)1))
        return fail(MCG_ERR_INVALID, "path matrix rows must be 16-byte aligned");
    int per_slice = 1, n_slices = 1;
    lsm_dual_slices(model->n_inner, n_steps, &per_slice, &n_slices);
    // the batch: as many chunks as the workspace bound holds, one at least, the grid's 65535 at most
    const int64_t all = (n + DUAL_CHUNK - 1) / DUAL_CHUNK * DUAL_CHUNK;
    const size_t per_path = (size_t)n_slices * (size_t)std::max(n_steps, 1);
    const size_t ws_bound = ctx->lsm_dual_ws_doubles ? ctx->lsm_dual_ws_doubles : DUAL_WS_DOUBLES;
    int64_t batch = (int64_t)(ws_bound / per_path) / DUAL_CHUNK * DUAL_CHUNK;
    batch = std::max<int64_t>(DUAL_CHUNK, std::min<int64_t>({batch, all, (int64_t)32768 * DUAL_CHUNK}));
    const int64_t n_blocks = (n + 255) / 256;
    // the table workspace: the policy's rows, the discounts, the words of stop bits, then the two counters
    const size_t n_coef = (size_t)rows * MCG_LSM_POLICY_STRIDE, n_words = ((size_t)rows + 63) / 64;
    int rc = ensure_cap(ctx, &ctx->partials, &ctx->partials_cap, 2 * (size_t)n_blocks);
    if (rc) return rc;
    const size_t ws_doubles = per_path * (size_t)batch, c_doubles = cont_out ? (size_t)n_steps * (size_t)n : 0;
    const size_t bytes = (ws_doubles + (size_t)n + c_doubles) * sizeof(double);
    void* pool = nullptr;
    rc = pool_alloc(ctx, bytes, &pool);
    if (rc) return rc;
    double *d_ws = (double*)pool, *d_d = d_ws + ws_doubles, *d_c = cont_out ? d_d + n : nullptr;
    std::vector<double> table(n_coef + (size_t)rows + n_words);
    std::copy(coef, coef + n_coef, table.begin());
    for (int j = 0; j < rows; ++j)  // (dual_continuation runs its chain from above the order; a hand-made row may hold anything there)
        for (int q = hdr->poly_order + 1; q < 16; ++q) table[(size_t)j * MCG_LSM_POLICY_STRIDE + q] = 0.0;
    lsm_policy_discounts(hdr, table.data() + n_coef);
    static_assert(sizeof(unsigned long long) == sizeof(double), "the stop bits travel in the table of doubles");
    for (size_t wd = 0; wd < n_words; ++wd) {
        unsigned long long bits = 0ull;
        for (size_t j = 64 * wd; j < std::min<size_t>(64 * wd + 64, (size_t)rows); ++j)
            if (j == (size_t)n_steps || coef[j * MCG_LSM_POLICY_STRIDE + 18] == (double)MCG_POL_EXERCISE_RULE) bits |= 1ull << (j - 64 * wd);
        std::memcpy(&table[n_coef + (size_t)rows + wd], &bits, sizeof(bits));
    }
    auto body = [&]() -> int {
        HostPiece up[] = {{table.data(), table.size() * sizeof(double)}};
        const int r1 = upload_params(ctx, up, 2);
        if (r1) return r1;
        unsigned long long* d_counters = reinterpret_cast<unsigned long long*>(up[0].at + table.size());
        MCG_HIP(hipMemsetAsync(d_counters, 0, 2 * sizeof(unsigned long long), ctx->stream));
        DualInnerArgs a;
        a.data = P->data;
        a.ld = P->ld;
        a.n = n;
        a.n_steps = n_steps;
        a.order = hdr->poly_order;
        a.is_call = hdr->is_call;
        a.n_inner = model->n_inner;
        a.per_slice = per_slice;
        a.path_begin = model->path_begin;
        a.k0 = (uint32_t)model->seed;
        a.k1 = (uint32_t)(model->seed >> 32);
        a.K = hdr->K;
        a.invK = 1.0 / hdr->K;
        a.a = model->sigma * std::sqrt(hdr->dt);
        a.m = (hdr->r - model->q - 0.5 * model->sigma * model->sigma) * hdr->dt;
        a.coef = up[0].at;
        a.disc = up[0].at + n_coef;
        a.stops = reinterpret_cast<const unsigned long long*>(up[0].at + n_coef + rows);
        a.ws = d_ws;
        a.counters = d_counters;
        a.tabs = (const double2*)ctx->log_tab;
        DualCombineArgs c;
        c.data = P->data;
        c.ld = P->ld;
        c.n = n;
        c.n_steps = n_steps;
        c.order = hdr->poly_order;
        c.is_call = hdr->is_call;
        c.n_slices = n_slices;
        c.K = hdr->K;
        c.invK = a.invK;
        c.n_inner = (double)model->n_inner;
        c.dt = hdr->dt;
        c.maturity = hdr->maturity;
        c.coef = a.coef;
        c.disc = a.disc;
        c.ws = d_ws;
        c.d_out = d_d;
        c.c_out = d_c;
        c.partials = ctx->partials;
        for (int64_t first = 0; first < n; first += batch) {
            const int64_t here = std::min(batch, n - first);
            const int64_t chunks = (here + DUAL_CHUNK - 1) / DUAL_CHUNK;
            a.first = c.first = first;
            a.ws_ld = c.ws_ld = chunks * DUAL_CHUNK;
            TimedLaunch tl(ctx, MCG_K_LSM_DUAL, n_steps > 0 ? 2 : 1);
            if (n_steps > 0) {
                const dim3 grid((unsigned)chunks, (unsigned)n_slices, (unsigned)n_steps);
                if (a.order <= 3) hipLaunchKernelGGL(k_lsm_dual_inner<3>, grid, dim3(256), 0, ctx->stream, a);
                else if (a.order <= 7) hipLaunchKernelGGL(k_lsm_dual_inner<7>, grid, dim3(256), 0, ctx->stream, a);
                else hipLaunchKernelGGL(k_lsm_dual_inner<15>, grid, dim3(256), 0, ctx->stream, a);
            }
            hipLaunchKernelGGL(k_lsm_dual_combine, dim3((unsigned)((here + 255) / 256)), dim3(256), 0, ctx->stream, c);
        }
        MCG_HIP(hipGetLastError());
        int r2 = finish_sums(ctx, n_blocks, n, out3);  // synchronises the stream
        if (r2) return r2;
        MCG_HIP(hipMemcpyAsync(counts, d_counters, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        if (d_out) MCG_HIP(hipMemcpyAsync(d_out, d_d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (cont_out && c_doubles) MCG_HIP(hipMemcpyAsync(cont_out, d_c, c_doubles * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MCG_HIP(hipStreamSynchronize(ctx->stream));
        return MCG_OK;
    };
    rc = body();
    if (rc) (void)hipStreamSynchronize(ctx->stream);  // nothing queued may still use the workspace or `table` afterwards
    pool_release(ctx, pool, bytes);
    return rc;
}

}  // namespace mcg

using namespace mcg;

int mcg_lsm_dual_upper(mcg_ctx* ctx, const mcg_lsm_policy_hdr* hdr, const double* coef, const mcg_paths* P,
                       const mcg_lsm_dual_model* model, double* upper, double* std_err, double* sums3, double* cont_out, double* d_out,
                       int64_t* inner_steps) {
    // what needs neither a ctx nor a matrix comes first: a host without a GPU answers it
    int rc = lsm_dual_check(hdr, coef, model);
    if (rc) return rc;
    if (!ctx || !P || !upper) return fail(MCG_ERR_INVALID, "ctx/paths/upper is NULL");
    if (P->ctx != ctx) return fail(MCG_ERR_INVALID, "paths belong to a different ctx");
    if (hdr->n_steps != P->n_steps) return fail(MCG_ERR_INVALID, "the policy has %d steps, the matrix %d", hdr->n_steps, P->n_steps);
    if (ctx->allreduce || ctx->rccl_comm || ctx->shm)
        return fail(MCG_ERR_INVALID, "this ctx holds a collective: bound each shard with its path_begin and add the shards' sums3 and inner_steps");
    if (P->n_paths < 1) return fail(MCG_ERR_EMPTY_PATHS, "no paths to bound");
    MCG_HIP(hipSetDevice(ctx->device));
    double s[3];
    unsigned long long counts[2] = {0ull, 0ull};
    rc = run_lsm_dual(ctx, hdr, coef, P, model, s, cont_out, d_out, counts);
    if (rc) return rc;
    ctx->lsm_dual_executed = (int64_t)counts[1];
    if (sums3)
        for (int q = 0; q < 3; ++q) sums3[q] = s[q];
    if (inner_steps) *inner_steps = (int64_t)counts[0];
    sums_to_mean_stderr(s[0], s[1], s[2], upper, std_err);
    return MCG_OK;
}

int mcg_debug_lsm_dual_workspace(mcg_ctx* ctx, size_t doubles) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    ctx->lsm_dual_ws_doubles = doubles;
    return MCG_OK;
}

int mcg_debug_lsm_dual_executed(mcg_ctx* ctx, int64_t* executed) {
    if (!ctx || !executed) return fail(MCG_ERR_INVALID, "ctx/executed is NULL");
    *executed = ctx->lsm_dual_executed;
    return MCG_OK;
}
