// Test hooks behind mcg_debug_eval and mcg_debug_eval_v: run one routine of fastmath.hpp, philox.hpp or the Heston
// steps (heston_device.hpp, heston_schemes.hpp, bates_device.hpp) elementwise so that tests can measure its error against
// mpmath / libm; behind mcg_debug_lsm_solve: the regression solves of lsm_device.hpp.  Not on any product path.
#include "bates_device.hpp"
#include "devmath.hpp"
#include "fastmath.hpp"
#include "heston_schemes.hpp"
#include "lsm_device.hpp"
#include "mcg_internal.hpp"

namespace mcg {

__global__ __launch_bounds__(256) void k_debug_eval(int fn, const double* x, double* y, int64_t n,
                                                    const double2* gtab, const double2* sincos2) {
    __shared__ fm::Tables tabs;
    const fm::Tables* tab = &tabs;
    fm::load_tables(&tabs, gtab);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    double a = 0.0, b = 0.0;
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    switch (fn) {
        case 0: a = fm::scaled_exp(1.0, v); break;
        case 1: a = fm::neg2log(v, tab->log); break;
        case 2: a = fm::sqrt_pos(v); break;
        case 3: fm::sincos_table((uint32_t)v, tab->sincos, a, b); break;
        case 4: fm::normal_quad_fast(1u, 0u, (uint64_t)v, 0u, STREAM_PRICE, tab, z); break;
        case 6: a = fm::scaled_exp_small(1.0, v); break;
        case 7: a = fm::scaled_exp_small6(1.0, v); break;
        case 8: fm::exp2_pair(v, v + 96.0, tab, a, b); break;  // 2^(v/256), 2^((v+96)/256)
        case 9: fm::normal_quad_fast<true>(1u, 0u, (uint64_t)v, 0u, STREAM_PRICE, tab, z); break;
        case 10: fm::sincos_two_level((uint32_t)v, sincos2, sincos2 + fm::SINCOS2_ENTRIES, a, b); break;  // (tables in device memory)
        case 11: a = fm::exp_full(v); break;
        case 12: fm::exp_full2(v, v + 0.375, a, b); break;
        case 13: fm::expm1_small6_2(v, -v, a, b); break;
        case 14: fm::expm1_small9_2(v, -v, a, b); break;
        case 15: a = sqrt_nonneg(v); break;
        default: normal_quad_ref(1u, 0u, (uint64_t)v, 0u, STREAM_PRICE, z); break;
    }
    if (fn < 4 || (fn > 5 && fn != 9)) {
        z[0] = a;
        z[1] = b;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) y[4 * i + e] = z[e];
}

// fn 16 of mcg_debug_eval, in a kernel of its own (k_debug_eval stays as it is): the normal of the Sobol' generators
__global__ __launch_bounds__(256) void k_debug_sobol_normal(const double* x, double* y, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    y[4 * i] = sobol_normal((uint32_t)x[i]);
#pragma unroll
    for (int e = 1; e < 4; ++e) y[4 * i + e] = 0.0;
}

// ---- mcg_debug_eval_v: routines with several inputs per element or wave-uniform parameters ----------------------------------
enum : int {
    V_QE_RCP = 0, V_QE_DIV, V_RADIUS, V_NEG2LOG_SCALED, V_BM_AFFINE, V_BM_AFFINE_SCALED, V_BM_AFFINE2, V_BM_AFFINE_SCALED2,
    V_QE_STEP, V_BATES_COUNT, V_COUNT
};
constexpr int V_MAX_PARAMS = 12;  // of DebugVArgs (V_BATES_COUNT's travel in its own argument block)
// {doubles per element, parameters} of each fn
constexpr int V_SHAPE[V_COUNT][2] = {{1, 0}, {2, 0}, {2, 0}, {1, 1}, {2, 2}, {2, 2}, {2, 2}, {2, 2}, {5, 12}, {5, 5 + JUMP_CAP}};

struct DebugVArgs {
    int fn, n_in;
    const double* x;
    double* y;
    int64_t n;
    double p[V_MAX_PARAMS];
    double scale;      // the scaled forms: vol^2, what the GBM kernels stage their logarithm table with
    fm::LogScale ls;   // ... and fm::make_log_scale of it, built on the host as launch_gbm does
    const double2* gtab;
    const double2* sincos2;
};

__global__ __launch_bounds__(256) void k_debug_eval_v(DebugVArgs a) {
    __shared__ fm::Tables tabs;
    const bool scaled = a.fn == V_NEG2LOG_SCALED || a.fn == V_BM_AFFINE_SCALED || a.fn == V_BM_AFFINE_SCALED2;  // (uniform)
    if (scaled) fm::load_tables_scaled(&tabs, a.gtab, a.scale);
    else fm::load_tables(&tabs, a.gtab);
    const fm::Tables* tab = &tabs;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const double* xi = a.x + i * a.n_in;
    const double2 *coarse = a.sincos2, *fine = a.sincos2 + fm::SINCOS2_ENTRIES;  // (in device memory)
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    switch (a.fn) {
        case V_QE_RCP: z[0] = qe_rcp(xi[0]); break;
        case V_QE_DIV: z[0] = qe_div(xi[0], xi[1]); break;
        case V_RADIUS: z[0] = radius_u01((uint32_t)xi[0], (uint32_t)xi[1]); break;
        case V_NEG2LOG_SCALED: z[0] = fm::neg2log_scaled(xi[0], tab->log, a.ls); break;
        case V_BM_AFFINE: fm::box_muller_pair_affine((uint32_t)xi[0], (uint32_t)xi[1], tab, a.p[0], a.p[1], z[0], z[1]); break;
        case V_BM_AFFINE_SCALED:
            fm::box_muller_pair_affine_scaled((uint32_t)xi[0], (uint32_t)xi[1], tab, a.ls, a.p[1], z[0], z[1]);
            break;
        case V_BM_AFFINE2:
            fm::box_muller_pair_affine2((uint32_t)xi[0], (uint32_t)xi[1], tab->log, coarse, fine, a.p[0], a.p[1], z[0], z[1]);
            break;
        default:
            fm::box_muller_pair_affine_scaled2((uint32_t)xi[0], (uint32_t)xi[1], tab->log, coarse, fine, a.ls, a.p[1], z[0], z[1]);
            break;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) a.y[4 * i + e] = z[e];
}

// One HestonQe::step.  The step asks for the path of its p-th path as `a.path_begin + (i + p)`; here every element names its own
// path, so path_begin is a pair of ids whose `+ p` picks one (i = 0).  Everything else of the argument block is what the
// step reads of HestonArgs.
struct DebugQePaths {
    uint64_t id[HESTON_PPL];
    __device__ __forceinline__ uint64_t operator+(uint64_t p) const { return id[p]; }
};
struct DebugQeArgs {
    HestonQe::Consts c;
    DebugQePaths path_begin;
    uint32_t k0, k1;
};

__global__ __launch_bounds__(256) void k_debug_qe_step(DebugVArgs a) {
    constexpr int PPL = HESTON_PPL;
    __shared__ fm::Tables tabs;
    fm::load_tables(&tabs, a.gtab);
    __syncthreads();
    // a lane takes two consecutive elements as its two paths.  Every lane of a launched wave runs the step -- the wave's
    // ballot decides whether the exponential branch is entered -- so a lane past the end repeats the last element and
    // stores nothing.
    const int64_t first = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PPL;
    DebugQeArgs q;
    q.c = HestonQe::Consts{a.p[0], a.p[1], a.p[2], a.p[3], a.p[4], a.p[5], a.p[6], a.p[7]};
    q.k0 = (uint32_t)a.p[8];
    q.k1 = (uint32_t)a.p[9];
    const uint32_t block = (uint32_t)a.p[10];
    const int elem = (int)a.p[11];
    double S[PPL], v[PPL], z1[PPL], z2[PPL], flag[PPL];
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        const int64_t e = first + p < a.n ? first + p : a.n - 1;
        const double* xi = a.x + e * 5;
        v[p] = xi[0];
        z1[p] = xi[1];
        z2[p] = xi[2];
        S[p] = xi[3];
        q.path_begin.id[p] = (uint64_t)xi[4];
        // the step's decision, from the step's own expressions
        const double m = __builtin_fma(v[p] - q.c.theta, q.c.E, q.c.theta);
        flag[p] = __builtin_fma(v[p], q.c.c1, q.c.c2) <= QE_PSI_C * (m * m) ? 0.0 : 1.0;
    }
    HestonQe scheme;
    scheme.new_block(q, (int64_t)0, block, &tabs);
    scheme.step(q, (int64_t)0, block, elem, &tabs, z1, z2, S, v);
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        if (first + p >= a.n) continue;
        double* yi = a.y + 4 * (first + p);
        yi[0] = v[p];
        yi[1] = S[p];
        yi[2] = flag[p];
        yi[3] = 0.0;
    }
}

// WithJumps::count and WithJumps::jump of the Bates generators on words the caller chooses.  Both read the thresholds
// T[2..15], mu_j and sigma_j straight from the kernel's argument block, at the place of c.rare in a HestonArgs that is the
// kernel's first and only argument (WithJumps::rare computes that address by hand).  So this kernel's first and only argument
// is that HestonArgs, of WithJumps<HestonEuler> (the count is the same code under either base scheme), and what else the kernel
// needs travels in fields the jump rule does not read: var = x ([n][5]: w0, w1, w2, w3, z3), out = y ([n][4]), n_paths = n,
// n_steps = the element 0..3 whose J is asked for.
using DebugBatesArgs = HestonArgs<WithJumps<HestonEuler>::Consts>;

__global__ __launch_bounds__(256) void k_debug_bates_count(DebugBatesArgs a) {
    constexpr int PPL = HESTON_PPL;
    // a lane takes two consecutive elements as its two paths, as in the product.  Every lane of a launched wave runs the count
    // -- the wave's ballots decide how far up the thresholds it goes -- so a lane past the end holds the word 0 four times,
    // which passes no threshold, and stores nothing.
    const int64_t first = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PPL;
    WithJumps<HestonEuler> s;
    Philox4 w[PPL];
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        const bool in = first + p < a.n_paths;
        const double* xi = a.var + (in ? first + p : 0) * 5;
        w[p].w0 = in ? (uint32_t)xi[0] : 0u;
        w[p].w1 = in ? (uint32_t)xi[1] : 0u;
        w[p].w2 = in ? (uint32_t)xi[2] : 0u;
        w[p].w3 = in ? (uint32_t)xi[3] : 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) s.z3[p][e] = xi[4];
        s.cnt[p] = 0u;
    }
    s.count(w, a);
    double J[PPL];
    switch (a.n_steps) {  // (wave-uniform; the product's element is a constant of its unrolled step)
        case 0: s.jump(a, 0, J); break;
        case 1: s.jump(a, 1, J); break;
        case 2: s.jump(a, 2, J); break;
        default: s.jump(a, 3, J); break;
    }
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        if (first + p >= a.n_paths) continue;
        double* yi = a.out + 4 * (first + p);
        yi[0] = (double)s.cnt[p];
        yi[1] = J[p];
        yi[2] = 0.0;
        yi[3] = 0.0;
    }
}

// ---- mcg_debug_lsm_solve: the regression solves of lsm_device.hpp on moments the caller chooses --------------------------------
// Launched as the product runs them: one workgroup per element, the moments staged in LDS (as k_lsm_reduce_solve hands them to
// the solve), thread 0 solving into a coefficient block in LDS, the centred forms' workspace in LDS.  Every case below calls
// the routine of lsm_device.hpp itself.
enum : int { L_SOLVE_NB = 0, L_SOLVE_NB_TAN, L_SOLVE_ONE, L_CENTERED, L_CENTERED_TAN, L_RCP_RSQRT, L_CONTINUATION, L_COUNT };
constexpr int L_MAX_MOMENTS = 4 * LSM_MAX_NB - 1;  // the tangent's centred solve at sixteen basis functions
constexpr int L_OUT = 2 * LSM_COEF_STRIDE;         // coef, dcoef

struct DebugLsmArgs {
    int fn, nb, n_moments;
    const double* moments;  // [n][n_moments]
    const double* params;   // [n][3]: min_count, K, mu
    double* out;            // [n][L_OUT]
};

template <int NB>
__device__ __forceinline__ double debug_lsm_continuation(const double* e) {
    double c[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) c[t] = e[t];
    return lsm_continuation<NB>(c, e[NB], e[NB + 1]);
}

#define MCG_DEBUG_LSM_NB(CALL) \
    switch (nb) {              \
        case 1: CALL(1); break; \
        case 2: CALL(2); break; \
        case 3: CALL(3); break; \
        case 4: CALL(4); break; \
        case 5: CALL(5); break; \
        case 6: CALL(6); break; \
        case 7: CALL(7); break; \
        case 8: CALL(8); break; \
        default: CALL(9); break; \
    }

__global__ __launch_bounds__(64) void k_debug_lsm_solve(DebugLsmArgs a) {
    __shared__ double sm_mom[L_MAX_MOMENTS + 1];
    __shared__ double sm_coef[L_OUT];
    __shared__ double sm_ws[lsm_ws_doubles(LSM_MAX_NB)];
    const int64_t i = blockIdx.x;
    for (int t = threadIdx.x; t < a.n_moments; t += 64) sm_mom[t] = a.moments[i * a.n_moments + t];
    for (int t = threadIdx.x; t < L_OUT; t += 64) sm_coef[t] = 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nb = a.nb;  // (uniform)
        const double min_count = a.params[3 * i], K = a.params[3 * i + 1], mu = a.params[3 * i + 2];
        double* coef = sm_coef;
        double* dcoef = sm_coef + LSM_COEF_STRIDE;
        switch (a.fn) {
            case L_SOLVE_NB:
#define CALL(NB) lsm_solve_nb<NB>(sm_mom, min_count, K, coef)
                MCG_DEBUG_LSM_NB(CALL)
#undef CALL
                break;
            case L_SOLVE_NB_TAN:
#define CALL(NB) lsm_solve_nb<NB, true>(sm_mom, min_count, K, coef, dcoef)
                MCG_DEBUG_LSM_NB(CALL)
#undef CALL
                break;
            case L_SOLVE_ONE: lsm_solve_one(sm_mom, nb, min_count, K, coef); break;
            case L_CENTERED: lsm_solve_centered(sm_mom, nb, mu, K, coef, sm_ws); break;
            case L_CENTERED_TAN: lsm_solve_centered_tan(sm_mom, nb, mu, K, coef, dcoef, sm_ws); break;
            case L_RCP_RSQRT:
                coef[0] = lsm_rcp(sm_mom[0]);
                coef[1] = lsm_rsqrt(sm_mom[0]);
                break;
            default:
#define CALL(NB) coef[0] = debug_lsm_continuation<NB>(sm_mom)
                MCG_DEBUG_LSM_NB(CALL)
#undef CALL
                break;
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < L_OUT; t += 64) a.out[i * L_OUT + t] = sm_coef[t];
}
#undef MCG_DEBUG_LSM_NB

}  // namespace mcg

extern "C" int mcg_debug_lsm_solve(mcg_ctx* ctx, int fn, int nb, const double* moments, int n_moments, const double* params,
                                   double* out, int64_t n) {
    using namespace mcg;
    static_assert(L_OUT == 48, "the header's 48 doubles per element");
    if (!ctx || !moments || !params || !out) return fail(MCG_ERR_INVALID, "NULL argument");
    if (n < 0 || fn < 0 || fn >= L_COUNT) return fail(MCG_ERR_INVALID, "bad arguments");
    if (n > (int64_t)1 << 20) return fail(MCG_ERR_INVALID, "at most 2^20 elements");
    const bool centred = fn == L_CENTERED || fn == L_CENTERED_TAN;
    const int nb_max = centred ? LSM_MAX_NB : 9;
    if (fn != L_RCP_RSQRT && (nb < 1 || nb > nb_max)) return fail(MCG_ERR_INVALID, "fn %d takes nb 1..%d", fn, nb_max);
    const int want = fn == L_RCP_RSQRT ? 1 : fn == L_CONTINUATION ? nb + 2 : fn == L_SOLVE_NB_TAN || fn == L_CENTERED_TAN ? 4 * nb - 1 : 3 * nb - 1;
    if (n_moments != want) return fail(MCG_ERR_INVALID, "fn %d at nb %d takes %d doubles per element", fn, nb, want);
    if (n == 0) return MCG_OK;
    MCG_HIP(hipSetDevice(ctx->device));
    const size_t n_in = (size_t)n * n_moments, n_par = (size_t)n * 3, n_out = (size_t)n * L_OUT;
    double* buf = nullptr;  // moments, params, out
    MCG_HIP(hipMalloc((void**)&buf, (n_in + n_par + n_out) * sizeof(double)));
    DebugLsmArgs a;
    a.fn = fn;
    a.nb = nb;
    a.n_moments = n_moments;
    a.moments = buf;
    a.params = buf + n_in;
    a.out = buf + n_in + n_par;
    int rc = MCG_OK;
    if (hipMemcpyAsync(buf, moments, n_in * sizeof(double), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(buf + n_in, params, n_par * sizeof(double), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        rc = fail(MCG_ERR_HIP, "H2D failed");
    if (rc == MCG_OK) {
        hipLaunchKernelGGL(k_debug_lsm_solve, dim3((unsigned)n), dim3(64), 0, ctx->stream, a);
        if (hipMemcpyAsync(out, a.out, n_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess)
            rc = fail(MCG_ERR_HIP, "debug lsm solve failed: %s", hipGetErrorString(hipGetLastError()));
    }
    (void)hipFree(buf);
    return rc;
}

extern "C" int mcg_debug_bates_constants(double lambda, double mu_j, double sigma_j, double dt, uint32_t T[16], double* comp) {
    using namespace mcg;
    static_assert(JUMP_CAP == 16, "the header's T[16]");
    if (!T || !comp) return fail(MCG_ERR_INVALID, "NULL output");
    uint32_t t[JUMP_CAP];
    bates_constants(lambda, mu_j, sigma_j, dt, t, *comp);
    for (int k = 0; k < JUMP_CAP; ++k) T[k] = t[k];
    return MCG_OK;
}

extern "C" int mcg_debug_eval_v(mcg_ctx* ctx, int fn, const double* x, int n_in, const double* params, int n_params, double* y,
                                int64_t n) {
    using namespace mcg;
    if (!ctx || !x || !y || n < 0 || fn < 0 || fn >= V_COUNT) return fail(MCG_ERR_INVALID, "bad arguments");
    if (n_in != V_SHAPE[fn][0] || n_params != V_SHAPE[fn][1] || (n_params > 0 && !params))
        return fail(MCG_ERR_INVALID, "fn %d takes %d doubles per element and %d parameters", fn, V_SHAPE[fn][0], V_SHAPE[fn][1]);
    if (n > (int64_t)1 << 24) return fail(MCG_ERR_INVALID, "at most 2^24 elements");
    DebugBatesArgs b = {};
    if (fn == V_BATES_COUNT) {
        const auto word = [](double w) { return w >= 0.0 && w < 0x1p32 && w == std::floor(w); };
        const double L = params[0], elem = params[4 + JUMP_CAP];
        if (!(L >= 0.0 && L <= 1.0) || !(elem == 0.0 || elem == 1.0 || elem == 2.0 || elem == 3.0))
            return fail(MCG_ERR_INVALID, "L must lie in [0, 1] and elem be 0..3");
        b.c.rare.mu_j = params[1];
        b.c.rare.sigma_j = params[2];
        b.c.comp = params[3];
        for (int k = 0; k < JUMP_CAP; ++k) {
            if (!word(params[4 + k])) return fail(MCG_ERR_INVALID, "threshold %d is no 32-bit word", k);
            b.c.rare.T[k] = (uint32_t)params[4 + k];
        }
        b.c.T0 = b.c.rare.T[0];
        b.c.T1 = b.c.rare.T[1];
        b.n_paths = n;
        b.n_steps = (int)elem;
        for (int64_t i = 0; i < n; ++i)
            for (int e = 0; e < 4; ++e)
                if (!word(x[5 * i + e])) return fail(MCG_ERR_INVALID, "element %lld: word %d is no 32-bit word", (long long)i, e);
    }
    DebugVArgs a;
    a.fn = fn;
    a.n_in = n_in;
    a.n = n;
    for (int k = 0; k < V_MAX_PARAMS; ++k) a.p[k] = k < n_params ? params[k] : 0.0;
    a.scale = fn == V_NEG2LOG_SCALED ? a.p[0] : a.p[0] * a.p[0];
    a.ls = fm::make_log_scale(a.scale);
    if (fn == V_QE_STEP) {
        const double k0 = a.p[8], k1 = a.p[9], block = a.p[10], elem = a.p[11];
        if (!(k0 >= 0.0 && k0 < 0x1p32 && k1 >= 0.0 && k1 < 0x1p32 && block >= 0.0 && block < 0x1p32 && elem >= 0.0 && elem <= 3.0))
            return fail(MCG_ERR_INVALID, "k0, k1, block must be 32-bit words and elem 0..3");
    }
    if (n == 0) return MCG_OK;
    MCG_HIP(hipSetDevice(ctx->device));
    double *dx = nullptr, *dy = nullptr;
    MCG_HIP(hipMalloc((void**)&dx, (size_t)n * n_in * sizeof(double)));
    if (hipMalloc((void**)&dy, (size_t)n * 4 * sizeof(double)) != hipSuccess) {
        (void)hipFree(dx);
        return fail(MCG_ERR_OOM, "hipMalloc failed");
    }
    a.x = dx;
    a.y = dy;
    b.var = dx;
    b.out = dy;
    a.gtab = (const double2*)ctx->log_tab;
    a.sincos2 = (const double2*)ctx->sincos2_tab;
    int rc = MCG_OK;
    if (hipMemcpyAsync(dx, x, (size_t)n * n_in * sizeof(double), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        rc = fail(MCG_ERR_HIP, "H2D failed");
    if (rc == MCG_OK) {
        if (fn == V_QE_STEP)
            hipLaunchKernelGGL(k_debug_qe_step, dim3((unsigned)((n + 511) / 512)), dim3(256), 0, ctx->stream, a);
        else if (fn == V_BATES_COUNT)
            hipLaunchKernelGGL(k_debug_bates_count, dim3((unsigned)((n + 511) / 512)), dim3(256), 0, ctx->stream, b);
        else hipLaunchKernelGGL(k_debug_eval_v, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, a);
        if (hipMemcpyAsync(y, dy, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess)
            rc = fail(MCG_ERR_HIP, "debug eval failed: %s", hipGetErrorString(hipGetLastError()));
    }
    (void)hipFree(dx);
    (void)hipFree(dy);
    return rc;
}

extern "C" int mcg_debug_eval(mcg_ctx* ctx, int fn, const double* x, double* y, int64_t n) {
    using namespace mcg;
    if (!ctx || !x || !y || n < 0 || fn < 0 || fn > 16) return fail(MCG_ERR_INVALID, "bad arguments");
    if (n == 0) return MCG_OK;
    MCG_HIP(hipSetDevice(ctx->device));
    double *dx = nullptr, *dy = nullptr;
    MCG_HIP(hipMalloc((void**)&dx, (size_t)n * sizeof(double)));
    if (hipMalloc((void**)&dy, (size_t)n * 4 * sizeof(double)) != hipSuccess) {
        (void)hipFree(dx);
        return fail(MCG_ERR_OOM, "hipMalloc failed");
    }
    int rc = MCG_OK;
    if (hipMemcpyAsync(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        rc = fail(MCG_ERR_HIP, "H2D failed");
    if (rc == MCG_OK) {
        if (fn == 16) hipLaunchKernelGGL(k_debug_sobol_normal, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, dx, dy, n);
        else
            hipLaunchKernelGGL(k_debug_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, fn, dx, dy, n,
                               (const double2*)ctx->log_tab, (const double2*)ctx->sincos2_tab);
        if (hipMemcpyAsync(y, dy, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess)
            rc = fail(MCG_ERR_HIP, "debug eval failed: %s", hipGetErrorString(hipGetLastError()));
    }
    (void)hipFree(dx);
    (void)hipFree(dy);
    return rc;
}
