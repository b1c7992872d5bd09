// C ABI of libmcgpu.so (include/mcgpu.h): context, device-buffer pool, error plumbing, timing,
// path-matrix handles and layout conversion.  The numerical kernels live in kernels_*.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../host/barrier_bridge.hpp"
#include "fastmath_tables.hpp"
#include "mcg_internal.hpp"

namespace mcg {

static thread_local std::string g_err;
Stats g_stats;

static void set_error_v(const char* fmt, va_list ap) {
    char buf[512];
    vsnprintf(buf, sizeof buf, fmt, ap);
    g_err = buf;
}

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    set_error_v(fmt, ap);
    va_end(ap);
}

int fail(int status, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    set_error_v(fmt, ap);
    va_end(ap);
    return status;
}

// ---- pool ------------------------------------------------------------------------------------
int pool_alloc(mcg_ctx* ctx, size_t bytes, void** out) {
    // best fit among cached buffers that are not more than 25% larger than requested
    int best = -1;
    for (size_t i = 0; i < ctx->pool.size(); ++i) {
        const size_t b = ctx->pool[i].bytes;
        if (b >= bytes && b <= bytes + bytes / 4 + 4096 && (best < 0 || b < ctx->pool[best].bytes)) best = (int)i;
    }
    if (best >= 0) {
        *out = ctx->pool[best].ptr;
        ctx->pool.erase(ctx->pool.begin() + best);
        return MCG_OK;
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        // drop the cache and retry once
        for (auto& b : ctx->pool) (void)hipFree(b.ptr);
        ctx->pool.clear();
        (void)hipGetLastError();
        e = hipMalloc(&p, bytes);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MCG_ERR_OOM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    }
    *out = p;
    return MCG_OK;
}

void pool_release(mcg_ctx* ctx, void* ptr, size_t bytes) {
    if (ptr) ctx->pool.push_back(PoolBuf{ptr, bytes});
}

int ensure_cap(mcg_ctx* ctx, double** buf, size_t* cap, size_t need_doubles) {
    if (*cap >= need_doubles && *buf) return MCG_OK;
    if (*buf) {
        MCG_HIP(hipStreamSynchronize(ctx->stream));
        MCG_HIP(hipFree(*buf));
        *buf = nullptr;
        *cap = 0;
    }
    size_t n = need_doubles + need_doubles / 2 + 1024;
    MCG_HIP(hipMalloc((void**)buf, n * sizeof(double)));
    *cap = n;
    return MCG_OK;
}

// ---- timing ----------------------------------------------------------------------------------
TimedLaunch::TimedLaunch(mcg_ctx* c, int k, int64_t launches) : ctx(c), kernel(k), on(c->timing && ((c->timing_mask >> k) & 1u)) {
    if (!on) return;
    if (!ctx->ev_free.empty()) {
        ev = ctx->ev_free.back();
        ctx->ev_free.pop_back();
    } else {
        if (hipEventCreate(&ev.a) != hipSuccess) {
            on = false;
            return;
        }
        if (hipEventCreate(&ev.b) != hipSuccess) {
            (void)hipEventDestroy(ev.a);
            on = false;
            return;
        }
    }
    ev.launches = launches;
    (void)hipEventRecord(ev.a, ctx->stream);
}

TimedLaunch::~TimedLaunch() {
    if (!on) return;
    (void)hipEventRecord(ev.b, ctx->stream);
    ctx->ev_live.emplace_back(kernel, ev);
}

static int timing_collect(mcg_ctx* ctx) {
    if (ctx->ev_live.empty()) return MCG_OK;
    MCG_HIP(hipStreamSynchronize(ctx->stream));
    for (auto& kv : ctx->ev_live) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, kv.second.a, kv.second.b) == hipSuccess) {
            ctx->t_total[kv.first] += ms;
            ctx->t_count[kv.first] += kv.second.launches;
        }
        ctx->ev_free.push_back(kv.second);
    }
    ctx->ev_live.clear();
    return MCG_OK;
}

// ---- path handles ----------------------------------------------------------------------------
int paths_new(mcg_ctx* ctx, int64_t n_paths, int n_steps, uint64_t path_begin, mcg_paths** out) {
    mcg_paths* P = new (std::nothrow) mcg_paths();
    if (!P) return fail(MCG_ERR_OOM, "host allocation failed");
    P->ctx = ctx;
    P->n_paths = n_paths;
    P->n_steps = n_steps;
    // rows start 2 KiB aligned and are padded to a whole 256-thread block, so generator kernels
    // store unconditionally (columns >= n_paths are scratch and never read back)
    P->ld = (n_paths + 255) / 256 * 256;
    if (P->ld == 0) P->ld = 256;
    P->path_begin = path_begin;
    P->bytes = (size_t)P->ld * (size_t)(n_steps + 1) * sizeof(double);
    void* p = nullptr;
    int rc = pool_alloc(ctx, P->bytes, &p);
    if (rc) {
        delete P;
        return rc;
    }
    P->data = (double*)p;
    ctx->live_paths.push_back(P);
    *out = P;
    return MCG_OK;
}

// The tail of a generator's entry point, behind its argument checks: a matrix of n_paths x n_steps for every non-null entry
// of outs (n_outs <= 9: eight assets and their combination), launch(H) -- H[k] is the handle of outs[k], or null -- when there
// are paths, and then either every handle freed and no output written, or the handles handed out, the first n_generated
// entries marked mcg_paths::generated.
template <class Launch>
static int generate(mcg_ctx* ctx, int64_t n_paths, int n_steps, uint64_t path_begin, mcg_paths** const* outs, int n_outs,
                    int n_generated, Launch&& launch) {
    mcg_paths* H[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int rc = MCG_OK;
    for (int k = 0; k < n_outs && rc == MCG_OK; ++k)
        if (outs[k]) rc = paths_new(ctx, n_paths, n_steps, path_begin, &H[k]);
    if (rc == MCG_OK && n_paths > 0) rc = launch(H);
    for (int k = 0; k < n_outs; ++k) {
        if (rc) {
            mcg_paths_free(H[k]);
        } else if (outs[k]) {
            H[k]->generated = k < n_generated;
            *outs[k] = H[k];
        }
    }
    return rc;
}

// ---- layout conversion -----------------------------------------------------------------------
// dst[c*dst_ld + r] = src[r*src_ld + c] for r < R, c < C, through a padded 32x32 LDS tile.
__global__ __launch_bounds__(256) void k_transpose(const double* __restrict__ src, int64_t src_ld,
                                                   double* __restrict__ dst, int64_t dst_ld, int64_t R, int64_t C) {
    __shared__ double tile[32][33];
    const int64_t c0 = (int64_t)blockIdx.x * 32, r0 = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int k = ty; k < 32; k += 8) {
        const int64_t r = r0 + k, c = c0 + tx;
        if (r < R && c < C) tile[k][tx] = src[r * src_ld + c];
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int64_t c = c0 + k, r = r0 + tx;
        if (r < R && c < C) dst[c * dst_ld + r] = tile[tx][k];
    }
}

static int transpose(mcg_ctx* ctx, const double* src, int64_t src_ld, double* dst, int64_t dst_ld, int64_t R,
                     int64_t C) {
    if (R == 0 || C == 0) return MCG_OK;
    // gridDim.y and gridDim.x are limited (65535 and 2^31-1 blocks): walk over-long dimensions in slabs
    constexpr int64_t MAX_Y = 65535ll * 32, MAX_X = 0x7fffffffll / 32 * 32;
    for (int64_t r0 = 0; r0 < R; r0 += MAX_Y) {
        const int64_t Rs = std::min(R - r0, MAX_Y);
        for (int64_t c0 = 0; c0 < C; c0 += MAX_X) {
            const int64_t Cs = std::min(C - c0, MAX_X);
            const int64_t gx = (Cs + 31) / 32, gy = (Rs + 31) / 32;
            TimedLaunch t(ctx, MCG_K_TRANSPOSE);
            hipLaunchKernelGGL(k_transpose, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, ctx->stream,
                               src + r0 * src_ld + c0, src_ld, dst + c0 * dst_ld + r0, dst_ld, Rs, Cs);
        }
    }
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

// chunk of paths moved per staging round trip (bounds the temporary to ~512 MiB)
static int64_t chunk_paths(int n_cols) {
    int64_t c = (int64_t)(512ull << 20) / ((int64_t)n_cols * 8);
    c = c / 64 * 64;
    return c < 64 ? 64 : c;
}

}  // namespace mcg

using namespace mcg;

extern "C" {

const char* mcg_last_error(void) { return g_err.c_str(); }

const char* mcg_version(void) { return "mcgpu 0.1 (gfx950, philox4x32-10, fp64)"; }

int mcg_device_count(int* count) {
    if (!count) return fail(MCG_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *count = 0;
        return fail(MCG_ERR_NO_DEVICE, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
    }
    *count = n;
    return MCG_OK;
}

static int init_impl(mcg_ctx** out, int device, bool adopt, void* external_stream) {
    if (!out) return fail(MCG_ERR_INVALID, "ctx out pointer is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(MCG_ERR_NO_DEVICE,
                    "no HIP device available (%s); libmcgpu has no CPU fallback by design",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    }
    if (device < 0 || device >= n) return fail(MCG_ERR_INVALID, "device %d out of range [0,%d)", device, n);
    MCG_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    MCG_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MCG_ERR_NO_DEVICE, "device %d is %s; libmcgpu is built for gfx950 (MI355X) only", device,
                    prop.gcnArchName);
    mcg_ctx* ctx = new (std::nothrow) mcg_ctx();
    if (!ctx) return fail(MCG_ERR_OOM, "host allocation failed");
    ctx->device = device;
    ctx->n_cus = prop.multiProcessorCount;
    ctx->coop_launch = true;
    if (adopt) {
        ctx->stream = (hipStream_t)external_stream;
        ctx->owns_stream = false;
    } else {
        hipError_t se = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (se != hipSuccess) {
            delete ctx;
            return fail(MCG_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(se));
        }
        ctx->owns_stream = true;
    }
    if (hipMalloc((void**)&ctx->scalars, SCALARS_DOUBLES * sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&ctx->clk_stamps, sizeof(unsigned long long) * 2 * GBM_CLK_SLOTS) != hipSuccess ||
        hipHostMalloc((void**)&ctx->h_scalars, SCALARS_DOUBLES * sizeof(double)) != hipSuccess) {
        mcg_finalize(ctx);
        return fail(MCG_ERR_OOM, "workspace allocation failed");
    }
    // (the three generated tables back to back = fm::Tables, fastmath.hpp)
    constexpr size_t n_log = sizeof(fm::LOG_TAB_HOST) / sizeof(double), n_sc = sizeof(fm::SINCOS_TAB_HOST) / sizeof(double);
    if (hipMalloc((void**)&ctx->log_tab, sizeof(fm::LOG_TAB_HOST) + sizeof(fm::SINCOS_TAB_HOST) + sizeof(fm::EXP2_TAB_HOST)) != hipSuccess ||
        hipMemcpy(ctx->log_tab, fm::LOG_TAB_HOST, sizeof(fm::LOG_TAB_HOST), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ctx->log_tab + n_log, fm::SINCOS_TAB_HOST, sizeof(fm::SINCOS_TAB_HOST), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ctx->log_tab + n_log + n_sc, fm::EXP2_TAB_HOST, sizeof(fm::EXP2_TAB_HOST), hipMemcpyHostToDevice) != hipSuccess) {
        mcg_finalize(ctx);
        return fail(MCG_ERR_OOM, "table upload failed");
    }
    constexpr size_t sincos2_bytes = sizeof(double) * 4 * SINCOS2_ENTRIES;
    if (hipMalloc((void**)&ctx->sincos2_tab, sincos2_bytes) != hipSuccess ||
        hipMemcpy(ctx->sincos2_tab, host_sincos2_tables(), sincos2_bytes, hipMemcpyHostToDevice) != hipSuccess) {
        mcg_finalize(ctx);
        return fail(MCG_ERR_OOM, "table upload failed");
    }
    *out = ctx;
    return MCG_OK;
}

int mcg_init(mcg_ctx** out, int device) { return init_impl(out, device, false, nullptr); }

int mcg_init_on_stream(mcg_ctx** out, int device, void* stream) { return init_impl(out, device, true, stream); }

int mcg_finalize(mcg_ctx* ctx) {
    if (!ctx) return MCG_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    comm_release(ctx);
    shm_release(ctx);
    for (mcg_paths* P : ctx->live_paths) {  // handles the caller still holds: orphan them (see mcg_paths_free)
        if (P->data) (void)hipFree(P->data);
        P->data = nullptr;
        P->ctx = nullptr;
    }
    ctx->live_paths.clear();
    for (auto& b : ctx->pool) (void)hipFree(b.ptr);
    ctx->pool.clear();
    for (auto& kv : ctx->ev_live) {
        (void)hipEventDestroy(kv.second.a);
        (void)hipEventDestroy(kv.second.b);
    }
    for (auto& ev : ctx->ev_free) {
        (void)hipEventDestroy(ev.a);
        (void)hipEventDestroy(ev.b);
    }
    if (ctx->partials) (void)hipFree(ctx->partials);
    if (ctx->fin_chunks) (void)hipFree(ctx->fin_chunks);
    if (ctx->scalars) (void)hipFree(ctx->scalars);
    if (ctx->clk_stamps) (void)hipFree(ctx->clk_stamps);
    if (ctx->h_scalars) (void)hipHostFree(ctx->h_scalars);
    if (ctx->weights) (void)hipFree(ctx->weights);
    if (ctx->lsm_v) (void)hipFree(ctx->lsm_v);
    if (ctx->lsm_dv) (void)hipFree(ctx->lsm_dv);
    if (ctx->log_tab) (void)hipFree(ctx->log_tab);
    if (ctx->sincos2_tab) (void)hipFree(ctx->sincos2_tab);
    if (ctx->batch_fork) (void)hipEventDestroy(ctx->batch_fork);
    if (ctx->batch_join) (void)hipEventDestroy(ctx->batch_join);
    if (ctx->batch_aux) (void)hipStreamDestroy(ctx->batch_aux);
    if (ctx->owns_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return MCG_OK;
}

int mcg_synchronize(mcg_ctx* ctx) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    MCG_HIP(hipStreamSynchronize(ctx->stream));
    return MCG_OK;
}

int mcg_trim(mcg_ctx* ctx) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    MCG_HIP(hipStreamSynchronize(ctx->stream));
    for (auto& b : ctx->pool) (void)hipFree(b.ptr);
    ctx->pool.clear();
    return MCG_OK;
}

int mcg_set_allreduce(mcg_ctx* ctx, mcg_allreduce_fn fn, void* user) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    shm_release(ctx);  // a collective installed from outside replaces the node-local one, mailbox included
    ctx->allreduce = fn;
    ctx->allreduce_user = user;
    return MCG_OK;
}

// ---- generation --------------------------------------------------------------------------------
static int check_gen_args(mcg_ctx* ctx, double S0, double dt, int n_steps, int64_t n_paths, mcg_paths** out) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    if (!out) return fail(MCG_ERR_INVALID, "out is NULL");
    if (n_steps < 1) return fail(MCG_ERR_INVALID, "n_steps must be >= 1 (got %d)", n_steps);
    if (n_paths < 0) return fail(MCG_ERR_INVALID, "n_paths must be >= 0 (got %lld)", (long long)n_paths);
    if (!(dt > 0.0)) return fail(MCG_ERR_INVALID, "dt must be > 0");
    if (!std::isfinite(S0)) return fail(MCG_ERR_INVALID, "S0 must be finite");
    MCG_HIP(hipSetDevice(ctx->device));
    return MCG_OK;
}

// sobol: null for the Philox stream `seed`; a Sobol' entry point passes the address of its own argument, so that a point set
// that is NULL is sobol_check_shape's to report (kernels_sobol.hip; `seed` is unused then)
static int gen_gbm(mcg_ctx* ctx, uint64_t seed, double S0, double r, double sigma, double dt, int n_steps,
                   uint64_t path_begin, int64_t n_paths, bool payoff, double K, int is_call, mcg_paths** out,
                   const mcg_sobol* const* sobol = nullptr) {
    int rc = sobol ? sobol_check_shape(*sobol, n_steps, path_begin, n_paths) : MCG_OK;
    if (rc) return rc;
    rc = check_gen_args(ctx, S0, dt, n_steps, n_paths, out);
    if (rc) return rc;
    if (!(sigma >= 0.0)) return fail(MCG_ERR_INVALID, "sigma must be >= 0");
    return generate(ctx, n_paths, n_steps, path_begin, &out, 1, 1, [&](mcg_paths* const* H) {
        return sobol ? launch_sobol(ctx, H[0], *sobol, S0, (r - 0.5 * sigma * sigma) * dt, sigma * std::sqrt(dt), nullptr, 0, nullptr, 0,
                                    payoff, K, is_call)
                     : launch_gbm(ctx, H[0], seed, S0, r, sigma, dt, payoff, K, is_call);
    });
}

int mcg_paths_gbm(mcg_ctx* ctx, uint64_t seed, double S0, double r, double sigma, double dt, int n_steps,
                  uint64_t path_begin, int64_t n_paths, mcg_paths** out) {
    return gen_gbm(ctx, seed, S0, r, sigma, dt, n_steps, path_begin, n_paths, false, 0.0, 0, out);
}

int mcg_paths_gbm_payoff(mcg_ctx* ctx, uint64_t seed, double S0, double r, double sigma, double dt, int n_steps,
                         uint64_t path_begin, int64_t n_paths, double K, int is_call, mcg_paths** out) {
    return gen_gbm(ctx, seed, S0, r, sigma, dt, n_steps, path_begin, n_paths, true, K, is_call, out);
}

int mcg_paths_gbm_sobol(mcg_ctx* ctx, const mcg_sobol* sobol, double S0, double r, double sigma, double dt, int n_steps,
                        uint64_t path_begin, int64_t n_paths, mcg_paths** out) {
    return gen_gbm(ctx, 0, S0, r, sigma, dt, n_steps, path_begin, n_paths, false, 0.0, 0, out, &sobol);
}

int mcg_paths_gbm_sobol_payoff(mcg_ctx* ctx, const mcg_sobol* sobol, double S0, double r, double sigma, double dt, int n_steps,
                               uint64_t path_begin, int64_t n_paths, double K, int is_call, mcg_paths** out) {
    return gen_gbm(ctx, 0, S0, r, sigma, dt, n_steps, path_begin, n_paths, true, K, is_call, out, &sobol);
}

static int gen_rb(mcg_ctx* ctx, uint64_t seed, double S0, double r, double xi, double H, double eta, double rho,
                  double dt, int n_steps, uint64_t path_begin, int64_t n_paths, bool payoff, double K, int is_call,
                  mcg_paths** out) {
    int rc = check_gen_args(ctx, S0, dt, n_steps, n_paths, out);
    if (rc) return rc;
    if (!(xi >= 0.0)) return fail(MCG_ERR_INVALID, "xi must be >= 0");
    if (!(H >= 0.0) || !std::isfinite(H)) return fail(MCG_ERR_INVALID, "H must be >= 0");
    if (!std::isfinite(eta)) return fail(MCG_ERR_INVALID, "eta must be finite");
    if (!(std::fabs(rho) <= 1.0)) return fail(MCG_ERR_INVALID, "|rho| must be <= 1");
    if (n_steps > (1 << 24)) return fail(MCG_ERR_INVALID, "rBergomi n_steps must be <= 2^24 (got %d)", n_steps);  // (66 000 years of trading days)
    return generate(ctx, n_paths, n_steps, path_begin, &out, 1, 1,
                    [&](mcg_paths* const* P) { return launch_rbergomi(ctx, P[0], seed, S0, r, xi, H, eta, dt, payoff, K, is_call); });
}

int mcg_paths_rbergomi(mcg_ctx* ctx, uint64_t seed, double S0, double r, double xi, double H, double eta, double rho,
                       double dt, int n_steps, uint64_t path_begin, int64_t n_paths, mcg_paths** out) {
    return gen_rb(ctx, seed, S0, r, xi, H, eta, rho, dt, n_steps, path_begin, n_paths, false, 0.0, 0, out);
}

int mcg_paths_rbergomi_payoff(mcg_ctx* ctx, uint64_t seed, double S0, double r, double xi, double H, double eta,
                              double rho, double dt, int n_steps, uint64_t path_begin, int64_t n_paths, double K,
                              int is_call, mcg_paths** out) {
    return gen_rb(ctx, seed, S0, r, xi, H, eta, rho, dt, n_steps, path_begin, n_paths, true, K, is_call, out);
}

static int gen_heston(mcg_ctx* ctx, uint64_t seed, double S0, double r, double v0, double kappa, double theta, double sigma_v,
                      double rho, double dt, int n_steps, uint64_t path_begin, int64_t n_paths, bool payoff, double K, int is_call,
                      mcg_paths** out, mcg_paths** var_out, bool qe = false, const double* jump = nullptr) {
    // jump: {lambda, mu_j, sigma_j} of mcg_paths_bates*, or null
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    const double args[] = {S0, r, v0, kappa, theta, sigma_v, rho, dt};
    const char* names[] = {"S0", "r", "v0", "kappa", "theta", "sigma_v", "rho", "dt"};
    for (int i = 0; i < 8; ++i)
        if (!std::isfinite(args[i])) return fail(MCG_ERR_INVALID, "Heston: %s must be finite", names[i]);
    if (payoff && !std::isfinite(K)) return fail(MCG_ERR_INVALID, "Heston: K must be finite");
    int rc = check_gen_args(ctx, S0, dt, n_steps, n_paths, out);
    if (rc) return rc;
    if (!(S0 > 0.0)) return fail(MCG_ERR_INVALID, "Heston: S0 must be > 0");
    if (!(v0 >= 0.0)) return fail(MCG_ERR_INVALID, "Heston: v0 must be >= 0");
    if (!(kappa >= 0.0)) return fail(MCG_ERR_INVALID, "Heston: kappa must be >= 0");
    if (!(theta >= 0.0)) return fail(MCG_ERR_INVALID, "Heston: theta must be >= 0");
    if (!(sigma_v >= 0.0)) return fail(MCG_ERR_INVALID, "Heston: sigma_v must be >= 0");
    if (!(std::fabs(rho) <= 1.0)) return fail(MCG_ERR_INVALID, "Heston: |rho| must be <= 1");
    if (qe && !(sigma_v > 0.0))
        return fail(MCG_ERR_INVALID, "Heston QE: sigma_v must be > 0 (the scheme divides by it); mcg_paths_heston takes sigma_v = 0");
    if (jump) {
        const double lambda = jump[0], mu_j = jump[1], sigma_j = jump[2];
        if (!std::isfinite(lambda)) return fail(MCG_ERR_INVALID, "Bates: lambda must be finite");
        if (!std::isfinite(mu_j)) return fail(MCG_ERR_INVALID, "Bates: mu_j must be finite");
        if (!std::isfinite(sigma_j)) return fail(MCG_ERR_INVALID, "Bates: sigma_j must be finite");
        if (!(lambda >= 0.0)) return fail(MCG_ERR_INVALID, "Bates: lambda must be >= 0");
        if (!(sigma_j >= 0.0)) return fail(MCG_ERR_INVALID, "Bates: sigma_j must be >= 0");
        if (!(lambda * dt <= 1.0))
            return fail(MCG_ERR_INVALID, "Bates: lambda * dt = %g exceeds the bound lambda * dt <= 1 of the jump count: use more steps",
                        lambda * dt);
        if (!(std::fabs(mu_j) <= 1.0)) return fail(MCG_ERR_INVALID, "Bates: |mu_j| must be <= 1");
        if (!(sigma_j <= 1.0)) return fail(MCG_ERR_INVALID, "Bates: sigma_j must be <= 1");
    }
    mcg_paths** const outs[2] = {out, var_out};  // (the variance matrix is a plain one)
    return generate(ctx, n_paths, n_steps, path_begin, outs, 2, 1, [&](mcg_paths* const* H) {
        if (jump)
            return launch_bates(ctx, H[0], H[1], seed, S0, r, v0, kappa, theta, sigma_v, rho, jump[0], jump[1], jump[2], dt, qe, payoff, K,
                                is_call);
        return (qe ? launch_heston_qe : launch_heston)(ctx, H[0], H[1], seed, S0, r, v0, kappa, theta, sigma_v, rho, dt, payoff, K, is_call);
    });
}

int mcg_paths_heston(mcg_ctx* ctx, uint64_t seed, double S0, double r, double v0, double kappa, double theta,
                     double sigma_v, double rho, double dt, int n_steps, uint64_t path_begin, int64_t n_paths,
                     mcg_paths** out, mcg_paths** var_out) {
    return gen_heston(ctx, seed, S0, r, v0, kappa, theta, sigma_v, rho, dt, n_steps, path_begin, n_paths, false, 0.0, 0, out,
                      var_out);
}

int mcg_paths_heston_payoff(mcg_ctx* ctx, uint64_t seed, double S0, double r, double v0, double kappa, double theta,
                            double sigma_v, double rho, double dt, int n_steps, uint64_t path_begin, int64_t n_paths,
                            double K, int is_call, mcg_paths** out, mcg_paths** var_out) {
    return gen_heston(ctx, seed, S0, r, v0, kappa, theta, sigma_v, rho, dt, n_steps, path_begin, n_paths, true, K, is_call,
                      out, var_out);
}

int mcg_paths_heston_qe(mcg_ctx* ctx, uint64_t seed, double S0, double r, double v0, double kappa, double theta,
                        double sigma_v, double rho, double dt, int n_steps, uint64_t path_begin, int64_t n_paths,
                        mcg_paths** out, mcg_paths** var_out) {
    return gen_heston(ctx, seed, S0, r, v0, kappa, theta, sigma_v, rho, dt, n_steps, path_begin, n_paths, false, 0.0, 0, out,
                      var_out, true);
}

int mcg_paths_heston_qe_payoff(mcg_ctx* ctx, uint64_t seed, double S0, double r, double v0, double kappa, double theta,
                               double sigma_v, double rho, double dt, int n_steps, uint64_t path_begin, int64_t n_paths,
                               double K, int is_call, mcg_paths** out, mcg_paths** var_out) {
    return gen_heston(ctx, seed, S0, r, v0, kappa, theta, sigma_v, rho, dt, n_steps, path_begin, n_paths, true, K, is_call,
                      out, var_out, true);
}

static int gen_bates(mcg_ctx* ctx, uint64_t seed, double S0, double r, double v0, double kappa, double theta, double sigma_v,
                     double rho, double lambda, double mu_j, double sigma_j, double dt, int n_steps, uint64_t path_begin,
                     int64_t n_paths, int scheme, bool payoff, double K, int is_call, mcg_paths** out, mcg_paths** var_out) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    if (scheme != MCG_HESTON_EULER && scheme != MCG_HESTON_QE)
        return fail(MCG_ERR_INVALID, "Bates: scheme must be MCG_HESTON_EULER (0) or MCG_HESTON_QE (1), not %d", scheme);
    const double jump[3] = {lambda, mu_j, sigma_j};
    return gen_heston(ctx, seed, S0, r, v0, kappa, theta, sigma_v, rho, dt, n_steps, path_begin, n_paths, payoff, K, is_call, out,
                      var_out, scheme == MCG_HESTON_QE, jump);
}

int mcg_paths_bates(mcg_ctx* ctx, uint64_t seed, double S0, double r, double v0, double kappa, double theta, double sigma_v,
                    double rho, double lambda, double mu_j, double sigma_j, double dt, int n_steps, uint64_t path_begin,
                    int64_t n_paths, int scheme, mcg_paths** out, mcg_paths** var_out) {
    return gen_bates(ctx, seed, S0, r, v0, kappa, theta, sigma_v, rho, lambda, mu_j, sigma_j, dt, n_steps, path_begin, n_paths,
                     scheme, false, 0.0, 0, out, var_out);
}

int mcg_paths_bates_payoff(mcg_ctx* ctx, uint64_t seed, double S0, double r, double v0, double kappa, double theta,
                           double sigma_v, double rho, double lambda, double mu_j, double sigma_j, double dt, int n_steps,
                           uint64_t path_begin, int64_t n_paths, int scheme, double K, int is_call, mcg_paths** out,
                           mcg_paths** var_out) {
    return gen_bates(ctx, seed, S0, r, v0, kappa, theta, sigma_v, rho, lambda, mu_j, sigma_j, dt, n_steps, path_begin, n_paths,
                     scheme, true, K, is_call, out, var_out);
}

// ---- multi-asset GBM and combinations ------------------------------------------------------------
// The weights of a combination as the kernels take them: `weights` checked, or ones.
static int combine_weights(int n_assets, int kind, const double* weights, double (&w)[8]) {
    if (kind != MCG_C_BASKET && kind != MCG_C_BEST_OF && kind != MCG_C_WORST_OF)
        return fail(MCG_ERR_INVALID, "combine: kind must be MCG_C_BASKET (0), MCG_C_BEST_OF (1) or MCG_C_WORST_OF (2), not %d", kind);
    for (int a = 0; a < n_assets; ++a) {
        w[a] = weights ? weights[a] : 1.0;
        if (!std::isfinite(w[a])) return fail(MCG_ERR_INVALID, "combine: weight %d must be finite", a);
        if (kind != MCG_C_BASKET && !(w[a] > 0.0))
            return fail(MCG_ERR_INVALID, "combine: weight %d must be > 0 for best-of / worst-of (got %g)", a, w[a]);
    }
    return MCG_OK;
}

int mcg_paths_gbm_multi(mcg_ctx* ctx, uint64_t seed, int n_assets, const double* S0, double r, const double* q,
                        const double* sigma, const double* corr, double dt, int n_steps, uint64_t path_begin, int64_t n_paths,
                        int combine, const double* weights, mcg_paths** assets_out, mcg_paths** combined_out) {
    // (every output handle is NULL on any error, whichever check fails)
    if (combined_out) *combined_out = nullptr;
    if (assets_out && n_assets >= 1 && n_assets <= 8)
        for (int a = 0; a < n_assets; ++a) assets_out[a] = nullptr;
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    if (n_assets < 1 || n_assets > 8) return fail(MCG_ERR_INVALID, "GBM multi: n_assets must be in [1, 8] (got %d)", n_assets);
    if (!S0 || !sigma || !corr) return fail(MCG_ERR_INVALID, "GBM multi: S0/sigma/corr is NULL");
    if (!assets_out && !combined_out) return fail(MCG_ERR_INVALID, "GBM multi: assets_out and combined_out are both NULL");
    if (n_steps < 1) return fail(MCG_ERR_INVALID, "n_steps must be >= 1 (got %d)", n_steps);
    if (n_paths < 0) return fail(MCG_ERR_INVALID, "n_paths must be >= 0 (got %lld)", (long long)n_paths);
    if (!std::isfinite(r)) return fail(MCG_ERR_INVALID, "GBM multi: r must be finite");
    if (!std::isfinite(dt)) return fail(MCG_ERR_INVALID, "GBM multi: dt must be finite");
    if (!(dt > 0.0)) return fail(MCG_ERR_INVALID, "dt must be > 0");
    double zeros[8] = {0, 0, 0, 0, 0, 0, 0, 0}, w[8] = {1, 1, 1, 1, 1, 1, 1, 1}, L[64];
    for (int a = 0; a < n_assets; ++a) {
        if (!std::isfinite(S0[a])) return fail(MCG_ERR_INVALID, "GBM multi: S0[%d] must be finite", a);
        if (!std::isfinite(sigma[a])) return fail(MCG_ERR_INVALID, "GBM multi: sigma[%d] must be finite", a);
        if (q && !std::isfinite(q[a])) return fail(MCG_ERR_INVALID, "GBM multi: q[%d] must be finite", a);
        if (!(S0[a] > 0.0)) return fail(MCG_ERR_INVALID, "GBM multi: S0[%d] must be > 0", a);
        if (!(sigma[a] >= 0.0)) return fail(MCG_ERR_INVALID, "GBM multi: sigma[%d] must be >= 0", a);
    }
    if (combine != MCG_C_NONE) {
        int rc = combine_weights(n_assets, combine, weights, w);
        if (rc) return rc;
    } else if (combined_out) {
        return fail(MCG_ERR_INVALID, "GBM multi: combined_out needs a combine other than MCG_C_NONE");
    }
    int rc = mcg_cholesky_corr(corr, n_assets, L);
    if (rc) return rc;
    MCG_HIP(hipSetDevice(ctx->device));
    mcg_paths** outs[9];  // the assets, then their combination
    for (int a = 0; a < n_assets; ++a) outs[a] = assets_out ? &assets_out[a] : nullptr;
    outs[n_assets] = combined_out;
    return generate(ctx, n_paths, n_steps, path_begin, outs, n_assets + 1, n_assets + 1, [&](mcg_paths* const* H) {
        return launch_gbm_multi(ctx, assets_out ? H : nullptr, H[n_assets], n_assets, seed, S0, r, q ? q : zeros, sigma, L, dt, combine, w);
    });
}

int mcg_paths_combine(mcg_ctx* ctx, const mcg_paths* const* assets, int n_assets, int kind, const double* weights,
                      mcg_paths** out) {
    if (out) *out = nullptr;
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    if (!assets || !out) return fail(MCG_ERR_INVALID, "combine: assets/out is NULL");
    if (n_assets < 1 || n_assets > 8) return fail(MCG_ERR_INVALID, "combine: n_assets must be in [1, 8] (got %d)", n_assets);
    double w[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    int rc = combine_weights(n_assets, kind, weights, w);
    if (rc) return rc;
    bool generated = true;
    for (int a = 0; a < n_assets; ++a) {
        if (!assets[a]) return fail(MCG_ERR_INVALID, "combine: assets[%d] is NULL", a);
        if (assets[a]->ctx != ctx) return fail(MCG_ERR_INVALID, "combine: assets[%d] belongs to a different ctx", a);
        if (assets[a]->n_paths != assets[0]->n_paths || assets[a]->n_steps != assets[0]->n_steps)
            return fail(MCG_ERR_INVALID, "combine: assets[%d] is %lld paths x %d steps, assets[0] %lld x %d", a, (long long)assets[a]->n_paths,
                        assets[a]->n_steps, (long long)assets[0]->n_paths, assets[0]->n_steps);
        generated = generated && assets[a]->generated;
    }
    MCG_HIP(hipSetDevice(ctx->device));
    return generate(ctx, assets[0]->n_paths, assets[0]->n_steps, assets[0]->path_begin, &out, 1, generated ? 1 : 0,
                    [&](mcg_paths* const* P) { return launch_paths_combine(ctx, assets, n_assets, kind, w, P[0]); });
}

// ---- local volatility ------------------------------------------------------------------------------
static int gen_localvol(mcg_ctx* ctx, uint64_t seed, double S0, double r, double q, const double* times, int n_t, double x_min,
                        double x_max, int n_x, const double* sigma, double dt, int n_steps, uint64_t path_begin, int64_t n_paths,
                        bool payoff, double K, int is_call, mcg_paths** out, const mcg_sobol* const* sobol = nullptr) {
    // (the model is checked before the ctx: what is wrong with a surface is reported on a machine without a GPU too)
    if (!out) return fail(MCG_ERR_INVALID, "local vol: out is NULL");
    int rc = sobol ? sobol_check_shape(*sobol, n_steps, path_begin, n_paths) : MCG_OK;  // (sobol: as gen_gbm's)
    if (rc) return rc;
    *out = nullptr;
    rc = localvol_check_surface(times, n_t, n_x, sigma, dt, n_steps);
    if (rc) return rc;
    rc = localvol_check_model(S0, r, q, x_min, x_max, payoff, K);
    if (rc) return rc;
    if (n_paths < 0) return fail(MCG_ERR_INVALID, "n_paths must be >= 0 (got %lld)", (long long)n_paths);
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    MCG_HIP(hipSetDevice(ctx->device));
    // (not marked `generated`: mcg_internal.hpp)
    return generate(ctx, n_paths, n_steps, path_begin, &out, 1, 0, [&](mcg_paths* const* P) {
        const int n_slices = n_t == 1 ? 1 : n_steps;
        std::vector<double> table((size_t)n_slices * (size_t)(n_x - 1) * 2);
        localvol_fill_table(times, n_t, n_x, sigma, dt, n_steps, table.data());
        const LocalVolScalars c = localvol_scalars(r, q, x_min, x_max, n_x, dt);
        return sobol ? launch_sobol(ctx, P[0], *sobol, S0, 0.0, 0.0, &c, n_x, table.data(), n_slices, payoff, K, is_call)
                     : launch_localvol(ctx, P[0], seed, S0, c, n_x, table.data(), n_slices, payoff, K, is_call);
    });
}

int mcg_paths_localvol(mcg_ctx* ctx, uint64_t seed, double S0, double r, double q, const double* times, int n_t, double x_min,
                       double x_max, int n_x, const double* sigma, double dt, int n_steps, uint64_t path_begin, int64_t n_paths,
                       mcg_paths** out) {
    return gen_localvol(ctx, seed, S0, r, q, times, n_t, x_min, x_max, n_x, sigma, dt, n_steps, path_begin, n_paths, false, 0.0, 0,
                        out);
}

int mcg_paths_localvol_payoff(mcg_ctx* ctx, uint64_t seed, double S0, double r, double q, const double* times, int n_t,
                              double x_min, double x_max, int n_x, const double* sigma, double dt, int n_steps,
                              uint64_t path_begin, int64_t n_paths, double K, int is_call, mcg_paths** out) {
    return gen_localvol(ctx, seed, S0, r, q, times, n_t, x_min, x_max, n_x, sigma, dt, n_steps, path_begin, n_paths, true, K,
                        is_call, out);
}

int mcg_paths_localvol_sobol(mcg_ctx* ctx, const mcg_sobol* sobol, double S0, double r, double q, const double* times, int n_t,
                             double x_min, double x_max, int n_x, const double* sigma, double dt, int n_steps, uint64_t path_begin,
                             int64_t n_paths, mcg_paths** out) {
    return gen_localvol(ctx, 0, S0, r, q, times, n_t, x_min, x_max, n_x, sigma, dt, n_steps, path_begin, n_paths, false, 0.0, 0, out,
                        &sobol);
}

int mcg_paths_localvol_sobol_payoff(mcg_ctx* ctx, const mcg_sobol* sobol, double S0, double r, double q, const double* times,
                                    int n_t, double x_min, double x_max, int n_x, const double* sigma, double dt, int n_steps,
                                    uint64_t path_begin, int64_t n_paths, double K, int is_call, mcg_paths** out) {
    return gen_localvol(ctx, 0, S0, r, q, times, n_t, x_min, x_max, n_x, sigma, dt, n_steps, path_begin, n_paths, true, K, is_call,
                        out, &sobol);
}

// ---- host <-> device ---------------------------------------------------------------------------
int mcg_paths_from_host(mcg_ctx* ctx, const double* row_major, int64_t n_paths, int n_cols, mcg_paths** out) {
    if (!ctx || !out) return fail(MCG_ERR_INVALID, "ctx/out is NULL");
    if (n_paths < 1 || n_cols < 1 || !row_major)
        return fail(MCG_ERR_EMPTY_PATHS, "LSM::PredictOptionPrice: Empty pricePaths.");
    MCG_HIP(hipSetDevice(ctx->device));
    mcg_paths* P = nullptr;
    int rc = paths_new(ctx, n_paths, n_cols - 1, 0, &P);
    if (rc) return rc;
    const int64_t chunk = chunk_paths(n_cols);
    void* tmp = nullptr;
    const size_t tmp_bytes = (size_t)std::min<int64_t>(chunk, n_paths) * n_cols * sizeof(double);
    rc = pool_alloc(ctx, tmp_bytes, &tmp);
    if (rc) {
        mcg_paths_free(P);
        return rc;
    }
    for (int64_t p0 = 0; p0 < n_paths && rc == MCG_OK; p0 += chunk) {
        const int64_t cnt = std::min<int64_t>(chunk, n_paths - p0);
        hipError_t e = hipMemcpyAsync(tmp, row_major + p0 * n_cols, (size_t)cnt * n_cols * sizeof(double),
                                      hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            rc = fail(MCG_ERR_HIP, "H2D copy failed: %s", hipGetErrorString(e));
            break;
        }
        // src rows = paths (cnt), cols = n_cols; dst[j*ld + p0 + p]
        rc = transpose(ctx, (const double*)tmp, n_cols, P->data + p0, P->ld, cnt, n_cols);
        if (rc == MCG_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(MCG_ERR_HIP, "sync failed");
    }
    pool_release(ctx, tmp, tmp_bytes);
    if (rc) {
        mcg_paths_free(P);
        return rc;
    }
    *out = P;
    return MCG_OK;
}

int mcg_paths_to_host(const mcg_paths* P, double* row_major_out) {
    if (!P || !row_major_out) return fail(MCG_ERR_INVALID, "paths/out is NULL");
    mcg_ctx* ctx = P->ctx;
    if (!ctx) return fail(MCG_ERR_INVALID, "paths outlived their ctx (mcg_finalize was called first)");
    if (P->n_paths == 0) return MCG_OK;
    MCG_HIP(hipSetDevice(ctx->device));
    const int n_cols = P->n_steps + 1;
    const int64_t chunk = chunk_paths(n_cols);
    void* tmp = nullptr;
    const size_t tmp_bytes = (size_t)std::min<int64_t>(chunk, P->n_paths) * n_cols * sizeof(double);
    int rc = pool_alloc(ctx, tmp_bytes, &tmp);
    if (rc) return rc;
    for (int64_t p0 = 0; p0 < P->n_paths && rc == MCG_OK; p0 += chunk) {
        const int64_t cnt = std::min<int64_t>(chunk, P->n_paths - p0);
        // src rows = steps (n_cols), cols = paths (cnt); dst[p*n_cols + j]
        rc = transpose(ctx, P->data + p0, P->ld, (double*)tmp, n_cols, n_cols, cnt);
        if (rc) break;
        hipError_t e = hipMemcpyAsync(row_major_out + p0 * n_cols, tmp, (size_t)cnt * n_cols * sizeof(double),
                                      hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = fail(MCG_ERR_HIP, "D2H copy failed: %s", hipGetErrorString(e));
    }
    pool_release(ctx, tmp, tmp_bytes);
    return rc;
}

int mcg_paths_to_host_step_major(const mcg_paths* P, double* out) {
    if (!P || !out) return fail(MCG_ERR_INVALID, "paths/out is NULL");
    if (!P->ctx) return fail(MCG_ERR_INVALID, "paths outlived their ctx (mcg_finalize was called first)");
    if (P->n_paths == 0) return MCG_OK;
    MCG_HIP(hipSetDevice(P->ctx->device));
    MCG_HIP(hipMemcpy2DAsync(out, (size_t)P->n_paths * sizeof(double), P->data, (size_t)P->ld * sizeof(double),
                             (size_t)P->n_paths * sizeof(double), (size_t)(P->n_steps + 1), hipMemcpyDeviceToHost,
                             P->ctx->stream));
    MCG_HIP(hipStreamSynchronize(P->ctx->stream));
    return MCG_OK;
}

int mcg_paths_info(const mcg_paths* P, int64_t* n_paths, int* n_steps, int64_t* ld, void** device_ptr) {
    if (!P) return fail(MCG_ERR_INVALID, "paths is NULL");
    if (n_paths) *n_paths = P->n_paths;
    if (n_steps) *n_steps = P->n_steps;
    if (ld) *ld = P->ld;
    if (device_ptr) *device_ptr = P->data;
    return MCG_OK;
}

int mcg_paths_free(mcg_paths* P) {
    if (!P) return MCG_OK;
    if (mcg_ctx* ctx = P->ctx) {  // NULL: the ctx was finalized first and took the device memory with it
        if (P->data) pool_release(ctx, P->data, P->bytes);
        for (size_t i = ctx->live_paths.size(); i-- > 0;) {  // usually the most recent handle
            if (ctx->live_paths[i] == P) {
                ctx->live_paths[i] = ctx->live_paths.back();
                ctx->live_paths.pop_back();
                break;
            }
        }
    }
    delete P;
    return MCG_OK;
}

// ---- pricing -----------------------------------------------------------------------------------
int mcg_price_european(mcg_ctx* ctx, const mcg_paths* P, double K, double r, double T, int is_call, double* mean,
                       double* std_err) {
    if (!ctx || !P || !mean) return fail(MCG_ERR_INVALID, "ctx/paths/mean is NULL");
    if (P->ctx != ctx) return fail(MCG_ERR_INVALID, "paths belong to a different ctx");
    MCG_HIP(hipSetDevice(ctx->device));
    double s[3];
    if (P->has_sums && P->sums_K == K && (P->sums_is_call != 0) == (is_call != 0)) {
        s[0] = P->sums[0];
        s[1] = P->sums[1];
        s[2] = P->sums[2];
    } else {
        if (P->n_paths > 0) {
            int rc = launch_payoff_sums(ctx, P, K, is_call, s);
            if (rc) return rc;
        } else {
            // an empty shard still has to take part in the collective
            int rc = ensure_cap(ctx, &ctx->partials, &ctx->partials_cap, 2);
            if (rc) return rc;
            rc = finish_sums(ctx, 0, 0, s);
            if (rc) return rc;
        }
    }
    const double n = s[2];
    if (!(n >= 1.0)) return fail(MCG_ERR_EMPTY_PATHS, "no paths to price");
    const double disc = std::exp(-r * T);
    sums_to_mean_stderr(s[0], s[1], n, mean, std_err);
    *mean = disc * *mean;
    if (std_err) *std_err = disc * *std_err;
    return MCG_OK;
}

int mcg_price_lsm(mcg_ctx* ctx, const mcg_paths* P, double r, double K, double maturity, double dt, int is_call,
                  int poly_order, double* mean, double* std_err) {
    if (!ctx || !P || !mean) return fail(MCG_ERR_INVALID, "ctx/paths/mean is NULL");
    if (P->ctx != ctx) return fail(MCG_ERR_INVALID, "paths belong to a different ctx");
    if (poly_order < 0 || poly_order > 15) return fail(MCG_ERR_INVALID, "poly_order must be in [0,15] (got %d)", poly_order);
    if (P->n_paths < 1 && !ctx->allreduce) return fail(MCG_ERR_EMPTY_PATHS, "LSM::PredictOptionPrice: Empty pricePaths.");
    MCG_HIP(hipSetDevice(ctx->device));
    return run_lsm(ctx, P, r, K, maturity, dt, is_call, poly_order, mean, std_err);
}

int mcg_price_lsm2(mcg_ctx* ctx, const mcg_paths* P, const mcg_paths* F, double r, double K, double maturity, double dt,
                   int is_call, int poly_order, double* mean, double* std_err, int64_t* n_dropped) {
    if (!ctx || !P || !F || !mean) return fail(MCG_ERR_INVALID, "ctx/paths/state/mean is NULL");
    if (P->ctx != ctx) return fail(MCG_ERR_INVALID, "paths belong to a different ctx");
    if (F->ctx != ctx) return fail(MCG_ERR_INVALID, "state belongs to a different ctx");
    if (F->n_paths != P->n_paths || F->n_steps != P->n_steps)
        return fail(MCG_ERR_INVALID, "state must have the shape of paths: %lld paths x %d steps (got %lld x %d)", (long long)P->n_paths,
                    P->n_steps, (long long)F->n_paths, F->n_steps);
    if (poly_order < 0 || poly_order > 3) return fail(MCG_ERR_INVALID, "poly_order must be in [0,3] for two regressors (got %d)", poly_order);
    if (!std::isfinite(r) || !std::isfinite(K) || !std::isfinite(maturity) || !std::isfinite(dt))
        return fail(MCG_ERR_INVALID, "r, K, maturity and dt must be finite");
    if (!(K > 0.0)) return fail(MCG_ERR_INVALID, "K must be > 0 (got %g)", K);
    if (!(dt > 0.0)) return fail(MCG_ERR_INVALID, "dt must be > 0 (got %g)", dt);
    if (ctx->allreduce || ctx->rccl_comm || ctx->shm)
        return fail(MCG_ERR_INVALID, "sharded two-regressor LSM is not supported: this ctx holds a collective");
    if (P->n_paths < 1) return fail(MCG_ERR_EMPTY_PATHS, "LSM::PredictOptionPrice: Empty pricePaths.");
    MCG_HIP(hipSetDevice(ctx->device));
    return run_lsm2(ctx, P, F, r, K, maturity, dt, is_call, poly_order, mean, std_err, n_dropped);
}

// ---- LSM exercise policies ---------------------------------------------------------------------
int mcg_lsm_fit(mcg_ctx* ctx, const mcg_paths* P, double r, double K, double maturity, double dt, int is_call, int poly_order,
                double* mean, double* std_err, mcg_lsm_policy_hdr* hdr_out, double* coef_out) {
    if (!ctx || !P || !mean || !hdr_out || !coef_out) return fail(MCG_ERR_INVALID, "ctx/paths/mean/hdr_out/coef_out is NULL");
    if (P->ctx != ctx) return fail(MCG_ERR_INVALID, "paths belong to a different ctx");
    int rc = lsm_policy_check_header(P->n_steps, poly_order, r, K, maturity, dt);
    if (rc) return rc;
    if (ctx->allreduce || ctx->rccl_comm || ctx->shm)
        return fail(MCG_ERR_INVALID, "sharded policy fits are not supported: this ctx holds a collective");
    if (P->n_paths < 1) return fail(MCG_ERR_EMPTY_PATHS, "LSM::PredictOptionPrice: Empty pricePaths.");
    MCG_HIP(hipSetDevice(ctx->device));
    rc = run_lsm_fit(ctx, P, r, K, maturity, dt, is_call, poly_order, mean, std_err, coef_out);
    if (rc) return rc;
    hdr_out->n_steps = P->n_steps;
    hdr_out->poly_order = poly_order;
    hdr_out->is_call = is_call != 0 ? 1 : 0;
    hdr_out->reserved = 0;
    hdr_out->r = r;
    hdr_out->K = K;
    hdr_out->maturity = maturity;
    hdr_out->dt = dt;
    lsm_policy_from_blocks(hdr_out, coef_out);
    return MCG_OK;
}

int mcg_lsm_apply(mcg_ctx* ctx, const mcg_lsm_policy_hdr* hdr, const double* coef, const mcg_paths* P, double* mean,
                  double* std_err, double* sums3, int64_t* tau_hist) {
    if (!ctx || !P || !hdr || !coef || !mean) return fail(MCG_ERR_INVALID, "ctx/paths/hdr/coef/mean is NULL");
    if (P->ctx != ctx) return fail(MCG_ERR_INVALID, "paths belong to a different ctx");
    if (hdr->n_steps != P->n_steps)
        return fail(MCG_ERR_INVALID, "the policy has %d steps, the matrix %d", hdr->n_steps, P->n_steps);
    int rc = lsm_policy_check(hdr, coef);
    if (rc) return rc;
    if (ctx->allreduce || ctx->rccl_comm || ctx->shm)
        return fail(MCG_ERR_INVALID, "this ctx holds a collective: apply the policy per shard and add the shards' sums3 and tau_hist");
    if (P->n_paths < 1) return fail(MCG_ERR_EMPTY_PATHS, "no paths to price");
    MCG_HIP(hipSetDevice(ctx->device));
    double s[3];
    rc = run_lsm_apply(ctx, hdr, coef, P, s, tau_hist);
    if (rc) return rc;
    if (sums3)
        for (int q = 0; q < 3; ++q) sums3[q] = s[q];
    sums_to_mean_stderr(s[0], s[1], s[2], mean, std_err);
    return MCG_OK;
}

// ---- Greeks ----------------------------------------------------------------------------------
static int greeks_args(mcg_ctx* ctx, const mcg_paths* P, mcg_greeks* out) {
    if (!ctx || !P || !out) return fail(MCG_ERR_INVALID, "ctx/paths/out is NULL");
    if (P->ctx != ctx) return fail(MCG_ERR_INVALID, "paths belong to a different ctx");
    if (ctx->allreduce || ctx->rccl_comm || ctx->shm)
        return fail(MCG_ERR_INVALID, "sharded Greeks are not supported yet: this ctx holds a collective");
    return MCG_OK;
}

int mcg_greeks_european(mcg_ctx* ctx, const mcg_paths* P, double K, double r, double T, int is_call, double sigma,
                        mcg_greeks* out) {
    int rc = greeks_args(ctx, P, out);
    if (rc) return rc;
    if (P->n_paths < 1) return fail(MCG_ERR_EMPTY_PATHS, "no paths to price");
    MCG_HIP(hipSetDevice(ctx->device));
    return run_greeks_european(ctx, P, K, r, T, is_call, sigma, out);
}

int mcg_greeks_lsm(mcg_ctx* ctx, const mcg_paths* P, double r, double K, double maturity, double dt, int is_call,
                   int poly_order, mcg_greeks* out) {
    int rc = greeks_args(ctx, P, out);
    if (rc) return rc;
    if (poly_order < 0 || poly_order > 8) return fail(MCG_ERR_INVALID, "poly_order must be in [0,8] for Greeks (got %d)", poly_order);
    if (P->n_paths < 1) return fail(MCG_ERR_EMPTY_PATHS, "LSM::PredictOptionPrice: Empty pricePaths.");
    MCG_HIP(hipSetDevice(ctx->device));
    return run_lsm_greeks(ctx, P, r, K, maturity, dt, is_call, poly_order, out);
}

// ---- path-dependent European payoffs ---------------------------------------------------------
} // extern "C"
namespace mcg {
int exotic_args(mcg_ctx* ctx, const mcg_paths* P, int first_row) {
    if (!ctx || !P) return fail(MCG_ERR_INVALID, "ctx/paths is NULL");
    if (P->ctx != ctx) return fail(MCG_ERR_INVALID, "paths belong to a different ctx");
    if (first_row < 0 || first_row > P->n_steps)
        return fail(MCG_ERR_INVALID, "first_row must be in [0, n_steps = %d] (got %d)", P->n_steps, first_row);
    return MCG_OK;
}

int exotic_contract_check(const mcg_exotic& x, const char* what, int c) {
    if (x.kind < MCG_X_ASIAN_ARITH_FIXED || x.kind > MCG_X_BARRIER_DOWN_IN)
        return fail(MCG_ERR_INVALID, "%s %d: kind must be in [0, 9] (got %d)", what, c, x.kind);
    const bool barrier = x.kind >= MCG_X_BARRIER_UP_OUT;
    const bool strike = barrier || x.kind == MCG_X_ASIAN_ARITH_FIXED || x.kind == MCG_X_ASIAN_GEO_FIXED || x.kind == MCG_X_LOOKBACK_FIXED;
    if (strike && !std::isfinite(x.K)) return fail(MCG_ERR_INVALID, "%s %d: K must be finite", what, c);
    if (barrier && !std::isfinite(x.barrier)) return fail(MCG_ERR_INVALID, "%s %d: barrier must be finite", what, c);
    if (barrier && !std::isfinite(x.rebate)) return fail(MCG_ERR_INVALID, "%s %d: rebate must be finite", what, c);
    return MCG_OK;
}
}  // namespace mcg
extern "C" {

int mcg_path_stats(mcg_ctx* ctx, const mcg_paths* P, int first_row, double* host_out5) {
    int rc = exotic_args(ctx, P, first_row);
    if (rc) return rc;
    if (!host_out5) return fail(MCG_ERR_INVALID, "host_out5 is NULL");
    if (P->n_paths < 1) return fail(MCG_ERR_EMPTY_PATHS, "no paths to take statistics of");
    MCG_HIP(hipSetDevice(ctx->device));
    return run_path_stats(ctx, P, first_row, host_out5);
}

int mcg_price_exotics(mcg_ctx* ctx, const mcg_paths* P, double r, double T, int first_row, const mcg_exotic* book, int n_contracts,
                      double* price, double* std_err, double* sums) {
    int rc = exotic_args(ctx, P, first_row);
    if (rc) return rc;
    if (!book || !price) return fail(MCG_ERR_INVALID, "book/price is NULL");
    if (n_contracts < 1 || n_contracts > 1024) return fail(MCG_ERR_INVALID, "n_contracts must be in [1, 1024] (got %d)", n_contracts);
    for (int c = 0; c < n_contracts; ++c) {
        rc = exotic_contract_check(book[c], "contract", c);
        if (rc) return rc;
    }
    if (P->n_paths < 1 && !ctx->allreduce) return fail(MCG_ERR_EMPTY_PATHS, "no paths to price");
    MCG_HIP(hipSetDevice(ctx->device));
    return run_exotics(ctx, P, r, T, first_row, book, n_contracts, price, std_err, sums);
}

int mcg_path_tangent_stats(mcg_ctx* ctx, const mcg_paths* P, int first_row, int with_logs, double* host_out10) {
    int rc = exotic_args(ctx, P, first_row);
    if (rc) return rc;
    if (!host_out10) return fail(MCG_ERR_INVALID, "host_out10 is NULL");
    if (P->n_paths < 1) return fail(MCG_ERR_EMPTY_PATHS, "no paths to take statistics of");
    MCG_HIP(hipSetDevice(ctx->device));
    return run_path_tangent_stats(ctx, P, first_row, with_logs != 0, host_out10);
}

int mcg_greeks_exotics(mcg_ctx* ctx, const mcg_paths* P, double r, double q, double sigma, double T, int first_row,
                       const mcg_exotic* book, int n_contracts, mcg_greeks* out) {
    int rc = exotic_args(ctx, P, first_row);
    if (rc) return rc;
    if (!book || !out) return fail(MCG_ERR_INVALID, "book/out is NULL");
    if (ctx->allreduce || ctx->rccl_comm || ctx->shm)
        return fail(MCG_ERR_INVALID, "sharded Greeks are not supported yet: this ctx holds a collective");
    if (n_contracts < 1 || n_contracts > 1024) return fail(MCG_ERR_INVALID, "n_contracts must be in [1, 1024] (got %d)", n_contracts);
    for (int c = 0; c < n_contracts; ++c) {
        rc = exotic_contract_check(book[c], "contract", c);
        if (rc) return rc;
    }
    if (!std::isfinite(r) || !std::isfinite(q) || !std::isfinite(sigma) || !std::isfinite(T))
        return fail(MCG_ERR_INVALID, "r, q, sigma and T must be finite");
    if (!(T > 0.0)) return fail(MCG_ERR_INVALID, "T must be positive (got %g)", T);
    if (P->n_paths < 1) return fail(MCG_ERR_EMPTY_PATHS, "no paths to price");
    if (P->n_steps < 1) return fail(MCG_ERR_INVALID, "the matrix must hold at least one step (row 1 carries the first step's normal)");
    MCG_HIP(hipSetDevice(ctx->device));
    return run_greeks_exotics(ctx, P, r, q, sigma, T, first_row, book, n_contracts, out);
}

// ---- continuous barriers: Brownian-bridge survival probabilities ------------------------------
} // extern "C"
namespace mcg {
// what both bridge entry points reject of (paths, var, sigma, dt) beyond exotic_args
static int bridge_args(mcg_ctx* ctx, const mcg_paths* P, const mcg_paths* V, double sigma, double dt) {
    if (P->n_steps < 1) return fail(MCG_ERR_INVALID, "the matrix must hold at least one step (n_steps = %d)", P->n_steps);
    if (V) {
        if (V->ctx != ctx) return fail(MCG_ERR_INVALID, "var belongs to a different ctx");
        if (V->n_paths != P->n_paths || V->n_steps != P->n_steps)
            return fail(MCG_ERR_INVALID, "var must have the shape of paths (%lld x %d; got %lld x %d)", (long long)P->n_paths, P->n_steps,
                        (long long)V->n_paths, V->n_steps);
    }
    return bridge_check_variance(V != nullptr, sigma, dt);
}
}  // namespace mcg
extern "C" {

int mcg_barrier_survival(mcg_ctx* ctx, const mcg_paths* P, const mcg_paths* var, double sigma, double dt, int first_row,
                         const double* barriers, const int* is_up, int n_levels, double* host_out) {
    int rc = exotic_args(ctx, P, first_row);
    if (rc) return rc;
    if (n_levels < 1 || n_levels > 1024) return fail(MCG_ERR_INVALID, "n_levels must be in [1, 1024] (got %d)", n_levels);
    if (!barriers || !is_up || !host_out) return fail(MCG_ERR_INVALID, "barriers/is_up/host_out is NULL");
    for (int l = 0; l < n_levels; ++l) {
        rc = bridge_check_level(barriers[l], "level", l);
        if (rc) return rc;
    }
    rc = bridge_args(ctx, P, var, sigma, dt);
    if (rc) return rc;
    if (P->n_paths < 1) return fail(MCG_ERR_EMPTY_PATHS, "no paths to take survival probabilities of");
    MCG_HIP(hipSetDevice(ctx->device));
    return run_barrier_survival(ctx, P, var, sigma, dt, first_row, barriers, is_up, n_levels, host_out);
}

int mcg_price_barriers_bridge(mcg_ctx* ctx, const mcg_paths* P, const mcg_paths* var, double sigma, double r, double T, int first_row,
                              const mcg_exotic* book, int n_contracts, double* price, double* std_err, double* sums) {
    int rc = exotic_args(ctx, P, first_row);
    if (rc) return rc;
    if (!book || !price) return fail(MCG_ERR_INVALID, "book/price is NULL");
    if (n_contracts < 1 || n_contracts > 1024) return fail(MCG_ERR_INVALID, "n_contracts must be in [1, 1024] (got %d)", n_contracts);
    for (int c = 0; c < n_contracts; ++c) {
        rc = bridge_check_kind(book[c], c);
        if (!rc) rc = exotic_contract_check(book[c], "contract", c);
        if (!rc) rc = bridge_check_level(book[c].barrier, "contract", c);
        if (rc) return rc;
    }
    if (!std::isfinite(r) || !std::isfinite(T)) return fail(MCG_ERR_INVALID, "r and T must be finite");
    if (!(T > 0.0)) return fail(MCG_ERR_INVALID, "T must be positive (got %g)", T);
    rc = bridge_args(ctx, P, var, sigma, P->n_steps >= 1 ? T / (double)P->n_steps : 1.0);
    if (rc) return rc;
    if (P->n_paths < 1 && !ctx->allreduce) return fail(MCG_ERR_EMPTY_PATHS, "no paths to price");
    MCG_HIP(hipSetDevice(ctx->device));
    return run_barriers_bridge(ctx, P, var, sigma, r, T, first_row, book, n_contracts, price, std_err, sums);
}

// ---- notes on an observation schedule: autocallables and cliquets -----------------------------
} // extern "C"
namespace mcg {
// what both schedule entry points reject of (ctx, paths, r, dt, the schedule, the book)
static int sched_args(mcg_ctx* ctx, const mcg_paths* P, double r, double dt, const mcg_obs* obs, int n_obs, const mcg_sched* book,
                      int n_contracts) {
    if (!ctx || !P || !obs || !book) return fail(MCG_ERR_INVALID, "ctx/paths/obs/book is NULL");
    if (P->ctx != ctx) return fail(MCG_ERR_INVALID, "paths belong to a different ctx");
    if (n_contracts < 1 || n_contracts > 1024) return fail(MCG_ERR_INVALID, "n_contracts must be in [1, 1024] (got %d)", n_contracts);
    if (n_obs < 1 || n_obs > P->n_steps + 1)
        return fail(MCG_ERR_INVALID, "n_obs must be in [1, n_steps + 1 = %d] (got %d)", P->n_steps + 1, n_obs);
    if (!std::isfinite(r)) return fail(MCG_ERR_INVALID, "r must be finite");
    if (!std::isfinite(dt) || !(dt > 0.0)) return fail(MCG_ERR_INVALID, "dt must be positive and finite (got %g)", dt);
    const int mask = MCG_OBS_COUPON | MCG_OBS_CALL | MCG_OBS_KI | MCG_OBS_RESET;
    int n_reset = 0;
    for (int k = 0; k < n_obs; ++k) {
        if (obs[k].row < 0 || obs[k].row > P->n_steps)
            return fail(MCG_ERR_INVALID, "observation %d: row must be in [0, n_steps = %d] (got %d)", k, P->n_steps, obs[k].row);
        if (k > 0 && obs[k].row <= obs[k - 1].row)
            return fail(MCG_ERR_INVALID, "observation %d: rows must be strictly increasing (%d after %d)", k, obs[k].row, obs[k - 1].row);
        if ((obs[k].flags & ~mask) != 0) return fail(MCG_ERR_INVALID, "observation %d: flags outside the mask 0x%x (got 0x%x)", k, mask, obs[k].flags);
        if ((obs[k].flags & MCG_OBS_RESET) != 0) ++n_reset;
    }
    for (int c = 0; c < n_contracts; ++c) {
        const mcg_sched& s = book[c];
        if (s.kind == MCG_S_AUTOCALL) {
            if (!(s.put_strike > 0.0)) return fail(MCG_ERR_INVALID, "contract %d: put_strike must be positive (got %g)", c, s.put_strike);
            if (!std::isfinite(s.coupon) || !std::isfinite(s.coupon_level) || !std::isfinite(s.ki_level))
                return fail(MCG_ERR_INVALID, "contract %d: coupon, coupon_level and ki_level must be finite", c);
            if (std::isnan(s.call_level)) return fail(MCG_ERR_INVALID, "contract %d: call_level is NaN", c);
        } else if (s.kind == MCG_S_CLIQUET) {
            if (n_reset < 2) return fail(MCG_ERR_INVALID, "contract %d: a cliquet needs two RESET dates in the schedule (it has %d)", c, n_reset);
            if (std::isnan(s.local_floor) || std::isnan(s.local_cap) || std::isnan(s.global_floor) || std::isnan(s.global_cap))
                return fail(MCG_ERR_INVALID, "contract %d: a cliquet bound is NaN", c);
            if (s.local_floor > s.local_cap || s.global_floor > s.global_cap)
                return fail(MCG_ERR_INVALID, "contract %d: a floor lies above its cap", c);
        } else {
            return fail(MCG_ERR_INVALID, "contract %d: kind must be in [0, 1] (got %d)", c, s.kind);
        }
    }
    return MCG_OK;
}
}  // namespace mcg
extern "C" {

int mcg_price_scheduled(mcg_ctx* ctx, const mcg_paths* P, double r, double dt, const mcg_obs* obs, int n_obs, const mcg_sched* book,
                        int n_contracts, double* price, double* std_err, double* sums, int64_t* stop_hist) {
    int rc = sched_args(ctx, P, r, dt, obs, n_obs, book, n_contracts);
    if (rc) return rc;
    if (!price) return fail(MCG_ERR_INVALID, "price is NULL");
    if (stop_hist && (ctx->allreduce || ctx->rccl_comm || ctx->shm))
        return fail(MCG_ERR_INVALID, "this ctx holds a collective: take stop_hist per shard and add the shards' counts");
    if (P->n_paths < 1 && !ctx->allreduce) return fail(MCG_ERR_EMPTY_PATHS, "no paths to price");
    MCG_HIP(hipSetDevice(ctx->device));
    return run_sched_book(ctx, P, r, dt, obs, n_obs, book, n_contracts, price, std_err, sums, stop_hist);
}

int mcg_sched_path_values(mcg_ctx* ctx, const mcg_paths* P, double r, double dt, const mcg_obs* obs, int n_obs, const mcg_sched* book,
                          int n_contracts, double* host_values, int32_t* host_stop) {
    int rc = sched_args(ctx, P, r, dt, obs, n_obs, book, n_contracts);
    if (rc) return rc;
    if (!host_values) return fail(MCG_ERR_INVALID, "host_values is NULL");
    if (P->n_paths < 1) return fail(MCG_ERR_EMPTY_PATHS, "no paths to take values of");
    MCG_HIP(hipSetDevice(ctx->device));
    return run_sched_values(ctx, P, r, dt, obs, n_obs, book, n_contracts, host_values, host_stop);
}

int mcg_lsm_one_launch_enabled(mcg_ctx* ctx, int* enabled) {
    if (!ctx || !enabled) return fail(MCG_ERR_INVALID, "ctx/enabled is NULL");
    *enabled = ctx->coop_launch ? 1 : 0;
    return MCG_OK;
}

int mcg_lsm_one_launch_reset(mcg_ctx* ctx) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    ctx->coop_launch = true;
    ctx->coop_retry_in = 0;
    return MCG_OK;
}

int mcg_debug_lsm_hooks(mcg_ctx* ctx, long long spin_limit, int poll_delay) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    if (spin_limit > 0xffffffffLL || poll_delay < 0 || poll_delay > 1000) return fail(MCG_ERR_INVALID, "bad hook values");
    ctx->lsm_spin_limit = spin_limit;
    ctx->lsm_poll_delay = poll_delay;
    return MCG_OK;
}

int mcg_price_asymptotic(mcg_ctx* ctx, const mcg_paths* P, double r, double K, double maturity, double dt, int is_call,
                         double sigma, double dividend, double* price) {
    if (!ctx || !P || !price) return fail(MCG_ERR_INVALID, "ctx/paths/price is NULL");
    if (P->ctx != ctx) return fail(MCG_ERR_INVALID, "paths belong to a different ctx");
    *price = 0.0;
    if (P->n_paths < 1 && !ctx->allreduce) return MCG_OK;  // AsymptoticAnalysisPricer.cpp:47-49
    if (sigma <= 0.0) return fail(MCG_ERR_INVALID, "AsymptoticAnalysis: Volatility must be positive.");  // :50-52
    MCG_HIP(hipSetDevice(ctx->device));
    return run_asymptotic(ctx, P, r, K, maturity, dt, is_call, sigma, dividend, price);
}

int mcg_price_martingale(mcg_ctx* ctx, const mcg_paths* P, double r, double K, double maturity, double dt, int is_call,
                         int poly_order, int max_iterations, double* price, double* lower, double* upper) {
    if (!ctx || !P || !price) return fail(MCG_ERR_INVALID, "ctx/paths/price is NULL");
    if (P->ctx != ctx) return fail(MCG_ERR_INVALID, "paths belong to a different ctx");
    if (P->n_paths < 1 && !ctx->allreduce) return fail(MCG_ERR_EMPTY_PATHS, "MartingaleOptimization: Empty pricePaths.");
    if (max_iterations <= 0) return fail(MCG_ERR_INVALID, "MartingaleOptimization: maxIterations must be positive.");
    if (poly_order < 0 || poly_order > 15) return fail(MCG_ERR_INVALID, "poly_order must be in [0,15] (got %d)", poly_order);
    MCG_HIP(hipSetDevice(ctx->device));
    return run_martingale(ctx, P, r, K, maturity, dt, is_call, poly_order, max_iterations, price, lower, upper);
}

int mcg_price_branching(mcg_ctx* ctx, const mcg_paths* P, double r, double K, double maturity, double dt, int is_call,
                        int num_branches, const int* exercise_times, int n_ex, uint64_t seed, double* price, double* lower,
                        double* upper) {
    if (!ctx || !P || !price) return fail(MCG_ERR_INVALID, "ctx/paths/price is NULL");
    if (P->ctx != ctx) return fail(MCG_ERR_INVALID, "paths belong to a different ctx");
    if (P->n_paths < 1 && !ctx->allreduce) return fail(MCG_ERR_EMPTY_PATHS, "BranchingProcesses: Empty pricePaths.");  // :22-24
    if (!exercise_times || n_ex < 1) return fail(MCG_ERR_INVALID, "BranchingProcesses: No exercise times.");              // :25-27
    if (K <= 0.0) return fail(MCG_ERR_INVALID, "BranchingProcesses: Strike must be positive.");                           // :28-30
    MCG_HIP(hipSetDevice(ctx->device));
    return run_branching(ctx, P, r, K, maturity, dt, is_call, num_branches, exercise_times, n_ex, seed, price, lower, upper);
}

// What mcg_batch_price_rows and mcg_batch_price_rows6 reject -- all of it BEFORE anything is allocated; out_name: "out" or "out6"
static int batch_args(mcg_ctx* ctx, const mcg_row* rows, int64_t n_rows, int n_paths, double dt, int poly_order, int max_iterations,
                      const double* out, const char* out_name) {
    if (!ctx || !out) return fail(MCG_ERR_INVALID, "ctx/%s is NULL", out_name);
    if (n_rows < 0 || (n_rows > 0 && !rows)) return fail(MCG_ERR_INVALID, "bad rows");
    // (the row kernels serve up to 256 paths per row and orders up to 4 -- the driver uses 250 and 2; anything beyond is
    // priced row by row through the single-contract entry points, run_batch_rows)
    if (n_paths < 1) return fail(MCG_ERR_INVALID, "n_paths must be >= 1 (got %d)", n_paths);
    if (poly_order < 0 || poly_order > 15) return fail(MCG_ERR_INVALID, "poly_order must be in [0,15] (got %d)", poly_order);
    if (max_iterations <= 0) return fail(MCG_ERR_INVALID, "MartingaleOptimization: maxIterations must be positive.");
    if (!(dt > 0.0)) return fail(MCG_ERR_INVALID, "dt must be > 0");
    if (n_rows > (int64_t)1 << 31) return fail(MCG_ERR_INVALID, "too many rows for one call (row ids are 32 bits of the Philox counter)");
    return MCG_OK;
}

int mcg_batch_price_rows(mcg_ctx* ctx, const mcg_row* rows, int64_t n_rows, int n_paths, double r, double dt,
                         int num_branches, int poly_order, int max_iterations, uint64_t seed, double* out) {
    const int bad = batch_args(ctx, rows, n_rows, n_paths, dt, poly_order, max_iterations, out, "out");
    if (bad || n_rows == 0) return bad;
    MCG_HIP(hipSetDevice(ctx->device));
    try {  // (the planner's host vectors: nothing may leave an extern "C" entry point as an exception)
        return run_batch_rows(ctx, rows, n_rows, n_paths, r, dt, num_branches, poly_order, max_iterations, seed, out, nullptr);
    } catch (const std::exception& e) {
        return fail(MCG_ERR_OOM, "mcg_batch_price_rows: %s", e.what());
    }
}

int mcg_batch_price_rows6(mcg_ctx* ctx, const mcg_row* rows, const double* features2, int64_t n_rows, int n_paths, double r,
                          double dt, int num_branches, int poly_order, int max_iterations, uint64_t seed, double* out6) {
    const int bad = batch_args(ctx, rows, n_rows, n_paths, dt, poly_order, max_iterations, out6, "out6");
    if (bad || n_rows == 0) return bad;
    std::vector<double> four;
    std::vector<unsigned char> priced;
    try {  // nothing may leave an extern "C" entry point as an exception
        four.resize((size_t)n_rows * 4);
        priced.resize((size_t)n_rows);
    } catch (const std::exception&) {
        return fail(MCG_ERR_OOM, "mcg_batch_price_rows6: no host memory for %lld rows", (long long)n_rows);
    }
    MCG_HIP(hipSetDevice(ctx->device));
    int rc;
    try {
        rc = run_batch_rows(ctx, rows, n_rows, n_paths, r, dt, num_branches, poly_order, max_iterations, seed, four.data(), priced.data());
    } catch (const std::exception& e) {
        return fail(MCG_ERR_OOM, "mcg_batch_price_rows6: %s", e.what());
    }
    if (rc) return rc;
    for (int64_t i = 0; i < n_rows; ++i) {
        const double* p = &four[(size_t)i * 4];
        double* o = out6 + 6 * i;
        // PredictionGen.cpp:739-805: a row the driver skips, or whose paths hold an inf / nan (the row kernels' scan of the row's
        // block, run_batch_chunk), is written as ",0,0,0,0,0,0" -- features included; every other row carries what its
        // pricers returned, finite or not, as the driver prints it (:809-816)
        const bool ok = priced[(size_t)i] != 0;
        for (int c = 0; c < 4; ++c) o[c] = ok ? p[c] : 0.0;
        o[4] = ok && features2 ? features2[2 * i] : 0.0;
        o[5] = ok && features2 ? features2[2 * i + 1] : 0.0;
    }
    return MCG_OK;
}

int mcg_row_features(const double* hist, size_t n, double* twenty_day_vol, double* twenty_day_momentum) {
    if (!twenty_day_vol || !twenty_day_momentum || (n > 0 && !hist)) return fail(MCG_ERR_INVALID, "bad arguments");
    host_row_features(hist, n, twenty_day_vol, twenty_day_momentum);
    return MCG_OK;
}

int mcg_row_build(const double* hist, size_t n, double underlying_last, double dte, double strike_dist_pct, int option_type,
                  double dividend, mcg_row* row, double features2[2]) {
    if (!row || !features2 || (n > 0 && !hist)) return fail(MCG_ERR_INVALID, "bad arguments");
    return host_row_build(hist, n, underlying_last, dte, strike_dist_pct, option_type, dividend, row, features2);
}

int mcg_probe_write_ceiling(mcg_ctx* ctx, int64_t n_paths, int n_steps, int reps, double* gb_per_s, double* ms_per_launch) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    if (n_paths < 512 || n_steps < 1 || reps < 1 || reps > 1000) return fail(MCG_ERR_INVALID, "bad probe shape");
    MCG_HIP(hipSetDevice(ctx->device));
    return probe_write_ceiling(ctx, n_paths, n_steps, reps, gb_per_s, ms_per_launch);
}

int mcg_generator_clock_arm(mcg_ctx* ctx, int on) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    ctx->clk_armed = on != 0;
    return MCG_OK;
}

int mcg_generator_clock(mcg_ctx* ctx, double* ghz_median, int* n_stamps, double* ghz_min, double* ghz_max) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    MCG_HIP(hipSetDevice(ctx->device));
    return generator_clock(ctx, ghz_median, n_stamps, ghz_min, ghz_max);
}

int mcg_stats(mcg_stats_t* out, int reset) {
    if (!out && !reset) return fail(MCG_ERR_INVALID, "out is NULL");
    std::atomic<int64_t>* src[] = {&g_stats.lsm_one_launch_sweeps, &g_stats.lsm_one_launch_timeouts, &g_stats.lsm_per_date_sweeps,
                                   &g_stats.lsm_per_date_launches, &g_stats.lsm_per_date_refits, &g_stats.lsm_per_date_faults,
                                   &g_stats.shm_barrier_failures, &g_stats.peer_mailbox_enabled, &g_stats.peer_mailbox_refused,
                                   &g_stats.batch_calls, &g_stats.batch_chunks, &g_stats.batch_rows, &g_stats.batch_rows_singly,
                                   &g_stats.batch_peak_workspace_bytes, &g_stats.peer_mailbox_kept,
                                   &g_stats.coalesced_rounds, &g_stats.coalesced_calls, &g_stats.coalesced_peak_calls_per_round,
                                   &g_stats.coalesced_fallbacks, &g_stats.coalesced_round_us, &g_stats.coalesced_device_wait_us,
                                   &g_stats.coalesced_wake_us, &g_stats.coalesced_prefetched, &g_stats.coalesced_prefetch_hits};
    static_assert(sizeof(mcg_stats_t) == sizeof(src) / sizeof(src[0]) * sizeof(int64_t), "mcg_stats_t lists the counters in this order");
    int64_t* dst = reinterpret_cast<int64_t*>(out);
    for (size_t k = 0; k < sizeof(src) / sizeof(src[0]); ++k) {
        const int64_t v = reset ? src[k]->exchange(0, std::memory_order_relaxed) : src[k]->load(std::memory_order_relaxed);
        if (out) dst[k] = v;
    }
    return MCG_OK;
}

int mcg_debug_lsm_date_fault(mcg_ctx* ctx, int mode, int date, int workgroup, int delay, long long spin_limit) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    if (mode < 0 || mode > 2 || delay < 0 || delay > 100000 || spin_limit > 0xffffffffLL) return fail(MCG_ERR_INVALID, "bad hook values");
    ctx->lsm_date_hook[0] = mode;
    ctx->lsm_date_hook[1] = date;
    ctx->lsm_date_hook[2] = workgroup;
    ctx->lsm_date_hook[3] = delay;
    ctx->lsm_date_spin_limit = spin_limit;
    return MCG_OK;
}

int mcg_debug_gbm_route(mcg_ctx* ctx, int route, int* last_route) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    if (route < -1 || route > 2) return fail(MCG_ERR_INVALID, "route must be 0 (auto), 1 (narrow), 2 (wide) or -1 (unchanged)");
    if (route >= 0) ctx->gbm_route = route;
    if (last_route) *last_route = ctx->gbm_last_route;
    return MCG_OK;
}

int mcg_debug_branch_route(mcg_ctx* ctx, int route, int slice_shift, int* last_route) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    if (route < -1 || route > 4) return fail(MCG_ERR_INVALID, "route must be 0 (auto), 1 (one launch), 2 (per date), 3 (binned), 4 (XCD) or -1 (unchanged)");
    if (route >= 0 && (slice_shift < 0 || slice_shift > 30)) return fail(MCG_ERR_INVALID, "slice_shift must be in [0,30] (got %d)", slice_shift);
    if (route >= 0) {
        ctx->branch_route = route;
        ctx->branch_shift = slice_shift;
    }
    if (last_route) *last_route = ctx->branch_last_route;
    return MCG_OK;
}

int mcg_debug_batch_budget(mcg_ctx* ctx, size_t bytes) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    ctx->batch_budget = bytes;
    return MCG_OK;
}

int mcg_debug_batch_row_dump(mcg_ctx* ctx, const mcg_row* rows, int64_t n_rows, int n_paths, double r, double dt, int num_branches,
                             int poly_order, int max_iterations, uint64_t seed, double* out, int64_t row, double* amp, double* comp,
                             double* block) {
    const int bad = batch_args(ctx, rows, n_rows, n_paths, dt, poly_order, max_iterations, out, "out");
    if (bad) return bad;
    if (!amp || !comp || !block) return fail(MCG_ERR_INVALID, "amp/comp/block is NULL");
    if (row < 0 || row >= n_rows) return fail(MCG_ERR_INVALID, "row %lld is not one of the call's %lld rows", (long long)row, (long long)n_rows);
    if (!batch_row_valid(rows[row])) return fail(MCG_ERR_INVALID, "row %lld is invalid (the call answers it with zeros): nothing to dump", (long long)row);
    if (batch_row_singly(rows[row], n_paths, poly_order))
        return fail(MCG_ERR_INVALID, "row %lld is priced singly (more than 1020 steps, more than 256 paths or an order above 4): the row kernels hold nothing of it",
                    (long long)row);
    MCG_HIP(hipSetDevice(ctx->device));
    BatchDump dump{row, amp, comp, block, false};
    struct Unset {   // the context forgets the dump on every way out
        mcg_ctx* c;
        ~Unset() { c->batch_dump = nullptr; }
    } unset{ctx};
    ctx->batch_dump = &dump;
    int rc;
    try {
        rc = run_batch_rows(ctx, rows, n_rows, n_paths, r, dt, num_branches, poly_order, max_iterations, seed, out, nullptr);
    } catch (const std::exception& e) {
        return fail(MCG_ERR_OOM, "mcg_debug_batch_row_dump: %s", e.what());
    }
    if (rc == MCG_OK && !dump.found) return fail(MCG_ERR_INVALID, "row %lld was in no chunk of the call", (long long)row);
    return rc;
}

// ---- host-only pieces --------------------------------------------------------------------------
int mcg_estimate_params(const double* hist, size_t n, double out5[5]) {
    if (!out5) return fail(MCG_ERR_INVALID, "out5 is NULL");
    return host_estimate_params(hist, n, out5);
}

int mcg_rbergomi_spectrum(double H, double eta, double dt, int n_steps, double* amp, double* comp, int* Mz) {
    if (n_steps < 1 || !amp || !comp) return fail(MCG_ERR_INVALID, "bad arguments");
    std::vector<double> k, c;
    int rc = host_rbergomi_spectrum(H, eta, dt, n_steps, k, c);
    if (rc) return rc;
    std::memcpy(amp, k.data(), k.size() * sizeof(double));
    std::memcpy(comp, c.data(), c.size() * sizeof(double));
    if (Mz) *Mz = (int)k.size();
    return MCG_OK;
}

// ---- timing ------------------------------------------------------------------------------------
int mcg_timing_enable(mcg_ctx* ctx, int on) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    ctx->timing = on != 0;
    return MCG_OK;
}

int mcg_timing_select(mcg_ctx* ctx, unsigned mask) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    ctx->timing_mask = mask;
    return MCG_OK;
}

int mcg_timing_reset(mcg_ctx* ctx) {
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    int rc = timing_collect(ctx);
    for (int i = 0; i < MCG_K_COUNT; ++i) {
        ctx->t_total[i] = 0.0;
        ctx->t_count[i] = 0;
    }
    return rc;
}

int mcg_timing_get(mcg_ctx* ctx, int kernel, double* total_ms, int64_t* launches) {
    if (!ctx || kernel < 0 || kernel >= MCG_K_COUNT) return fail(MCG_ERR_INVALID, "bad ctx/kernel id");
    int rc = timing_collect(ctx);
    if (rc) return rc;
    if (total_ms) *total_ms = ctx->t_total[kernel];
    if (launches) *launches = ctx->t_count[kernel];
    return MCG_OK;
}

}  // extern "C"
