// Internal definitions behind include/mcgpu.h: context, device-buffer pool, error plumbing,
// per-kernel HIP-event timing.  Not installed; not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mcgpu.h"
#include "../../include/mcgpu_debug.h"

namespace mcg {

void set_error(const char* fmt, ...);
int fail(int status, const char* fmt, ...);

// Timing-study switches (another grid size, another variant): read from the environment in A/B builds only
// (tools/build_variant.sh ... -DMCG_STUDY_SWITCHES); the product library reads no such variable.
inline int study_switch(const char* name, int fallback) {
#ifdef MCG_STUDY_SWITCHES
    if (const char* e = std::getenv(name)) return std::atoi(e);
#else
    (void)name;
#endif
    return fallback;
}

// Process-wide event counters behind mcg_stats (relaxed atomics: any thread, any ctx).
struct Stats {
    std::atomic<int64_t> lsm_one_launch_sweeps{0}, lsm_one_launch_timeouts{0}, lsm_per_date_sweeps{0}, lsm_per_date_launches{0},
        lsm_per_date_refits{0}, lsm_per_date_faults{0}, shm_barrier_failures{0}, peer_mailbox_enabled{0}, peer_mailbox_refused{0},
        batch_calls{0}, batch_chunks{0}, batch_rows{0}, batch_rows_singly{0}, batch_peak_workspace_bytes{0}, peer_mailbox_kept{0},
        coalesced_rounds{0}, coalesced_calls{0}, coalesced_peak_calls_per_round{0}, coalesced_fallbacks{0},
        coalesced_round_us{0}, coalesced_device_wait_us{0}, coalesced_wake_us{0}, coalesced_prefetched{0}, coalesced_prefetch_hits{0};
};
extern Stats g_stats;

#define MCG_HIP(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return ::mcg::fail(_e == hipErrorOutOfMemory ? MCG_ERR_OOM : MCG_ERR_HIP,          \
                               "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                               __LINE__);                                                      \
    } while (0)

struct PoolBuf {
    void* ptr;
    size_t bytes;
};

struct EventPair {
    hipEvent_t a, b;
    int64_t launches;  // kernel launches the pair brackets (1, or a whole queued sequence: TimedLaunch)
};

struct BatchDump {  // mcg_debug_batch_row_dump: where the chunk that holds `row` copies that row's device data (run_batch_chunk)
    int64_t row;
    double *amp, *comp, *block;
    bool found;
};

struct ShmComm;  // comm_shm.cpp: node-local collective over POSIX shared memory
constexpr int SHM_MAX_RANKS = 16;     // processes (GPUs) sharing one segment
constexpr int SHM_MAX_ROUNDS = 4096;  // exchange rounds of one LSM sweep the device mailbox holds (2 per exercise date at most)
constexpr int SHM_ROW_DOUBLES = 16;   // one rank's row of a round: up to 14 moments (orders <= 4)
constexpr int SHM_ALLREDUCE_MAX = 62; // doubles one host all-reduce of the segment carries (a rank's slot row holds 64)

}  // namespace mcg

struct mcg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    int n_cus = 256;
    bool coop_launch = false;    // the one-launch LSM sweep (k_lsm_coop / k_lsm_big) is allowed on this context
    int coop_retry_in = 0;       // after a hand-shake time-out: LSM prices left before it is allowed again (0: stays off until reset)
    long long lsm_spin_limit = -1;  // test hooks (mcg_debug_lsm_hooks): polling rounds before a spin gives up (< 0: default)
    int lsm_poll_delay = 0;         //   workgroups other than 0 reach their coefficient poll late
    long long lsm_date_spin_limit = -1;  // mcg_debug_lsm_date_fault: polls before a consumer of k_lsm_date gives a slot up (< 0: default)
    int lsm_date_hook[4] = {0, 0, 0, 0}; //   {mode, date, workgroup, delay}: that workgroup's partial moments never land (1) / land late (2)
    size_t batch_budget = 0;             // mcg_debug_batch_budget: workspace bytes of one chunk of mcg_batch_price_rows (0: a quarter of free memory)
    mcg::BatchDump* batch_dump = nullptr;  // mcg_debug_batch_row_dump: set for the length of its one call
    // batched rows (kernels_batch.hip): the two latency-bound row pricers run beside the two issue-bound ones on a second stream
    hipStream_t batch_aux = nullptr;
    hipEvent_t batch_fork = nullptr, batch_join = nullptr;

    // cached device buffers (path matrices are tens of GB: never hipMalloc per call in steady state)
    std::vector<mcg::PoolBuf> pool;
    // path-matrix handles handed out and not yet freed: mcg_finalize takes their device memory back and orphans
    // them (ctx = data = NULL), so a late mcg_paths_free only deletes the handle instead of touching a dead ctx
    std::vector<mcg_paths*> live_paths;
    // small persistent workspace
    double* partials = nullptr;  // per-block partial sums
    size_t partials_cap = 0;     // in doubles
    double* fin_chunks = nullptr;  // finish_sums: chunk sums of a long partials list
    size_t fin_chunks_cap = 0;
    double* scalars = nullptr;   // device: sums, moments, coefficients
    double* h_scalars = nullptr; // pinned host mirror
    double* weights = nullptr;   // rBergomi spectral amplitudes + compensator
    size_t weights_cap = 0;
    double* lsm_v = nullptr;     // LSM value vector
    size_t lsm_v_cap = 0;
    double* lsm_dv = nullptr;    // its K-tangent (mcg_greeks_lsm)
    size_t lsm_dv_cap = 0;
    unsigned long long* clk_stamps = nullptr;  // [GBM_CLK_SLOTS][2] {shader cycles, 100 MHz ticks} of the last GBM launch's stamping workgroups
    int clk_slots_used = 0;
    bool clk_armed = false;                    // mcg_generator_clock_arm: only armed launches stamp (and pay the memset ahead of them)
    double* log_tab = nullptr;   // device copy of fm::LOG_TAB_HOST + fm::SINCOS_TAB_HOST + fm::EXP2_TAB_HOST (34 KiB), staged to LDS
    double* sincos2_tab = nullptr;  // device copy of host_sincos2_tables(): coarse, then fine (128 KiB; fm::sincos_two_level)
    int gbm_route = 0;           // mcg_debug_gbm_route: 0 = launch_gbm chooses, 1 = k_gbm_paths, 2 = k_gbm_paths_wide
    int gbm_last_route = 0;      //   what the last GBM launch took (1 or 2; 0: none yet)
    int branch_route = 0;        // mcg_debug_branch_route: 0 = run_branching's plan chooses, 1..4 = that route where it can run
    int branch_shift = 0;        //   the slice shift the plan starts from (0: the default, 18)
    int branch_last_route = 0;   //   what the last mcg_price_branching took (1..4; 0: none yet)
    int64_t lsm_dual_executed = 0;  // mcg_debug_lsm_dual_executed: path-steps the waves of the last mcg_lsm_dual_upper ran through
    size_t lsm_dual_ws_doubles = 0;  // mcg_debug_lsm_dual_workspace: the workspace bound of one batch of mcg_lsm_dual_upper (0: default)

    // collective
    mcg_allreduce_fn allreduce = nullptr;
    void* allreduce_user = nullptr;
    void* rccl_comm = nullptr;
    mcg::ShmComm* shm = nullptr;  // mcg_comm_init_shm
    int n_ranks = 1, rank = 0;

    // timing
    bool timing = false;
    unsigned timing_mask = ~0u;  // bit k: kernel k is bracketed while timing is on (mcg_timing_select)
    std::vector<mcg::EventPair> ev_free;
    std::vector<std::pair<int, mcg::EventPair>> ev_live;
    double t_total[MCG_K_COUNT] = {0};
    int64_t t_count[MCG_K_COUNT] = {0};
};

struct mcg_paths {
    mcg_ctx* ctx = nullptr;
    double* data = nullptr;
    size_t bytes = 0;
    int64_t n_paths = 0;
    int n_steps = 0;
    int64_t ld = 0;
    uint64_t path_begin = 0;
    // made by a generator (mcg_paths_gbm* / mcg_paths_gbm_multi and combinations of generated matrices / mcg_paths_rbergomi* / the price matrix of mcg_paths_heston* / mcg_paths_heston_qe* / mcg_paths_bates*): S_T is proportional to e^{rT} (mcg_greeks_european's rho).
    // Not mcg_paths_localvol*: under sigma(t, S) S_T is homogeneous in S0 but not proportional to e^{rT}; its matrix is a plain one.
    bool generated = false;
    // fused terminal-payoff sums left by *_payoff generators
    bool has_sums = false;
    double sums_K = 0.0;
    int sums_is_call = 0;
    double sums[3] = {0, 0, 0};  // host copy {sum, sumsq, n}: all-reduced totals when the ctx has a collective
};

namespace mcg {

constexpr int SINCOS2_ENTRIES = 4096;  // entries {cos, sin} of each of the two tables of fm::sincos_two_level
constexpr int GBM_CLK_SLOTS = 64;     // stamping workgroups of a GBM generator launch (mcg_generator_clock)
constexpr int SCALARS_DOUBLES = 256;
// layout of ctx->scalars (doubles)
constexpr int SC_SUMS = 0;     // [0..3)  sum, sumsq, n
constexpr int SC_GREEKS = 4;   // [4..18) Greeks sums: {sum, sum^2} of up to six estimators, then min and max of row 0
constexpr int SC_COEF = 40;    // [40..60) the LSM coefficient block of the current date (lsm_device.hpp: LSM_C_*)
constexpr int SC_FINAL = 64;   // [64..67) LSM final sums
constexpr int SC_BARRIER = 72; // [72] 32-bit timeout flag of k_lsm_coop's hand-shake
constexpr int SC_TICKET = 80;  // [80] 64-bit share ticket of the persistent rBergomi generator (zeroed before each launch)
constexpr int SC_GBM_TICKET = 81;  // [81] 32-bit tile ticket of the wide GBM generator (k_gbm_paths_wide; zeroed before each launch)
constexpr int SC_LSM_TICKET = 160; // [160..225) 129 32-bit "workgroups done" tickets of the per-date LSM kernel (k_lsm_date)
constexpr int SC_LSM_MSG = 96;     // [96..144) per-date LSM message: the 3p+2 <= 47 moments the next launch solves (the all-reduced part)
constexpr int SC_LSM_STATE = 144;  // [144..147) per-date LSM state: date, phase, centre (kernels_lsm.hip: LSM_ST_*)

int pool_alloc(mcg_ctx* ctx, size_t bytes, void** out);
void pool_release(mcg_ctx* ctx, void* ptr, size_t bytes);
// Pool buffers of one scope: whatever alloc() handed out goes back to the pool on every way out of it.  Nothing queued may still
// use a buffer then: the holder sets `busy` while launches that use them may be pending, and the lease waits for the stream first
// (or the holder synchronises itself on its error paths, as run_batch_chunk does).
struct PoolLease {
    mcg_ctx* ctx;
    std::vector<PoolBuf> held;
    bool busy = false;
    explicit PoolLease(mcg_ctx* c) : ctx(c) {}
    PoolLease(const PoolLease&) = delete;
    PoolLease& operator=(const PoolLease&) = delete;
    int alloc(size_t bytes, void** out) {
        held.reserve(held.size() + 1);  // (a bad_alloc here leaves no buffer out)
        const int rc = pool_alloc(ctx, bytes, out);
        if (!rc) held.push_back(PoolBuf{*out, bytes});
        return rc;
    }
    ~PoolLease() {
        if (busy) (void)hipStreamSynchronize(ctx->stream);
        for (const PoolBuf& b : held) pool_release(ctx, b.ptr, b.bytes);
    }
};
int ensure_cap(mcg_ctx* ctx, double** buf, size_t* cap, size_t need_doubles);
// timing scope: records events around a launch when ctx->timing is on
struct TimedLaunch {
    mcg_ctx* ctx;
    int kernel;
    EventPair ev{};
    bool on;
    // launches > 1: ONE event pair around a queued sequence of that many launches (the per-date LSM route: an event
    // pair per launch costs 9 us of the 60 a date takes); the reported time then includes what lies between them
    TimedLaunch(mcg_ctx* c, int k, int64_t launches = 1);
    ~TimedLaunch();
};

void comm_release(mcg_ctx* ctx);  // comm_rccl.cpp
int comm_rccl_count(mcg_ctx* ctx);  // ncclCommCount of the built-in communicator (0: none / not available)
// comm_shm.cpp
void shm_release(mcg_ctx* ctx);
int shm_arm_mailbox(mcg_ctx* ctx, int rounds, uint64_t sentinel_bits);
int shm_sum_flag(mcg_ctx* ctx, int flag, int* total);
void shm_poison(mcg_ctx* ctx);  // a rank failed between two collective steps: every later barrier fails at once on every rank
double* shm_mailbox_device(mcg_ctx* ctx);        // the mailbox this rank polls (host segment, or its own HBM)
double* const* shm_mailbox_peers(mcg_ctx* ctx);  // peer-memory mode: every rank's mailbox as mapped here; else nullptr
int shm_rank(mcg_ctx* ctx);
int shm_n_ranks(mcg_ctx* ctx);
int shm_attached(mcg_ctx* ctx);
bool shm_peer_active(mcg_ctx* ctx);
int peer_ping(mcg_ctx* ctx, double* const* peers, int n, int rank);  // comm_peer.hip
int peer_arm(mcg_ctx* ctx, double* mbox, int rounds, int n, uint64_t sentinel);  // comm_peer.hip: 0 = armed and synchronised

int paths_new(mcg_ctx* ctx, int64_t n_paths, int n_steps, uint64_t path_begin, mcg_paths** out);

// generator launchers, each in the .hip file of its name; the Heston and Bates ones derive their scheme's constants and share
// heston_device.hpp's launch_heston_scheme.  All of them are written on paths_host.hpp: the grid's checks, the launch frame
// (PathLaunch), the argument struct's common members, the flag dispatch and the parameter upload are stated there.  launch_gbm
// and launch_rbergomi count their own units (tiles of the wide route, pairs per share) and pass them through launch_units.
int launch_gbm(mcg_ctx* ctx, mcg_paths* P, uint64_t seed, double S0, double r, double sigma, double dt,
               bool want_payoff, double K, int is_call);
int launch_rbergomi(mcg_ctx* ctx, mcg_paths* P, uint64_t seed, double S0, double r, double xi, double H,
                    double eta, double dt, bool want_payoff, double K, int is_call);
// V: the variance matrix (same shape as P), or null
int launch_heston(mcg_ctx* ctx, mcg_paths* P, mcg_paths* V, uint64_t seed, double S0, double r, double v0, double kappa,
                  double theta, double sigma_v, double rho, double dt, bool want_payoff, double K, int is_call);
// the same by Andersen's QE scheme (kernels_heston_qe.hip); sigma_v > 0
int launch_heston_qe(mcg_ctx* ctx, mcg_paths* P, mcg_paths* V, uint64_t seed, double S0, double r, double v0, double kappa,
                     double theta, double sigma_v, double rho, double dt, bool want_payoff, double K, int is_call);
// either scheme with compound-Poisson log-normal jumps (kernels_bates.hip); 0 <= lambda dt <= 1
int launch_bates(mcg_ctx* ctx, mcg_paths* P, mcg_paths* V, uint64_t seed, double S0, double r, double v0, double kappa,
                 double theta, double sigma_v, double rho, double lambda, double mu_j, double sigma_j, double dt, bool qe,
                 bool want_payoff, double K, int is_call);
// multi-asset GBM (kernels_gbm_multi.hip): assets (n_assets matrices) or comb may be null, not both; L: the lower Cholesky factor
// of the correlation matrix; q and weights: n_assets values each
int launch_gbm_multi(mcg_ctx* ctx, mcg_paths* const* assets, mcg_paths* comb, int n_assets, uint64_t seed, const double* S0,
                     double r, const double* q, const double* sigma, const double* L, double dt, int kind,
                     const double* weights);
int launch_paths_combine(mcg_ctx* ctx, const mcg_paths* const* assets, int n_assets, int kind, const double* weights,
                         mcg_paths* out);
// local volatility (kernels_localvol.hip): table = the n_slices * (n_x - 1) entries {a, d} of mcg_localvol_table, on the host;
// it is uploaded on the ctx's stream.  The scalars come from host/localvol.cpp.
constexpr int LOCALVOL_MAX_NT = 64, LOCALVOL_MAX_NX = 128;
struct LocalVolScalars {
    double inv_dx, u0, m;  // (n_x - 1) / (x_max - x_min);  -x_min inv_dx;  (r - q) dt
};
int launch_localvol(mcg_ctx* ctx, mcg_paths* P, uint64_t seed, double S0, const LocalVolScalars& c, int n_x, const double* table,
                    int n_slices, bool want_payoff, double K, int is_call);
// Sobol' paths (kernels_sobol.hip): GBM with gm = (r - sigma^2 / 2) dt and gs = sigma sqrt(dt) when lv is null, otherwise local
// volatility with launch_localvol's scalars and table.  host/sobol.cpp: what every entry point rejects of an mcg_sobol, and of
// the shape of a Sobol' matrix (n_steps > 1024, ids beyond 2^32; n_steps < 1 and n_paths < 0 are left to the model's own checks).
int launch_sobol(mcg_ctx* ctx, mcg_paths* P, const mcg_sobol* sobol, double S0, double gm, double gs, const LocalVolScalars* lv,
                 int n_x, const double* table, int n_slices, bool want_payoff, double K, int is_call);
int sobol_check(const mcg_sobol* s);
int sobol_check_shape(const mcg_sobol* s, int n_steps, uint64_t path_begin, int64_t n_paths);
int launch_payoff_sums(mcg_ctx* ctx, const mcg_paths* P, double K, int is_call, double out3[3]);
int generator_clock(mcg_ctx* ctx, double* ghz_median, int* n_stamps, double* ghz_min, double* ghz_max);  // kernels_gbm.hip
int finish_sums(mcg_ctx* ctx, int64_t n_blocks, int64_t n_local, double out3[3]);
// {sum, sum of squares, n} of an estimator -> its mean and (std_err may be null) standard error
inline void sums_to_mean_stderr(double sum, double sum2, double n, double* mean, double* std_err) {
    const double m = sum / n;
    *mean = m;
    if (std_err) {
        const double var = n > 1.0 ? std::max(0.0, (sum2 - n * m * m) / (n - 1.0)) : 0.0;
        *std_err = std::sqrt(var / n);
    }
}
int run_lsm(mcg_ctx* ctx, const mcg_paths* P, double r, double K, double maturity, double dt, int is_call,
            int poly_order, double* mean, double* std_err);
// mean and std error of the value vector ctx->lsm_v a per-date sweep left (k_lsm_final over `grid` workgroups + finish_sums)
int lsm_finish(mcg_ctx* ctx, int grid, int64_t n_paths, double* mean, double* std_err);
// the two-regressor sweep (kernels_lsm2.hip): F has P's shape
int run_lsm2(mcg_ctx* ctx, const mcg_paths* P, const mcg_paths* F, double r, double K, double maturity, double dt, int is_call,
             int poly_order, double* mean, double* std_err, int64_t* n_dropped);
// LSM exercise policies: the exporting per-date sweep (kernels_lsm.hip), the forward pass (kernels_lsm_policy.hip) and the
// host side (host/lsm_policy.cpp: checks, the rows exported blocks become, the discount table exp(-r dt j))
int run_lsm_fit(mcg_ctx* ctx, const mcg_paths* P, double r, double K, double maturity, double dt, int is_call, int poly_order,
                double* mean, double* std_err, double* blocks_out);
int run_lsm_apply(mcg_ctx* ctx, const mcg_lsm_policy_hdr* hdr, const double* coef, const mcg_paths* P, double out3[3],
                  int64_t* tau_hist);
int lsm_policy_check_header(int n_steps, int poly_order, double r, double K, double maturity, double dt);
int lsm_policy_check(const mcg_lsm_policy_hdr* hdr, const double* coef);
void lsm_policy_from_blocks(const mcg_lsm_policy_hdr* hdr, double* coef);
void lsm_policy_discounts(const mcg_lsm_policy_hdr* hdr, double* disc);
// Greeks (kernels_greeks.hip; the LSM tangent sweep in kernels_lsm.hip)
int run_greeks_european(mcg_ctx* ctx, const mcg_paths* P, double K, double r, double T, int is_call, double sigma,
                        mcg_greeks* out);
int run_lsm_greeks(mcg_ctx* ctx, const mcg_paths* P, double r, double K, double maturity, double dt, int is_call,
                   int poly_order, mcg_greeks* out);
int greeks_lsm_final(mcg_ctx* ctx, const mcg_paths* P, double K, const double* V, const double* dV, mcg_greeks* out);
// ... the host arithmetic every Greeks entry point ends in:
// mean and standard error of an estimator from its sum and sum of squares over n paths, times `scale`
inline void mean_se(double sum, double sum2, double n, double scale, double* mean, double* se) {
    sums_to_mean_stderr(sum, sum2, n, mean, se);
    *mean = scale * *mean;
    *se = std::fabs(scale) * *se;
}
inline void greeks_all_nan(mcg_greeks* out) {
    const double nan = std::nan("");
    *out = mcg_greeks{nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan};
}
// the x grid of a Greeks or book kernel: it depends on the path count only
inline int book_blocks(const mcg_ctx* ctx, int64_t n) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)ctx->n_cus * 8));
}
// k_greeks_reduce over n_chunks sets of n_blocks x nf partials into d_out[n_chunks][nf] (no timing span of its own)
void enqueue_greeks_reduce(mcg_ctx* ctx, const double* d_part, int n_blocks, int nf, int n_chunks, double* d_out);
// Greeks of the exotics book (kernels_exotic_greeks.hip): k_path_tangent_stats over rows first_row .. n_steps (and, with logs,
// the rows before them for Q) of P into d_stats[10][n_paths]; one launch under MCG_K_EXOTIC
int launch_path_tangent_stats(mcg_ctx* ctx, const mcg_paths* P, int first_row, bool logs, double* d_stats);
int run_path_tangent_stats(mcg_ctx* ctx, const mcg_paths* P, int first_row, bool logs, double* host_out10);
int run_greeks_exotics(mcg_ctx* ctx, const mcg_paths* P, double r, double q, double sigma, double T, int first_row,
                       const mcg_exotic* book, int n_contracts, mcg_greeks* out);
// path-dependent European payoffs (kernels_exotic.hip)
int run_path_stats(mcg_ctx* ctx, const mcg_paths* P, int first_row, double* host_out5);
int run_exotics(mcg_ctx* ctx, const mcg_paths* P, double r, double T, int first_row, const mcg_exotic* book, int n_contracts,
                double* price, double* std_err, double* sums);
// ... their pieces, shared with the control-variate pricer (kernels_exotic_cv.hip) and the bridge pricer
// (kernels_barrier_bridge.hip); the device's share is exotic_device.hpp:
// does this contract, or this control, read the geometric mean
inline bool reads_g(const mcg_exotic& x) { return x.kind == MCG_X_ASIAN_GEO_FIXED || x.kind == MCG_X_ASIAN_GEO_FLOAT; }
inline bool reads_g(const mcg_control& k) { return k.form == MCG_CV_G || (k.form == MCG_CV_PAYOFF && reads_g(k.x)); }
// k_path_stats over rows first_row .. n_steps of P into d_stats[5][n_paths] (G only with geo); one launch under MCG_K_EXOTIC
int launch_path_stats(mcg_ctx* ctx, const mcg_paths* P, int first_row, bool geo, double* d_stats);
// the all-reduce of a payload that may exceed what the node-local collective carries in one call
int exotic_allreduce_sums(mcg_ctx* ctx, double* d, int count);
// launch(d_stats) into a pool buffer of 5 n_paths doubles, its download into host_out5, the buffer's release (`what` names the
// statistics in the message); a failed launch is synchronised first: nothing queued may use a buffer that is back in the pool.
// n_stats: the statistics per path where they are not five (the ten of mcg_path_tangent_stats)
int download_stats(mcg_ctx* ctx, int64_t n_paths, double* host_out5, const char* what, const std::function<int(double*)>& launch,
                   int n_stats = 5);
// The frame of a book's sums: a pool workspace of ws_doubles doubles whose last n_sums are the sums; fill(ws, d_sums) queues what
// computes them from a shard of n > 0 paths, an empty shard's are zeroed (it still takes part in the collective); then the
// all-reduce where a collective is installed and the download into h.  On an error the stream is synchronised before the
// workspace goes back to the pool: nothing queued may still use it, or what fill uploaded from.
int exotic_sums_frame(mcg_ctx* ctx, int64_t n, size_t ws_doubles, int n_sums, std::vector<double>& h,
                      const std::function<int(double* ws, double* d_sums)>& fill);
// mcg_api.hip: what mcg_price_exotics rejects of (ctx, paths, first_row) and of one contract (`what` names it in the message)
int exotic_args(mcg_ctx* ctx, const mcg_paths* P, int first_row);
int exotic_contract_check(const mcg_exotic& x, const char* what, int index);
// k_book_reduce<XB_CH, XB_NS> over the (n_contracts + XB_CH - 1) / XB_CH chunks of the partials of k_exotic_book or
// k_bridge_book (no timing span of its own)
void enqueue_exotic_reduce(mcg_ctx* ctx, const double* d_part, int n_blocks, int n_contracts, double n_local, double* d_sums);
// The end of run_exotics and run_barriers_bridge: h = {sum, sum^2} of n_contracts payoffs, slot s that of contract order[s]
// (order null: the book's own), then the path count -> discounted price and std_err (optional) per contract, and sums
// (optional) as include/mcgpu.h states them, in the book's order
int exotic_prices_from_sums(const std::vector<double>& h, int n_contracts, const int* order, double r, double T, double* price,
                            double* std_err, double* sums);
// Brownian-bridge barrier prices (kernels_barrier_bridge.hip; the host part in host/barrier_bridge.cpp).  V: the variance
// matrix of P's shape, or null for the scalar route w = (sigma sigma) dt.
int run_barrier_survival(mcg_ctx* ctx, const mcg_paths* P, const mcg_paths* V, double sigma, double dt, int first_row,
                         const double* barriers, const int* is_up, int n_levels, double* host_out);
int run_barriers_bridge(mcg_ctx* ctx, const mcg_paths* P, const mcg_paths* V, double sigma, double r, double T, int first_row,
                        const mcg_exotic* book, int n_contracts, double* price, double* std_err, double* sums);
// notes on an observation schedule (kernels_sched.hip): the book kernel's sums and stop counts, and the per-path values.
// mcg_api.hip has checked the arguments (sched_args)
int run_sched_book(mcg_ctx* ctx, const mcg_paths* P, double r, double dt, const mcg_obs* obs, int n_obs, const mcg_sched* book,
                   int n_contracts, double* price, double* std_err, double* sums, int64_t* stop_hist);
int run_sched_values(mcg_ctx* ctx, const mcg_paths* P, double r, double dt, const mcg_obs* obs, int n_obs, const mcg_sched* book,
                     int n_contracts, double* host_values, int32_t* host_stop);

// MartingaleOptimization's refit (its driver re-accumulates on request): mo_mode 1 = first pass, leave the refinement
// request in the coefficient block; 2 = the moments are about mo_mu, solve them with lsm_solve_centered.
int lsm_reduce_allreduce_solve(mcg_ctx* ctx, int grid, int nm, int nb, double min_count, double K, int mo_mode, double mo_mu);
int run_martingale(mcg_ctx* ctx, const mcg_paths* P, double r, double K, double maturity, double dt, int is_call,
                   int poly_order, int max_iterations, double* price, double* lower, double* upper);
int run_branching(mcg_ctx* ctx, const mcg_paths* P, double r, double K, double maturity, double dt, int is_call,
                  int num_branches, const int* exercise_times, int n_ex, uint64_t seed, double* price, double* lower,
                  double* upper);
// priced (optional, n_rows bytes): 1 where the row was priced, 0 where the driver's own checks answer it with zeros
int run_batch_rows(mcg_ctx* ctx, const mcg_row* rows, int64_t n_rows, int n_paths, double r, double dt, int num_branches,
                   int poly_order, int max_iterations, uint64_t seed, double* out, unsigned char* priced);
// run_batch_rows' own two questions about a row: would the reference's driver answer it with zeros, and does it leave the row
// kernels for the single-contract entry points (mcg_debug_batch_row_dump asks them before it runs anything)
bool batch_row_valid(const mcg_row& s);
bool batch_row_singly(const mcg_row& s, int n_paths, int poly_order);
int probe_write_ceiling(mcg_ctx* ctx, int64_t n_paths, int n_steps, int reps, double* gb_per_s, double* ms_per_launch);  // kernels_probe.hip
int run_asymptotic(mcg_ctx* ctx, const mcg_paths* P, double r, double K, double maturity, double dt, int is_call,
                   double sigma, double dividend, double* price);

// host-side math (host/volterra.cpp, host/estimators.cpp, host/asymptotic.cpp)
// host/sincos2.cpp: 2 * SINCOS2_ENTRIES doubles of the coarse table, then as many of the fine one (built on first use)
const double* host_sincos2_tables();
void host_asymptotic_tables(int n_cols, double r, double K, double maturity, double dt, int is_call, double sigma,
                            double dividend, std::vector<double>& bnd, std::vector<double>& disc);
int host_estimate_params(const double* hist, size_t n, double out5[5]);
void host_row_features(const double* hist, size_t n, double* vol, double* momentum);  // host/features.cpp
int host_row_build(const double* hist, size_t n, double underlying_last, double dte, double strike_dist_pct, int option_type,
                   double dividend, mcg_row* row, double features2[2]);
int host_rbergomi_spectrum(double H, double eta, double dt, int n_steps, std::vector<double>& amp,
                           std::vector<double>& comp);
// host/localvol.cpp: what mcg_localvol_table and mcg_paths_localvol* reject alike, the table, and the step's scalars
int localvol_check_surface(const double* times, int n_t, int n_x, const double* sigma, double dt, int n_steps);
int localvol_check_model(double S0, double r, double q, double x_min, double x_max, bool payoff, double K);
void localvol_fill_table(const double* times, int n_t, int n_x, const double* sigma, double dt, int n_steps, double* table);
LocalVolScalars localvol_scalars(double r, double q, double x_min, double x_max, int n_x, double dt);
// host/mlmc.cpp: what mcg_mlmc_localvol_level rejects of T and of a level's shape (kernels_mlmc.hip)
int mlmc_check_level(const mcg_mlmc_level* lv, double T);

}  // namespace mcg
