// Notes on an observation schedule (mcg_price_scheduled, mcg_sched_path_values; the contract is stated in include/mcgpu.h):
// autocallables (coupons with memory, early redemption, a knock-in put at maturity) and cliquets (sums of capped and floored
// period returns).  A path's payoff is a small state machine walked over the schedule's dates, so there is no statistics
// pass: ONE book kernel in k_exotic_book's layout (blockIdx.y a chunk of XB_CH contracts whose state lives in registers,
// blockIdx.x strides over the paths) reads only the scheduled rows, straight from the step-major matrix.
//   * A lane owns two adjacent paths (16-byte loads; the last path of an odd count stands alone: its neighbour column is the
//     row's padding, loaded and never used).  XS_ROWS scheduled rows are requested before the first of them is decided on.
//   * The schedule {row, flags}, the discounts and the book are read through the constant address space under wave-uniform
//     indices (scalar loads), like k_lsm_apply's policy: the schedule's length is no limit and nothing is staged in LDS.
//   * A date flagged KI alone costs two fmin per lane whatever the book holds: the knock-in test of the dates since the last
//     decision (a COUPON or CALL date) is taken there, on their minimum.  The correctly rounded division by s0 > 0 is monotone,
//     so min_k (S_k / s0) is (min_k S_k) / s0 to the bit, and a note's `alive` cannot change between two decisions.
//   * Once no lane of a wave holds a live contract the wave stops reading its paths.  A called autocallable is final and a
//     cliquet never dies (its bit stays set), so the skip is taken only where every result is final: it changes no bit.
//   * {sum Y, sum Y^2} per contract: book_partials / block_sum per workgroup, then k_book_reduce: fixed order, no
//     floating-point atomics.  The histogram of stopping dates is counted per wavefront (popcount of a ballot), kept per
//     workgroup in LDS where XB_CH (n_obs + 1) counters fit SC_HIST_LDS, and flushed with 64-bit integer adds (else added to
//     the global counters directly).
// mcg_sched_path_values runs the same walk and stores Y and stop per path.
#include <algorithm>
#include <cmath>
#include <vector>

#include "devmath.hpp"
#include "exotic_device.hpp"
#include "paths_host.hpp"

namespace mcg {

constexpr int SC_REF = 16;          // host-made flag beside MCG_OBS_RESET: a RESET date that has a reference (not the first)
constexpr int SC_HIST_LDS = 2048;   // counters a workgroup keeps in LDS: XB_CH contracts x up to 256 stops

// written before the launch and only read in it: the constant address space, a wave-uniform index gives scalar loads
typedef const double __attribute__((address_space(4))) * sc_doubles;
typedef const int __attribute__((address_space(4))) * sc_ints;
typedef const mcg_sched __attribute__((address_space(4))) * sc_contracts;

struct SchedArgs {
    const double* data;  // step-major matrix: 16-byte aligned rows (even ld)
    int64_t ld, n_paths;
    int n_obs, n_contracts;
    const double* disc;  // exp(-r row_k dt), k = 0 .. n_obs - 1
    const int* obs;      // {row_k, flags_k (with SC_REF)}
    const mcg_sched* book;
    double disc_reset;   // the discount of the last RESET date (cliquets)
    double* partials;    // k_sched_book: [(chunk * n_blocks + block) * XB_NF] {sum, sum of squares} per contract
    unsigned long long* hist;  // k_sched_book: [n_contracts][n_obs + 1] counters, zeroed before the launch; or null
    double* values;      // k_sched_values: [n_contracts][n_paths]
    int* stop;           //   likewise, or null
};

// The contracts c0 .. c0 + XB_CH of the book on the two paths of a unit (col: the unit's place in row 0; valid[w]: path w
// exists).  y: the present values.  alive: bit q of alive[w] is set where contract q was never called on path w (a cliquet's
// stays set): those stop at n_obs.  on_call(k, q, called): at every CALL date k, per autocallable q, which paths it calls.
// Every `if` below but the ones on a path's own state is wave-uniform.
template <class OnCall>
__device__ __forceinline__ void sched_walk(const SchedArgs& a, int c0, const double* col, const bool (&valid)[2], double (&y)[XB_CH][2],
                                           unsigned (&alive)[2], OnCall&& on_call) {
    const sc_contracts bk = (sc_contracts)a.book + c0;
    const sc_doubles discs = (sc_doubles)a.disc;
    const sc_ints obs = (sc_ints)a.obs;
    const int n_obs = a.n_obs;
    const int live = min(XB_CH, a.n_contracts - c0);
    unsigned cliq = 0u;
#pragma unroll
    for (int q = 0; q < XB_CH; ++q)
        if (q < live && bk[q].kind == MCG_S_CLIQUET) cliq |= 1u << q;
    const unsigned all = (1u << live) - 1u, autos = all & ~cliq;
    unsigned ki[2] = {0u, 0u};
    int missed[XB_CH][2];
    double s0[2], prev[2], last[2], low[2];
    xs_load<2>(col, s0);
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        alive[w] = valid[w] ? all : 0u;
        prev[w] = last[w] = s0[w];
        low[w] = std::numeric_limits<double>::infinity();
#pragma unroll
        for (int q = 0; q < XB_CH; ++q) {
            y[q][w] = 0.0;
            missed[q][w] = 0;
        }
    }
    for (int k0 = 0; k0 < n_obs; k0 += XS_ROWS) {
        double x[XS_ROWS][2];
#pragma unroll
        for (int d = 0; d < XS_ROWS; ++d)  // (behind the schedule's end: its last row again)
            xs_load<2>(col + (int64_t)obs[2 * min(k0 + d, n_obs - 1)] * a.ld, x[d]);
#pragma unroll
        for (int d = 0; d < XS_ROWS; ++d) {
            const int k = k0 + d;
            if (k >= n_obs) goto walked;
            const int flags = obs[2 * k + 1];
            last[0] = x[d][0];
            last[1] = x[d][1];
            if ((flags & MCG_OBS_RESET) != 0) {
                if ((flags & SC_REF) != 0 && cliq != 0u) {
#pragma unroll
                    for (int w = 0; w < 2; ++w) {
                        const double ret = x[d][w] / prev[w] - 1.0;
#pragma unroll
                        for (int q = 0; q < XB_CH; ++q)
                            if (((cliq >> q) & 1u) != 0u) y[q][w] += fmin(bk[q].local_cap, fmax(bk[q].local_floor, ret));
                    }
                }
                prev[0] = x[d][0];
                prev[1] = x[d][1];
            }
            if ((flags & MCG_OBS_KI) != 0 && autos != 0u) {
                low[0] = fmin(low[0], x[d][0]);
                low[1] = fmin(low[1], x[d][1]);
            }
            if ((flags & (MCG_OBS_COUPON | MCG_OBS_CALL)) != 0 && autos != 0u) {
                const double disc = discs[k];
                const double X[2] = {x[d][0] / s0[0], x[d][1] / s0[1]};
                const double Xlow[2] = {low[0] / s0[0], low[1] / s0[1]};
                low[0] = low[1] = std::numeric_limits<double>::infinity();
#pragma unroll
                for (int q = 0; q < XB_CH; ++q) {
                    if (((autos >> q) & 1u) == 0u) continue;
                    const unsigned bit = 1u << q;
                    bool called[2] = {false, false};
#pragma unroll
                    for (int w = 0; w < 2; ++w) {
                        const bool al = (alive[w] & bit) != 0u;
                        if (al && Xlow[w] <= bk[q].ki_level) ki[w] |= bit;
                        if ((flags & MCG_OBS_COUPON) != 0 && al) {
                            if (X[w] >= bk[q].coupon_level) {
                                y[q][w] += bk[q].coupon * (double)(1 + (bk[q].memory != 0 ? missed[q][w] : 0)) * disc;
                                missed[q][w] = 0;
                            } else {
                                missed[q][w] += 1;
                            }
                        }
                        if ((flags & MCG_OBS_CALL) != 0 && al && X[w] >= bk[q].call_level) {
                            y[q][w] += disc;
                            alive[w] &= ~bit;
                            called[w] = true;
                        }
                    }
                    if ((flags & MCG_OBS_CALL) != 0) on_call(k, q, called);
                }
                // nothing of this wave is left to decide: the remaining rows are not read
                if ((flags & MCG_OBS_CALL) != 0 && __builtin_amdgcn_ballot_w64((alive[0] | alive[1]) != 0u) == 0ull) goto walked;
            }
        }
    }
walked:
    const double disc_last = discs[n_obs - 1];
#pragma unroll
    for (int q = 0; q < XB_CH; ++q) {
        if (q >= live) continue;
        const unsigned bit = 1u << q;
        if ((cliq & bit) != 0u) {
#pragma unroll
            for (int w = 0; w < 2; ++w) y[q][w] = fmin(bk[q].global_cap, fmax(bk[q].global_floor, y[q][w])) * a.disc_reset;
        } else {
            const double ps = bk[q].put_strike;
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                if ((alive[w] & bit) == 0u) continue;
                const double xl = last[w] / s0[w];
                const bool in = (ki[w] & bit) != 0u || low[w] / s0[w] <= bk[q].ki_level;  // (the KI dates behind the last decision)
                const double R = (in && xl < ps) ? xl / ps : 1.0;
                y[q][w] += R * disc_last;
            }
        }
    }
}

// partials[(chunk * gridDim.x + blockIdx.x) * XB_NF + XB_NS * q + {0: sum, 1: sum of squares}] of the chunk's contract q
__global__ __launch_bounds__(256) void k_sched_book(const SchedArgs a) {
    __shared__ double red[XB_NF * 4];
    __shared__ unsigned sm_hist[SC_HIST_LDS];
    const int c0 = blockIdx.y * XB_CH;
    const int live = min(XB_CH, a.n_contracts - c0);
    const int nh = a.n_obs + 1;
    const bool want_hist = a.hist != nullptr;                         // (uniform)
    const bool lds_hist = want_hist && XB_CH * nh <= SC_HIST_LDS;     // (uniform)
    if (lds_hist) {
        for (int i = threadIdx.x; i < XB_CH * nh; i += 256) sm_hist[i] = 0u;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    // the paths of this wave that stop at k under contract q: one integer add by the wave's first active lane
    auto count = [&](int k, int q, const bool (&s)[2]) {
        const unsigned long long b0 = __builtin_amdgcn_ballot_w64(s[0]), b1 = __builtin_amdgcn_ballot_w64(s[1]);
        if ((b0 | b1) == 0ull) return;  // (uniform)
        if (lane == __ffsll((long long)__builtin_amdgcn_ballot_w64(true)) - 1) {
            const unsigned cnt = (unsigned)(__popcll(b0) + __popcll(b1));
            if (lds_hist) atomicAdd(&sm_hist[q * nh + k], cnt);
            else atomicAdd(a.hist + (int64_t)(c0 + q) * nh + k, (unsigned long long)cnt);
        }
    };
    book_partials<XB_NF>((a.n_paths + 1) / 2, red, a.partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * XB_NF,
                         [&](int64_t u, double (&e)[XB_NF]) {
                             const bool valid[2] = {true, 2 * u + 1 < a.n_paths};
                             double y[XB_CH][2];
                             unsigned alive[2];
                             sched_walk(a, c0, a.data + 2 * u, valid, y, alive, [&](int k, int q, const bool (&called)[2]) {
                                 if (want_hist) count(k, q, called);
                             });
#pragma unroll
                             for (int q = 0; q < XB_CH; ++q) {
                                 if (q >= live) continue;
                                 if (want_hist) {
                                     const bool end[2] = {((alive[0] >> q) & 1u) != 0u, ((alive[1] >> q) & 1u) != 0u};
                                     count(a.n_obs, q, end);
                                 }
#pragma unroll
                                 for (int w = 0; w < 2; ++w) {
                                     if (!valid[w]) continue;
                                     e[XB_NS * q] += y[q][w];
                                     e[XB_NS * q + 1] = fma(y[q][w], y[q][w], e[XB_NS * q + 1]);
                                 }
                             }
                         });
    if (lds_hist) {  // (block_sum's barrier follows every wave's last LDS counter add)
        for (int i = threadIdx.x; i < live * nh; i += 256) {
            const unsigned cnt = sm_hist[i];
            if (cnt != 0u) atomicAdd(a.hist + (int64_t)c0 * nh + i, (unsigned long long)cnt);
        }
    }
}

// One lane per two adjacent paths, blockIdx.y a chunk of XB_CH contracts: the walk's Y and stop of every path
__global__ __launch_bounds__(256) void k_sched_values(const SchedArgs a) {
    const int c0 = blockIdx.y * XB_CH;
    const int live = min(XB_CH, a.n_contracts - c0);
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (2 * u >= a.n_paths) return;
    const bool valid[2] = {true, 2 * u + 1 < a.n_paths};
    double y[XB_CH][2];
    unsigned alive[2];
    int stop[XB_CH][2];
#pragma unroll
    for (int q = 0; q < XB_CH; ++q) stop[q][0] = stop[q][1] = a.n_obs;
    sched_walk(a, c0, a.data + 2 * u, valid, y, alive, [&](int k, int q, const bool (&called)[2]) {
        if (called[0]) stop[q][0] = k;
        if (called[1]) stop[q][1] = k;
    });
#pragma unroll
    for (int q = 0; q < XB_CH; ++q) {
        if (q >= live) continue;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            if (!valid[w]) continue;
            const int64_t at = (int64_t)(c0 + q) * a.n_paths + 2 * u + w;
            a.values[at] = y[q][w];
            if (a.stop) a.stop[at] = stop[q][w];
        }
    }
}

// The host's tables of one call: the discounts, the schedule with SC_REF, and what the kernels' arguments share
struct SchedTables {
    std::vector<double> disc;
    std::vector<int> obs;
    double disc_reset = 0.0;

    SchedTables(double r, double dt, const mcg_obs* o, int n_obs) : disc((size_t)n_obs), obs(2 * (size_t)n_obs) {
        bool ref = false;
        for (int k = 0; k < n_obs; ++k) {
            disc[(size_t)k] = std::exp(-r * ((double)o[k].row * dt));
            int flags = o[k].flags;
            if ((flags & MCG_OBS_RESET) != 0) {
                if (ref) flags |= SC_REF;
                ref = true;
                disc_reset = disc[(size_t)k];
            }
            obs[2 * (size_t)k] = o[k].row;
            obs[2 * (size_t)k + 1] = flags;
        }
    }
    // uploads the tables and the book (room for extra_doubles behind them: *extra) and fills the arguments
    int upload(mcg_ctx* ctx, const mcg_paths* P, const mcg_sched* book, int nc, size_t extra_doubles, SchedArgs& a, double** extra) const {
        if ((P->ld & 1) != 0 || (reinterpret_cast<uintptr_t>(P->data) & 15) != 0)
            return fail(MCG_ERR_INVALID, "path matrix rows must be 16-byte aligned");
        HostPiece up[] = {{disc.data(), disc.size() * sizeof(double)}, {obs.data(), obs.size() * sizeof(int)}, {book, (size_t)nc * sizeof(mcg_sched)}};
        const int rc = upload_params(ctx, up, extra_doubles);
        if (rc) return rc;
        a = SchedArgs{};
        a.data = P->data;
        a.ld = P->ld;
        a.n_paths = P->n_paths;
        a.n_obs = (int)disc.size();
        a.n_contracts = nc;
        a.disc = up[0].at;
        a.obs = reinterpret_cast<const int*>(up[1].at);
        a.book = reinterpret_cast<const mcg_sched*>(up[2].at);
        a.disc_reset = disc_reset;
        *extra = up[2].at + (up[2].bytes + 7) / 8;
        return MCG_OK;
    }
};

// Workspace (one pool buffer): [n_chunks * n_blocks * XB_NF partials][2 n_contracts + 1 sums]; the counters stand behind the
// uploaded tables.  The arguments have been checked (mcg_api.hip).
int run_sched_book(mcg_ctx* ctx, const mcg_paths* P, double r, double dt, const mcg_obs* obs, int n_obs, const mcg_sched* book, int nc,
                   double* price, double* std_err, double* sums, int64_t* stop_hist) {
    const int64_t n = P->n_paths;
    const int n_sums = 2 * nc + 1, n_chunks = (nc + XB_CH - 1) / XB_CH;
    const int n_blocks = book_blocks(ctx, (n + 1) / 2);
    const size_t n_part = (size_t)n_chunks * n_blocks * XB_NF, n_hist = stop_hist ? (size_t)nc * (n_obs + 1) : 0;
    const SchedTables tables(r, dt, obs, n_obs);
    unsigned long long* d_hist = nullptr;
    std::vector<double> h;
    int rc = exotic_sums_frame(ctx, n, n_part + n_sums, n_sums, h, [&](double* d_part, double* d_sums) -> int {
        SchedArgs a;
        double* extra = nullptr;
        const int r2 = tables.upload(ctx, P, book, nc, n_hist, a, &extra);
        if (r2) return r2;
        a.partials = d_part;
        if (stop_hist) {
            d_hist = reinterpret_cast<unsigned long long*>(extra);
            MCG_HIP(hipMemsetAsync(d_hist, 0, n_hist * sizeof(unsigned long long), ctx->stream));
            a.hist = d_hist;
        }
        {
            TimedLaunch t(ctx, MCG_K_EXOTIC, 2);
            hipLaunchKernelGGL(k_sched_book, dim3(n_blocks, n_chunks), dim3(256), 0, ctx->stream, a);
            enqueue_exotic_reduce(ctx, d_part, n_blocks, nc, (double)n, d_sums);
        }
        MCG_HIP(hipGetLastError());
        return MCG_OK;
    });
    if (rc) return rc;
    rc = exotic_prices_from_sums(h, nc, nullptr, 0.0, 0.0, price, std_err, sums);  // (Y is a present value: no further discount)
    if (rc) return rc;
    if (stop_hist) {
        static_assert(sizeof(int64_t) == sizeof(unsigned long long), "the counters are downloaded as they are");
        MCG_HIP(hipMemcpyAsync(stop_hist, d_hist, n_hist * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        MCG_HIP(hipStreamSynchronize(ctx->stream));
    }
    return MCG_OK;
}

// download_stats' pattern with two outputs: [n_contracts n doubles][n_contracts n ints] in one pool buffer
int run_sched_values(mcg_ctx* ctx, const mcg_paths* P, double r, double dt, const mcg_obs* obs, int n_obs, const mcg_sched* book, int nc,
                     double* host_values, int32_t* host_stop) {
    const int64_t n = P->n_paths;
    const int64_t n_blocks = launch_units(((n + 1) / 2 + 255) / 256);
    if (n_blocks < 0) return MCG_ERR_INVALID;
    const size_t count = (size_t)nc * (size_t)n;
    const size_t bytes = count * (sizeof(double) + sizeof(int32_t));
    const SchedTables tables(r, dt, obs, n_obs);
    void* ws = nullptr;
    int rc = pool_alloc(ctx, bytes, &ws);
    if (rc) return rc;
    auto body = [&]() -> int {
        SchedArgs a;
        double* extra = nullptr;
        const int r2 = tables.upload(ctx, P, book, nc, 0, a, &extra);
        if (r2) return r2;
        a.values = (double*)ws;
        a.stop = host_stop ? reinterpret_cast<int*>((double*)ws + count) : nullptr;
        {
            TimedLaunch t(ctx, MCG_K_EXOTIC);
            hipLaunchKernelGGL(k_sched_values, dim3((unsigned)n_blocks, (nc + XB_CH - 1) / XB_CH), dim3(256), 0, ctx->stream, a);
        }
        MCG_HIP(hipGetLastError());
        MCG_HIP(hipMemcpyAsync(host_values, a.values, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (host_stop) MCG_HIP(hipMemcpyAsync(host_stop, a.stop, count * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        MCG_HIP(hipStreamSynchronize(ctx->stream));
        return MCG_OK;
    };
    rc = body();
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    pool_release(ctx, ws, bytes);
    return rc;
}

}  // namespace mcg
