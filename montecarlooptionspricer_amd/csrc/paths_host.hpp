// The host's share of the step-major path generators' skeleton (paths_device.hpp has the device's): what every launcher
// (launch_gbm, launch_rbergomi, launch_heston_scheme, launch_localvol, launch_sobol, launch_gbm_multi / launch_paths_combine,
// launch_gbm_twin_stats) does around its kernel.  This header states once
//   launch_blocks     the grid of a generator: workgroups of 256 lanes, the launch limit, rows padded to 256 columns
//   stream_grid       the grid of a kernel that reads the matrix back, one lane per one or two adjacent paths
//   PathLaunch        the launch frame: the partial sums' buffer, the timing span, the launch error, the fused sums
//   keep_sums         what a *_payoff generator leaves in its matrix handle
//   set_shape_key, set_payoff   the members every generator's argument struct has under the same names
//   dispatch_flags    run-time bools -> template arguments
//   upload_params     host parameters into ctx->weights, and who keeps their source alive until when
// A launcher supplies its own checks, its model's members of the argument struct, and the enqueue of its kernel.
#pragma once
#include <type_traits>

#include "mcg_internal.hpp"

namespace mcg {

// n_units if one launch can have so many workgroups (or tiles, or shares); -1 after fail(MCG_ERR_INVALID, ...) otherwise,
// or where a row of P is not padded to 256 columns: the kernels store whole workgroups' columns unconditionally
inline int64_t launch_units(int64_t n_units, const mcg_paths* P = nullptr) {
    if (n_units > 0x7fffffffLL) return fail(MCG_ERR_INVALID, "n_paths too large for one launch"), -1;
    if (P && (P->ld & 255) != 0) return fail(MCG_ERR_INVALID, "path matrix rows must be padded to 256 columns"), -1;
    return n_units;
}
// The grid of a step-major path generator: workgroups of 256 lanes with ppl paths each over n_paths, or over the padded
// rows of P
inline int64_t launch_blocks(int64_t n_paths, int ppl, const mcg_paths* P = nullptr) {
    return launch_units((n_paths + 256 * ppl - 1) / (256 * ppl), P);
}
inline int64_t launch_blocks(const mcg_paths* P, int ppl) { return launch_blocks(P->n_paths, ppl, P); }

// The grid of a kernel that streams P (and V, where given) with one lane per W adjacent paths (lane_paths, exotic_device.hpp):
// wide, W = 2, where every row of either matrix is 16-byte aligned (even ld, aligned base); n_blocks as launch_units gives it
struct StreamGrid {
    bool wide;
    int64_t n_blocks;
};
inline StreamGrid stream_grid(const mcg_paths* P, const mcg_paths* V = nullptr) {
    auto aligned = [](const mcg_paths* M) { return !M || ((M->ld & 1) == 0 && (reinterpret_cast<uintptr_t>(M->data) & 15) == 0); };
    const bool wide = aligned(P) && aligned(V);
    const int64_t lanes = wide ? (P->n_paths + 1) / 2 : P->n_paths;
    return {wide, launch_units((lanes + 255) / 256)};
}

// the end of a *_payoff generator: rc is what finish_sums or launch_payoff_sums returned for P->sums; on success P
// holds the (all-reduced, if a collective is installed) totals of the (K, is_call) payoff
inline int keep_sums(int rc, mcg_paths* P, double K, int is_call) {
    if (rc) return rc;
    P->has_sums = true;
    P->sums_K = K;
    P->sums_is_call = is_call;
    return MCG_OK;
}

// One generator launch of n_blocks units (each leaves one {sum, sum of squares} when the form is fused) over P.
//   reserve()   sizes ctx->partials for a fused form: BEFORE the caller takes ctx->partials into its arguments
//   run()       the timing span of `kernel` around enqueue() -- exactly the launches that belong to it; memsets of tickets
//               and stamps and uploads go in front of run() --, the launch error, and for a fused form the sums of
//               ctx->partials into P (finish_sums synchronises the stream)
// A launch without a payoff (launch_gbm_multi, launch_gbm_twin_stats) is PathLaunch{ctx, n_blocks}.
struct PathLaunch {
    mcg_ctx* ctx;
    int64_t n_blocks;
    mcg_paths* P = nullptr;
    bool fused = false;
    double K = 0.0;
    int is_call = 0;

    int reserve() const { return fused ? ensure_cap(ctx, &ctx->partials, &ctx->partials_cap, (size_t)(2 * n_blocks)) : MCG_OK; }
    template <class Enqueue>
    int run(int kernel, Enqueue&& enqueue) const {
        {
            TimedLaunch t(ctx, kernel);
            enqueue();
        }
        MCG_HIP(hipGetLastError());
        if (fused) return keep_sums(finish_sums(ctx, n_blocks, P->n_paths, P->sums), P, K, is_call);
        return MCG_OK;
    }
};

// The matrix, its shape, the ids of its paths and the Philox key (= seed) of an argument struct that names them so
template <class Args>
inline void set_shape_key(Args& a, const mcg_paths* P, uint64_t seed) {
    a.out = P->data;
    a.ld = P->ld;
    a.n_paths = P->n_paths;
    a.n_steps = P->n_steps;
    a.path_begin = P->path_begin;
    a.k0 = (uint32_t)seed;
    a.k1 = (uint32_t)(seed >> 32);
}
// ... and the payoff of a fused form with where its partial sums go (after PathLaunch::reserve)
template <class Args>
inline void set_payoff(Args& a, const mcg_ctx* ctx, double K, int is_call) {
    a.K = K;
    a.is_call = is_call;
    a.partials = ctx->partials;
}

// f(std::bool_constant<flags>...): run-time flags as template arguments.  Every combination of the flags is compiled: a
// combination that has no kernel is excluded inside f with `if constexpr`.
template <class F>
inline void dispatch_flags(F&& f) {
    f();
}
template <class F, class... Flags>
inline void dispatch_flags(F&& f, bool flag, Flags... flags) {
    if (flag) dispatch_flags([&](auto... rest) { f(std::true_type{}, rest...); }, flags...);
    else dispatch_flags([&](auto... rest) { f(std::false_type{}, rest...); }, flags...);
}

// Host parameters of a launch into ctx->weights, on the ctx's stream: the pieces back to back in the order given, each
// from the next whole double on, with room for extra_doubles behind the last; HostPiece::at is where a piece landed.
// Lifetime: the sources are pageable memory, and a copy queued from pageable memory may still read its source after
// hipMemcpyAsync has returned.  So the CALLER keeps every source alive until the stream has been synchronised behind the
// copies.  Where the sources are locals or the caller's arrays and a path to the return holds no synchronisation -- the
// generators (rBergomi, local volatility, Sobol': a plain form returns right behind its launch) and the asymptotic,
// martingale and branching pricers -- the call site synchronises right behind the upload.  The others (LSM policy, LSM
// dual, the exotics) end in a download of their sums that synchronises before the sources go, and add nothing; only a
// HIP error between the upload and that download returns earlier.
struct HostPiece {
    const void* src;
    size_t bytes;
    double* at = nullptr;
};
template <size_t N>
inline int upload_params(mcg_ctx* ctx, HostPiece (&pieces)[N], size_t extra_doubles = 0) {
    size_t need = extra_doubles;
    for (const HostPiece& p : pieces) need += (p.bytes + 7) / 8;
    const int rc = ensure_cap(ctx, &ctx->weights, &ctx->weights_cap, need);
    if (rc) return rc;
    double* at = ctx->weights;
    for (HostPiece& p : pieces) {
        p.at = at;
        if (p.bytes) MCG_HIP(hipMemcpyAsync(at, p.src, p.bytes, hipMemcpyHostToDevice, ctx->stream));
        at += (p.bytes + 7) / 8;
    }
    return MCG_OK;
}

}  // namespace mcg
