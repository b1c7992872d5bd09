// BranchingProcesses::PredictOptionPrice on a device-resident step-major path matrix (gfx950).
//
// Reference: /root/reference/src/models/BranchingProcessPricer.cpp:12-134.
//   lower bound (:41-72): per path, the first exercise date (t <= maturity) with a positive discounted payoff;
//   upper bound (:74-134): per path, max over exercise dates of max(discounted payoff now, continuation), where
//     the continuation at date t resamples `numBranches` paths uniformly at random and averages their best
//     discounted payoff over all LATER columns k (t_k <= maturity), :104-121;
//   price = midpoint (:37).
// The inner O(T) rescan per (path, date, branch) collapses to a lookup: with
//   F[j][p] = max_{k >= j, t_k <= maturity} e^{-r t_k} Payoff(S[k][p])   (suffix maximum, floored at 0)
// the reference's bestFut * e^{-r t} equals F[t_idx+1][rp].  k_branch_suffix builds F with one backward
// stream (read S, write F: 16 B per element); k_branch_bounds then does the O(N T B) random gathers inside row
// t_idx+1 of F (L2/MALL-resident rows) with Philox-drawn path indices (stream 2, counter = (path, date, branch/4)).
// The reference draws from an unseeded shared mt19937, so parity of the upper bound is statistical; the lower
// bound is deterministic.  Sharded use resamples within the local shard (the matrix is never exchanged).
#include "branching_device.hpp"
#include "paths_host.hpp"

namespace mcg {

// F[j][p] for j = n_cols-1 .. 0.  disc[j] = e^{-r j dt}; columns j >= n_dates (t_j > maturity) contribute 0.
__global__ __launch_bounds__(256) void k_branch_suffix(const double* S, double* F, int64_t ld, int64_t n, int n_cols,
                                                       int n_dates, const double* disc, double K, int is_call) {
    const bool call = is_call != 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        double run = 0.0;
        for (int j = n_cols - 1; j >= 0; --j) {
            if (j < n_dates) {
                const double d = disc[j] * payoff_of(call, S[(int64_t)j * ld + p], K);
                if (d > run) run = d;
            }
            F[(int64_t)j * ld + p] = run;
        }
    }
}

struct BranchArgs {
    const double* S;
    const double* F;
    int64_t ld, n;
    uint64_t path_begin;
    uint32_t k0, k1;
    const int* ex;        // [n_ex] exercise column indices with t <= maturity (leading part of the list)
    const double* disc;   // [n_cols]
    int n_ex, ex_last, num_branches;
    int n_cols;           // rows of S and F: the continuation of date t gathers from row t+1 < n_cols only
    double K;
    int is_call;
};

// ---- the pieces every bounds kernel is made of ---------------------------------------------------------------------------------
// Does the exercise date on column t_idx have a continuation (:104-121)?  Not the list's LAST entry (exerciseTimes.back(), :104 --
// not its largest), and not an index on the last column: a trailing exercise index at or beyond the last column (the reference
// tolerates one behind its `t > maturity` break, :97-99) leaves its `k` loop (:110) empty for t_idx = n_cols - 1, continuation 0.
__host__ __device__ inline bool date_branches(int t_idx, int ex_last, int n_cols) { return t_idx < ex_last && t_idx + 1 < n_cols; }

// the row of F that date t_idx gathers from (where it has no continuation: its own row, never read)
__device__ __forceinline__ const double* branch_row_f(const BranchArgs& a, int t_idx, bool branch) {
    return a.F + (int64_t)(branch ? t_idx + 1 : t_idx) * a.ld;
}

__device__ __forceinline__ PhiloxLane branch_rng(const BranchArgs& a, int64_t p) {
    return philox_lane_setup(a.path_begin + (uint64_t)p, STREAM_BRANCH, a.k1);
}

// THE BOUNDS RULE of one path at one exercise date: `now` its discounted payoff there, `cont` its continuation where the date
// branches.  :62-65 -- the first positive discounted payoff is the lower bound (lower > 0 <=> it has been seen: lower is only ever
// set to a now > 0); :123-127 -- the upper bound is the running maximum of max(now, cont).
__device__ __forceinline__ void branch_update(double& lower, double& upper, double now, double cont, bool branch) {
    if (!(lower > 0.0) && now > 0.0) lower = now;
    double better = now;
    if (branch && cont > better) better = cont;
    if (better > upper) upper = better;
}

// A path's bounds between the launches of a per-date route: `state` = {lower, upper} per path, 32 B per path and date, read and
// written past the caches.
typedef double br_v2d __attribute__((ext_vector_type(2)));
__device__ __forceinline__ br_v2d branch_state_load(const double2* state, int first_date, int64_t p) {
    return first_date ? br_v2d{0.0, 0.0} : __builtin_nontemporal_load(reinterpret_cast<const br_v2d*>(state) + p);
}
__device__ __forceinline__ double branch_now(const BranchArgs& a, const double* rowS, double dsc, int64_t p) {  // rowS, dsc: of the date's column
    return dsc * payoff_of(a.is_call != 0, __builtin_nontemporal_load(rowS + p), a.K);
}
__device__ __forceinline__ void branch_state_store(double2* state, int64_t p, bool live, br_v2d st, double now, double cont, bool branch) {
    double lower = st.x, upper = st.y;
    branch_update(lower, upper, now, cont, branch);
    if (live) __builtin_nontemporal_store(br_v2d{lower, upper}, reinterpret_cast<br_v2d*>(state) + p);
}

// The dates are the OUTER loop: every thread carries the bounds of its BR_PPT paths in registers and all resident
// threads work on one exercise date at about the same time, so the device's gathers of that moment fall into ONE row of
// F instead of being spread over the whole matrix (round 2: paths outermost, each thread walking its own dates: 7.7 ms
// for the 5 10^8 gathers of a 1M x 50 matrix; 5.4 ms this way).  A launch covers gridDim.x * 256 * BR_PPT paths
// starting at p0; larger shards take several launches.
//
// Round 4 -- the row in SLICES.  The counters (profiles/r04_branching_counters_before.json) put numbers on where a gather is
// served: a row that fits an XCD's 4 MiB of L2 (250k paths: 2 MB) is gathered at 188 G/s with 94 % L2 hits; the 8 MB row
// of a million paths at 92 G/s with 34 %, two thirds of the gathers going out to the fabric as one 64-byte request
// each (61 G requests/s: the rate at which the memory side serves random sectors, whatever cache they hit); the 32 MB
// row of 4M paths at 55 G/s with 4.5 %.  So the row is walked in slices of 2 MB: a thread draws the indices of all its
// branches for the date ONCE, keeps them in registers (4 QUADS words per path) and then passes over the slices, gathering
// in pass s only the indices that fall into slice s -- every lane of the device is in the same couple of slices at a
// time, which the L2 of every XCD holds.  The loads stay unconditional (a lane whose index lies elsewhere reads the
// slice's first element -- one line for all of them -- and adds zero), so all of a pass's loads are in flight together.
// Rows beyond 16 MB take 8 slices of n/8 (more passes would cost more instructions than the misses they avoid).
constexpr int BR_PPT = 4;
constexpr int BR_SLICE_SHIFT = 18;  // 2^18 paths = 2 MB of a row of F
constexpr int BR_MAX_SLICES = 8;
constexpr int BR_DATE_MAX_SLICES = 4;  // per-date launches pay for rows of up to four slices (8 MB: a million paths), see run_branching
constexpr int BR_WGS_PER_CU = 4;    // resident workgroups per CU the register budget is held to: a launch's grid is one resident wave

struct BranchLane {  // one thread's BR_PPT paths
    int64_t p[BR_PPT];
    bool live[BR_PPT];
    double lower[BR_PPT], upper[BR_PPT];
    PhiloxLane rng[BR_PPT];  // block numbers are wave-uniform
};

// The paths of a lane: path q of thread t of workgroup w is p0 + (w 256 + t) + q (gridDim.x 256); a lane beyond the shard is
// clamped to the last path (reads stay in range; the result is dropped).  The two per-date kernels have the same three lines
// inside their own path loops.
__device__ __forceinline__ void branch_lane_setup(BranchLane& t, const BranchArgs& a, int64_t p0) {
    const int64_t stride = (int64_t)gridDim.x * 256;
#pragma unroll
    for (int q = 0; q < BR_PPT; ++q) {
        t.p[q] = p0 + (int64_t)blockIdx.x * 256 + threadIdx.x + q * stride;
        t.live[q] = t.p[q] < a.n;
        if (!t.live[q]) t.p[q] = a.n - 1;
        t.lower[q] = t.upper[q] = 0.0;
        t.rng[q] = branch_rng(a, t.p[q]);
    }
}

__device__ __forceinline__ void branch_lane_finish(const BranchLane& t, double* red, double* partials) {
    double v[2] = {0.0, 0.0};
#pragma unroll
    for (int q = 0; q < BR_PPT; ++q) {
        if (t.live[q]) {
            v[0] += t.lower[q];
            v[1] += t.upper[q];
        }
    }
    block_sum_store2(v, red, partials);
}

// an empty shard still takes part in the collective that follows: its workgroups' partials are zeros
__device__ __forceinline__ bool branch_empty_shard(const BranchArgs& a, double* partials) {
    if (a.n > 0) return false;
    if (threadIdx.x == 0) partials[2 * (int64_t)blockIdx.x] = partials[2 * (int64_t)blockIdx.x + 1] = 0.0;
    return true;
}

// QUADS = Philox blocks per path and date = ceil(num_branches / 4) <= 3 (the driver's 10 branches: 3); more branches than
// twelve take k_branch_bounds_any, which gathers as it draws.
template <int QUADS>
__global__ __launch_bounds__(256, BR_WGS_PER_CU) void k_branch_bounds(BranchArgs a, int64_t p0, double* partials, int slice_shift, int n_slices) {
    __shared__ double red[2 * 4];
    const bool call = a.is_call != 0;
    const double inv_b = a.num_branches > 0 ? 1.0 / (double)a.num_branches : 0.0;
    if (branch_empty_shard(a, partials)) return;
    BranchLane t;
    branch_lane_setup(t, a, p0);
    for (int e = 0; e < a.n_ex; ++e) {
        const int t_idx = a.ex[e];
        const double* rowS = a.S + (int64_t)t_idx * a.ld;
        const double dsc = a.disc[t_idx];
        const bool branch = date_branches(t_idx, a.ex_last, a.n_cols) && a.num_branches > 0;
        const double* rowF = branch_row_f(a, t_idx, branch);
        double now[BR_PPT], sum[BR_PPT];
#pragma unroll
        for (int q = 0; q < BR_PPT; ++q) {
            now[q] = dsc * payoff_of(call, rowS[t.p[q]], a.K);
            sum[q] = 0.0;
        }
        if (branch) {  // (wave-uniform)
            uint32_t idx[BR_PPT][4 * QUADS];  // uniform on [0, n); a draw beyond num_branches gets an index in no slice
#pragma unroll
            for (int q = 0; q < BR_PPT; ++q) {
                branch_draw<QUADS>(t.rng[q], e, a.k0, a.k1,
                                   [&](int b, uint32_t word) { idx[q][b] = b < a.num_branches ? branch_index(word, (uint32_t)a.n) : 0xFFFFFFFFu; });
            }
            // pass sl gathers only the indices that fall into slice sl; the sum over a path's branches is formed in SLICE order
            for (int sl = 0; sl < n_slices; ++sl) {
                const uint32_t first = (uint32_t)sl << slice_shift;  // (< n: the slices cover [0, n))
#pragma unroll
                for (int q = 0; q < BR_PPT; ++q) {
#pragma unroll
                    for (int b = 0; b < 4 * QUADS; ++b) {
                        const bool in = (idx[q][b] >> slice_shift) == (uint32_t)sl;
                        const double v = rowF[in ? idx[q][b] : first];
                        sum[q] += in ? v : 0.0;
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < BR_PPT; ++q) branch_update(t.lower[q], t.upper[q], now[q], sum[q] * inv_b, branch);
    }
    branch_lane_finish(t, red, partials);
}

// ONE EXERCISE DATE per launch (rows of F beyond one slice): inside one launch of ~100 us the workgroups stay within a
// slice or two of each other, which a whole sweep's worth of drift in k_branch_bounds does not -- its 1M-path row was still
// gathered with 42 % L2 hits (profiles/r04_branching_counters_before.json).  The bounds of a path travel between the launches in
// `state` = {lower, upper} per path (lower > 0 <=> the first positive payoff has been seen): 32 B per path and date.
template <int QUADS>
__global__ __launch_bounds__(256, BR_WGS_PER_CU) void k_branch_date(BranchArgs a, int64_t p0, int e, double2* state, int first_date,
                                                                   int slice_shift, int n_slices) {
    // The lane's paths, the draws (branching_device.hpp's contract), k_branch_bounds' slice walk and the bounds rule (branch_update, on
    // the pair in place) are WRITTEN OUT here: through branch_draw, and again with only branch_state_load / branch_state_store and a
    // shared slice walk, this kernel measured 0.4-0.6 % slower at 1M x 50, beyond the parent's own spread.
    // As it stands its three code objects are the parent commit's, instruction for instruction.
    const uint32_t n32 = (uint32_t)a.n;
    const double inv_b = 1.0 / (double)a.num_branches;
    const int t_idx = a.ex[e];
    const double* rowS = a.S + (int64_t)t_idx * a.ld;
    // :104-121.  No continuation at the list's last date nor at an index on the last column (k_branch_bounds): n_slices = 0
    const bool branch = n_slices > 0;
    const double* rowF = branch_row_f(a, t_idx, branch);
    const double dsc = a.disc[t_idx];
    const int64_t stride = (int64_t)gridDim.x * 256;
    int64_t p[BR_PPT];
    bool live[BR_PPT];
    double now[BR_PPT], sum[BR_PPT];
    br_v2d st[BR_PPT];
    uint32_t idx[BR_PPT][4 * QUADS];
#pragma unroll
    for (int q = 0; q < BR_PPT; ++q) {
        p[q] = p0 + (int64_t)blockIdx.x * 256 + threadIdx.x + q * stride;
        live[q] = p[q] < a.n;
        if (!live[q]) p[q] = a.n - 1;
        st[q] = first_date ? br_v2d{0.0, 0.0} : __builtin_nontemporal_load(reinterpret_cast<const br_v2d*>(state) + p[q]);
        now[q] = branch_now(a, rowS, dsc, p[q]);
        sum[q] = 0.0;
        if (branch) {  // (wave-uniform)
            const PhiloxLane rng = branch_rng(a, p[q]);
#pragma unroll
            for (int k = 0; k < QUADS; ++k) {
                const Philox4 w = philox4x32_10_lane(rng, (uint32_t)(e * QUADS + k), a.k0, a.k1);
                const uint32_t ws[4] = {w.w0, w.w1, w.w2, w.w3};
#pragma unroll
                for (int s = 0; s < 4; ++s) idx[q][4 * k + s] = 4 * k + s < a.num_branches ? branch_index(ws[s], n32) : 0xFFFFFFFFu;
            }
        }
    }
    for (int sl = 0; sl < n_slices; ++sl) {
        const uint32_t first = (uint32_t)sl << slice_shift;
#pragma unroll
        for (int q = 0; q < BR_PPT; ++q) {
#pragma unroll
            for (int b = 0; b < 4 * QUADS; ++b) {
                const bool in = (idx[q][b] >> slice_shift) == (uint32_t)sl;
                const double v = rowF[in ? idx[q][b] : first];
                sum[q] += in ? v : 0.0;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < BR_PPT; ++q) {
        if (!(st[q].x > 0.0) && now[q] > 0.0) st[q].x = now[q];  // :62-65, first positive discounted payoff
        double better = now[q];
        const double cont = sum[q] * inv_b;
        if (branch && cont > better) better = cont;
        if (better > st[q].y) st[q].y = better;
        if (live[q]) __builtin_nontemporal_store(st[q], reinterpret_cast<br_v2d*>(state) + p[q]);
    }
}

// ONE EXERCISE DATE per launch, rows of MANY slices (round 5; beyond four slices = more than a million paths): the walk
// over the slices with every index tested in every pass costs a load instruction per index and pass however few lanes
// take part (4M x 50, 16 slices: 44.7 ms that way, 29.6 in one launch with 8 slices).  Here every thread SORTS its
// 4 QUADS PPT indices by slice first -- a counting sort into its own column of an LDS array (bins[pos][thread]: no two
// threads share an entry, no atomics, no barrier), the sixteen counters packed six bits each into two 64-bit registers
// -- and then walks the slices in order, gathering from its bin exactly the indices that fall into the slice: a pass costs
// as many load instructions as the fullest bin among the wave's lanes (~9 of 40 entries at sixteen slices) instead of 40,
// and every lane of the device is still in the same slice or two of the row at a time.  The owner of a gathered value (which
// of the thread's four paths) rides in the top two bits of the stored index -- rows of up to 2^30 - 2 paths -- and the value
// is added to that path's sum in the thread's own LDS cell (ds_add_f64 on a private address: program order, deterministic;
// selecting among PPT register sums costs four compare-select-add groups per gathered value instead).
// The sum over a path's branches is formed in slice order -- like k_branch_bounds / k_branch_date, not in branch order.
// What bounds this kernel is how many paths are RESIDENT at a time: every generation of resident workgroups pulls every slice
// of the row into the L2 of every XCD once (4M x 50: 32 MB x 8 XCDs per generation and date), so the bins hold the
// num_branches indices a path really has (dynamic LDS, 40 B per path at the driver's 10 branches + 8 B of sum), four paths
// per thread: 48 KiB per workgroup, three per CU, 786 432 paths per generation (three paths per thread: 38 KiB, 589 824).
// Three or four paths per thread (run_branching picks per shape: the generation whose LAST launch is fuller -- a nearly
// empty generation still pulls the whole row through every L2).
inline size_t brb_lds_bytes(int num_branches, int ppt) { return (size_t)256 * ((size_t)num_branches * ppt * sizeof(uint32_t) + 4 * sizeof(double)); }
template <int QUADS, int PPT>
__global__ __launch_bounds__(256, 3) void k_branch_date_binned(BranchArgs a, int64_t p0, int e, double2* state, int first_date,
                                                               int slice_shift, int n_slices) {
    static_assert(12 * PPT <= 63 && PPT <= 4, "bin positions are six-bit fields; the owner is two bits");
    extern __shared__ double brb_lds[];
    double (*sums)[256] = reinterpret_cast<double (*)[256]>(brb_lds);                // [owner][thread]
    uint32_t (*bins)[256] = reinterpret_cast<uint32_t (*)[256]>(brb_lds + 4 * 256);  // [pos][thread], pos < num_branches PPT
    // The lane's paths and branch_draw WRITTEN OUT, a path at a time: on a shared per-date frame and on branch_draw this kernel came out
    // 0.7-0.8 % slower (1.3M x 50: 4.30 -> 4.34 ms); as it stands only its last block (the bounds rule and the store) differs from the parent commit's instructions.
    const uint32_t n32 = (uint32_t)a.n;
    const double inv_b = 1.0 / (double)a.num_branches;
    const int t_idx = a.ex[e];
    const double* rowS = a.S + (int64_t)t_idx * a.ld;
    const bool branch = n_slices > 0;  // (no continuation at the list's last date nor at an index on the last column)
    const double* rowF = branch_row_f(a, t_idx, branch);
    const double dsc = a.disc[t_idx];
    const int64_t stride = (int64_t)gridDim.x * 256;
    const unsigned tid = threadIdx.x;
    int64_t p[PPT];
    bool live[PPT];
    double now[PPT];
    br_v2d st[PPT];
    // six-bit fields: slices 0..9 in lo, 10..15 in hi
    uint64_t f_lo = 0, f_hi = 0;
    auto field_shift = [](uint32_t sl) { return 6u * (sl >= 10u ? sl - 10u : sl); };
    auto bump = [&](uint32_t sl) -> uint32_t {  // returns the field's value, then adds one to it
        const bool up = sl >= 10u;
        const uint32_t sh = field_shift(sl);
        const uint32_t old = (uint32_t)((up ? f_hi : f_lo) >> sh) & 63u;
        const uint64_t one = 1ull << sh;
        f_lo += up ? 0ull : one;
        f_hi += up ? one : 0ull;
        return old;
    };
    uint32_t idx[PPT][4 * QUADS];
#pragma unroll
    for (int q = 0; q < 4; ++q) sums[q][tid] = 0.0;
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        p[q] = p0 + (int64_t)blockIdx.x * 256 + threadIdx.x + q * stride;
        live[q] = p[q] < a.n;
        if (!live[q]) p[q] = a.n - 1;
        st[q] = branch_state_load(state, first_date, p[q]);
        now[q] = branch_now(a, rowS, dsc, p[q]);
        if (branch) {  // (wave-uniform) the draws of branching_device.hpp's contract
            const PhiloxLane rng = branch_rng(a, p[q]);
#pragma unroll
            for (int k = 0; k < QUADS; ++k) {
                const Philox4 w = philox4x32_10_lane(rng, (uint32_t)(e * QUADS + k), a.k0, a.k1);
                const uint32_t ws[4] = {w.w0, w.w1, w.w2, w.w3};
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    idx[q][4 * k + s] = branch_index(ws[s], n32);
                    if (4 * k + s < a.num_branches) (void)bump(idx[q][4 * k + s] >> slice_shift);  // count
                }
            }
        }
    }
    if (branch) {
        // counts -> first positions (exclusive prefix over the slices)
        {
            uint64_t o_lo = 0, o_hi = 0;
            uint32_t run = 0;
#pragma unroll
            for (uint32_t sl = 0; sl < 16u; ++sl) {
                const uint32_t sh = field_shift(sl);
                const uint32_t c = (uint32_t)((sl >= 10u ? f_hi : f_lo) >> sh) & 63u;
                if (sl >= 10u) o_hi |= (uint64_t)run << sh;
                else o_lo |= (uint64_t)run << sh;
                run += c;
            }
            f_lo = o_lo;
            f_hi = o_hi;
        }
        // place: afterwards every field holds the END of its slice's bin
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
#pragma unroll
            for (int b = 0; b < 4 * QUADS; ++b) {
                if (b < a.num_branches) {
                    const uint32_t pos = bump(idx[q][b] >> slice_shift);
                    bins[pos][tid] = idx[q][b] | ((uint32_t)q << 30);
                }
            }
        }
        // walk the slices; within a slice four entries of the bin per trip (all four loads in flight together).  One thread's
        // LDS accesses execute in program order: its reads of bins[] see its own writes, its adds to sums[] line up.
        uint32_t pos = 0;
#pragma unroll 1
        for (uint32_t sl = 0; sl < (uint32_t)n_slices; ++sl) {
            const uint32_t end = (uint32_t)((sl >= 10u ? f_hi : f_lo) >> field_shift(sl)) & 63u;
            while (__builtin_amdgcn_ballot_w64(pos < end) != 0ull) {
                uint32_t w[4];
                double v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) w[u] = pos + u < end ? bins[pos + u][tid] : 0xFFFFFFFFu;
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = w[u] != 0xFFFFFFFFu ? rowF[w[u] & 0x3FFFFFFFu] : 0.0;
#pragma unroll
                for (int u = 0; u < 4; ++u)  // (an empty entry adds 0.0 to the fourth path's cell)
                    __hip_atomic_fetch_add(&sums[w[u] >> 30][tid], v[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                pos = pos + 4u < end ? pos + 4u : end;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        branch_state_store(state, p[q], live[q], st[q], now[q], sums[q][tid] * inv_b, branch);
    }
}

// ---- XCD-AFFINE per-date gathers (round 6): rows of F beyond ~14 MB (more than 1.8M paths) ------------------
// The binned kernel above pulls every slice of the row through the L2 of every XCD once per generation of resident paths
// (4M x 50: 200 MB beyond L2 per launch, 53 % hits, profiles/r05_branching_binned_counters.json).  Here the row is dealt out to
// the XCDs in sixteen equal chunks: workgroup w (XCD w & 7 -- workgroups are handed to the XCDs round-robin) draws ALL the
// indices of its tile's paths and gathers ONLY those whose chunk belongs to its XCD, so an XCD's L2 only ever sees its eighth
// of the row (92 % hits at 4M paths: a 4 MB share in a 4 MB L2); every tile is worked on by eight workgroups, one per XCD,
// each leaving its partial sum per path in a cell of its own (cells[xcd][path]); k_branch_date_xcd_finish adds the eight
// cells in XCD order (deterministic: the same bits every run) and updates the bounds.  Costs: the Philox draws eight times
// over -- the gather kernel is VALU-bound, 0.83 busy --, 64 B of cells written and 64 + 40 B read per path and date.
// 4M x 50: 21.8 -> 15.1 ms, 3M x 50: 16.0 -> 11.1, 8M x 20: 21.4 -> 16.9, 2M x 50: 7.9 -> 7.5; 1.2M x 50 LOSES (4.19 -> 4.61:
// its row fits two L2s), hence the threshold (gpurun_out/r6o_branch_xcd.log; counters: profiles/r06_branching_xcd_counters.json).
// Tried on the way: the finishing pass folded into the next date's gather launch (an eighth of the tile per workgroup, first
// wave): 15.7 -> 17.1 ms, dropped; chunks of 2^13 / 2^15 / 2^18 paths taken from the INDEX instead of the word's top bits:
// 17.3 / 16.6 / 15.7 ms, and unbalanced whenever n is not a multiple of eight chunks (gpurun_out/r6n_branch_xcd.log).
constexpr int BRX_PPT = 2;

// bounds of path p after exercise date e: its eight cells added in XCD order (the same bits every run), then the bounds rule
__device__ __forceinline__ void brx_finish_path(const BranchArgs& a, int e, const double* cells, int64_t ldc, double2* state, int first_date,
                                                int branch, int64_t p) {
    const int t_idx = a.ex[e];
    const br_v2d st = branch_state_load(state, first_date, p);
    const double now = branch_now(a, a.S + (int64_t)t_idx * a.ld, a.disc[t_idx], p);
    double c = 0.0;
    if (branch) {
#pragma unroll
        for (int x = 0; x < 8; ++x) c += __builtin_nontemporal_load(cells + (int64_t)x * ldc + p);
    }
    branch_state_store(state, p, true, st, now, c * (1.0 / (double)a.num_branches), branch != 0);
}

// A tile = 512 paths; workgroup w works on tile w >> 3 for XCD w & 7.  Which XCD a draw belongs to is read off the TOP bits of its
// Philox word (index = umulhi(word, n): the word's top four bits cut the row into sixteen equal chunks, chunk c to XCD c & 7 --
// two chunks of n / 16 paths per XCD whatever n is), so a draw that is not this XCD's costs a bit-field extract, a compare and one
// add-with-carry into the thread's mask; the words go to LDS four at a time and only the few that are kept are turned into indices.
template <int QUADS>
__global__ __launch_bounds__(256) void k_branch_date_xcd(BranchArgs a, int e, double* cells, int64_t ldc) {
    // [Philox block of the thread][thread][word]: a thread only ever reads its own column (hipcc merges the four stores of a block
    // into one ds_write_b128, as many in the assembly as when a uint4 was stored: DESIGN.md section 8 f3)
    __shared__ __attribute__((aligned(16))) uint32_t buf[QUADS * BRX_PPT][256][4];
    constexpr int DRAWS = 4 * QUADS * BRX_PPT;
    const unsigned tid = threadIdx.x;
    const uint32_t xcd = blockIdx.x & 7u;
    const int64_t tile = (int64_t)(blockIdx.x >> 3);
    const uint32_t n32 = (uint32_t)a.n;
    const double* rowF = branch_row_f(a, a.ex[e], true);
    // draws that exist: branch b < num_branches of either path; draw i (in drawing order) sits at bit DRAWS - 1 - i of the mask
    uint32_t exists = 0;
#pragma unroll
    for (int i = 0; i < DRAWS; ++i) exists |= ((i % (4 * QUADS)) < a.num_branches ? 1u : 0u) << (DRAWS - 1 - i);
    uint32_t m = 0;
    int64_t p[BRX_PPT];
#pragma unroll
    for (int q = 0; q < BRX_PPT; ++q) {
        p[q] = tile * (256 * BRX_PPT) + tid + q * 256;
        const bool live = p[q] < a.n;
        const PhiloxLane rng = branch_rng(a, live ? p[q] : a.n - 1);
        branch_draw<QUADS>(rng, e, a.k0, a.k1, [&](int b, uint32_t word) {
            buf[q * QUADS + (b >> 2)][tid][b & 3] = word;
            m = m + m + ((((word >> 28) & 7u) == xcd && live) ? 1u : 0u);
        });
    }
    m &= exists;
    double sum[BRX_PPT];
#pragma unroll
    for (int q = 0; q < BRX_PPT; ++q) sum[q] = 0.0;
    auto word_of = [&](uint32_t bit) {  // the Philox word of the draw at mask bit `bit`
        const uint32_t i = (uint32_t)(DRAWS - 1) - bit;
        return buf[i >> 2][tid][i & 3u];
    };
    while (__builtin_amdgcn_ballot_w64(m != 0u) != 0ull) {  // two of the thread's own gathers per trip
        const bool h0 = m != 0u;
        const uint32_t b0 = h0 ? (uint32_t)__builtin_ctz(m) : 0u;
        m &= m - (h0 ? 1u : 0u);
        const bool h1 = m != 0u;
        const uint32_t b1 = h1 ? (uint32_t)__builtin_ctz(m) : 0u;
        m &= m - (h1 ? 1u : 0u);
        const uint32_t w0 = word_of(b0), w1 = word_of(b1);
        const double v0 = h0 ? rowF[branch_index(w0, n32)] : 0.0;
        const double v1 = h1 ? rowF[branch_index(w1, n32)] : 0.0;
        // (bits >= 4 QUADS belong to the thread's FIRST path: it was drawn first)
        if (b0 >= 4u * QUADS) sum[0] += v0;
        else sum[BRX_PPT - 1] += v0;
        if (b1 >= 4u * QUADS) sum[0] += v1;
        else sum[BRX_PPT - 1] += v1;
    }
#pragma unroll
    for (int q = 0; q < BRX_PPT; ++q)
        if (p[q] < a.n) __builtin_nontemporal_store(sum[q], cells + (int64_t)xcd * ldc + p[q]);
}

__global__ __launch_bounds__(256) void k_branch_date_xcd_finish(BranchArgs a, int e, const double* cells, int64_t ldc, double2* state, int first_date,
                                                                int branch) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < a.n; p += (int64_t)gridDim.x * 256)
        brx_finish_path(a, e, cells, ldc, state, first_date, branch, p);
}

// sum of {lower, upper} over the paths -> partials[grid][2]
__global__ __launch_bounds__(256) void k_branch_finish(const double2* state, int64_t n, double* partials) {
    __shared__ double red[2 * 4];
    double v[2] = {0.0, 0.0};
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const double2 st = state[p];
        v[0] += st.x;
        v[1] += st.y;
    }
    block_sum_store2(v, red, partials);
}

// any number of branches: the indices are used as they are drawn (no slices)
__global__ __launch_bounds__(256) void k_branch_bounds_any(BranchArgs a, int64_t p0, double* partials) {
    __shared__ double red[2 * 4];
    const bool call = a.is_call != 0;
    const uint32_t n32 = (uint32_t)a.n;
    const int quads = (a.num_branches + 3) >> 2;
    const double inv_b = a.num_branches > 0 ? 1.0 / (double)a.num_branches : 0.0;
    if (branch_empty_shard(a, partials)) return;
    BranchLane t;
    branch_lane_setup(t, a, p0);
    for (int e = 0; e < a.n_ex; ++e) {
        const int t_idx = a.ex[e];
        const double* rowS = a.S + (int64_t)t_idx * a.ld;
        const double dsc = a.disc[t_idx];
        const bool branch = date_branches(t_idx, a.ex_last, a.n_cols) && a.num_branches > 0;
        const double* rowF = branch_row_f(a, t_idx, branch);
#pragma unroll
        for (int q = 0; q < BR_PPT; ++q) {
            const double now = dsc * payoff_of(call, rowS[t.p[q]], a.K);
            double sum = 0.0;
            if (branch) {
                branch_draw(t.rng[q], e, quads, a.k0, a.k1, [&](int b, uint32_t word) {
                    if (b < a.num_branches) sum += rowF[branch_index(word, n32)];
                });
            }
            branch_update(t.lower[q], t.upper[q], now, sum * inv_b, branch);
        }
    }
    branch_lane_finish(t, red, partials);
}

// ---- the host side ---------------------------------------------------------------------------------------------------------
// Which kernels price a shard, and on what grid: computed once, from the shard's size and the branch count.
enum : int { BR_ROUTE_ONE_LAUNCH = 1, BR_ROUTE_PER_DATE = 2, BR_ROUTE_BINNED = 3, BR_ROUTE_XCD = 4 };  // (mcg_debug_branch_route's numbers)
struct BranchPlan {
    int route;
    int slice_shift, n_slices;       // the slices of a gathered row on that route (XCD: none, its chunks come off the Philox word)
    int quads, ppt;                  // Philox blocks per path and date; paths per thread
    int grid;                        // workgroups of a full launch
    int64_t per_launch, n_launches;  // paths a full launch covers; launches that cover the shard
    size_t lds_bytes;                // dynamic LDS per workgroup (the binned kernel's bins)
};
constexpr int64_t BRX_MIN_PATHS = (int64_t)7 << 18;  // 1.835M paths = rows of 14 MB: below, the binned kernel is at least as fast

static BranchPlan plan_branching(const mcg_ctx* ctx, int64_t n, int num_branches, bool have_dates) {
    BranchPlan pl{};
    pl.quads = (num_branches + 3) / 4;
    // slices of the gathered row: 2 MB each (mcg_debug_branch_route: another size to start from), at most `cap` of them -- then of
    // n / cap, rounded up to a power of two
    const int64_t last = (n > 0 ? n : 1) - 1;
    auto slices = [&](int cap) {
        pl.slice_shift = ctx->branch_shift ? ctx->branch_shift : BR_SLICE_SHIFT;
        while ((last >> pl.slice_shift) + 1 > cap) ++pl.slice_shift;
        pl.n_slices = (int)((last >> pl.slice_shift) + 1);
    };
    // What the per-date kernels need: indices kept in registers (up to twelve branches) and a date to launch for; the binned and
    // XCD kernels keep the owner of an index in its top two bits: rows of up to 2^30 - 2 paths.
    const bool dates_ok = pl.quads >= 1 && pl.quads <= 3 && have_dates;
    const bool bins_ok = dates_ok && n < ((int64_t)1 << 30) - 1;
    // Rows of more than four slices (more than a million paths): per-date launches of the BINNED kernel (k_branch_date_binned:
    // every thread walks its indices sorted by slice), sixteen slices of >= 2 MB; from BRX_MIN_PATHS on the XCD-affine gathers.
    // Rows of two to four slices: one launch per exercise date, bounds in `state`.  A/B on one board, 1M x 50: 5.55 ms
    // (one launch, no slices) -> 5.25 (one launch, slices: 42 % L2 hits) -> 2.83 (per-date launches).  A pass costs
    // ~40 cycles per wave-load however few lanes take part, so rows of many slices lose what the hits gain (4M x 50,
    // 16 slices: 44.7 ms per date-launches against 29.6 in one launch with 8 slices and 35.3 without): where the binned kernel
    // cannot run those keep the one-launch kernel.
    slices(16);
    const bool many = bins_ok && pl.n_slices > BR_DATE_MAX_SLICES;
    slices(BR_MAX_SLICES);
    pl.route = many ? (n >= BRX_MIN_PATHS ? BR_ROUTE_XCD : BR_ROUTE_BINNED)
                    : dates_ok && pl.n_slices > 1 && pl.n_slices <= BR_DATE_MAX_SLICES ? BR_ROUTE_PER_DATE : BR_ROUTE_ONE_LAUNCH;
    // a forced route, where it can run at all (the per-date kernels clamp dead lanes to path n - 1: never an empty shard)
    const int forced = ctx->branch_route;
    if (forced >= BR_ROUTE_ONE_LAUNCH && n >= 1 && dates_ok && (forced <= BR_ROUTE_PER_DATE || bins_ok)) pl.route = forced;

    int wgs_per_cu = BR_WGS_PER_CU;  // launches of one resident wave of workgroups: all of them walk a row's slices together
    pl.ppt = BR_PPT;
    if (pl.route == BR_ROUTE_BINNED) {
        slices(16);
        // Paths per thread: a generation is three resident workgroups per CU of 256 x PPT paths, and a launch that is nearly
        // empty still walks -- and pulls through every XCD's L2 -- the whole row.  A/B on one board (round 5): 4M x 50
        // 21.4 ms at three paths per thread (6.8 generations) against 23.4 at four (5.1); 2M x 50 8.76 against 8.12
        // (3.4 / 2.5 generations).  So: whichever leaves the fuller last generation.
        const double gen4 = (double)n / (double)((int64_t)ctx->n_cus * 3 * 256 * 4), gen3 = (double)n / (double)((int64_t)ctx->n_cus * 3 * 256 * 3);
        pl.ppt = std::ceil(gen3) - gen3 < std::ceil(gen4) - gen4 ? 3 : 4;
        pl.lds_bytes = brb_lds_bytes(num_branches, pl.ppt);  // <= 56 KiB (twelve branches, four paths); 48 KiB at the driver's ten
        wgs_per_cu = (int)std::min<size_t>(3, ((size_t)160 << 10) / pl.lds_bytes);
    }
    const int64_t per_wg = 256 * (int64_t)pl.ppt;
    pl.grid = (int)std::max<int64_t>(1, std::min<int64_t>((n + per_wg - 1) / per_wg, (int64_t)ctx->n_cus * wgs_per_cu));
    if (pl.route == BR_ROUTE_XCD) {  // one launch over every tile of 512 paths, eight workgroups a tile
        pl.slice_shift = pl.n_slices = 0;
        pl.ppt = BRX_PPT;
        pl.grid = (int)((n + 256 * BRX_PPT - 1) / (256 * BRX_PPT));
    }
    pl.per_launch = (int64_t)pl.grid * 256 * pl.ppt;
    pl.n_launches = std::max<int64_t>(1, (n + pl.per_launch - 1) / pl.per_launch);
    if (pl.route == BR_ROUTE_XCD) pl.grid *= 8;
    return pl;
}

int run_branching(mcg_ctx* ctx, const mcg_paths* P, double r, double K, double maturity, double dt, int is_call,
                  int num_branches, const int* exercise_times, int n_ex_in, uint64_t seed, double* price, double* lower,
                  double* upper) {
    const int n_cols = P->n_steps + 1;
    const int64_t n = P->n_paths;
    if (n >= (int64_t)0xFFFFFFFFLL) return fail(MCG_ERR_INVALID, "BranchingProcesses: too many paths in one shard");
    std::vector<double> disc((size_t)n_cols);
    int n_dates = 0;
    for (int j = 0; j < n_cols; ++j) {
        const double t = j * dt;
        if (!(t > maturity) && n_dates == j) n_dates = j + 1;
        disc[(size_t)j] = std::exp(-r * t);
    }
    std::vector<int> ex;
    for (int e = 0; e < n_ex_in; ++e) {
        const int t_idx = exercise_times[e];
        if (t_idx * dt > maturity) break;  // :57-59, :97-99 (tested before the column is touched, like the reference)
        if (t_idx < 0 || t_idx >= n_cols) return fail(MCG_ERR_INVALID, "BranchingProcesses: exercise time %d outside [0,%d)", t_idx, n_cols);
        ex.push_back(t_idx);
    }
    const int ex_last = exercise_times[n_ex_in - 1];  // exerciseTimes.back(), :104
    const int n_ex = (int)ex.size();

    const BranchPlan pl = plan_branching(ctx, n, num_branches, n_ex > 0);
    ctx->branch_last_route = pl.route;
    // the grid-stride kernels (k_branch_suffix, the XCD finishing pass, k_branch_finish, whose partials the per-date routes sum)
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)ctx->n_cus * 8));
    const int64_t n_partials = pl.route == BR_ROUTE_ONE_LAUNCH ? (int64_t)pl.grid * pl.n_launches : grid;
    int rc = ensure_cap(ctx, &ctx->partials, &ctx->partials_cap, (size_t)2 * (size_t)n_partials);
    if (rc) return rc;

    PoolLease lease(ctx);  // F; on the per-date routes the paths' states; on the XCD route the cells
    double s[3];           // {sum lower, sum upper, N}
    // Everything that is queued, up to the sums.  THE ONE WAY OUT is the lease's: from the first launch until the sums have been
    // synchronised it is `busy`, and whatever ends this function meanwhile -- an error code or an exception -- it waits for the stream
    // before it hands back a buffer that a queued kernel may still be writing.
    auto queue_and_sum = [&]() -> int {
        void *Fbuf = nullptr, *state = nullptr, *cells = nullptr;
        const int64_t ldc = (n + 511) / 512 * 512;
        int rc = lease.alloc(P->bytes, &Fbuf);
        if (!rc && pl.route != BR_ROUTE_ONE_LAUNCH) rc = lease.alloc((size_t)n * sizeof(double2), &state);
        if (!rc && pl.route == BR_ROUTE_XCD) rc = lease.alloc((size_t)8 * ldc * sizeof(double), &cells);
        if (rc) return rc;
        HostPiece par[] = {{disc.data(), (size_t)n_cols * sizeof(double)}, {ex.data(), ex.size() * sizeof(int)}};
        rc = upload_params(ctx, par);
        // disc and ex die at return (upload_params)
        if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == MCG_OK) rc = fail(MCG_ERR_HIP, "BranchingProcesses: table upload failed");
        if (rc) return rc;
        lease.busy = true;
        {
            TimedLaunch t(ctx, MCG_K_BRANCHING);
            hipLaunchKernelGGL(k_branch_suffix, dim3(grid), dim3(256), 0, ctx->stream, P->data, (double*)Fbuf, P->ld, n, n_cols, n_dates,
                               par[0].at, K, is_call);
        }
        BranchArgs a;
        a.S = P->data;
        a.F = (const double*)Fbuf;
        a.ld = P->ld;
        a.n = n;
        a.path_begin = P->path_begin;
        a.k0 = (uint32_t)seed;
        a.k1 = (uint32_t)(seed >> 32);
        a.ex = reinterpret_cast<const int*>(par[1].at);
        a.disc = par[0].at;
        a.n_ex = n_ex;
        a.ex_last = ex_last;
        a.n_cols = n_cols;
        a.num_branches = num_branches;
        a.K = K;
        a.is_call = is_call;

        typedef void (*BoundsKernel)(BranchArgs, int64_t, double*, int, int);
        typedef void (*DateKernel)(BranchArgs, int64_t, int, double2*, int, int, int);
        typedef void (*XcdKernel)(BranchArgs, int, double*, int64_t);
        static const BoundsKernel bounds_kernel[3] = {k_branch_bounds<1>, k_branch_bounds<2>, k_branch_bounds<3>};
        static const DateKernel date_kernel[3] = {k_branch_date<1>, k_branch_date<2>, k_branch_date<3>};
        static const DateKernel binned_kernel[3][2] = {{k_branch_date_binned<1, 3>, k_branch_date_binned<1, 4>},
                                                       {k_branch_date_binned<2, 3>, k_branch_date_binned<2, 4>},
                                                       {k_branch_date_binned<3, 3>, k_branch_date_binned<3, 4>}};
        static const XcdKernel xcd_kernel[3] = {k_branch_date_xcd<1>, k_branch_date_xcd<2>, k_branch_date_xcd<3>};
        // The per-date routes: for every exercise date the route's launches over the paths -- launch(e, p0, workgroups, branch), `per`
        // kernels each; the last launch's grid covers the paths that are left (a workgroup without a live path would still draw,
        // sort and gather for the clamped ones) --, then the sums of the states.  One event pair around the whole sequence.
        auto per_date = [&](int per, auto&& launch) {
            TimedLaunch t(ctx, MCG_K_BRANCHING, (int64_t)n_ex * per * pl.n_launches + 1);
            const int64_t per_wg = 256 * (int64_t)pl.ppt;
            for (int e = 0; e < n_ex; ++e) {
                const bool branch = date_branches(ex[(size_t)e], ex_last, n_cols);
                for (int64_t l = 0; l < pl.n_launches; ++l) {
                    const int64_t left = n - l * pl.per_launch;
                    launch(e, l * pl.per_launch, (unsigned)std::min<int64_t>(pl.grid, (left + per_wg - 1) / per_wg), branch);
                }
            }
            hipLaunchKernelGGL(k_branch_finish, dim3(grid), dim3(256), 0, ctx->stream, (const double2*)state, n, ctx->partials);
        };
        if (pl.route == BR_ROUTE_XCD) {  // a gather launch where the date branches (all the tiles: pl.grid) and a finishing pass
            per_date(2, [&](int e, int64_t, unsigned, bool branch) {
                if (branch) hipLaunchKernelGGL(xcd_kernel[pl.quads - 1], dim3((unsigned)pl.grid), dim3(256), 0, ctx->stream, a, e, (double*)cells, ldc);
                hipLaunchKernelGGL(k_branch_date_xcd_finish, dim3(grid), dim3(256), 0, ctx->stream, a, e, (const double*)cells, ldc, (double2*)state,
                                   e == 0, branch ? 1 : 0);
            });
        } else if (pl.route != BR_ROUTE_ONE_LAUNCH) {
            const DateKernel k = pl.route == BR_ROUTE_BINNED ? binned_kernel[pl.quads - 1][pl.ppt - 3] : date_kernel[pl.quads - 1];
            if (pl.lds_bytes > ((size_t)48 << 10)) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes);
            per_date(1, [&](int e, int64_t p0, unsigned g, bool branch) {
                hipLaunchKernelGGL(k, dim3(g), dim3(256), pl.lds_bytes, ctx->stream, a, p0, e, (double2*)state, e == 0, pl.slice_shift,
                                   branch ? pl.n_slices : 0);
            });
        } else {
            for (int64_t l = 0; l < pl.n_launches; ++l) {
                TimedLaunch t(ctx, MCG_K_BRANCHING);
                double* part = ctx->partials + 2 * l * pl.grid;
                const dim3 g(pl.grid), b(256);
                if (pl.quads <= 3) hipLaunchKernelGGL(bounds_kernel[std::max(pl.quads, 1) - 1], g, b, 0, ctx->stream, a, l * pl.per_launch, part, pl.slice_shift, pl.n_slices);
                else hipLaunchKernelGGL(k_branch_bounds_any, g, b, 0, ctx->stream, a, l * pl.per_launch, part);
            }
        }
        if (hipGetLastError() != hipSuccess) return fail(MCG_ERR_HIP, "BranchingProcesses: kernel launch failed");
        rc = finish_sums(ctx, n_partials, n, s);  // synchronises the stream
        if (!rc) lease.busy = false;
        return rc;
    };
    rc = queue_and_sum();
    if (rc) return rc;
    if (!(s[2] >= 1.0)) return fail(MCG_ERR_EMPTY_PATHS, "BranchingProcesses: Empty pricePaths.");
    const double lo = s[0] / s[2], up = s[1] / s[2];
    if (lower) *lower = lo;
    if (upper) *upper = up;
    *price = 0.5 * (lo + up);  // :37
    return MCG_OK;
}

}  // namespace mcg
