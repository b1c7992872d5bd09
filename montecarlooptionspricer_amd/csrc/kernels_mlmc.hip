// Multilevel Monte Carlo for local volatility (include/mcgpu.h: mcg_mlmc_localvol_level, mcg_mlmc_localvol_level_ex).
//
// k_mlmc_localvol_level<COARSE, ONE_SLICE, MILSTEIN, NL>   one level of the estimator in one launch, on the generators' skeleton of
//                    paths_device.hpp (two adjacent paths per lane, fm::Tables in LDS, walk_blocks over the FINE steps): the fine
//                    path is mcg_paths_localvol's at (T / n_fine, n_fine), step for step (localvol_step, draw n of stream 0); the
//                    coarse path runs on n_fine / 2 steps of twice the length from the same Brownian path -- its draw k is
//                    (z_2k + z_2k+1) sqrt(1/2), one addition and one multiplication, and it steps behind fine step 2k + 1.  A
//                    Philox block feeds four fine steps and two coarse ones; each normal_pairs call yields one coarse draw.  Both
//                    paths are reduced to the five statistics of mcg_path_stats in registers (as k_gbm_twin_stats does): no
//                    matrix is stored, 80 B a path are written (40 without a coarse path), nothing is read but the tables.
//                    The slices: ONE_SLICE stages the fine and the coarse slice once behind the tables; otherwise the slices of
//                    the NEXT Philox block (four fine, two coarse) are fetched at the top of a block and land in the other
//                    staging buffer at its end, one barrier per block, exactly k_localvol_paths' scheme (kernels_localvol.hip
//                    says why the LDS wait in front of that barrier is written out).
//                    Issue-bound on the VALU like the generators' loops: per 8 fine path-steps (one Philox block of a lane) two
//                    Philox blocks, two Box-Muller pairs, 8 + 4 surface steps with their exponentials.
//                    MILSTEIN adds the correction of localvol_step_vol to both grids' steps (three FMAs and a select a step).
//                    NL in {0, 1, 2, 4}: the Brownian-bridge survival probability of NL barrier levels along both grids, in
//                    registers (per path, grid and level the distance d to the level at the last row and the running product;
//                    per path and grid the extremes of X for the safe test): X and the step volatility are at hand, so a step
//                    costs one fp64 division a path and grid, and per level a subtraction, three multiplies and -- unless every
//                    lane of the wave is at or below ML_SKIP -- an exponential; a coarse step two of each, through its midpoint.
//                    <.., false, 0> is the kernel of mcg_mlmc_localvol_level, instruction for instruction.
// k_mlmc_book        the book on the statistics: per contract {sum Y, sum Y^2, sum P_f, sum P_f^2, sum P_c, sum P_c^2}, Y = P_f -
//                    P_c, four contracts (24 accumulators) a workgroup on blockIdx.y, on book_partials, then
//                    k_book_reduce<ML_CH, ML_NS> in a fixed order (both exotic_device.hpp's).  No float atomics.
// k_mlmc_book_bridge  the same with a slot per contract: a barrier contract takes bridge_payoff on its level's P_f and P_c.
// The host arithmetic on the sums (mcg_mlmc_combine, mcg_mlmc_plan) and what a level's shape must satisfy are host/mlmc.cpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>

#include "devmath.hpp"
#include "exotic_device.hpp"
#include "fastmath.hpp"
#include "localvol_device.hpp"
#include "../host/mlmc.hpp"
#include "paths_host.hpp"
#include "paths_device.hpp"

namespace mcg {

constexpr int ML_PPL = 2;                            // paths per lane
constexpr int ML_SLICE_MAX = LOCALVOL_MAX_NX - 1;    // entries of a slice
constexpr int ML_FINE_STAGE = 4 * ML_SLICE_MAX;      // a staging buffer: the four fine slices of a Philox block ...
constexpr int ML_FINE_PER_LANE = (ML_FINE_STAGE + 255) / 256;
constexpr int ML_COARSE_STAGE = 2 * ML_SLICE_MAX;    // ... and behind them its two coarse ones: at most one entry a lane
static_assert(ML_COARSE_STAGE <= 256, "the coarse slices of a block are staged with one entry a lane");
constexpr int ML_Q = 5;                              // statistics per path and grid: 0 S_T, 1 A, 2 G, 3 min, 4 max
constexpr int ML_CH = 4;                             // contracts one workgroup of k_mlmc_book keeps in registers
constexpr int ML_NS = 6;                             // sums per contract
constexpr int ML_NF = ML_CH * ML_NS;
constexpr double ML_SQRT_HALF = 0x1.6a09e667f3bcdp-1;  // sqrt(0.5) in binary64
constexpr int ML_L_MAX = MCG_MLMC_BRIDGE_L_MAX;      // bridge levels a launch keeps in registers
// x <= ML_SKIP: exp(x) < 2^-54, so 1 - exp(x) rounds to 1.0 and the factor changes no bit of the product (k_bridge_survival's rule)
constexpr double ML_SKIP = -38.0;
constexpr double ML_FLOOR = -64.0;

struct MlmcArgs {
    LocalVolArgs f;         // the fine grid as k_localvol_paths takes it: n_steps = n_fine, m = (r - q) dt_f, surf = its table
    double m_c;             // (r - q) dt_c
    const double2* surf_c;  // [n_slices_c][nx1] the coarse table
    double* stats;          // [10 or 5][n_paths]
    int stride_f, stride_c; // a grid's monitored rows: the multiples of its stride
    int first_obs;          // 0: row 0 (S0) is monitored too
    double nd_f, nd_c;      // monitored rows per grid
};
// ... and the bridge levels of the instances with NL > 0 (the others take MlmcArgs as it was: their kernel arguments, too, are
// those of mcg_mlmc_localvol_level's kernel): slot l < n_live is written, the slots behind repeat the last live one
struct MlmcBridgeArgs : MlmcArgs {
    double h[ML_L_MAX];     // ln(B / S0), formed on the host in binary64
    unsigned up_mask;       // bit l: slot l is an up level
    int n_live;
    double* surv;           // [(1 or 2) n_live][n_paths]: the fine grid's levels, then the coarse one's
};
template <int NL>
using MlmcArgsOf = std::conditional_t<NL == 0, MlmcArgs, MlmcBridgeArgs>;

// One grid's path pair: the state of the step and the running statistics; `left`: rows until the next monitored one (wave-uniform)
struct MlmcGrid {
    double S[ML_PPL], X[ML_PPL], sumS[ML_PPL], sumX[ML_PPL], mn[ML_PPL], mx[ML_PPL];
    int left;
};

// One grid's survival state for NL levels: d at the last row and the running product per path and level, and the extremes of
// X over the rows so far (row 0: X = 0; a coarse midpoint is a row).  Untouched, and so no register, where NL = 0.
template <int NL>
struct MlmcSurvival {
    double dprev[ML_PPL][NL ? NL : 1], prod[ML_PPL][NL ? NL : 1], lo[ML_PPL], hi[ML_PPL];
};

// The sub-interval that ends in the row x of both paths, c = -2 / w: bridge_row's arithmetic (kernels_barrier_bridge.hip) on X
// itself, no logarithm.  The exponent is held at ML_FLOOR from below, where the factor is 1.0 as everywhere below ML_SKIP: w = 0
// gives c = -inf and an exponent of -inf or NaN, both end there (fmax returns its other operand for a NaN) -- factor 1, as
// the contract says, with no flag kept.  The exponentials are exp_full2's: the polynomial of the step's scaled_exp, whose
// constants the loop already holds in scalar registers.
template <int NL>
__device__ __forceinline__ void mlmc_bridge_row(const MlmcBridgeArgs& g, const double (&x)[ML_PPL], const double (&c)[ML_PPL],
                                                MlmcSurvival<NL>& V) {
#pragma unroll
    for (int p = 0; p < ML_PPL; ++p) {
        V.lo[p] = __builtin_fmin(V.lo[p], x[p]);
        V.hi[p] = __builtin_fmax(V.hi[p], x[p]);
    }
#pragma unroll
    for (int q = 0; q < NL; ++q) {
        double t[ML_PPL];
        bool live = false;
#pragma unroll
        for (int p = 0; p < ML_PPL; ++p) {
            const double d = x[p] - g.h[q];
            const double m = __builtin_fmax(V.dprev[p][q] * d, 0.0);
            t[p] = __builtin_fmax(m * c[p], ML_FLOOR);
            V.dprev[p][q] = d;
            live = live || t[p] > ML_SKIP;
        }
        if (__builtin_amdgcn_ballot_w64(live) != 0ull) {  // (wave-uniform)
            static_assert(ML_PPL == 2, "one exp_full2 a level");
            double e[ML_PPL];
            fm::exp_full2(t[0], t[1], e[0], e[1]);
#pragma unroll
            for (int p = 0; p < ML_PPL; ++p) V.prod[p][q] *= 1.0 - e[p];
        }
    }
}

template <bool COARSE, bool ONE_SLICE, bool MILSTEIN, int NL>
__global__ __launch_bounds__(256) void k_mlmc_localvol_level(MlmcArgsOf<NL> g) {
    constexpr int PPL = ML_PPL;
    constexpr bool PLAIN = !MILSTEIN && NL == 0;  // mcg_mlmc_localvol_level's kernel
    constexpr int STAGE = ML_FINE_STAGE + (COARSE ? ML_COARSE_STAGE : 0);
    __shared__ fm::Tables tabs;
    __shared__ double2 slices[ONE_SLICE ? (COARSE ? 2 : 1) * ML_SLICE_MAX : 2 * STAGE];
    fm::load_tables(&tabs, g.f.tabs);
    const fm::Tables* tab = &tabs;
    const LocalVolArgs& a = g.f;
    LocalVolArgs c = g.f;  // the coarse grid's step: the same lookup, its own drift
    c.m = g.m_c;
    const int nx1 = a.nx1;
    const int n_coarse = a.n_steps >> 1;
    // entries of the staging buffer of `block`: four fine slices and two coarse ones, fewer in the tail
    auto fine_count = [&](const uint32_t block) { return min(4, a.n_steps - (int)(block << 2)) * nx1; };
    auto coarse_count = [&](const uint32_t block) { return min(2, n_coarse - (int)(block << 1)) * nx1; };
    if (ONE_SLICE) {
        if ((int)threadIdx.x < nx1) {
            slices[threadIdx.x] = a.surf[threadIdx.x];
            if (COARSE) slices[ML_SLICE_MAX + threadIdx.x] = g.surf_c[threadIdx.x];
        }
    } else {
        const int cnt = fine_count(0);
#pragma unroll
        for (int k = 0; k < ML_FINE_PER_LANE; ++k) {
            const int e = (int)threadIdx.x + 256 * k;
            if (e < cnt) slices[e] = a.surf[e];
        }
        if (COARSE && (int)threadIdx.x < coarse_count(0)) slices[ML_FINE_STAGE + threadIdx.x] = g.surf_c[threadIdx.x];
    }
    __syncthreads();
    // Every lane walks through all blocks, so that the barriers match; a lane beyond the last path keeps its results to itself.
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PPL;  // first path of this lane
    const bool row0 = g.first_obs == 0;                                 // X_0 = 0, S_0 = S0 is monitored
    const double inf = std::numeric_limits<double>::infinity();
    MlmcGrid F, C;
    PhiloxLane rng[PPL];
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        F.S[p] = C.S[p] = a.S0;
        F.X[p] = C.X[p] = 0.0;
        F.sumS[p] = C.sumS[p] = row0 ? a.S0 : 0.0;
        F.sumX[p] = C.sumX[p] = 0.0;
        F.mn[p] = C.mn[p] = row0 ? a.S0 : inf;
        F.mx[p] = C.mx[p] = row0 ? a.S0 : -inf;
        rng[p] = philox_lane_setup(a.path_begin + (uint64_t)(i + p), STREAM_PRICE, a.k1);
    }
    F.left = g.stride_f;
    C.left = g.stride_c;
    MlmcSurvival<NL> VF, VC;
    if constexpr (NL > 0) {
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
            VF.lo[p] = VF.hi[p] = VC.lo[p] = VC.hi[p] = 0.0;
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                VF.dprev[p][q] = VC.dprev[p][q] = 0.0 - g.h[q];
                VF.prod[p][q] = VC.prod[p][q] = 1.0;
            }
        }
    }
    // behind a step of grid G: its new row is monitored where its index is a multiple of the stride
    auto watch = [&](MlmcGrid& G, const int stride) {
        if (--G.left == 0) {  // (wave-uniform)
            G.left = stride;
#pragma unroll
            for (int p = 0; p < PPL; ++p) {
                G.sumS[p] += G.S[p];
                G.sumX[p] += G.X[p];
                G.mn[p] = __builtin_fmin(G.mn[p], G.S[p]);
                G.mx[p] = __builtin_fmax(G.mx[p], G.S[p]);
            }
        }
    };
    uint32_t block = 0;  // the Philox block of the current four fine steps
    const double2* cur = slices;
    // Staging of the slices of block + 1 (multi-slice kernels), as in k_localvol_paths: fetch() issues the global loads, land()
    // writes them into the buffer the workgroup is not stepping through.  The barrier at the top of the next block orders
    // land() against that block's reads, and this block's reads against the land() of the block after.
    double2 held[ML_FINE_PER_LANE], held_c;
    auto fetch = [&]() {
        const int cnt = fine_count(block + 1);  // <= 0 behind the last block
        const double2* src = a.surf + (size_t)(block + 1) * 4 * nx1;
#pragma unroll
        for (int k = 0; k < ML_FINE_PER_LANE; ++k) {
            const int e = (int)threadIdx.x + 256 * k;
            double2 v = make_double2(0.0, 0.0);  // (every element assigned: a half-written array would live in a private segment)
            if (e < cnt) v = src[e];
            held[k] = v;
        }
        held_c = make_double2(0.0, 0.0);
        if (COARSE && (int)threadIdx.x < coarse_count(block + 1)) held_c = g.surf_c[(size_t)(block + 1) * 2 * nx1 + threadIdx.x];
    };
    auto land = [&]() {
        const int cnt = fine_count(block + 1);
        double2* dst = slices + ((block + 1) & 1u) * STAGE;
#pragma unroll
        for (int k = 0; k < ML_FINE_PER_LANE; ++k) {
            const int e = (int)threadIdx.x + 256 * k;
            if (e < cnt) dst[e] = held[k];
        }
        if (COARSE && (int)threadIdx.x < coarse_count(block + 1)) dst[ML_FINE_STAGE + threadIdx.x] = held_c;
    };
    // The barrier between two blocks.  The wait in front of it is written out: the land() of the block before reaches this
    // barrier over the loop's back edge, and hipcc puts no wait for its LDS writes there (kernels_localvol.hip).
    auto stage_barrier = [&]() {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
    };
    Philox4 w[PPL];
    double za[PPL], zb[PPL];
    walk_blocks(
        a.n_steps, block,
        [&](auto whole) {  // the tail fetches nothing: no block follows it
            if (!ONE_SLICE) {
                if (block) stage_barrier();
                cur = slices + (block & 1u) * STAGE;
                if (whole) fetch();
            }
#pragma unroll
            for (int p = 0; p < PPL; ++p) w[p] = philox4x32_10_lane(rng[p], block, a.k0, a.k1);
            normal_pairs(w, false, tab, za, zb);
        },
        [&] { normal_pairs(w, true, tab, za, zb); },
        [&](auto elem) {
            constexpr int k = decltype(elem)::value;
            const double2* sl = ONE_SLICE ? cur : cur + k * nx1;
            if constexpr (PLAIN) {
#pragma unroll
                for (int p = 0; p < PPL; ++p) localvol_step(a, sl, (k & 1 ? zb : za)[p], F.S[p], F.X[p]);
            } else {  // the sub-interval (X_n, X_n+1) with w = s s
                double cw[PPL];
#pragma unroll
                for (int p = 0; p < PPL; ++p) {
                    const double s = localvol_step_vol<MILSTEIN>(a, sl, (k & 1 ? zb : za)[p], F.S[p], F.X[p]);
                    cw[p] = -2.0 / (s * s);
                }
                if constexpr (NL > 0) mlmc_bridge_row<NL>(g, F.X, cw, VF);
            }
            watch(F, g.stride_f);
            if constexpr (COARSE && (k & 1) != 0) {  // fine steps 2j and 2j + 1 are done: coarse step j on the sum of their draws
                const double2* sc = ONE_SLICE ? slices + ML_SLICE_MAX : cur + ML_FINE_STAGE + (k >> 1) * nx1;
                if constexpr (PLAIN) {
#pragma unroll
                    for (int p = 0; p < PPL; ++p) {
                        const double zc = (za[p] + zb[p]) * ML_SQRT_HALF;
                        localvol_step(c, sc, zc, C.S[p], C.X[p]);
                    }
                } else {  // through the midpoint, drawn from the difference of the two draws: (X_k, xm) and (xm, X_k+1), w = s s / 2 each
                    double cw[PPL], xm[PPL];
#pragma unroll
                    for (int p = 0; p < PPL; ++p) {
                        const double zc = (za[p] + zb[p]) * ML_SQRT_HALF, x0 = C.X[p];
                        const double s = localvol_step_vol<MILSTEIN>(c, sc, zc, C.S[p], C.X[p]);
                        xm[p] = __builtin_fma(0.5 * s, (za[p] - zb[p]) * ML_SQRT_HALF, 0.5 * (x0 + C.X[p]));
                        cw[p] = -2.0 / (0.5 * (s * s));
                    }
                    if constexpr (NL > 0) {
                        mlmc_bridge_row<NL>(g, xm, cw, VC);
                        mlmc_bridge_row<NL>(g, C.X, cw, VC);
                    }
                }
                watch(C, g.stride_c);
            }
        },
        [&] {
            if (!ONE_SLICE) land();
        });
    const int64_t n = a.n_paths;
    auto finish = [&](const MlmcGrid& G, const double nd, double* out) {
        double gm[PPL];
        fm::exp_full2(G.sumX[0] / nd, G.sumX[1] / nd, gm[0], gm[1]);
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
            const int64_t col = i + p;
            if (col < n) {
                out[0 * n + col] = G.S[p];
                out[1 * n + col] = G.sumS[p] / nd;
                out[2 * n + col] = a.S0 * gm[p];
                out[3 * n + col] = G.mn[p];
                out[4 * n + col] = G.mx[p];
            }
        }
    };
    finish(F, g.nd_f, g.stats);
    if (COARSE) finish(C, g.nd_c, g.stats + ML_Q * n);
    if constexpr (NL > 0) {  // P = 0 where a row was unsafe: the extremes of X against h, the complement of d > 0 (d < 0) on every row
        auto survive = [&](const MlmcSurvival<NL>& V, double* out) {
#pragma unroll
            for (int p = 0; p < PPL; ++p) {
                const int64_t col = i + p;
#pragma unroll
                for (int q = 0; q < NL; ++q) {
                    const bool safe = ((g.up_mask >> q) & 1u) ? V.hi[p] < g.h[q] : V.lo[p] > g.h[q];
                    if (col < n && q < g.n_live) out[(int64_t)q * n + col] = safe ? V.prod[p][q] : 0.0;
                }
            }
        };
        survive(VF, g.surv);
        if (COARSE) survive(VC, g.surv + (int64_t)g.n_live * n);
    }
}

// blockIdx.y: a chunk of ML_CH contracts; blockIdx.x strides over the paths.  stats: [10][n] with a coarse path, else [5][n].
// partials[(chunk * gridDim.x + blockIdx.x) * ML_NF + ML_NS * q + k]: sum k of the chunk's contract q
__global__ __launch_bounds__(256) void k_mlmc_book(const double* stats, int64_t n, int has_coarse, const mcg_exotic* book, int n_contracts,
                                                   double* partials) {
    __shared__ double red[ML_NF * 4];
    const int c0 = blockIdx.y * ML_CH;
    const int live = min(ML_CH, n_contracts - c0);
    book_partials<ML_NF>(n, red, partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * ML_NF, [&](int64_t i, double (&e)[ML_NF]) {
        const double st = stats[i], A = stats[n + i], G = stats[2 * n + i], mn = stats[3 * n + i], mx = stats[4 * n + i];
        double cst = 0.0, cA = 0.0, cG = 0.0, cmn = 0.0, cmx = 0.0;
        if (has_coarse) {
            const double* cs = stats + ML_Q * n;
            cst = cs[i];
            cA = cs[n + i];
            cG = cs[2 * n + i];
            cmn = cs[3 * n + i];
            cmx = cs[4 * n + i];
        }
#pragma unroll
        for (int q = 0; q < ML_CH; ++q) {
            if (q < live) {
                const double pf = exotic_payoff(book[c0 + q], st, A, G, mn, mx);
                const double pc = has_coarse ? exotic_payoff(book[c0 + q], cst, cA, cG, cmn, cmx) : 0.0;
                const double y = pf - pc;
                double* s = e + ML_NS * q;
                s[0] += y;
                s[1] = fma(y, y, s[1]);
                s[2] += pf;
                s[3] = fma(pf, pf, s[3]);
                s[4] += pc;
                s[5] = fma(pc, pc, s[5]);
            }
        }
    });
}

// k_mlmc_book with bridge levels.  slot[c] >= 0: a barrier contract on level slot[c], surv[(grid * n_live + slot) * n + i] its
// P (bridge_payoff); MLMC_SLOT_UNTOUCHED: a barrier never touched, P = 1; MLMC_SLOT_NONE: another kind, as k_mlmc_book.
__global__ __launch_bounds__(256) void k_mlmc_book_bridge(const double* stats, const double* surv, int n_live, int64_t n, int has_coarse,
                                                          const mcg_exotic* book, const int* slot, int n_contracts, double* partials) {
    __shared__ double red[ML_NF * 4];
    const int c0 = blockIdx.y * ML_CH;
    const int live = min(ML_CH, n_contracts - c0);
    book_partials<ML_NF>(n, red, partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * ML_NF, [&](int64_t i, double (&e)[ML_NF]) {
        const double st = stats[i], A = stats[n + i], G = stats[2 * n + i], mn = stats[3 * n + i], mx = stats[4 * n + i];
        double cst = 0.0, cA = 0.0, cG = 0.0, cmn = 0.0, cmx = 0.0;
        if (has_coarse) {
            const double* cs = stats + ML_Q * n;
            cst = cs[i];
            cA = cs[n + i];
            cG = cs[2 * n + i];
            cmn = cs[3 * n + i];
            cmx = cs[4 * n + i];
        }
#pragma unroll
        for (int q = 0; q < ML_CH; ++q) {
            if (q < live) {
                const mcg_exotic& x = book[c0 + q];
                const int sl = slot[c0 + q];
                double pf, pc = 0.0;
                if (sl == MLMC_SLOT_NONE) {
                    pf = exotic_payoff(x, st, A, G, mn, mx);
                    if (has_coarse) pc = exotic_payoff(x, cst, cA, cG, cmn, cmx);
                } else {
                    pf = bridge_payoff(x, st, sl < 0 ? 1.0 : surv[(int64_t)sl * n + i]);
                    if (has_coarse) pc = bridge_payoff(x, cst, sl < 0 ? 1.0 : surv[(int64_t)(n_live + sl) * n + i]);
                }
                const double y = pf - pc;
                double* s = e + ML_NS * q;
                s[0] += y;
                s[1] = fma(y, y, s[1]);
                s[2] += pf;
                s[3] = fma(pf, pf, s[3]);
                s[4] += pc;
                s[5] = fma(pc, pc, s[5]);
            }
        }
    });
}

// One level: the tables and the book go up, the level kernel fills the statistics, the book kernel and its reduction the sums.
// Workspace (one pool buffer): [10 n or 5 n statistics][(2 or 1) n_live n survival probabilities][n_chunks * n_blocks * ML_NF
// partials][6 n_contracts + 1 sums].  Parameters (ctx->weights): [fine table][coarse table][book][slots].  plan null: no
// bridge (k_mlmc_book); otherwise its levels are the kernel's slots, padded to 1, 2 or 4 with the last one.  On an error the stream is synchronised before the workspace
// goes back to the pool.
// The bridge levels of a call (host/mlmc.hpp: mlmc_bridge_plan)
struct MlmcBridgePlan {
    double barrier[ML_L_MAX];
    int up[ML_L_MAX];
    int n_levels;
    std::vector<int> slot;  // [n_contracts]
};

static int run_mlmc_level(mcg_ctx* ctx, double S0, double r, double q, const double* times, int n_t, double x_min, double x_max, int n_x,
                          const double* sigma, double T, const mcg_mlmc_level* lv, bool milstein, const MlmcBridgePlan* plan,
                          const mcg_exotic* book, int nc, double* sums, double* host_stats10, double* host_surv) {
    const int64_t n = lv->n_paths;
    const bool coarse = lv->has_coarse != 0;
    const int n_fine = lv->n_fine, n_coarse = n_fine / 2;
    const double dt_f = T / (double)n_fine, dt_c = 2.0 * dt_f;
    const int64_t n_gen = launch_blocks(n, ML_PPL);
    if (n_gen < 0) return MCG_ERR_INVALID;
    const int slices_f = n_t == 1 ? 1 : n_fine, slices_c = !coarse ? 0 : n_t == 1 ? 1 : n_coarse;
    const size_t per_slice = (size_t)(n_x - 1) * 2;
    std::vector<double> tab_f(slices_f * per_slice), tab_c(slices_c * per_slice);
    localvol_fill_table(times, n_t, n_x, sigma, dt_f, n_fine, tab_f.data());
    if (coarse) localvol_fill_table(times, n_t, n_x, sigma, dt_c, n_coarse, tab_c.data());
    const LocalVolScalars sf = localvol_scalars(r, q, x_min, x_max, n_x, dt_f), sc = localvol_scalars(r, q, x_min, x_max, n_x, dt_c);

    const int n_q = coarse ? 2 * ML_Q : ML_Q;
    const int n_sums = ML_NS * nc + 1, n_chunks = (nc + ML_CH - 1) / ML_CH;
    const int n_blocks = book_blocks(ctx, n);
    const int n_live = plan ? plan->n_levels : 0;
    const size_t n_stats = (size_t)n_q * n, n_part = (size_t)n_chunks * n_blocks * ML_NF;
    const size_t n_surv = (size_t)(coarse ? 2 : 1) * n_live * n;
    const size_t ws_bytes = (n_stats + n_surv + n_part + n_sums) * sizeof(double);
    void* ws = nullptr;
    int rc = pool_alloc(ctx, ws_bytes, &ws);
    if (rc) return rc;
    double *d_stats = (double*)ws, *d_surv = d_stats + n_stats, *d_part = d_surv + n_surv, *d_sums = d_part + n_part;
    auto body = [&]() -> int {
        HostPiece up[] = {{tab_f.data(), tab_f.size() * sizeof(double)},
                          {tab_c.data(), tab_c.size() * sizeof(double)},
                          {book, (size_t)nc * sizeof(mcg_exotic)},
                          {plan ? plan->slot.data() : nullptr, plan ? (size_t)nc * sizeof(int) : 0}};
        int r2 = upload_params(ctx, up);
        if (r2) return r2;
        MlmcBridgeArgs g;
        std::memset(&g, 0, sizeof(g));
        g.f.n_paths = n;
        g.f.n_steps = n_fine;
        g.f.nx1 = n_x - 1;
        g.f.path_begin = lv->path_begin;
        g.f.k0 = (uint32_t)lv->seed;
        g.f.k1 = (uint32_t)(lv->seed >> 32);
        g.f.S0 = S0;
        g.f.inv_dx = sf.inv_dx;
        g.f.u0 = sf.u0;
        g.f.m = sf.m;
        g.f.u_max = (double)(n_x - 1);
        g.f.surf = (const double2*)up[0].at;
        g.f.tabs = (const double2*)ctx->log_tab;
        g.m_c = sc.m;
        g.surf_c = (const double2*)up[1].at;
        g.stats = d_stats;
        g.stride_f = lv->stride_fine;
        g.stride_c = coarse ? lv->stride_coarse : 1;
        g.first_obs = lv->first_obs;
        g.nd_f = (double)(n_fine / lv->stride_fine + 1 - lv->first_obs);
        g.nd_c = coarse ? (double)(n_coarse / lv->stride_coarse + 1 - lv->first_obs) : 1.0;
        for (int l = 0; l < ML_L_MAX && n_live; ++l) {
            const int src = std::min(l, n_live - 1);
            g.h[l] = std::log(plan->barrier[src] / S0);
            if (plan->up[src]) g.up_mask |= 1u << l;
        }
        g.n_live = n_live;
        g.surv = d_surv;
        const int nl = n_live <= 2 ? n_live : ML_L_MAX;  // 0, 1, 2 or 4 slots
        r2 = PathLaunch{ctx, n_gen}.run(MCG_K_LOCALVOL, [&] {
            dispatch_flags(
                [&](auto coarse_, auto one_slice, auto milstein_, auto hi, auto lo) {
                    constexpr int NL = hi.value ? (lo.value ? ML_L_MAX : 2) : (lo.value ? 1 : 0);
                    hipLaunchKernelGGL((k_mlmc_localvol_level<coarse_.value, one_slice.value, milstein_.value, NL>), dim3((unsigned)n_gen),
                                       dim3(256), 0, ctx->stream, static_cast<const MlmcArgsOf<NL>&>(g));
                },
                coarse, n_t == 1, milstein, nl >= 2, nl == 1 || nl == ML_L_MAX);
        });
        if (r2) return r2;
        {
            TimedLaunch t(ctx, MCG_K_EXOTIC, 2);
            if (plan)
                hipLaunchKernelGGL(k_mlmc_book_bridge, dim3(n_blocks, n_chunks), dim3(256), 0, ctx->stream, d_stats, d_surv, n_live, n,
                                   coarse ? 1 : 0, reinterpret_cast<const mcg_exotic*>(up[2].at), reinterpret_cast<const int*>(up[3].at), nc,
                                   d_part);
            else
                hipLaunchKernelGGL(k_mlmc_book, dim3(n_blocks, n_chunks), dim3(256), 0, ctx->stream, d_stats, n, coarse ? 1 : 0,
                                   reinterpret_cast<const mcg_exotic*>(up[2].at), nc, d_part);
            hipLaunchKernelGGL((k_book_reduce<ML_CH, ML_NS>), dim3(n_chunks), dim3(256), 0, ctx->stream, d_part, n_blocks, nc, (double)n, d_sums);
        }
        MCG_HIP(hipGetLastError());
        MCG_HIP(hipMemcpyAsync(sums, d_sums, n_sums * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (host_stats10) MCG_HIP(hipMemcpyAsync(host_stats10, d_stats, n_stats * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (host_surv && n_surv) MCG_HIP(hipMemcpyAsync(host_surv, d_surv, n_surv * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MCG_HIP(hipStreamSynchronize(ctx->stream));
        return MCG_OK;
    };
    rc = body();
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    pool_release(ctx, ws, ws_bytes);
    return rc;
}

}  // namespace mcg

using namespace mcg;

int mcg_mlmc_localvol_level_ex(mcg_ctx* ctx, double S0, double r, double q, const double* times, int n_t, double x_min, double x_max,
                               int n_x, const double* sigma, double T, const mcg_mlmc_level* lv, int scheme, int bridge,
                               const mcg_exotic* book, int n_contracts, double* sums, double* host_stats10, double* host_surv) {
    // (the model and the level are checked before the ctx: what is wrong with them is reported on a machine without a GPU too)
    if (!lv || !book || !sums) return fail(MCG_ERR_INVALID, "mlmc: lv/book/sums is NULL");
    int rc = mlmc_check_level(lv, T);
    if (rc) return rc;
    rc = localvol_check_surface(times, n_t, n_x, sigma, T / (double)lv->n_fine, lv->n_fine);
    if (rc) return rc;
    rc = localvol_check_model(S0, r, q, x_min, x_max, false, 0.0);
    if (rc) return rc;
    if (n_contracts < 1 || n_contracts > 1024) return fail(MCG_ERR_INVALID, "n_contracts must be in [1, 1024] (got %d)", n_contracts);
    for (int c = 0; c < n_contracts; ++c) {
        rc = exotic_contract_check(book[c], "contract", c);
        if (rc) return rc;
    }
    rc = mlmc_check_scheme(scheme, bridge);
    if (rc) return rc;
    MlmcBridgePlan plan;
    if (bridge) {
        plan.slot.resize((size_t)n_contracts);
        rc = mlmc_bridge_plan(book, n_contracts, plan.barrier, plan.up, plan.slot.data(), &plan.n_levels);
        if (rc) return rc;
    }
    if (lv->n_paths < 1) return fail(MCG_ERR_EMPTY_PATHS, "mlmc: no paths on this level");
    if (!ctx) return fail(MCG_ERR_INVALID, "ctx is NULL");
    MCG_HIP(hipSetDevice(ctx->device));
    return run_mlmc_level(ctx, S0, r, q, times, n_t, x_min, x_max, n_x, sigma, T, lv, scheme == MCG_MLMC_MILSTEIN, bridge ? &plan : nullptr,
                          book, n_contracts, sums, host_stats10, host_surv);
}

int mcg_mlmc_localvol_level(mcg_ctx* ctx, double S0, double r, double q, const double* times, int n_t, double x_min, double x_max,
                            int n_x, const double* sigma, double T, const mcg_mlmc_level* lv, const mcg_exotic* book, int n_contracts,
                            double* sums, double* host_stats10) {
    return mcg_mlmc_localvol_level_ex(ctx, S0, r, q, times, n_t, x_min, x_max, n_x, sigma, T, lv, MCG_MLMC_LOG_EULER, 0, book, n_contracts,
                                      sums, host_stats10, nullptr);
}
