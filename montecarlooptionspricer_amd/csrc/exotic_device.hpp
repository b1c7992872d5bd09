// The payoff of one mcg_exotic contract on a path's five statistics: shared by the book kernels of kernels_exotic.hip,
// kernels_exotic_cv.hip and kernels_exotic_greeks.hip; and the pieces of the streaming scan that reduces a path to its
// statistics.  Device-only code for gfx950.
#pragma once
#include "../../include/mcgpu.h"
#include "devmath.hpp"

namespace mcg {

// The pieces of a streaming scan of the matrix that k_path_stats (kernels_exotic.hip) and k_path_tangent_stats
// (kernels_exotic_greeks.hip) share: the rows of a group, the load of a lane's W adjacent paths, the mantissa split.
typedef double xs_d2 __attribute__((ext_vector_type(2)));

constexpr int XS_ROWS = 8;   // rows per unrolled group: 8 x 16 B in flight per lane, 32 KiB per workgroup
// The book layout k_exotic_book and k_bridge_book (kernels_barrier_bridge.hip) share, and k_exotic_reduce reads:
constexpr int XB_CH = 8;     // contracts one workgroup of a book kernel keeps in registers
constexpr int XB_NF = 2 * XB_CH;

template <int W>
__device__ __forceinline__ void xs_load(const double* p, double (&x)[W]) {
    if constexpr (W == 2) {
        const xs_d2 v = __builtin_nontemporal_load(reinterpret_cast<const xs_d2*>(p));
        x[0] = v.x;
        x[1] = v.y;
    } else {
        x[0] = __builtin_nontemporal_load(p);
    }
}

// x = m 2^k with m in [1, 2), for a positive normal x: returns m and adds k to e (three integer instructions, no log).
__device__ __forceinline__ double xs_split(double x, int& e) {
    const int hi = __double2hiint(x);
    e += ((hi >> 20) & 0x7ff) - 1023;
    return __hiloint2double((hi & 0x000fffff) | 0x3ff00000, __double2loint(x));
}

// The undiscounted payoffs of include/mcgpu.h, on one path's statistics.  Strike and barrier tests are plain comparisons
// of the stored doubles.
__device__ __forceinline__ double exotic_payoff(const mcg_exotic& c, double st, double A, double G, double mn, double mx) {
    const bool call = c.is_call != 0;
    switch (c.kind) {
        case MCG_X_ASIAN_ARITH_FIXED: return payoff_of(call, A, c.K);
        case MCG_X_ASIAN_ARITH_FLOAT: return payoff_of(call, st, A);
        case MCG_X_ASIAN_GEO_FIXED: return payoff_of(call, G, c.K);
        case MCG_X_ASIAN_GEO_FLOAT: return payoff_of(call, st, G);
        case MCG_X_LOOKBACK_FIXED: return call ? fmax(0.0, mx - c.K) : fmax(0.0, c.K - mn);
        case MCG_X_LOOKBACK_FLOAT: return call ? st - mn : mx - st;
        default: {
            const bool up = c.kind == MCG_X_BARRIER_UP_OUT || c.kind == MCG_X_BARRIER_UP_IN;
            const bool in = c.kind == MCG_X_BARRIER_UP_IN || c.kind == MCG_X_BARRIER_DOWN_IN;
            const bool hit = up ? mx >= c.barrier : mn <= c.barrier;
            return hit == in ? payoff_of(call, st, c.K) : c.rebate;
        }
    }
}

}  // namespace mcg
