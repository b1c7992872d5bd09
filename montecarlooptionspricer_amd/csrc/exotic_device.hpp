// The payoff of one mcg_exotic contract on a path's five statistics: shared by the book kernels of kernels_exotic.hip and
// kernels_exotic_cv.hip.  Device-only code for gfx950.
#pragma once
#include "../../include/mcgpu.h"
#include "devmath.hpp"

namespace mcg {

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
