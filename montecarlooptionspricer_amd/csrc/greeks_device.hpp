// The end of a Greeks kernel's workgroup, shared by kernels_greeks.hip and kernels_exotic_greeks.hip: the block's partial
// sums of its estimators and the range of row 0.  Device-only code for gfx950.
#pragma once
#include "devmath.hpp"

namespace mcg {

// Partials of one block: NE estimators {sum[0..NE), sum of squares[NE..2NE)}, then min and max of row 0 (NF = 2 NE + 2).
template <int NE>
__device__ __forceinline__ void greeks_block_store(double (&e)[2 * NE], double lo, double hi, double* red, double* out) {
    constexpr int NW = 4;
    __shared__ double mm[2 * NW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, o));
        hi = fmax(hi, __shfl_xor(hi, o));
    }
    if (lane == 0) {
        mm[wave] = lo;
        mm[NW + wave] = hi;
    }
    block_sum<2 * NE, NW>(e, red);  // (its barrier also publishes mm)
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 2 * NE; ++q) out[q] = e[q];
        for (int w = 1; w < NW; ++w) {
            lo = fmin(lo, mm[w]);
            hi = fmax(hi, mm[NW + w]);
        }
        out[2 * NE] = lo;
        out[2 * NE + 1] = hi;
    }
}

}  // namespace mcg
