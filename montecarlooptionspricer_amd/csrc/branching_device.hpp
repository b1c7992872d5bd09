// The resampling draw of BranchingProcesses (BranchingProcessPricer.cpp:104-121), shared by the single-contract kernels
// (kernels_branching.hip) and the batched row kernel (k_batch_branching, kernels_batch.hip).
#pragma once
#include "devmath.hpp"

namespace mcg {

// THE RNG CONTRACT of the resampling (the test oracle's "philox" mode restates it: by it every route equals the oracle at 1e-12).
//   * a path draws from Philox stream STREAM_BRANCH of its own id (philox_lane_setup(path id, STREAM_BRANCH, k1));
//   * exercise date number e of the call's list (its position in the list, not its column) takes QUADS = ceil(num_branches / 4)
//     blocks, block k at counter e * QUADS + k;
//   * word s of block k is draw b = 4 k + s, and draw b exists iff b < num_branches;
//   * draw b resamples path branch_index(word, n) = floor(word n / 2^32), uniform on [0, n).
// What a consumer does with a word -- keep the index, count it into a bin, send it to LDS -- is its own.
enum : uint32_t { STREAM_BRANCH = 2u };

__device__ __forceinline__ uint32_t branch_index(uint32_t word, uint32_t n) { return __umulhi(word, n); }

// f(b, word) for the draws b = 0 .. 4 QUADS - 1 of (rng's path, date e), in drawing order (the consumer tests b < num_branches)
template <int QUADS, class F>
__device__ __forceinline__ void branch_draw(const PhiloxLane& rng, int e, uint32_t k0, uint32_t k1, F&& f) {
#pragma unroll
    for (int k = 0; k < QUADS; ++k) {
        const Philox4 w = philox4x32_10_lane(rng, (uint32_t)(e * QUADS + k), k0, k1);
        const uint32_t ws[4] = {w.w0, w.w1, w.w2, w.w3};
#pragma unroll
        for (int s = 0; s < 4; ++s) f(4 * k + s, ws[s]);
    }
}

// the same with the number of blocks known at run time only (more than twelve branches; the batched rows)
template <class F>
__device__ __forceinline__ void branch_draw(const PhiloxLane& rng, int e, int quads, uint32_t k0, uint32_t k1, F&& f) {
    for (int k = 0; k < quads; ++k) {
        const Philox4 w = philox4x32_10_lane(rng, (uint32_t)(e * quads + k), k0, k1);
        const uint32_t ws[4] = {w.w0, w.w1, w.w2, w.w3};
#pragma unroll
        for (int s = 0; s < 4; ++s) f(4 * k + s, ws[s]);
    }
}

}  // namespace mcg
