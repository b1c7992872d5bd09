// The skeleton of the step-major path generators for gfx950 (the Heston family of heston_device.hpp, kernels_localvol.hip,
// kernels_gbm_multi.hip and the in-register twin of kernels_exotic_cv.hip): two adjacent paths per lane, fm::Tables in LDS,
// one Philox block per stream and four steps, a wave-uniform row pointer plus a constant lane offset.  This header states
// once
//   store_pair16      the 16-byte nontemporal row store with its two hazard guards
//   walk_blocks       the walk over whole Philox blocks and the tail of <= 3 steps
//   walk_bridge       the depth-first walk over a Brownian bridge of Sobol' dimensions (kernels_sobol.hip)
//   normal_pairs      Box-Muller on words 0/1 or 2/3 of the lane's Philox blocks
//   payoff_partials   the terminal-payoff sums of a fused (*_payoff) form
// and paths_host.hpp the host's share (grid and shape checks, the launch frame, uploads).  A generator supplies its argument
// struct, what it keeps in registers, and the hooks of walk_blocks: its draws and its step rule.
// (k_gbm_paths, the benchmark's generator, keeps its own loops and store: kernels_gbm.hip.)
#pragma once
#include <type_traits>

#include "devmath.hpp"
#include "fastmath.hpp"

namespace mcg {

// 16 bytes per lane at (wave-uniform row pointer) + (constant lane offset, bytes): hipcc picks the scalar-base form for the
// first store only and rebuilds a 64-bit vector address inside a loop, hence the explicit instruction.  An asm statement is
// opaque to hipcc's hazard handling, so both guards belong to the statement:
//   `s_nop 1` behind   on gfx940+ a store of more than 64 bits reads its data registers AFTER issue, and a VALU instruction
//                      that overwrites them within the next two wait states corrupts what is stored; the next step's FMA
//                      follows right behind (round 4 stored foreign words in matrix rows this way).
//   `s_nop 4` in front these kernels hold more scalars than there are registers, so hipcc keeps some in spare vector lanes,
//                      and where the row pointer is one of them its v_readlane lands right before the store: a VMEM
//                      instruction must not read an SGPR as its address within 5 wait states of a VALU write.
// tools/check_asm_hazards.py finds either pattern in the assembly.  Seven idle cycles per row against ~10^3 of arithmetic.
__device__ __forceinline__ void store_pair16(double* row, unsigned lane_bytes, double x0, double x1) {
    typedef double v2d __attribute__((ext_vector_type(2)));
    const v2d d = {x0, x1};
    asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 nt\n\ts_nop 1" : : "v"(lane_bytes), "v"(d), "s"(row) : "memory");
}

// Steps 0 .. n_steps - 1 in Philox blocks of four: the loop takes whole blocks, the tail the last <= 3 steps (wave-uniform
// throughout).  `block` is the caller's counter, so that the hooks see it; it starts at 0.  Per block, in this order:
//   begin(whole)  the block's draws and its first pair of normals; whole: std::true_type in the loop, std::false_type in the tail
//   step(k)       step 4 * block + k; k: std::integral_constant<int, 0..3>, a constant inside the hook
//   second()      the second pair of normals, between steps 1 and 2 (only where step 2 exists)
//   end()         behind step 3 of a whole block; nothing follows the tail
// Every lane that calls this walks through every block, whatever it does in the hooks: they may hold barriers.
template <class Begin, class Second, class Step, class End>
__device__ __forceinline__ void walk_blocks(const int n_steps, uint32_t& block, Begin&& begin, Second&& second, Step&& step, End&& end) {
    using std::integral_constant;
    const uint32_t n_blocks = (uint32_t)(n_steps >> 2);
#pragma unroll 1
    for (; block < n_blocks; ++block) {
        begin(std::true_type{});
        step(integral_constant<int, 0>{});
        step(integral_constant<int, 1>{});
        second();
        step(integral_constant<int, 2>{});
        step(integral_constant<int, 3>{});
        end();
    }
    const int rest = n_steps & 3;
    if (rest) {
        begin(std::false_type{});
        step(integral_constant<int, 0>{});
        if (rest >= 2) step(integral_constant<int, 1>{});
        if (rest == 3) {
            second();
            step(integral_constant<int, 2>{});
        }
    }
}

// The Brownian bridge of the Sobol' generators (include/mcgpu.h: mcg_sobol_bridge), walked depth first so that the unit
// intervals [t, t + 1] come out in time order.  The host flattens the walk into one BridgeOp per node, in the order of the
// walk (kernels_sobol.hip: bridge_program): the node's dimension, its weights, and where the values live.  Only the values
// of the current node's ancestors are live, one slot per tree level (slot 0 holds B(0) = 0, slot 1 the endpoint B(n), a node
// of depth k slot k + 2: BRIDGE_SLOTS of them for n <= 1024), kept in LDS because the slot is an index: each lane owns the
// double2 {path 0, path 1} at slots[slot * 256 + threadIdx.x] and no other lane reads it, so the walk holds no barrier.
struct BridgeOp {
    double wl, wr, sd;  // B(t) = wl B(l) + (wr B(r) + sd z)
    uint32_t dim_t;     // dimension | t << 16
    uint32_t slots;     // slot of l | slot of r << 4 | slot of t << 8 | emit << 12
                        //   emit bit 0: [t - 1, t] is a unit interval (l = t - 1), bit 1: so is [t, t + 1] (r = t + 1)
};
constexpr int BRIDGE_SLOTS = 12;
typedef const BridgeOp __attribute__((address_space(4))) * bridge_program;  // wave-uniform reads: scalar loads

// Per op, in this order:
//   draw(dim, z)   the two paths' normals of that dimension
//   step(t, dz)    step t (S_t -> S_{t+1}) with the increments dz = B(t + 1) - B(t), for each unit interval the node closes
// mine: this lane's double2 of slot 0.
template <class Draw, class Step>
__device__ __forceinline__ void walk_bridge(const int n_ops, bridge_program prog, double2* mine, Draw&& draw, Step&& step) {
    mine[0] = make_double2(0.0, 0.0);
#pragma unroll 1
    for (int k = 0; k < n_ops; ++k) {
        const double wl = prog[k].wl, wr = prog[k].wr, sd = prog[k].sd;
        const uint32_t dim_t = prog[k].dim_t, slots = prog[k].slots;
        double z[2];
        draw((int)(dim_t & 0xFFFFu), z);
        const double2 bl = mine[(slots & 15u) * 256u], br = mine[((slots >> 4) & 15u) * 256u];
        double2 b;
        b.x = __builtin_fma(wl, bl.x, __builtin_fma(wr, br.x, sd * z[0]));
        b.y = __builtin_fma(wl, bl.y, __builtin_fma(wr, br.y, sd * z[1]));
        mine[((slots >> 8) & 15u) * 256u] = b;
        const int t = (int)(dim_t >> 16);
        if (slots & (1u << 12)) {
            const double dz[2] = {b.x - bl.x, b.y - bl.y};
            step(t - 1, dz);
        }
        if (slots & (2u << 12)) {
            const double dz[2] = {br.x - b.x, br.y - b.y};
            step(t, dz);
        }
    }
}

// The normals of two steps of PPL paths from one stream's blocks w: words 0/1, or (second) words 2/3 (philox.hpp).
template <int PPL>
__device__ __forceinline__ void normal_pairs(const Philox4 (&w)[PPL], const bool second, const fm::Tables* tab, double (&za)[PPL],
                                             double (&zb)[PPL]) {
#pragma unroll
    for (int p = 0; p < PPL; ++p) fm::box_muller_pair(second ? w[p].w2 : w[p].w0, second ? w[p].w3 : w[p].w1, tab, za[p], zb[p]);
}

// {sum, sum of squares} of the (K, is_call) payoff of the terminal prices S of a workgroup of 256 lanes, into
// partials[2 * blockIdx.x ..]; i: the lane's first column, in_row: whether it lies inside the padded row.  Every lane of
// the workgroup calls this.
template <int PPL>
__device__ __forceinline__ void payoff_partials(const bool in_row, const int64_t i, const int64_t n_paths, const double (&S)[PPL],
                                                const double K, const int is_call, double* partials) {
    __shared__ double red[2 * 4];
    double acc[2] = {0.0, 0.0};
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        const double pay = (in_row && i + p < n_paths) ? payoff_of(is_call != 0, S[p], K) : 0.0;
        acc[0] += pay;
        acc[1] += pay * pay;
    }
    block_sum<2, 4>(acc, red);
    if (threadIdx.x == 0) {
        partials[2 * (int64_t)blockIdx.x] = acc[0];
        partials[2 * (int64_t)blockIdx.x + 1] = acc[1];
    }
}

}  // namespace mcg
