// The jump rule of the Bates and Merton paths for gfx950, as stated in include/mcgpu.h (mcg_paths_bates*): compound-Poisson
// log-normal jumps composed onto either variance scheme of heston_schemes.hpp as one more step rule.  kernels_bates.hip
// instantiates the kernel of heston_device.hpp with it and derives its constants; kernels_debug.hip runs its count and its
// jump size on words a test chooses (mcg_debug_eval_v fn 9).
//
// The jump of a step is independent of its diffusion, so the rule only adds J = comp + N mu_J + sigma_J sqrt(N) z3 to the
// exponent the base scheme hands to its one exponential; the variance never sees it.  Jumps are rare (lambda dt = 0.004 on
// daily steps at one jump a year), and what a wave does not need it skips on the scalar unit:
//   - the jump counts of a Philox block's four steps come from one stream-4 block, drawn in new_block() and counted in
//     count().  The Poisson thresholds rise, so threshold k + 1 is looked at only in a wave where some lane passed threshold k;
//   - the stream-5 block and its two Box-Muller pairs are computed only in a wave where some lane jumps somewhere in the
//     block, and a step adds the constant comp to every lane where none jumps in that step.
// Philox is counter-based: skipping changes no bit, and a path's result never depends on its neighbours.
//
// uN > c_k is decided on the word itself: uN = (w + 1/2) 2^-32 and c_k 2^32 - 1/2 is exact in binary64 (c_k <= 1 leaves
// twenty bits below the half), so uN > c_k <=> w > floor(c_k 2^32 - 1/2), the sixteen 32-bit thresholds of Consts::Rare::T.
#pragma once
#include "heston_schemes.hpp"

namespace mcg {

constexpr uint32_t STREAM_JUMP_COUNT = 4u, STREAM_JUMP_SIZE = 5u;
constexpr int JUMP_CAP = 16;  // thresholds c_0 .. c_15: with lambda dt <= 1 the count stays below it (1 - c_15 < 2^-33)

// The jump constants of include/mcgpu.h in binary64, on the host: comp = -lambda kbar dt and the sixteen thresholds
// T[k] = floor(min(c_k, 1) 2^32 - 1/2).  What launch_with_jumps puts into Consts, and what mcg_debug_bates_constants returns.
void bates_constants(double lambda, double mu_j, double sigma_j, double dt, uint32_t (&T)[JUMP_CAP], double& comp);

template <class Base>
struct WithJumps {
    static constexpr int PPL = HESTON_PPL;
    // What only a jumping wave reads stays in the kernel's argument block until then (rare()): held in scalar registers from
    // the start, as hipcc holds every kernel argument a loop reads, these eighteen words would push the polynomial constants of
    // the exponential and the logarithm out into vector lanes (the skeleton is short of scalar registers already).
    struct Rare {
        double mu_j, sigma_j;
        uint32_t T[JUMP_CAP];  // floor(c_k 2^32 - 1/2); the kernel reads k >= 2 here
    };
    struct Consts {
        typename Base::Consts base;
        double comp;           // -lambda kbar dt
        uint32_t T0, T1;       // T[0], T[1]
        Rare rare;
    };
    // a.c.rare, read where it is used: the empty asm keeps the loads behind it from being hoisted out of the step loop.
    // The address is that of the kernel's argument block plus the place of c.rare in HestonArgs, which is right as long as
    // HestonArgs is the first and only argument of the kernel (noted at the signatures of k_heston_paths and of
    // k_debug_bates_count).
    static __device__ __forceinline__ const Rare __attribute__((address_space(4))) * rare() {
        static_assert(std::is_standard_layout_v<HestonArgs<Consts>>, "offsetof below");
        typedef const char __attribute__((address_space(4))) * bytes;
        typedef const Rare __attribute__((address_space(4))) * ptr;
        ptr r = (ptr)((bytes)__builtin_amdgcn_kernarg_segment_ptr() + __builtin_offsetof(HestonArgs<Consts>, c) +
                      __builtin_offsetof(Consts, rare));
        asm volatile("" : "+s"(r));
        return r;
    }
    Base base;
    uint32_t cnt[PPL];         // the jump counts of the block's four steps, one byte each (element e: bits 8e .. 8e+7)
    double z3[PPL][4] = {};    // the block's stream-5 normals, where some lane of the wave jumps in the block
    // cnt[], zero on entry, from the block's stream-4 words: byte e of cnt[p] = #{k : word e of w[p] > T[k]}
    __device__ __forceinline__ void count(const Philox4 (&w)[PPL], const HestonArgs<Consts>& a) {
        uint32_t T[JUMP_CAP] = {a.c.T0, a.c.T1};
#pragma unroll
        for (int k = 0; k < JUMP_CAP; ++k) {
            if (k == 2 || k == 6) {  // two or six jumps in one step somewhere in the wave: the next thresholds, in two loads
                const auto r = rare();
#pragma unroll
                for (int j = k; j < (k == 2 ? 6 : JUMP_CAP); ++j) T[j] = r->T[j];
            }
            const uint32_t t = T[k];
            bool hit = false;
#pragma unroll
            for (int p = 0; p < PPL; ++p) {
                const bool g0 = w[p].w0 > t, g1 = w[p].w1 > t, g2 = w[p].w2 > t, g3 = w[p].w3 > t;
                cnt[p] += (g0 ? 1u : 0u) + (g1 ? 1u << 8 : 0u) + (g2 ? 1u << 16 : 0u) + (g3 ? 1u << 24 : 0u);
                hit = hit || g0 || g1 || g2 || g3;
            }
            if (__builtin_amdgcn_ballot_w64(hit) == 0ull) break;  // no lane of the wave has more than k jumps in any step
            asm volatile("" ::);  // keep this a real (scalar) branch
        }
    }
    __device__ __forceinline__ void new_block(const HestonArgs<Consts>& a, const int64_t i, const uint32_t block, const fm::Tables* tab) {
        base.new_block(a, i, block, tab);
        Philox4 w[PPL];
#pragma unroll
        for (int p = 0; p < PPL; ++p) {  // (the per-path part is set up here rather than held in registers, as for QE's stream 3)
            w[p] = philox4x32_10_lane(philox_lane_setup(a.path_begin + (uint64_t)(i + p), STREAM_JUMP_COUNT, a.k1), block, a.k0, a.k1);
            cnt[p] = 0u;
        }
        count(w, a);
        if (__builtin_amdgcn_ballot_w64((cnt[0] | cnt[1]) != 0u) != 0ull) {
            asm volatile("" ::);
#pragma unroll
            for (int p = 0; p < PPL; ++p) {
                const Philox4 s =
                    philox4x32_10_lane(philox_lane_setup(a.path_begin + (uint64_t)(i + p), STREAM_JUMP_SIZE, a.k1), block, a.k0, a.k1);
                fm::box_muller_pair(s.w0, s.w1, tab, z3[p][0], z3[p][1]);
                fm::box_muller_pair(s.w2, s.w3, tab, z3[p][2], z3[p][3]);
            }
        }
    }
    // J[] of step `elem` of the block, from cnt[] and z3[]: comp + N mu_J + sigma_J sqrt(N) z3
    __device__ __forceinline__ void jump(const HestonArgs<Consts>& a, const int elem, double (&J)[PPL]) {
        uint32_t n[PPL];
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
            n[p] = (cnt[p] >> (8 * elem)) & 0xffu;
            J[p] = a.c.comp;
        }
        if (__builtin_amdgcn_ballot_w64((n[0] | n[1]) != 0u) != 0ull) {
            asm volatile("" ::);  // keep this a real (scalar) branch
            const auto r = rare();
            const double mu_j = r->mu_j, sigma_j = r->sigma_j;
#pragma unroll
            for (int p = 0; p < PPL; ++p) {
                const double dn = (double)n[p];
                const double amp = sigma_j * fm::sqrt_pos(__builtin_fmax(dn, 1.0));
                const double j = __builtin_fma(amp, z3[p][elem], __builtin_fma(dn, mu_j, a.c.comp));
                J[p] = n[p] != 0u ? j : a.c.comp;  // z3 counts only where the path jumps
            }
        }
    }
    __device__ __forceinline__ void step(const HestonArgs<Consts>& a, const int64_t i, const uint32_t block, const int elem,
                                         const fm::Tables* tab, const double (&z1)[PPL], const double (&z2)[PPL], double (&S)[PPL],
                                         double (&v)[PPL]) {
        double J[PPL];
        jump(a, elem, J);
        base.step(a, i, block, elem, tab, z1, z2, S, v, [&J](int p, double e) { return e + J[p]; });
    }
};

}  // namespace mcg
