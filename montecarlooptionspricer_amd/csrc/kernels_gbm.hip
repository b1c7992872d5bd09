// GBM path generation for gfx950: one path per lane, Philox normals (four per block), S in a register,
// step-major stores so a wavefront writes 64 consecutive doubles (512 B, four full 128-B lines)
// per time step, and a wavefront-shuffle reduction of the terminal payoff.
//
// Replaces, on the device, the stepping loop of /root/reference/src/models/RoughVolatility.cpp:354-364
// with v == sigma^2 (GBM is contained in the reference as that special case) and
// PayoffFunction (include/core/common.h:8-14) on the last column.
//
// Roofline: HBM write, 8*(n_steps+1) bytes per path, reads ~0.  No MFMA: the step is elementwise.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "devmath.hpp"
#include "fastmath.hpp"
#include "paths_host.hpp"
#include "paths_device.hpp"

#ifndef MCG_GBM_TABLES
#define MCG_GBM_TABLES 0
#endif

namespace mcg {

struct GbmArgs {
    double* out;       // [n_steps+1][ld]
    int64_t ld;
    int64_t n_paths;
    int n_steps;
    uint64_t path_begin;
    uint32_t k0, k1;   // Philox key = seed
    double S0, drift, vol;
    fm::LogScale ls;   // MODE >= 2: the logarithm's constants times vol^2 (fm::neg2log_scaled)
    double K;
    int is_call;
    double* partials;  // [gridDim.x][2]
    const double2* log_tab;  // fm::LOG_TAB_HOST on the device
    // mcg_generator_clock: the workgroups whose index is clk_first modulo 2^clk_shift stamp their life with the shader-cycle
    // and the 100 MHz counters into slot (index >> clk_shift) -- two scalar reads at each end of <= 64 workgroups per
    // launch; the start stamps wait in LDS, not in registers (the kernel has no scalar register to spare: held in four
    // of them for the kernel's life, the stamps pushed Horner constants out into spilled lanes)
    unsigned long long* clk;
    unsigned clk_first, clk_shift;
    // k_gbm_paths_wide only (there the stamping units are tiles, and partials is [n_tiles][2])
    const double2* sincos2;  // host_sincos2_tables() on the device: coarse, then fine
    unsigned* ticket;        // tile counter, zeroed on the stream before the launch
    unsigned n_tiles;        // ld / 128
};

// MODE 0: any parameters.  MODE 1 (SMALL): the host has checked |drift| + vol * 7.55 <= 0.125, so every step's exponent
// fits fm::scaled_exp_small (no range reduction, two fewer polynomial terms).  MODE 2: SMALL and vol > 0 folded into
// the logarithm (fm::neg2log_scaled): one multiply less per pair.  MODE 3: MODE 2 with the bound at 0.1, where e^a needs
// one polynomial term less (fm::scaled_exp_small6).
// PPL: paths per lane.  1: a wavefront writes 512 B per step.  2: a lane carries two adjacent paths and writes them with
// one 16-byte store (1 KB per wavefront and step; half the store instructions, half the loop and addressing overhead,
// two independent chains per lane) -- tools/ubench_write.hip: with 40 FMAs of work per path-step the 16-byte pattern
// runs 5.24 TB/s against 5.02.  A workgroup then covers 512 columns; rows are padded to 256, so the upper two waves of
// the last workgroup may lie beyond the row and sit the generation out (wave-uniform).
template <bool PAYOFF, int MODE, int PPL>
__global__ __launch_bounds__(256) void k_gbm_paths(GbmArgs a) {
    constexpr bool SMALL = MODE >= 1;
    typedef double v2d __attribute__((ext_vector_type(2)));
    // MCG_GBM_TABLES (A/B builds): 0 = all three tables of the rBergomi kernels (34 KiB: 4 workgroups per CU), 1 = logarithm
    // + 1024-entry sin/cos (32 KiB: 5), 2 = logarithm + 512-entry sin/cos (24 KiB: 6; one more cosine term per pair)
#if MCG_GBM_TABLES == 0
    typedef fm::Tables GbmTables;
    __shared__ GbmTables tabs;
    if (MODE >= 2) fm::load_tables_scaled(&tabs, a.log_tab, a.vol * a.vol);
    else fm::load_tables(&tabs, a.log_tab);
#else
    typedef fm::NormalTables<MCG_GBM_TABLES == 1 ? 10 : 9> GbmTables;
    __shared__ GbmTables tabs;
    fm::load_normal_tables(&tabs, a.log_tab, MODE >= 2 ? a.vol * a.vol : 1.0);
#endif
    const GbmTables* tab = &tabs;
    __syncthreads();
#ifdef MCG_GBM_NO_STAMPS  // (A/B builds: the kernel without its clock stamps)
    const bool stamps = false;
#else
    const bool stamps = a.clk != nullptr && (blockIdx.x & ((1u << a.clk_shift) - 1u)) == a.clk_first;  // (wave-uniform)
#endif
    // (everything the end of the kernel needs -- whether this workgroup stamps, where to, the start stamps -- waits in LDS)
    __shared__ unsigned long long stamp0[3];
    if (threadIdx.x == 0) {
        stamp0[2] = 0;
        if (stamps && (blockIdx.x >> a.clk_shift) < (unsigned)GBM_CLK_SLOTS) {
            stamp0[2] = (unsigned long long)(a.clk + 2 * (blockIdx.x >> a.clk_shift));
            stamp0[0] = __builtin_amdgcn_s_memtime();
            stamp0[1] = __builtin_amdgcn_s_memrealtime();
        }
    }
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PPL;  // first column of this lane
    const bool in_row = PPL == 1 || i < a.ld;
    double S[PPL];
#pragma unroll
    for (int p = 0; p < PPL; ++p) S[p] = a.S0;
    if (in_row) {
        // The address of a store is (wave-uniform row pointer) + (lane offset): the row pointer advances on the scalar
        // unit and the lane offset never changes, so a step spends no vector instruction on addressing.
        double* row = a.out + (int64_t)blockIdx.x * (256 * PPL);
        const unsigned lane_bytes = threadIdx.x * (8u * PPL);
        // (hipcc picks the scalar-base form for the first store only and rebuilds a 64-bit vector address inside the
        // loop, hence the explicit instruction)
        auto store_row = [&](double* r) {
            if constexpr (PPL == 1) {
                asm volatile("global_store_dwordx2 %0, %1, %2 nt" : : "v"(lane_bytes), "v"(S[0]), "s"(r) : "memory");
            } else {
                // The `s_nop 1` belongs to the store: on gfx940+ a store of more than 64 bits reads its data registers
                // AFTER issue, and a VALU instruction that overwrites them within the next two wait states corrupts what is
                // stored (ISA: required software-inserted wait states).  hipcc covers its own stores; an asm statement is
                // opaque to it, and S[] is overwritten by the next step's FMA right behind this store.  Round 4: a build
                // whose scheduling put that FMA first stored foreign low / high words in rows 0, 1 and 5 of the matrix
                // (1.2e-10 and percent-size errors in a quarter of the lanes, tools/diag_stamps.py) while the chain in
                // the registers stayed right; tools/check_asm_hazards.py finds the pattern in the assembly.
                const v2d v = {S[0], S[PPL - 1]};
                asm volatile("global_store_dwordx4 %0, %1, %2 nt\n\ts_nop 1" : : "v"(lane_bytes), "v"(v), "s"(r) : "memory");
            }
        };
        store_row(row);
        // One Philox block feeds two Box-Muller pairs = four steps.  The main loop takes whole blocks (both pairs
        // written out, so no register copies select a pair); the tail runs pair by pair over the last <= 3 steps.
        PhiloxLane lane_rng[PPL];
#pragma unroll
        for (int p = 0; p < PPL; ++p) lane_rng[p] = philox_lane_setup(a.path_begin + (uint64_t)(i + p), STREAM_PRICE, a.k1);
        auto step = [&](const double (&e)[PPL]) {
#pragma unroll
            for (int p = 0; p < PPL; ++p)
                S[p] = MODE == 3 ? fm::scaled_exp_small6(S[p], e[p]) : SMALL ? fm::scaled_exp_small(S[p], e[p]) : fm::scaled_exp(S[p], e[p]);
            row += a.ld;
            store_row(row);
        };
        auto pair_exponents = [&](uint32_t wa, uint32_t wb, double& e0, double& e1) {  // drift + vol*z of two steps
            if (MODE >= 2) fm::box_muller_pair_affine_scaled(wa, wb, tab, a.ls, a.drift, e0, e1);
            else fm::box_muller_pair_affine(wa, wb, tab, a.vol, a.drift, e0, e1);
        };
        const int n_blocks = a.n_steps >> 2;
#pragma unroll 1
        for (int b = 0; b < n_blocks; ++b) {
            Philox4 w[PPL];
#pragma unroll
            for (int p = 0; p < PPL; ++p) w[p] = philox4x32_10_lane(lane_rng[p], (uint32_t)b, a.k0, a.k1);
            double e0[PPL], e1[PPL];
#pragma unroll
            for (int p = 0; p < PPL; ++p) pair_exponents(w[p].w0, w[p].w1, e0[p], e1[p]);
            step(e0);
            step(e1);
#pragma unroll
            for (int p = 0; p < PPL; ++p) pair_exponents(w[p].w2, w[p].w3, e0[p], e1[p]);
            step(e0);
            step(e1);
        }
        const int rest = a.n_steps & 3;
        if (rest) {  // wave-uniform
            Philox4 w[PPL];
#pragma unroll
            for (int p = 0; p < PPL; ++p) w[p] = philox4x32_10_lane(lane_rng[p], (uint32_t)n_blocks, a.k0, a.k1);
            double e0[PPL], e1[PPL];
#pragma unroll
            for (int p = 0; p < PPL; ++p) pair_exponents(w[p].w0, w[p].w1, e0[p], e1[p]);
            step(e0);
            if (rest >= 2) step(e1);
            if (rest == 3) {
#pragma unroll
                for (int p = 0; p < PPL; ++p) pair_exponents(w[p].w2, w[p].w3, e0[p], e1[p]);
                step(e0);
            }
        }
    }
    if (threadIdx.x == 0 && stamp0[2] != 0) {
        const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        unsigned long long* dst = (unsigned long long*)stamp0[2];
        dst[0] = c1 - stamp0[0];
        dst[1] = r1 - stamp0[1];
    }
    if (PAYOFF) payoff_partials(in_row, i, a.n_paths, S, a.K, a.is_call, a.partials);
}

// The generator for large launches: sin/cos of the Box-Muller angle from TWO 4096-entry tables and one complex product
// (fm::sincos_two_level: 4 fp64 instructions per pair instead of 12; the kernel's clock follows its fp64 count).  With the
// logarithm's table that is 144 KiB of the CU's 160 KiB of LDS, so ONE workgroup of 16 waves owns a CU -- the 4 waves per SIMD
// of k_gbm_paths<., ., 2> -- and the kernel is persistent: grid = number of CUs, the tables are staged once behind the only
// barrier, and from there every WAVE is on its own.  A wave takes tiles of 128 columns (two adjacent paths per lane: 1 KiB
// per row and store, as the narrow kernel's waves), the first by its position and every later one from a ticket counter,
// runs all steps of the tile and stores every column of ld (a multiple of 256): the padded columns hold the stream's next
// paths.  (Tickets, not a fixed stride: waves do not all run at the same speed, and the rBergomi generator's record has a
// fixed stride 10 % slower.)  Nothing a tile writes
// depends on which wave ran it: the payoff sums of a tile are reduced inside the wave and land in partials[tile].
// A plain grid of such workgroups would leave the CU idle while each of them stages its tables and while its last wave
// drains (nothing else is resident): about 19 times per 10M-path launch.
struct WideTables {
    double2 log[fm::LOG_TAB_ENTRIES];       // {1/c_i, -2 ln c_i}; the second column times vol^2 in modes 2 and 3
    double2 coarse[fm::SINCOS2_ENTRIES];    // {cos, sin}(2 pi i / 4096)
    double2 fine[fm::SINCOS2_ENTRIES];      // {cos, sin}(2 pi (j + 1/2) / 2^24)
};
constexpr int WIDE_WAVES = 16, WIDE_TILE = 128;
static_assert(fm::SINCOS2_ENTRIES == SINCOS2_ENTRIES, "host/sincos2.cpp builds what fm::sincos_two_level indexes");
static_assert(sizeof(WideTables) == 147456, "144 KiB: one workgroup per CU");

template <bool PAYOFF, int MODE>
__global__ __launch_bounds__(64 * WIDE_WAVES) void k_gbm_paths_wide(GbmArgs a) {
    constexpr bool SMALL = MODE >= 1;
    typedef double v2d __attribute__((ext_vector_type(2)));
    __shared__ WideTables tabs;
    __shared__ unsigned long long stamp0[WIDE_WAVES][2];  // a stamping tile's start stamps wait here, not in registers
    {
        const double scale = a.vol * a.vol;
        for (int i = threadIdx.x; i < fm::LOG_TAB_ENTRIES; i += 64 * WIDE_WAVES) {
            double2 e = a.log_tab[i];
            if (MODE >= 2) e.y *= scale;   // (as fm::load_tables_scaled)
            tabs.log[i] = e;
        }
        double2* sc = reinterpret_cast<double2*>(&tabs) + fm::LOG_TAB_ENTRIES;  // coarse and fine, back to back in both places
        for (int i = threadIdx.x; i < 2 * fm::SINCOS2_ENTRIES; i += 64 * WIDE_WAVES) sc[i] = a.sincos2[i];
    }
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned lane_bytes = lane * 16u;
    // What only the start and the end of a tile need (matrix base, stream position, payoff, stamps, the counter) is re-read
    // from the kernel-argument segment there -- scalar loads of cached lines, twice per 128 x (n_steps + 1) values -- instead
    // of holding scalar registers across the steps: the Horner constants need those, and the kernel has none to spare (with
    // everything carried, 23 of them went to spilled lanes).  The empty asm keeps the loads where they are written.
    typedef const __attribute__((address_space(4))) GbmArgs* TileArgs;
    auto tile_args = [] {
        TileArgs p = (TileArgs)__builtin_amdgcn_kernarg_segment_ptr();  // (GbmArgs is the kernel's only argument)
        asm volatile("" : "+s"(p));
        return p;
    };
    auto stamping = [](TileArgs t, unsigned tile) {  // wave-uniform
        return t->clk != nullptr && (tile & ((1u << t->clk_shift) - 1u)) == t->clk_first && (tile >> t->clk_shift) < (unsigned)GBM_CLK_SLOTS;
    };
    unsigned tile = blockIdx.x * WIDE_WAVES + wave;  // the first tile by position, every later one from the counter
    while (tile < tile_args()->n_tiles) {
        const TileArgs t = tile_args();
        if (stamping(t, tile) && lane == 0) {
            stamp0[wave][0] = __builtin_amdgcn_s_memtime();
            stamp0[wave][1] = __builtin_amdgcn_s_memrealtime();
        }
        const int64_t col = (int64_t)tile * WIDE_TILE + lane * 2;  // first column of this lane
        double S[2] = {t->S0, t->S0};
        double* row = t->out + (int64_t)tile * WIDE_TILE;
        // (the store of k_gbm_paths<., ., 2>, with its own `s_nop 1`: see there)
        auto store_row = [&](double* r) {
            const v2d v = {S[0], S[1]};
            asm volatile("global_store_dwordx4 %0, %1, %2 nt\n\ts_nop 1" : : "v"(lane_bytes), "v"(v), "s"(r) : "memory");
        };
        store_row(row);
        PhiloxLane lane_rng[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) lane_rng[p] = philox_lane_setup(t->path_begin + (uint64_t)(col + p), STREAM_PRICE, a.k1);
        auto step = [&](const double (&e)[2]) {
#pragma unroll
            for (int p = 0; p < 2; ++p)
                S[p] = MODE == 3 ? fm::scaled_exp_small6(S[p], e[p]) : SMALL ? fm::scaled_exp_small(S[p], e[p]) : fm::scaled_exp(S[p], e[p]);
            row += a.ld;
            store_row(row);
        };
        auto pair_exponents = [&](uint32_t wa, uint32_t wb, double& e0, double& e1) {  // drift + vol*z of two steps
            if (MODE >= 2) fm::box_muller_pair_affine_scaled2(wa, wb, tabs.log, tabs.coarse, tabs.fine, a.ls, a.drift, e0, e1);
            else fm::box_muller_pair_affine2(wa, wb, tabs.log, tabs.coarse, tabs.fine, a.vol, a.drift, e0, e1);
        };
        const int n_blocks = a.n_steps >> 2;
#pragma unroll 1
        for (int b = 0; b < n_blocks; ++b) {
            Philox4 w[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) w[p] = philox4x32_10_lane(lane_rng[p], (uint32_t)b, a.k0, a.k1);
            double e0[2], e1[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) pair_exponents(w[p].w0, w[p].w1, e0[p], e1[p]);
            step(e0);
            step(e1);
#pragma unroll
            for (int p = 0; p < 2; ++p) pair_exponents(w[p].w2, w[p].w3, e0[p], e1[p]);
            step(e0);
            step(e1);
        }
        const int rest = tile_args()->n_steps & 3;  // (re-read: three branch conditions less to carry through the steps)
        if (rest) {  // wave-uniform
            Philox4 w[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) w[p] = philox4x32_10_lane(lane_rng[p], (uint32_t)n_blocks, a.k0, a.k1);
            double e0[2], e1[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) pair_exponents(w[p].w0, w[p].w1, e0[p], e1[p]);
            step(e0);
            if (rest >= 2) step(e1);
            if (rest == 3) {
#pragma unroll
                for (int p = 0; p < 2; ++p) pair_exponents(w[p].w2, w[p].w3, e0[p], e1[p]);
                step(e0);
            }
        }
        const TileArgs e = tile_args();
        if (stamping(e, tile) && lane == 0) {
            const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
            unsigned long long* dst = e->clk + 2 * (tile >> e->clk_shift);
            dst[0] = c1 - stamp0[wave][0];
            dst[1] = r1 - stamp0[wave][1];
        }
        if (PAYOFF) {
            double v[2] = {0.0, 0.0};
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const double pay = col + p < e->n_paths ? payoff_of(e->is_call != 0, S[p], e->K) : 0.0;
                v[0] += pay;
                v[1] += pay * pay;
            }
            wave_sum_all<2>(v);  // (a fixed butterfly: the tile's sums are the same bits whichever wave ran it)
            if (lane == 0) {
                e->partials[2 * (int64_t)tile] = v[0];
                e->partials[2 * (int64_t)tile + 1] = v[1];
            }
        }
        // one lane's atomic add, broadcast (a wave waits for it once per tile, behind its last stores; the SIMD's other
        // three waves are in the middle of their tiles meanwhile)
        unsigned drawn = 0;
        if (lane == 0) drawn = atomicAdd(e->ticket, 1u);
        tile = __builtin_amdgcn_readfirstlane(drawn) + gridDim.x * WIDE_WAVES;
    }
}

// Terminal payoff over a stored matrix: reads the last row only (8 B per path).
__global__ __launch_bounds__(256) void k_payoff_sums(const double* last_row, int64_t n_paths, double K,
                                                     int is_call, double* partials) {
    __shared__ double red[2 * 4];
    double v[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_paths; i += (int64_t)gridDim.x * 256) {
        const double pay = payoff_of(is_call != 0, last_row[i], K);
        v[0] += pay;
        v[1] += pay * pay;
    }
    block_sum<2, 4>(v, red);
    if (threadIdx.x == 0) {
        partials[2 * (int64_t)blockIdx.x] = v[0];
        partials[2 * (int64_t)blockIdx.x + 1] = v[1];
    }
}

// Fixed-order reduction of per-block partials {sum, sum of squares} (deterministic for a given count): one block for
// up to FIN_CHUNK pairs; beyond that (the fused payoff of a 10M-path generator leaves 39 063 pairs, an rBergomi one up
// to 250 000) a first launch sums chunks of FIN_CHUNK pairs, each in the same fixed order, and the single block finishes
// over the chunk sums -- 15.7 us of one block's strided reads become two launches of ~3 us.
constexpr int64_t FIN_CHUNK = 8192;

__device__ __forceinline__ void sum_pairs(const double* partials, int64_t n, double (&v)[2], double* red) {
    v[0] = 0.0;
    v[1] = 0.0;
    for (int64_t b = threadIdx.x; b < n; b += 1024) {
        v[0] += partials[2 * b];
        v[1] += partials[2 * b + 1];
    }
    block_sum<2, 16>(v, red);
}

__global__ __launch_bounds__(1024) void k_sum_chunks(const double* partials, int64_t n, double* chunk_out) {
    __shared__ double red[2 * 16];
    const int64_t begin = (int64_t)blockIdx.x * FIN_CHUNK;
    double v[2];
    sum_pairs(partials + 2 * begin, n - begin < FIN_CHUNK ? n - begin : FIN_CHUNK, v, red);
    if (threadIdx.x == 0) {
        chunk_out[2 * (int64_t)blockIdx.x] = v[0];
        chunk_out[2 * (int64_t)blockIdx.x + 1] = v[1];
    }
}

__global__ __launch_bounds__(1024) void k_finish_sums(const double* partials, int64_t n_blocks, double n_local,
                                                      double* out3) {
    __shared__ double red[2 * 16];
    double v[2];
    sum_pairs(partials, n_blocks, v, red);
    if (threadIdx.x == 0) {
        out3[0] = v[0];
        out3[1] = v[1];
        out3[2] = n_local;
    }
}

int finish_sums(mcg_ctx* ctx, int64_t n_blocks, int64_t n_local, double out3[3]) {
    double* d = ctx->scalars + SC_SUMS;
    const double* src = ctx->partials;
    int64_t n = n_blocks;
    if (n > FIN_CHUNK) {
        const int64_t n_chunks = (n + FIN_CHUNK - 1) / FIN_CHUNK;  // <= 2^31 / 8192
        int rc = ensure_cap(ctx, &ctx->fin_chunks, &ctx->fin_chunks_cap, (size_t)(2 * n_chunks));
        if (rc) return rc;
        TimedLaunch t(ctx, MCG_K_PAYOFF);
        hipLaunchKernelGGL(k_sum_chunks, dim3((unsigned)n_chunks), dim3(1024), 0, ctx->stream, src, n, ctx->fin_chunks);
        src = ctx->fin_chunks;
        n = n_chunks;
    }
    {
        TimedLaunch t(ctx, MCG_K_PAYOFF);
        hipLaunchKernelGGL(k_finish_sums, dim3(1), dim3(1024), 0, ctx->stream, src, n, (double)n_local, d);
    }
    MCG_HIP(hipGetLastError());
    if (ctx->allreduce) {
        if (ctx->allreduce(ctx->allreduce_user, d, 3, (void*)ctx->stream) != 0)
            return fail(MCG_ERR_COMM, "all-reduce of payoff sums failed");
    }
    MCG_HIP(hipMemcpyAsync(ctx->h_scalars + SC_SUMS, d, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MCG_HIP(hipStreamSynchronize(ctx->stream));
    out3[0] = ctx->h_scalars[SC_SUMS];
    out3[1] = ctx->h_scalars[SC_SUMS + 1];
    out3[2] = ctx->h_scalars[SC_SUMS + 2];
    return MCG_OK;
}

template <bool PAYOFF, int PPL>
static void launch_gbm_mode(mcg_ctx* ctx, const GbmArgs& a, int mode, unsigned n_blocks) {
    const dim3 grid(n_blocks), block(256);
    if (mode == 3) hipLaunchKernelGGL((k_gbm_paths<PAYOFF, 3, PPL>), grid, block, 0, ctx->stream, a);
    else if (mode == 2) hipLaunchKernelGGL((k_gbm_paths<PAYOFF, 2, PPL>), grid, block, 0, ctx->stream, a);
    else if (mode == 1) hipLaunchKernelGGL((k_gbm_paths<PAYOFF, 1, PPL>), grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_gbm_paths<PAYOFF, 0, PPL>), grid, block, 0, ctx->stream, a);
}

template <bool PAYOFF>
static void launch_gbm_wide_mode(mcg_ctx* ctx, const GbmArgs& a, int mode) {
    // (a launch with fewer tiles than the device has waves: only the workgroups whose first tile exists)
    const unsigned n_groups = std::min<unsigned>((unsigned)ctx->n_cus, (a.n_tiles + WIDE_WAVES - 1) / WIDE_WAVES);
    const dim3 grid(n_groups), block(64 * WIDE_WAVES);
    if (mode == 3) hipLaunchKernelGGL((k_gbm_paths_wide<PAYOFF, 3>), grid, block, 0, ctx->stream, a);
    else if (mode == 2) hipLaunchKernelGGL((k_gbm_paths_wide<PAYOFF, 2>), grid, block, 0, ctx->stream, a);
    else if (mode == 1) hipLaunchKernelGGL((k_gbm_paths_wide<PAYOFF, 1>), grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_gbm_paths_wide<PAYOFF, 0>), grid, block, 0, ctx->stream, a);
}

// The wide kernel (k_gbm_paths_wide) from GBM_WIDE_MIN_PATHS paths on: the smallest of the measured sizes from which it is
// not slower than k_gbm_paths (DESIGN.md section 5 has the times); mcg_debug_gbm_route overrides.
constexpr int64_t GBM_WIDE_MIN_PATHS = 2000000;
static bool gbm_takes_wide(const mcg_ctx* ctx, int64_t n_paths) {
    if (ctx->gbm_route == 1 || ctx->gbm_route == 2) return ctx->gbm_route == 2;
    return n_paths >= GBM_WIDE_MIN_PATHS;
}

// paths per lane: 2 once every CU has several workgroups of 512 paths to work on
static int gbm_paths_per_lane(const mcg_ctx* ctx, int64_t n_paths) {
    static const int forced = study_switch("MCG_GBM_PPL", 0);
    if (forced == 1 || forced == 2) return forced;
    return n_paths >= (int64_t)ctx->n_cus * 512 * 8 ? 2 : 1;
}

int launch_gbm(mcg_ctx* ctx, mcg_paths* P, uint64_t seed, double S0, double r, double sigma, double dt,
               bool want_payoff, double K, int is_call) {
    const bool wide = gbm_takes_wide(ctx, P->n_paths);
    const int ppl = gbm_paths_per_lane(ctx, P->n_paths);
    // the units that leave partial sums and stamp the clock: workgroups of the narrow kernel, tiles of the wide one
    const int64_t n_blocks = wide ? launch_units(P->ld / WIDE_TILE, P) : launch_blocks(P, ppl);
    if (n_blocks < 0) return MCG_ERR_INVALID;
    const PathLaunch launch{ctx, n_blocks, P, want_payoff, K, is_call};
    const int rc = launch.reserve();
    if (rc) return rc;
    GbmArgs a;
    set_shape_key(a, P, seed);
    set_payoff(a, ctx, K, is_call);
    a.S0 = S0;
    a.drift = (r - 0.5 * sigma * sigma) * dt;
    a.vol = sigma * std::sqrt(dt);
    a.log_tab = (const double2*)ctx->log_tab;
    a.sincos2 = (const double2*)ctx->sincos2_tab;
    a.ticket = reinterpret_cast<unsigned*>(ctx->scalars + SC_GBM_TICKET);
    a.n_tiles = wide ? (unsigned)n_blocks : 0u;
    // shader-clock stamps (armed launches only, mcg_generator_clock_arm): one workgroup (tile) in every 2^shift, the smallest
    // shift that needs at most GBM_CLK_SLOTS slots
    a.clk = nullptr;
    a.clk_first = 0;
    a.clk_shift = 0;
    ctx->clk_slots_used = 0;
    if (ctx->clk_armed && ctx->clk_stamps && n_blocks >= 64) {
        unsigned shift = 2;
        while (((n_blocks - 1) >> shift) >= GBM_CLK_SLOTS) ++shift;
        a.clk = ctx->clk_stamps;
        a.clk_shift = shift;
        a.clk_first = (1u << shift) / 2;   // (the middle of each stretch; the last stretch may end before it)
        ctx->clk_slots_used = (int)(((n_blocks - 1 - a.clk_first) >> shift) + 1);
        MCG_HIP(hipMemsetAsync(ctx->clk_stamps, 0, sizeof(unsigned long long) * 2 * GBM_CLK_SLOTS, ctx->stream));
    }
    if (wide) MCG_HIP(hipMemsetAsync(a.ticket, 0, sizeof(unsigned), ctx->stream));
    ctx->gbm_last_route = wide ? 2 : 1;
    const double reach = std::fabs(a.drift) + std::fabs(a.vol) * fm::MAX_ABS_NORMAL;
    // vol^2 (-2 ln u) must stay a normal positive double for modes 2 and 3
    const int mode = !(reach <= fm::SMALL_EXP_BOUND) ? 0 : !(a.vol > 1e-100) ? 1 : reach <= fm::SMALL6_EXP_BOUND ? 3 : 2;
    a.ls = fm::make_log_scale(a.vol * a.vol);
    return launch.run(MCG_K_GBM, [&] {
        dispatch_flags(
            [&](auto payoff, auto two) {
                if (wide) launch_gbm_wide_mode<payoff.value>(ctx, a, mode);
                else launch_gbm_mode<payoff.value, two.value ? 2 : 1>(ctx, a, mode, (unsigned)n_blocks);
            },
            want_payoff, ppl == 2);
    });
}

// Median (and range) of the stamping workgroups' clocks of the last GBM launch: cycles / (100 MHz ticks) x 0.1 GHz.
int generator_clock(mcg_ctx* ctx, double* ghz_median, int* n_stamps, double* ghz_min, double* ghz_max) {
    if (ghz_median) *ghz_median = 0.0;
    if (n_stamps) *n_stamps = 0;
    if (ghz_min) *ghz_min = 0.0;
    if (ghz_max) *ghz_max = 0.0;
    if (!ctx->clk_stamps || ctx->clk_slots_used < 1) return MCG_OK;
    unsigned long long h[2 * GBM_CLK_SLOTS];
    MCG_HIP(hipStreamSynchronize(ctx->stream));
    MCG_HIP(hipMemcpy(h, ctx->clk_stamps, sizeof h, hipMemcpyDeviceToHost));
    std::vector<double> g;
    for (int k = 0; k < ctx->clk_slots_used; ++k)
        if (h[2 * k + 1] > 100) g.push_back((double)h[2 * k] / (double)h[2 * k + 1] * 0.1);  // (a stamp shorter than 1 us says nothing)
    if (g.empty()) return MCG_OK;
    std::sort(g.begin(), g.end());
    if (ghz_median) *ghz_median = g[g.size() / 2];
    if (n_stamps) *n_stamps = (int)g.size();
    if (ghz_min) *ghz_min = g.front();
    if (ghz_max) *ghz_max = g.back();
    return MCG_OK;
}

int launch_payoff_sums(mcg_ctx* ctx, const mcg_paths* P, double K, int is_call, double out3[3]) {
    int64_t n_blocks = (P->n_paths + 255) / 256;
    if (n_blocks > 4096) n_blocks = 4096;
    int rc = ensure_cap(ctx, &ctx->partials, &ctx->partials_cap, (size_t)(2 * n_blocks));
    if (rc) return rc;
    {
        TimedLaunch t(ctx, MCG_K_PAYOFF);
        hipLaunchKernelGGL(k_payoff_sums, dim3((unsigned)n_blocks), dim3(256), 0, ctx->stream,
                           P->data + (int64_t)P->n_steps * P->ld, P->n_paths, K, is_call, ctx->partials);
    }
    MCG_HIP(hipGetLastError());
    return finish_sums(ctx, n_blocks, P->n_paths, out3);
}

}  // namespace mcg
