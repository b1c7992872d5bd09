// Correlated multi-asset GBM paths for gfx950 and the reduction of d asset matrices to one (include/mcgpu.h:
// mcg_paths_gbm_multi, mcg_paths_combine).
//
// k_gbm_multi<D, STORE_ASSETS, STORE_COMBINED> has the generators' skeleton of paths_device.hpp and takes its row store from
// there: two adjacent paths per lane with the D prices of each in registers, fm::Tables in LDS, one Philox stream per driver
// (stream 0, then 16..22), a wave-uniform row offset plus a constant lane offset.  It walks its blocks itself: draw() makes
// all four steps' exponents at once, and through walk_blocks hipcc allots D = 5 with the combined row alone 168 vector
// registers for 169.  The model's constants
// (drifts, the lower triangle A = diag(sigma sqrt(dt)) L, the weights) sit in LDS behind the tables: 52 doubles, read with
// one broadcast ds_read each, so that no D costs scalar registers for them.  The per-(path, driver) Philox state is not held:
// three words per path stay in registers, and one 32x32 -> 64 product (two multiply instructions) per path, driver and block
// rebuilds the rest.
//
// Roofline: HBM write, 8 B per path-step and stored matrix (the combined row alone: 8 B however many assets), reads ~0.
// k_paths_combine streams D rows in and one out: (D + 1) * 8 B per path-step.
#include <cstring>

#include "devmath.hpp"
#include "fastmath.hpp"
#include "paths_host.hpp"
#include "paths_device.hpp"

namespace mcg {

constexpr int MULTI_MAX = 8;                                  // assets of one call
constexpr int MULTI_TRI = MULTI_MAX * (MULTI_MAX + 1) / 2;    // entries of a packed lower triangle
constexpr int MULTI_PPL = 2;                                  // paths per lane

// Philox stream of driver b: the price driver, then 16..22 (1..5 belong to the Heston, QE, branching and Bates kernels).
__host__ __device__ constexpr uint32_t multi_stream(int b) { return b == 0 ? 0u : 15u + (uint32_t)b; }

struct MultiConsts {
    double drift[MULTI_MAX];  // (r - q_a - sigma_a^2 / 2) dt
    double A[MULTI_TRI];      // A_ab = sigma_a sqrt(dt) L_ab at [a (a + 1) / 2 + b], b <= a
    double w[MULTI_MAX];      // weights of the combination (1 where none were given)
};
constexpr int MULTI_NCONST = sizeof(MultiConsts) / sizeof(double);

struct MultiArgs {
    double* out[MULTI_MAX];  // [n_steps+1][ld] per asset (STORE_ASSETS kernels only)
    double* comb;            // [n_steps+1][ld] (STORE_COMBINED kernels only)
    int64_t ld;
    int n_steps;
    int kind;                // enum mcg_combine_kind
    uint64_t path_begin;
    uint32_t k0, k1;         // Philox key = seed
    double S0[MULTI_MAX];
    double c[MULTI_NCONST];  // MultiConsts, as doubles
    const double2* tabs;     // fm::Tables on the device
};

struct CombineArgs {
    const double* in[MULTI_MAX];
    double* out;
    double w[MULTI_MAX];
    int64_t ld;
    int n_rows;
    int n_assets;
    int kind;
};

// The combination of the contract, x_a = w_a S^a: BASKET acc = x_0, then acc = fma(w_a, S^a, acc) in asset order; BEST_OF
// max_a x_a; WORST_OF min_a x_a.  One definition for the fused generator (n = NMAX = D) and for k_paths_combine (n at run
// time): their matrices agree bit for bit because both run exactly these operations.  n, kind: wave-uniform; S and w are
// indexed by constants only.
template <int NMAX, class W>
__device__ __forceinline__ double combine_assets(const double (&S)[NMAX], const W& w, const int n, const int kind) {
    double acc = w[0] * S[0];
#pragma unroll
    for (int a = 1; a < NMAX; ++a) {
        if (a < n) {
            if (kind == MCG_C_BASKET) acc = __builtin_fma(w[a], S[a], acc);
            else if (kind == MCG_C_BEST_OF) acc = __builtin_fmax(acc, w[a] * S[a]);
            else acc = __builtin_fmin(acc, w[a] * S[a]);
        }
    }
    return acc;
}

template <int D, bool STORE_ASSETS, bool STORE_COMBINED>
__global__ __launch_bounds__(256) void k_gbm_multi(MultiArgs a) {
    static_assert(D >= 1 && D <= MULTI_MAX && (STORE_ASSETS || STORE_COMBINED), "");
    constexpr int PPL = MULTI_PPL;
    __shared__ fm::Tables tabs;
    __shared__ MultiConsts cst;
    fm::load_tables(&tabs, a.tabs);
    if (threadIdx.x == 0) {  // (constant indices: scalar loads from the argument block, no private copy of it)
        double* dst = reinterpret_cast<double*>(&cst);
#pragma unroll
        for (int k = 0; k < MULTI_NCONST; ++k) dst[k] = a.c[k];
    }
    const fm::Tables* tab = &tabs;
    __syncthreads();
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PPL;  // first column of this lane
    // rows are padded to 256 columns and a workgroup covers 512: the upper two waves of the last one may lie beyond the row
    if (!(i < a.ld)) return;  // (wave-uniform)
    double S[PPL][D];
#pragma unroll
    for (int p = 0; p < PPL; ++p)
#pragma unroll
        for (int d = 0; d < D; ++d) S[p][d] = a.S0[d];
    // what a path contributes to rounds 1 and 2 of its Philox blocks whatever the stream: path_hi, and the two words of
    // M0 * path_lo (philox_lane_setup)
    uint32_t path_hi[PPL], lo0[PPL], hi0[PPL];
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        const uint64_t path = a.path_begin + (uint64_t)(i + p);
        const uint64_t p0 = (uint64_t)0xD2511F53u * (uint32_t)path;
        path_hi[p] = (uint32_t)(path >> 32);
        lo0[p] = (uint32_t)p0;
        hi0[p] = (uint32_t)(p0 >> 32);
    }
    const unsigned lane_bytes = threadIdx.x * (8u * PPL);
    int64_t row_off = (int64_t)blockIdx.x * (256 * PPL);  // (wave-uniform) this workgroup's columns of the current row
    auto store_rows = [&]() {
        if (STORE_ASSETS) {
#pragma unroll
            for (int d = 0; d < D; ++d) store_pair16(a.out[d] + row_off, lane_bytes, S[0][d], S[1][d]);
        }
        if (STORE_COMBINED) {
            double x[PPL];
#pragma unroll
            for (int p = 0; p < PPL; ++p) x[p] = combine_assets(S[p], cst.w, D, a.kind);
            store_pair16(a.comb + row_off, lane_bytes, x[0], x[1]);
        }
    };
    store_rows();
    double e[PPL][D][4];  // the exponents of the current block's four steps
    // One Philox block per driver feeds two Box-Muller pairs = four steps of that driver; driver b enters the exponents of the
    // assets a >= b, so every e_a is summed in increasing b.
    auto draw = [&](const uint32_t block) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double dr = cst.drift[d];
#pragma unroll
            for (int p = 0; p < PPL; ++p)
#pragma unroll
                for (int k = 0; k < 4; ++k) e[p][d][k] = dr;
        }
#pragma unroll
        for (int b = 0; b < D; ++b) {
            double z[PPL][4];
#pragma unroll
            for (int p = 0; p < PPL; ++p) {
                uint32_t h = hi0[p];
                asm volatile("" : "+v"(h));  // (rebuilt per block: hoisted, the products of D streams would cost 2 D registers a path)
                const uint64_t p1b = (uint64_t)0xCD9E8D57u * (h ^ (multi_stream(b) ^ a.k1));
                const PhiloxLane L{path_hi[p], lo0[p], (uint32_t)(p1b >> 32), (uint32_t)p1b};
                const Philox4 w = philox4x32_10_lane(L, block, a.k0, a.k1);
                fm::box_muller_pair(w.w0, w.w1, tab, z[p][0], z[p][1]);
                fm::box_muller_pair(w.w2, w.w3, tab, z[p][2], z[p][3]);
            }
#pragma unroll
            for (int d = b; d < D; ++d) {
                const double A = cst.A[d * (d + 1) / 2 + b];
#pragma unroll
                for (int p = 0; p < PPL; ++p)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        e[p][d][k] = __builtin_fma(A, z[p][k], e[p][d][k]);
                        // (the sum is wanted HERE: hipcc otherwise sinks the chains of steps 1..3 into the steps' own blocks and
                        // keeps every driver's radii, sines and cosines alive till then -- 70 registers a driver, 292 at D = 4
                        // and a private segment at D = 8, against 146 and 233 with the exponents pinned)
                        asm volatile("" : "+v"(e[p][d][k]));
                    }
            }
        }
    };
    auto step = [&](const int k) {
#pragma unroll
        for (int d = 0; d < D; ++d)
#pragma unroll
            for (int p = 0; p < PPL; ++p) S[p][d] = fm::scaled_exp(S[p][d], e[p][d][k]);
        row_off += a.ld;
        store_rows();
    };
    const uint32_t n_blocks = (uint32_t)(a.n_steps >> 2);
    uint32_t block = 0;
#pragma unroll 1
    for (; block < n_blocks; ++block) {
        draw(block);
        step(0);
        step(1);
        step(2);
        step(3);
    }
    const int rest = a.n_steps & 3;
    if (rest) {  // wave-uniform
        draw(block);
        step(0);
        if (rest >= 2) step(1);
        if (rest == 3) step(2);
    }
}

// out row = combination of the same row of n_assets matrices.  A lane takes two adjacent paths of one row at a time: 16-byte
// loads, the generator's 16-byte store; blockIdx.y walks the rows.
__global__ __launch_bounds__(256) void k_paths_combine(CombineArgs a) {
    constexpr int PPL = MULTI_PPL;
    typedef double v2d __attribute__((ext_vector_type(2)));
    const int64_t col0 = (int64_t)blockIdx.x * (256 * PPL);
    const int64_t i = col0 + (int64_t)threadIdx.x * PPL;
    if (!(i < a.ld)) return;  // (wave-uniform: ld is a multiple of 256)
    const unsigned lane_bytes = threadIdx.x * (8u * PPL);
    for (int r = blockIdx.y; r < a.n_rows; r += gridDim.y) {
        const int64_t off = (int64_t)r * a.ld;
        double S[PPL][MULTI_MAX];
#pragma unroll
        for (int d = 0; d < MULTI_MAX; ++d) {
            if (d < a.n_assets) {  // (wave-uniform)
                // (columns n_paths .. ld - 1 are read too: inside the allocation, but of an uploaded matrix nobody ever wrote
                // them -- what comes out of them lands in out's own padding, which is never read back: paths_new)
                const v2d v = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(a.in[d] + off + i));
                S[0][d] = v.x;
                S[1][d] = v.y;
            } else {
                S[0][d] = 0.0;
                S[1][d] = 0.0;
            }
        }
        double x[PPL];
#pragma unroll
        for (int p = 0; p < PPL; ++p) x[p] = combine_assets(S[p], a.w, a.n_assets, a.kind);
        store_pair16(a.out + off + col0, lane_bytes, x[0], x[1]);
    }
}

template <int D>
static void launch_multi_d(mcg_ctx* ctx, const MultiArgs& a, bool assets, bool combined, unsigned n_blocks) {
    dispatch_flags(
        [&](auto sa, auto sc) {
            if constexpr (sa.value || sc.value)  // (a launch stores something: launch_gbm_multi's callers see to it)
                hipLaunchKernelGGL((k_gbm_multi<D, sa.value, sc.value>), dim3(n_blocks), dim3(256), 0, ctx->stream, a);
        },
        assets, combined);
}

// One launch of k_gbm_multi over the asset matrices (assets: n_assets handles of one shape, or null) and / or the combined
// matrix (comb, or null).  L: the lower Cholesky factor of the correlation matrix, row-major; q, weights: never null here.
int launch_gbm_multi(mcg_ctx* ctx, mcg_paths* const* assets, mcg_paths* comb, int n_assets, uint64_t seed, const double* S0,
                     double r, const double* q, const double* sigma, const double* L, double dt, int kind,
                     const double* weights) {
    const mcg_paths* P = assets ? assets[0] : comb;
    const int64_t n_blocks = launch_blocks(P, MULTI_PPL);
    if (n_blocks < 0) return MCG_ERR_INVALID;
    MultiArgs a{};
    MultiConsts c{};
    const double sq = std::sqrt(dt);
    for (int d = 0; d < n_assets; ++d) {
        if (assets) {
            if (assets[d]->ld != P->ld || assets[d]->n_steps != P->n_steps)
                return fail(MCG_ERR_INVALID, "the asset matrices must have one shape");
            a.out[d] = assets[d]->data;
        }
        a.S0[d] = S0[d];
        c.drift[d] = (r - q[d] - 0.5 * sigma[d] * sigma[d]) * dt;
        for (int b = 0; b <= d; ++b) c.A[d * (d + 1) / 2 + b] = sigma[d] * sq * L[d * n_assets + b];
        c.w[d] = weights[d];
    }
    if (comb && (comb->ld != P->ld || comb->n_steps != P->n_steps))
        return fail(MCG_ERR_INVALID, "the combined matrix must have the shape of the asset matrices");
    a.comb = comb ? comb->data : nullptr;
    a.ld = P->ld;
    a.n_steps = P->n_steps;
    a.kind = kind;
    a.path_begin = P->path_begin;
    a.k0 = (uint32_t)seed;
    a.k1 = (uint32_t)(seed >> 32);
    static_assert(sizeof(a.c) == sizeof(c), "MultiArgs::c carries a MultiConsts");
    std::memcpy(a.c, &c, sizeof c);
    a.tabs = (const double2*)ctx->log_tab;
    return PathLaunch{ctx, n_blocks}.run(MCG_K_MULTI, [&] {
        const bool sa = assets != nullptr, sc = comb != nullptr;
        const unsigned g = (unsigned)n_blocks;
        switch (n_assets) {
            case 1: launch_multi_d<1>(ctx, a, sa, sc, g); break;
            case 2: launch_multi_d<2>(ctx, a, sa, sc, g); break;
            case 3: launch_multi_d<3>(ctx, a, sa, sc, g); break;
            case 4: launch_multi_d<4>(ctx, a, sa, sc, g); break;
            case 5: launch_multi_d<5>(ctx, a, sa, sc, g); break;
            case 6: launch_multi_d<6>(ctx, a, sa, sc, g); break;
            case 7: launch_multi_d<7>(ctx, a, sa, sc, g); break;
            default: launch_multi_d<8>(ctx, a, sa, sc, g); break;
        }
    });
}

// One launch of k_paths_combine: out = combination of n_assets matrices of out's shape; weights: never null here.
int launch_paths_combine(mcg_ctx* ctx, const mcg_paths* const* assets, int n_assets, int kind, const double* weights,
                         mcg_paths* out) {
    const int64_t n_blocks = launch_blocks(out, MULTI_PPL);
    if (n_blocks < 0) return MCG_ERR_INVALID;
    CombineArgs a{};
    for (int d = 0; d < n_assets; ++d) {
        if (assets[d]->ld != out->ld) return fail(MCG_ERR_INVALID, "the matrices must have one row stride");
        a.in[d] = assets[d]->data;
        a.w[d] = weights[d];
    }
    a.out = out->data;
    a.ld = out->ld;
    a.n_rows = out->n_steps + 1;
    a.n_assets = n_assets;
    a.kind = kind;
    return PathLaunch{ctx, n_blocks}.run(MCG_K_MULTI, [&] {
        const dim3 grid((unsigned)n_blocks, (unsigned)std::min(a.n_rows, 65535)), block(256);
        hipLaunchKernelGGL(k_paths_combine, grid, block, 0, ctx->stream, a);
    });
}

}  // namespace mcg
