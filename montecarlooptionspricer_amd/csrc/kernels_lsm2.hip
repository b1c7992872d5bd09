// The two-regressor Longstaff-Schwartz sweep (mcg_price_lsm2; the fit rule is stated as a contract in include/mcgpu.h):
// the continuation value is regressed on the price S_j AND a second per-path state F_j (Heston: the variance).
//
// mcg_price_lsm's exercise rule (k_lsm_date's `update`, branch for branch) with another fit.  Both regressors are
// standardised over the date's in-the-money paths, so the moments of the monomials zx^a zw^b are formed about the date's
// own centre and scale -- which have to be known BEFORE the moments are summed.  Per exercise date the host therefore
// queues four launches, never looking at a result (no read-back, no data-dependent launch, and no workgroup ever waits
// for another inside a kernel: what the one-regressor route exchanges through tickets travels between launches here):
//   k_lsm2_centre        row j-1: {count, sum S, sum S^2, sum F, sum F^2} over the in-the-money paths, per workgroup   16 B
//   k_lsm2_centre_reduce one workgroup, fixed blockIdx order: mu and 1/sigma of both regressors -> the centre block
//   k_lsm2_update<P>     V <- update with date j's fit; the moments of date j-1 about its centre from S_{j-1}, F_{j-1}
//                        and the new V, in registers, then block_sum and per-workgroup partials                       48 B
//   k_lsm2_reduce_solve<P> one workgroup sums the partials in fixed blockIdx order, one thread solves (lsm2_solve) and
//                        leaves date j-1's coefficient block, centres and scales included; dropped columns are counted
// per path and date 64 B against k_lsm_date's 32.  The final sums are k_lsm_final / finish_sums.
// As in k_lsm_date: two adjacent paths per lane (16-byte loads and stores), a grid of one resident wave of workgroups,
// consecutive dates walk the paths in opposite directions, the second path of an odd count's last unit is computed from
// the row's padding, stored into V's slack and never counted.
#include "lsm2_device.hpp"
#include "mcg_internal.hpp"

namespace mcg {

constexpr int LSM2_DEPTH = 2;  // units a thread has in flight

// where the sweep keeps its small blocks: the per-date message slot of the one-regressor route (48 doubles), which is
// idle while this sweep runs (one stream per ctx)
constexpr int LSM2_SC_COEF = SC_LSM_MSG;                         // date j's coefficient block
constexpr int LSM2_SC_CENTRE = SC_LSM_MSG + LSM2_COEF_DOUBLES;   // date j-1's centre block
constexpr int LSM2_SC_DROPPED = LSM2_SC_CENTRE + LSM2_CENTRE_DOUBLES;
static_assert(LSM2_SC_DROPPED < SC_LSM_MSG + 48, "the blocks fit the message slot");

struct Lsm2Args {
    const double* S;  // step-major price matrix
    const double* F;  // step-major state matrix, same shape
    int64_t ld_s, ld_f, n;
    double* V;
    double K, disc;
    int is_call;
    int j;                // the row this launch works on
    int init, reg, have;  // row j: terminal payoff / regresses; row j-1 regresses (its moments are formed here)
    const double* coef;   // date j's coefficient block (lsm2_device.hpp: LSM2_C_*)
    const double* centre; // date j-1's centre block
    double* partials;     // [n sums][gridDim.x] (sum-major: the reducing workgroup reads contiguously)
};

// The paths of this launch as units of two, in chunks of one unit per thread of the grid; rev: walked backwards.
struct Lsm2Walk {
    int64_t n_units, chunk, n_chunks, lane_unit;
    bool rev;
    __device__ Lsm2Walk(int64_t n, bool rev_) : rev(rev_) {
        n_units = (n + 1) / 2;
        chunk = (int64_t)gridDim.x * 256;
        n_chunks = (n_units + chunk - 1) / chunk;
        lane_unit = (int64_t)blockIdx.x * 256 + threadIdx.x;
    }
    __device__ int64_t unit(int64_t k) const { return k < n_chunks ? (rev ? n_chunks - 1 - k : k) * chunk + lane_unit : n_units; }
};

__global__ __launch_bounds__(256) void k_lsm2_centre(Lsm2Args a) {
    constexpr int D = LSM2_DEPTH;
    __shared__ double red[LSM2_CENTRE_SUMS * 4];
    const bool call = a.is_call != 0;
    const double2* S_m = reinterpret_cast<const double2*>(a.S + (int64_t)(a.j - 1) * a.ld_s);
    const double2* F_m = reinterpret_cast<const double2*>(a.F + (int64_t)(a.j - 1) * a.ld_f);
    const Lsm2Walk w(a.n, (a.j & 1) == 0);  // against the update pass of row j, which reads row j-1 next
    int64_t u[D];
    double2 s[D], f[D];
    auto fetch = [&](int d, int64_t k) {
        u[d] = w.unit(k);
        s[d] = make_double2(0.0, 0.0);
        f[d] = make_double2(0.0, 0.0);
        if (u[d] < w.n_units) {
            s[d] = S_m[u[d]];
            f[d] = F_m[u[d]];
        }
    };
#pragma unroll
    for (int d = 0; d < D; ++d) fetch(d, d);
    double m[LSM2_CENTRE_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    auto add = [&](bool live, double sv, double fv) {
        if (live && payoff_of(call, sv, a.K) > LSM_ITM_EPS) {
            m[0] += 1.0;
            m[1] += sv;
            m[2] = fma(sv, sv, m[2]);
            m[3] += fv;
            m[4] = fma(fv, fv, m[4]);
        }
    };
    for (int64_t k0 = 0; k0 < w.n_chunks; k0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (u[d] < w.n_units) {
                add(true, s[d].x, f[d].x);
                add(2 * u[d] + 1 < a.n, s[d].y, f[d].y);
            }
            fetch(d, k0 + d + D);
        }
    }
    block_sum<LSM2_CENTRE_SUMS, 4>(m, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < LSM2_CENTRE_SUMS; ++q) a.partials[(int64_t)q * gridDim.x + blockIdx.x] = m[q];
    }
}

// One workgroup: partials[nm][n_blocks] -> sm[nm] in a fixed order (as k_lsm_reduce_solve: wave w sums w, w+4, ...;
// its lanes stride over the workgroups, then the wavefront butterfly).
__device__ __forceinline__ void lsm2_reduce(const double* partials, int n_blocks, int nm, double* sm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int q = wave; q < nm; q += 4) {
        double s = 0.0;
#pragma unroll 8
        for (int b = lane; b < n_blocks; b += 64) s += partials[(int64_t)q * n_blocks + b];
        s = wave_sum(s);
        if (lane == 0) sm[q] = s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_lsm2_centre_reduce(const double* partials, int n_blocks, double* centre) {
    __shared__ double sm[LSM2_CENTRE_SUMS];
    lsm2_reduce(partials, n_blocks, LSM2_CENTRE_SUMS, sm);
    if (threadIdx.x == 0) {
        double mu_x = 0.0, isd_x = 0.0, mu_w = 0.0, isd_w = 0.0;
        if (sm[0] > 0.0) {
            lsm2_standardise(sm[0], sm[1], sm[2], mu_x, isd_x);
            lsm2_standardise(sm[0], sm[3], sm[4], mu_w, isd_w);
        }
        centre[0] = sm[0];
        centre[1] = mu_x;
        centre[2] = isd_x;
        centre[3] = mu_w;
        centre[4] = isd_w;
    }
}

template <int P>
__global__ __launch_bounds__(256) void k_lsm2_update(Lsm2Args a) {
    constexpr int NB = lsm2_count(P), NP = lsm2_count(2 * P), NM = NP + NB;
    constexpr int D = LSM2_DEPTH;
    __shared__ double red[NM * 4];
    __shared__ double sm_c[LSM2_COEF_DOUBLES + LSM2_CENTRE_DOUBLES];
    const bool call = a.is_call != 0;
    const bool init = a.init != 0, reg = a.reg != 0, have = a.have != 0;
    const double2* S_j = reinterpret_cast<const double2*>(a.S + (int64_t)a.j * a.ld_s);
    const double2* F_j = reinterpret_cast<const double2*>(a.F + (int64_t)a.j * a.ld_f);
    const double2* S_m = reinterpret_cast<const double2*>(a.S + (int64_t)(have ? a.j - 1 : a.j) * a.ld_s);
    const double2* F_m = reinterpret_cast<const double2*>(a.F + (int64_t)(have ? a.j - 1 : a.j) * a.ld_f);
    double2* V2 = reinterpret_cast<double2*>(a.V);
    const Lsm2Walk w(a.n, (a.j & 1) != 0);
    int64_t u[D];
    double2 s[D], f[D], v[D], sp[D], fp[D];
    auto fetch = [&](int d, int64_t k) {
        u[d] = w.unit(k);
        s[d] = f[d] = v[d] = sp[d] = fp[d] = make_double2(0.0, 0.0);
        if (u[d] < w.n_units) {
            typedef double v2d __attribute__((ext_vector_type(2)));
            const v2d ts = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(S_j + u[d]));  // row j is not needed again
            s[d] = make_double2(ts.x, ts.y);
            if (reg) {  // (the state enters the fit only)
                const v2d tf = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(F_j + u[d]));
                f[d] = make_double2(tf.x, tf.y);
            }
            if (!init) v[d] = V2[u[d]];
            if (have) {
                sp[d] = S_m[u[d]];
                fp[d] = F_m[u[d]];
            }
        }
    };
#pragma unroll
    for (int d = 0; d < D; ++d) fetch(d, d);
    if (threadIdx.x < LSM2_COEF_DOUBLES) sm_c[threadIdx.x] = reg ? a.coef[threadIdx.x] : 0.0;
    else if (threadIdx.x < LSM2_COEF_DOUBLES + LSM2_CENTRE_DOUBLES)
        sm_c[threadIdx.x] = have ? a.centre[threadIdx.x - LSM2_COEF_DOUBLES] : 0.0;
    __syncthreads();
    double c[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) c[k] = sm_c[k];
    const double n_itm = sm_c[LSM2_C_COUNT];
    const double mu_x = sm_c[LSM2_C_MU_X], isd_x = sm_c[LSM2_C_ISD_X], mu_w = sm_c[LSM2_C_MU_W], isd_w = sm_c[LSM2_C_ISD_W];
    const double* cen = sm_c + LSM2_COEF_DOUBLES;
    const double pmu_x = cen[1], pisd_x = cen[2], pmu_w = cen[3], pisd_w = cen[4];  // date j-1's
    double m[NM];
#pragma unroll
    for (int q = 0; q < NM; ++q) m[q] = 0.0;
    auto update = [&](double s_now, double f_now, double v_old) {  // k_lsm_date's update with the two-regressor fit
        if (init) return payoff_of(call, s_now, a.K);
        if (!reg) return v_old * a.disc;
        const double pay = payoff_of(call, s_now, a.K);
        if (pay > LSM_ITM_EPS && n_itm > 0.0) {
            double phi[NB];
            lsm2_monomials<P>((s_now - mu_x) * isd_x, (f_now - mu_w) * isd_w, phi);
            double fit = c[0];
#pragma unroll
            for (int k = 1; k < NB; ++k) fit = fma(c[k], phi[k], fit);
            return fmax(pay, fit);
        }
        if (pay < LSM_ITM_EPS) return v_old * a.disc;
        return 0.0;  // payoff == LSM_ITM_EPS exactly falls through both branches
    };
    auto accumulate = [&](bool live, double s_prev, double f_prev, double v_new) {  // regression inputs of date j-1
        if (live && payoff_of(call, s_prev, a.K) > LSM_ITM_EPS) {
            double phi[NP];
            lsm2_monomials<2 * P>((s_prev - pmu_x) * pisd_x, (f_prev - pmu_w) * pisd_w, phi);
            const double y = v_new * a.disc;
#pragma unroll
            for (int q = 0; q < NP; ++q) m[q] += phi[q];
#pragma unroll
            for (int k = 0; k < NB; ++k) m[NP + k] = fma(phi[k], y, m[NP + k]);
        }
    };
    for (int64_t k0 = 0; k0 < w.n_chunks; k0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (u[d] < w.n_units) {
                const double2 vn = make_double2(update(s[d].x, f[d].x, v[d].x), update(s[d].y, f[d].y, v[d].y));
                V2[u[d]] = vn;
                if (have) {
                    accumulate(true, sp[d].x, fp[d].x, vn.x);
                    accumulate(2 * u[d] + 1 < a.n, sp[d].y, fp[d].y, vn.y);
                }
            }
            fetch(d, k0 + d + D);
        }
    }
    if (!have) return;  // (uniform over the grid)
    block_sum<NM, 4>(m, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NM; ++q) a.partials[(int64_t)q * gridDim.x + blockIdx.x] = m[q];
    }
}

// One workgroup: date j-1's moments from the partials, its coefficient block from the moments (one thread; P is a
// template parameter so that lsm2_solve's loops unroll), its dropped columns added to the sweep's count.
template <int P>
__global__ __launch_bounds__(256) void k_lsm2_reduce_solve(const double* partials, int n_blocks, const double* centre,
                                                           double* coef, double* n_dropped) {
    constexpr int NB = lsm2_count(P), NM = lsm2_count(2 * P) + NB;
    __shared__ double sm[NM];
    __shared__ double sm_coef[NB];
    lsm2_reduce(partials, n_blocks, NM, sm);
    if (threadIdx.x != 0) return;
    const double count = sm[0];
#pragma unroll
    for (int k = 0; k < NB; ++k) sm_coef[k] = 0.0;
    if (count > 0.0) *n_dropped += (double)lsm2_solve<P>(sm, sm_coef);  // (a date without such a path fits and drops nothing)
    for (int k = 0; k < LSM2_COEF_DOUBLES; ++k) coef[k] = k < NB ? sm_coef[k] : 0.0;
    coef[LSM2_C_COUNT] = count;
    coef[LSM2_C_MU_X] = centre[1];
    coef[LSM2_C_ISD_X] = centre[2];
    coef[LSM2_C_MU_W] = centre[3];
    coef[LSM2_C_ISD_W] = centre[4];
}

typedef void (*Lsm2UpdateKernel)(Lsm2Args);
typedef void (*Lsm2SolveKernel)(const double*, int, const double*, double*, double*);
static Lsm2UpdateKernel update_kernel(int p) {
    static const Lsm2UpdateKernel k[LSM2_MAX_ORDER + 1] = {k_lsm2_update<0>, k_lsm2_update<1>, k_lsm2_update<2>, k_lsm2_update<3>};
    return k[p];
}
static Lsm2SolveKernel solve_kernel(int p) {
    static const Lsm2SolveKernel k[LSM2_MAX_ORDER + 1] = {k_lsm2_reduce_solve<0>, k_lsm2_reduce_solve<1>, k_lsm2_reduce_solve<2>,
                                                          k_lsm2_reduce_solve<3>};
    return k[p];
}

// Grid: 512 paths per workgroup and trip, at most one resident wave of the update kernel's workgroups.
static int lsm2_grid(mcg_ctx* ctx, int64_t N, int p) {
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)update_kernel(p), 256, 0) != hipSuccess || occ < 1) {
        (void)hipGetLastError();
        occ = 1;
    }
    const int64_t grid = std::min<int64_t>((N + 511) / 512, (int64_t)ctx->n_cus * std::min(occ, 3));  // (three per CU: date_kernel_occupancy)
    return grid < 1 ? 1 : (int)grid;
}

int run_lsm2(mcg_ctx* ctx, const mcg_paths* P, const mcg_paths* F, double r, double K, double maturity, double dt, int is_call,
             int poly_order, double* mean, double* std_err, int64_t* n_dropped) {
    const int64_t N = P->n_paths;
    const int M = P->n_steps + 1;
    const int nm = lsm2_count(2 * poly_order) + lsm2_count(poly_order);
    const int grid = lsm2_grid(ctx, N, poly_order);
    int rc = ensure_cap(ctx, &ctx->lsm_v, &ctx->lsm_v_cap, (size_t)N + 1);  // (a whole two-path unit at the end)
    if (rc) return rc;
    // (the centre pass's five sums exceed order 0's two moments; k_lsm_final leaves 2 per workgroup)
    rc = ensure_cap(ctx, &ctx->partials, &ctx->partials_cap, (size_t)grid * (size_t)std::max(nm, LSM2_CENTRE_SUMS));
    if (rc) return rc;

    Lsm2Args a;
    a.S = P->data;
    a.F = F->data;
    a.ld_s = P->ld;
    a.ld_f = F->ld;
    a.n = N;
    a.V = ctx->lsm_v;
    a.K = K;
    a.disc = std::exp(-r * dt);
    a.is_call = is_call;
    a.coef = ctx->scalars + LSM2_SC_COEF;
    a.centre = ctx->scalars + LSM2_SC_CENTRE;
    a.partials = ctx->partials;
    double* d_coef = ctx->scalars + LSM2_SC_COEF;
    double* d_centre = ctx->scalars + LSM2_SC_CENTRE;
    double* d_dropped = ctx->scalars + LSM2_SC_DROPPED;
    MCG_HIP(hipMemsetAsync(d_coef, 0, (LSM2_SC_DROPPED + 1 - LSM2_SC_COEF) * sizeof(double), ctx->stream));
    int64_t launches = 0;
    for (int j = M - 1; j >= 0; --j)
        launches += j >= 1 && !((j - 1) * dt > maturity) ? 4 : 1;
    {
        // timing: ONE event pair around the queued sequence, as on the one-regressor per-date route
        TimedLaunch t(ctx, MCG_K_LSM_SWEEP, launches);
        for (int j = M - 1; j >= 0; --j) {
            a.j = j;
            a.init = j == M - 1;
            a.reg = !a.init && !(j * dt > maturity);
            a.have = j >= 1 && !((j - 1) * dt > maturity);  // date j-1 regresses: its centre, then its moments
            if (a.have) {
                hipLaunchKernelGGL(k_lsm2_centre, dim3(grid), dim3(256), 0, ctx->stream, a);
                hipLaunchKernelGGL(k_lsm2_centre_reduce, dim3(1), dim3(256), 0, ctx->stream, ctx->partials, grid, d_centre);
            }
            hipLaunchKernelGGL(update_kernel(poly_order), dim3(grid), dim3(256), 0, ctx->stream, a);
            if (a.have)
                hipLaunchKernelGGL(solve_kernel(poly_order), dim3(1), dim3(256), 0, ctx->stream, ctx->partials, grid, d_centre,
                                   d_coef, d_dropped);
        }
    }
    MCG_HIP(hipGetLastError());
    MCG_HIP(hipMemcpyAsync(ctx->h_scalars + LSM2_SC_DROPPED, d_dropped, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    rc = lsm_finish(ctx, grid, N, mean, std_err);  // (synchronises: the count above has arrived)
    if (rc) return rc;
    if (n_dropped) *n_dropped = (int64_t)ctx->h_scalars[LSM2_SC_DROPPED];
    return MCG_OK;
}

}  // namespace mcg
