/* mcgpu_debug.h -- TEST HOOKS of libmcgpu.so.  Not part of the drop-in boundary: a maintainer of the reference binds
 * include/mcgpu.h only.  These entry points let tests/ force conditions a healthy device never shows (a hand-shake that times
 * out, a partial sum that never arrives, a tiny workspace budget) and run the host-only parts (the node segment's join /
 * barrier protocol, the peer-mailbox decision table, single device math routines) on their own.  The symbols are exported by
 * the same library; tests/test_abi_symbols.py checks them like the product's. */
#ifndef MCGPU_DEBUG_H
#define MCGPU_DEBUG_H
#include "mcgpu.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Test hook: evaluate one device math routine of the path kernels elementwise (csrc/fastmath.hpp).
 * y has 4n doubles; element i's results start at y[4i].
 * fn 0: y[0] = 1*e^x          fn 1: y[0] = -2 ln x (x in (0,1])       fn 2: y[0] = sqrt(x)
 * fn 3: x holds a 32-bit Philox word wb as a double; y[0], y[1] = cos, sin(2 pi ((wb>>8)+1/2) 2^-24)
 * fn 4: x holds a path id as a double; y[0..3] = the four normals of block 0, stream 0, seed 1
 * fn 5: as 4 through the reference-grade (device library) implementation.
 * fn 6: y[0] = e^x for |x| <= 0.125 (the branch-free step exponential)   fn 7: the same for |x| <= 0.1.
 * fn 8: y[0], y[1] = 2^(x/256), 2^((x+96)/256): both chains of fm::exp2_pair, x already in units of (ln 2)/256.
 * fn 9: as 4 with the four table entries of the block requested together (normal_quad_fast<true>).
 * fn 10: as 3 by the two 4096-entry tables (fm::sincos_two_level), read from device memory.
 * fn 11: y[0] = e^x with the range reduction always on (fm::exp_full).
 * fn 12: y[0], y[1] = e^x, e^(x + 0.375): both chains of fm::exp_full2.
 * fn 13: y[0], y[1] = e^x - 1, e^-x - 1 for |x| <= 0.1: both chains of fm::expm1_small6_2.   fn 14: the same for |x| <= 0.34
 *        (fm::expm1_small9_2).
 * fn 15: y[0] = sqrt_nonneg(x) of the Heston steps: 0 for x <= 0, the root of max(x, 2^-1000) otherwise.
 * fn 16: x holds a 32-bit Sobol' coordinate as a double; y[0] = Phi^-1((x + 1/2) 2^-32), the normal of the Sobol' generators
 *        (sobol_normal: AS241 as include/mcgpu.h states it). */
int mcg_debug_eval(mcg_ctx* ctx, int fn, const double* x, double* y, int64_t n);
/* Test hook: the same for routines with several inputs per element or with wave-uniform parameters.  x holds n_in doubles per
 * element, params n_params doubles for the whole launch (both must be what the fn takes); y has 4n doubles as above.  32-bit
 * Philox words and path ids travel as doubles.
 * fn 0: x = {d}: y[0] = qe_rcp(d)             fn 1: x = {n, d}: y[0] = qe_div(n, d)      (csrc/heston_schemes.hpp)
 * fn 2: x = {wa, wb}: y[0] = the radius uniform ((wb & 0xFF) 2^32 + wa + 1/2) 2^-40      (radius_u01)
 * fn 3: x = {u}, params = {vol2}: y[0] = vol2 (-2 ln u) by fm::neg2log_scaled, its table staged by fm::load_tables_scaled(vol2)
 *       and its constants built by fm::make_log_scale(vol2), as the GBM kernels do.
 * fn 4..7: x = {wa, wb}, params = {vol, drift}: y[0], y[1] = drift + vol z_even, drift + vol z_odd of the pair (the GBM step's
 *       exponents) by fm::box_muller_pair_affine (4), _affine_scaled (5; staging and constants of fn 3 with vol2 = vol vol),
 *       _affine2 (6) and _affine_scaled2 (7), the last two with the context's two-level sin/cos tables in device memory.
 * fn 8: one HestonQe::step.  x = {v, z1, z2, S, path id}; params = the scheme's constants {theta, E, c1, c2, drift, K1, K2, K3}
 *       as they stand (not the model's parameters), then {k0, k1, block, elem}: the Philox key and the place of the step's
 *       stream-3 uniform.  A lane takes elements 2j and 2j + 1 as its two paths (the lanes of the last wave beyond n repeat
 *       the last element); y = {v', S', 1 if s2 > 1.5 m^2 (the exponential branch) else 0}.
 * fn 9: the jump count and the jump size of the Bates generators (WithJumps::count and WithJumps::jump of csrc/bates_device.hpp,
 *       the code the product kernels run) on words the caller chooses.  x = {w0, w1, w2, w3, z3}: the four stream-4 words of a
 *       path's Philox block and the stream-5 normal of the step asked for; params = {L, mu_j, sigma_j, comp, T[0..15], elem}:
 *       L = lambda dt (refused outside [0, 1], as by mcg_paths_bates; the count reads the thresholds, not L), the jump
 *       parameters, comp and the sixteen thresholds as mcg_debug_bates_constants returns them, and the element 0..3 whose jump
 *       size is returned.  A lane takes elements 2j and 2j + 1 as its two paths and 128 consecutive elements form a wave, as
 *       in the product; the lanes of the last wave beyond n hold the word 0, which passes no threshold.
 *       y = {cnt, J}: cnt = N_0 + 2^8 N_1 + 2^16 N_2 + 2^24 N_3, the counts of the four words (N_e = #{k : w_e > T[k]}), and
 *       J = comp + N_elem mu_j + sigma_j sqrt(N_elem) z3 (comp where N_elem = 0, whatever z3 holds). */
int mcg_debug_eval_v(mcg_ctx* ctx, int fn, const double* x, int n_in, const double* params, int n_params, double* y, int64_t n);
/* Test hook: the regression solves of the LSM sweeps (csrc/lsm_device.hpp) on moments the caller chooses, launched as the product
 * runs them: one workgroup per element, thread 0 solving, moments and the centred forms' workspace in LDS.  Element i reads
 * moments[i n_moments ..) and params[3i ..) = {min_count, K, mu} and writes out[48i ..): two coefficient blocks of
 * LSM_COEF_STRIDE = 24 doubles (coefficients 0..15, then COUNT, CENTER, REFINE, HINT at 16..19), the second the tangent's
 * dcoef; what a fn does not write is 0.  With p = nb - 1 the moments are the power sums m[0..2p], the cross sums m[2p+1..3p+1]
 * and, for the tangent forms, the tangent's cross sums m[3p+2..4p+2].
 * fn 0: lsm_solve_nb<nb>, nb 1..9, n_moments = 3 nb - 1      fn 1: lsm_solve_nb<nb, true>, n_moments = 4 nb - 1
 * fn 2: lsm_solve_one(nb), the run-time dispatch, as fn 0
 * fn 3: lsm_solve_centered, nb 1..16, n_moments = 3 nb - 1, the moments taken about mu       fn 4: lsm_solve_centered_tan, 4 nb - 1
 * fn 5: n_moments = 1 (nb is not read): out[0] = lsm_rcp(x), out[1] = lsm_rsqrt(x) of x = moments[0]
 * fn 6: lsm_continuation<nb>(c, centre, x), nb 1..9; the element is {c[0..nb), centre, x}, n_moments = nb + 2; out[0].
 * NULL pointers, n < 0, n > 2^20, nb outside the fn's range and any other n_moments are refused with a message and nothing is
 * launched; n = 0 does nothing. */
int mcg_debug_lsm_solve(mcg_ctx* ctx, int fn, int nb, const double* moments, int n_moments, const double* params, double* out,
                        int64_t n);
/* Test hook, host-only: the jump constants of mcg_paths_bates* as its launcher derives them (the same function) -- *comp =
 * -lambda kbar dt and T[k] = floor(min(c_k, 1) 2^32 - 1/2), the word thresholds of the count: uN > c_k <=> word > T[k].  Nothing
 * is validated: the product's bound lambda dt <= 1 is mcg_paths_bates's. */
int mcg_debug_bates_constants(double lambda, double mu_j, double sigma_j, double dt, uint32_t T[16], double* comp);
/* Test hook, host-only: the two tables of fm::sincos_two_level as the contexts upload them, 4096 {cos, sin} pairs each:
 * coarse[i] = (cos, sin)(2 pi i / 4096), fine[j] = (cos, sin)(2 pi (j + 1/2) / 2^24). */
int mcg_debug_sincos2_tables(double* coarse, double* fine);
/* Test hook: which kernel the GBM generators of this context launch -- route 0 = by size (the product's choice), 1 = the
 * narrow kernel (k_gbm_paths), 2 = the wide one (k_gbm_paths_wide), -1 = leave it as it is; *last_route (may be NULL) = what
 * the last GBM launch took (1 or 2; 0 before the first). */
int mcg_debug_gbm_route(mcg_ctx* ctx, int route, int* last_route);
/* Test hook: which kernels mcg_price_branching runs on this context -- route 0 = by size (the product's choice), 1 = one launch
 * over all dates (k_branch_bounds), 2 = a launch per exercise date (k_branch_date), 3 = the same with the indices sorted into
 * bins (k_branch_date_binned), 4 = the XCD-affine gathers (k_branch_date_xcd), -1 = leave route and slice_shift as they are.
 * slice_shift: the gathered row is walked in slices of 2^slice_shift paths (0: the default, 18), raised until the route's slice
 * count holds (8 on routes 1 and 2, 16 on route 3; route 4 has no slices).  A forced route is taken only where it can run: at
 * least one path, one to twelve branches, an exercise date within the maturity, and fewer than 2^30 - 1 paths for routes 3 and
 * 4; otherwise the size decides.  *last_route (may be NULL) = what the last mcg_price_branching took (1..4; 0 before the first).
 * No price depends on the route beyond the order in which a path's branch values are added. */
int mcg_debug_branch_route(mcg_ctx* ctx, int route, int slice_shift, int* last_route);
/* Measurement hook: the path-steps the wavefronts of this context's last mcg_lsm_dual_upper ran through -- for every step a
 * wavefront executed, the outer paths it holds, whether the inner path of each was still alive or not.  inner_steps over this
 * is the share of live lane-steps (1 where no inner path stops before the last date). */
int mcg_debug_lsm_dual_executed(mcg_ctx* ctx, int64_t* executed);
/* Test hook: mcg_lsm_dual_upper works through its outer paths in batches whose workspace (slices x dates x outer paths of the
 * batch, in doubles) stays under a bound, 2^24 by default; `doubles` sets that bound for this context (0: the default).  A batch
 * is a multiple of 512 outer paths and never fewer, so a small bound makes a few hundred outer paths take several batches.
 * No result depends on the bound. */
int mcg_debug_lsm_dual_workspace(mcg_ctx* ctx, size_t doubles);
/* Test hooks of the one-launch LSM sweeps' hand-shake: spin_limit = polling rounds before a wait gives up (0: every
 * wait gives up at once, which drives the time-out -> per-date fall-back on a healthy device; < 0: the default);
 * poll_delay = units of ~4 us by which workgroups other than the reducing one reach their coefficient poll late. */
int mcg_debug_lsm_hooks(mcg_ctx* ctx, long long spin_limit, int poll_delay);
/* Test hooks of the per-date LSM route's exchange (k_lsm_date): mode 1 = workgroup `workgroup` withholds its partial
 * moments at exercise date `date` (a store that never lands: mcg_price_lsm must fail with MCG_ERR_HIP, never return a
 * price); mode 2 = it sends them `delay` x ~4 us AFTER drawing its ticket (a store that lands late: the consumer waits
 * for it, the price is the usual one); mode 0 = off.  spin_limit = polls before a consumer gives up (< 0: default). */
int mcg_debug_lsm_date_fault(mcg_ctx* ctx, int mode, int date, int workgroup, int delay, long long spin_limit);
/* Test hook: workspace bytes one chunk of mcg_batch_price_rows* may use (0: the default, a quarter of free memory). */
int mcg_debug_batch_budget(mcg_ctx* ctx, size_t bytes);
/* Test hook: mcg_batch_price_rows with the same arguments -- the same classification, plan, chunks and launches, the same `out`
 * bit for bit -- that also copies out what the row kernels held for row `row` when its chunk had finished: amp[M] (M = the
 * power of two >= n_steps), comp[n_steps] (both written by k_batch_weights) and block[(n_steps + 1) x n_paths], the row's path
 * matrix, step-major.  MCG_ERR_INVALID, before anything runs, for a row index outside the call, an invalid row (the call answers
 * it with zeros) and a row that is priced singly (more than 1020 steps, more than 256 paths per row, or an order above 4). */
int mcg_debug_batch_row_dump(mcg_ctx* ctx, const mcg_row* rows, int64_t n_rows, int n_paths, double r, double dt, int num_branches,
                             int poly_order, int max_iterations, uint64_t seed, double* out, int64_t row, double* amp, double* comp,
                             double* block);
/* Class-API coalescing (mcg_compat_set_coalescing): at most max_slots calling threads get a matrix slot of the device arena from
 * now on (< 0: the default, 512); a thread that gets none prices on a context of its own.  For the test of that fall-back. */
int mcg_debug_coalesce_slots(int max_slots);
/* The combiner's protocol -- one queue and service thread per kind of call, sleeps and wake-ups, requests queued ahead and taken
 * later or drained, slots, thread exit -- WITHOUT a GPU: n_threads host threads make calls_per_thread calls each, answered by a
 * stand-in for the device that takes ~50 us per round.  *wrong = wrong or missing answers.  Call it in a process that has not
 * used the class API (it switches the combiner to the stand-in for the life of the process). */
int mcg_debug_coalesce_selftest(int n_threads, int calls_per_thread, int* wrong);
/* Test hook, host-only: the decision whether a rank maps a peer's mailbox (1) or all ranks stay on the host mailbox (0),
 * from what it knows about the peer: same process?, does its PCI bus id resolve to a visible device?, the same device?,
 * is peer access available? */
int mcg_debug_peer_decision(int same_process, int bus_id_resolves, int same_device, int can_access_peer);
/* Test hooks, host-only (no GPU needed): the shared segment's protocol on its own -- join `name` as `rank` of
 * `n_ranks` (a stale segment of a crashed job under the same name is never joined), barrier (fails at once on every
 * rank after a time-out or a poison), poison, leave. */
int mcg_debug_shm_attach(const char* name, int n_ranks, int rank, double timeout_s, void** handle);
int mcg_debug_shm_barrier(void* handle);
int mcg_debug_shm_poison(void* handle);
int mcg_debug_shm_detach(void* handle);

#ifdef __cplusplus
}
#endif
#endif /* MCGPU_DEBUG_H */
