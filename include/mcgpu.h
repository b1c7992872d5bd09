/* mcgpu.h -- C ABI of the MI355X-native Monte Carlo path engine (libmcgpu.so).
 *
 * This is the drop-in boundary for the hot path of bcosm/MonteCarloOptionsPricer
 * (RNG -> GBM / rBergomi time-stepping -> per-path payoff -> Longstaff-Schwartz sweep).
 * Plain pointers and sizes only; no C++ or torch types cross it.  The host-side C++ classes with
 * the reference's exact signatures (include/models/RoughVolatility.h, include/models/LSMPricer.h)
 * are thin shims over these entry points; INTEGRATION.md shows the reference-side binding.
 *
 * Conventions
 *   - every function returns an int status (MCG_OK == 0); nothing throws across the ABI;
 *     mcg_last_error() returns a thread-local message for the last non-zero status on this thread.
 *   - all arithmetic and storage is IEEE binary64, like the reference.
 *   - a path matrix lives on the device, STEP-MAJOR: element (step j, path p) at data[j*ld + p],
 *     j = 0..n_steps (column 0 = S0, like RoughVolatility.cpp:344,:354), p = 0..n_paths-1.
 *     The reference's host layout (path-major vector<vector<double>>) is produced/consumed by
 *     mcg_paths_to_host / mcg_paths_from_host.
 *   - RNG contract: Philox4x32-10, key = seed, counter = (global path id, block, stream); a path's
 *     values depend only on (seed, global path id), never on how paths are sharded over GPUs.
 *   - re-entrant: one mcg_ctx per host thread (or per GPU); a ctx owns its stream and workspace.
 */
#ifndef MCGPU_H
#define MCGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcg_ctx mcg_ctx;     /* device, stream, workspace, optional collective */
typedef struct mcg_paths mcg_paths; /* device-resident (n_steps+1) x n_paths matrix      */

enum mcg_status {
    MCG_OK = 0,
    MCG_ERR_INVALID = 1,           /* bad argument                                        */
    MCG_ERR_NO_DEVICE = 2,         /* no usable MI355X / HIP runtime                      */
    MCG_ERR_HIP = 3,               /* a HIP call failed (message has the HIP error)       */
    MCG_ERR_OOM = 4,               /* device allocation failed                            */
    MCG_ERR_HISTORY_TOO_SMALL = 5, /* == RoughVolatility.cpp:317-319                      */
    MCG_ERR_EMPTY_PATHS = 6,       /* == LSMPricer.cpp:28-30                              */
    MCG_ERR_COMM = 7               /* collective failed                                   */
};

/* kernels whose device time mcg_timing_get reports */
enum mcg_kernel {
    MCG_K_GBM = 0,        /* GBM path generation (+ fused payoff partials)  */
    MCG_K_RBERGOMI = 1,   /* rBergomi path generation                       */
    MCG_K_PAYOFF = 2,     /* terminal payoff reduction over a stored matrix */
    MCG_K_LSM_SWEEP = 3,  /* LSM sweep: the one launch, or the queued per-date sequence (launches, gaps, collectives) */
    MCG_K_LSM_SOLVE = 4,  /* LSM per-date reduce+solve kernels              */
    MCG_K_TRANSPOSE = 5,  /* layout change for the host class API           */
    MCG_K_ASYM = 6,       /* AsymptoticAnalysis boundary scan               */
    MCG_K_MARTINGALE = 7, /* MartingaleOptimization primal/offset/dual scans */
    MCG_K_BRANCHING = 8,  /* BranchingProcesses suffix-max + bounds kernels   */
    MCG_K_BATCH = 9,      /* the six kernels of mcg_batch_price_rows (one span) */
    MCG_K_EXOTIC = 10,    /* path statistics + contract book of mcg_path_stats / mcg_price_exotics / mcg_greeks_exotics / mcg_price_barriers_bridge */
    MCG_K_HESTON = 11,    /* Heston path generation (+ fused payoff partials) */
    MCG_K_MULTI = 12,     /* multi-asset GBM path generation and mcg_paths_combine */
    MCG_K_LOCALVOL = 13,  /* local-volatility path generation (+ fused payoff partials) */
    MCG_K_LSM_APPLY = 14, /* mcg_lsm_apply: the forward pass of an exercise policy over a stored matrix */
    MCG_K_LSM_DUAL = 15,  /* mcg_lsm_dual_upper: the nested simulation and the martingale recursion (two launches a batch) */
    MCG_K_SOBOL = 16,     /* Sobol' path generation, GBM and local volatility (+ fused payoff partials) */
    MCG_K_COUNT = 17
};

const char* mcg_last_error(void);
const char* mcg_version(void);
int mcg_device_count(int* count);

/* ---- context ---------------------------------------------------------------------------- */
/* mcg_init: the ctx creates its own non-blocking stream.
 * mcg_init_on_stream: the ctx launches on the caller's hipStream_t (e.g. torch's current stream);
 * NULL there means the legacy default stream.  Use this form when a collective installed with
 * mcg_set_allreduce enqueues work on that same stream. */
int mcg_init(mcg_ctx** ctx, int device);
int mcg_init_on_stream(mcg_ctx** ctx, int device, void* stream);
int mcg_finalize(mcg_ctx* ctx);
int mcg_synchronize(mcg_ctx* ctx);
int mcg_trim(mcg_ctx* ctx); /* release cached device buffers */

/* Optional sum-all-reduce used when paths are sharded over several GPUs (one process per GPU).
 * fn must sum `count` doubles at device pointer `buf` in place over all ranks, ordered on
 * `stream` (a hipStream_t).  With a collective installed, mcg_price_european / mcg_price_lsm
 * return the GLOBAL price on every rank.  Payloads are 3 doubles (European) or 3p+2 doubles per
 * exercise date (LSM regression moments). */
typedef int (*mcg_allreduce_fn)(void* user, double* buf, int count, void* stream);
int mcg_set_allreduce(mcg_ctx* ctx, mcg_allreduce_fn fn, void* user);

/* Built-in RCCL collective (librccl is dlopen'ed on first use).  The 128-byte id comes from rank
 * 0's mcg_comm_unique_id and is broadcast by the launcher (torch.distributed store, MPI, ...). */
int mcg_comm_unique_id(unsigned char id[128]);
int mcg_comm_init_rank(mcg_ctx* ctx, const unsigned char id[128], int n_ranks, int rank);

/* Node-local collective over POSIX shared memory (one process per GPU, all on one host): `name` is a segment name
 * starting with '/', the same on every rank and unique to the job (rank 0 creates it, mcg_finalize removes it).
 * Installs a host all-reduce for the payoff sums AND lets the one-launch LSM sweeps exchange their per-date
 * regression moments between the GPUs INSIDE the kernel, through a device-mapped mailbox in the segment: a sharded
 * American price then costs one launch per GPU instead of three launches and one collective per exercise date.
 * At most 16 ranks. */
int mcg_comm_init_shm(mcg_ctx* ctx, const char* name, int n_ranks, int rank);
/* The ranks may also be THREADS of one process, one ctx each (one host thread per GPU -- the shape of the reference's own
 * OpenMP driver): every collective call then blocks until all of them have made it, so each rank needs its own thread. */

/* Opt-in, after mcg_comm_init_shm, collective over its ranks: keep the in-kernel mailbox in the GPUs' own HBM instead
 * of the host segment.  Every rank allocates a mailbox in device memory, exports it (hipIpcGetMemHandle, handed over
 * through the segment) and opens the peers' (hipIpcOpenMemHandle: on a multi-GPU node, peer memory over xGMI); a
 * reducing workgroup then PUSHES its moments into every peer's mailbox and polls local memory only.  Taken into use
 * only if every rank got through allocation, export, open and an in-kernel ping over the mappings; otherwise all
 * ranks stay on the host mailbox together (status MCG_OK, *active = 0).  enable = 0 goes back to the host mailbox.
 * The host segment keeps serving the barrier, the flags and the host all-reduce.
 * Lifetime: a rank's mailbox outlives every peer that maps it.  Between processes the IPC mapping sees to that by itself;
 * rank THREADS of one process use the owner's pointer as it stands, so the library counts them in the segment: a rank that
 * finalises (or switches back) while a rank thread still holds its mailbox leaves the mailbox to the LAST of them to let go,
 * which frees it -- nobody waits, nothing leaks, in whatever order the rank threads' contexts are closed. */
int mcg_comm_shm_peer_mailbox(mcg_ctx* ctx, int enable, int* active);

/* What collective this ctx holds and how many ranks it has SEEN: kind 0 none, 1 callback (mcg_set_allreduce),
 * 2 built-in RCCL, 3 node-local shared memory (host mailbox), 4 the same with the peer-memory mailbox active;
 * n_ranks / rank as given at set-up; seen_ranks = ncclCommCount of the communicator (kind 2) or the number of
 * processes attached to the segment (kinds 3, 4), 0 for a callback.  Any out pointer may be NULL. */
int mcg_comm_info(mcg_ctx* ctx, int* kind, int* n_ranks, int* rank, int* seen_ranks);

/* ---- path generation (replaces RoughVolatility.cpp:346-365, device side) ---------------- */
/* GBM: the stepping loop of RoughVolatility.cpp:354-364 with v == sigma^2.
 * Paths [path_begin, path_begin + n_paths) of the global Philox stream `seed`. */
int mcg_paths_gbm(mcg_ctx* ctx, uint64_t seed, double S0, double r, double sigma, double dt,
                  int n_steps, uint64_t path_begin, int64_t n_paths, mcg_paths** out);

/* rBergomi as the reference simulates it (RoughVolatility.cpp:342-364) with explicit parameters.
 * rho is accepted for interface parity; it does not change the law.
 * Paths are generated in pairs: path_begin must be even.
 * A path's draws depend on (seed, global path id) only, and repeated calls are bit-identical.  Shards: from 17 to 2048 steps a
 * wavefront picks the exponential of a tile of price steps by the largest exponent |ln(S_{n+1}/S_n)| among ITS paths (up to 0.1,
 * up to 0.34, beyond), so a shard is promised to reproduce the one-call matrix bit for bit only if it begins at a multiple of
 * 2 * rb_pairs_per_block(Mz) = 8192 / Mz columns (8 at 2048; Mz = n_steps rounded up to a power of two): the wavefronts are then
 * the same sets of paths.  A shard that begins at another even column agrees to rounding (1e-15 relative); it has the same bits
 * as long as every wavefront takes the same exponential in both runs, which is the rule while the exponents stay below 0.1, but no
 * promise: the unused steps of an unfinished last tile vote too.  Up to 16 and beyond 2048 steps a path is computed on its own and
 * every split at an even column is bit-identical. */
int mcg_paths_rbergomi(mcg_ctx* ctx, uint64_t seed, double S0, double r, double xi, double H,
                       double eta, double rho, double dt, int n_steps, uint64_t path_begin,
                       int64_t n_paths, mcg_paths** out);

/* Fused GBM generation + terminal payoff reduction in one kernel (the measured headline path):
 * writes the full matrix AND leaves {sum payoff, sum payoff^2, n} for mcg_price_european to reuse
 * when called with the same (K, is_call). */
int mcg_paths_gbm_payoff(mcg_ctx* ctx, uint64_t seed, double S0, double r, double sigma, double dt,
                         int n_steps, uint64_t path_begin, int64_t n_paths, double K, int is_call,
                         mcg_paths** out);
int mcg_paths_rbergomi_payoff(mcg_ctx* ctx, uint64_t seed, double S0, double r, double xi, double H,
                              double eta, double rho, double dt, int n_steps, uint64_t path_begin,
                              int64_t n_paths, double K, int is_call, mcg_paths** out);

/* Heston stochastic volatility, full-truncation log-Euler.  For step n = 0 .. n_steps-1, with S_0 = S0 and v_0 = v0:
 *   z1 = draw n of (path, price driver),  z2 = draw n of (path, volatility driver)
 *        (Philox streams 0 and 1 of `seed`: block n >> 2, element n & 3 -- the RNG contract of DESIGN.md)
 *   vp = max(v_n, 0);  s = sqrt(vp * dt)
 *   S_{n+1} = S_n * exp((r - vp/2) dt + s (rho z2 + sqrt(1 - rho^2) z1))
 *   v_{n+1} = v_n + kappa (theta - vp) dt + sigma_v s z2
 * Row n of *out is S_n.  var_out may be NULL; otherwise *var_out receives a second matrix of the same shape whose row n is
 * v_n, untruncated (negative where the scheme overshoots; the caller frees both).  A path depends only on (seed, global
 * path id): paths [path_begin, path_begin + n_paths) of any split reproduce the one-call matrix bit for bit, and repeated
 * calls are bit-identical.  path_begin may be odd.
 * The price matrix is marked as generated, like GBM's (S_T proportional to e^{rT}): mcg_greeks_european with sigma <= 0
 * returns price, delta, rho and dual delta on it, gamma and vega NaN.  The variance matrix is a plain matrix.
 * The _payoff form also leaves {sum payoff, sum payoff^2, n} for mcg_price_european, as mcg_paths_gbm_payoff does (all-reduced
 * on a ctx with a collective).
 * MCG_ERR_INVALID with a message: a NULL ctx or out; a non-finite S0, r, v0, kappa, theta, sigma_v, rho, dt (or K);
 * S0 <= 0; dt <= 0; v0, kappa, theta or sigma_v < 0; |rho| > 1; n_steps < 1; n_paths < 0.
 * Out of scope: exact (Broadie-Kaya) schemes; QE's martingale correction and a caller-chosen psi_c or gamma weights;
 * sensitivities to the Heston parameters; Heston in the batch rows, the coalescing layer and the drop-in classes. */
int mcg_paths_heston(mcg_ctx* ctx, uint64_t seed, double S0, double r, double v0, double kappa, double theta,
                     double sigma_v, double rho, double dt, int n_steps, uint64_t path_begin, int64_t n_paths,
                     mcg_paths** out, mcg_paths** var_out);
int mcg_paths_heston_payoff(mcg_ctx* ctx, uint64_t seed, double S0, double r, double v0, double kappa, double theta,
                            double sigma_v, double rho, double dt, int n_steps, uint64_t path_begin, int64_t n_paths,
                            double K, int is_call, mcg_paths** out, mcg_paths** var_out);

/* Heston by Andersen's quadratic-exponential (QE) scheme (Andersen 2008, without the martingale correction; central
 * weights gamma1 = gamma2 = 1/2).  Unlike the Euler scheme above it is unbiased at a few steps a year, also where
 * 2 kappa theta < sigma_v^2.  Constants, computed once on the host in binary64:
 *   E  = exp(-kappa dt)
 *   c1 = sigma_v^2 E (1-E)/kappa
 *   c2 = theta sigma_v^2 (1-E)^2 / (2 kappa)        kappa == 0: c1 = sigma_v^2 dt, c2 = 0
 *   g  = kappa rho / sigma_v - 1/2
 *   K0 = -rho kappa theta dt / sigma_v
 *   K1 = dt g/2 - rho/sigma_v
 *   K2 = dt g/2 + rho/sigma_v
 *   K3 = K4 = dt (1 - rho^2)/2
 *   psi_c = 1.5
 * For step n = 0 .. n_steps-1, with S_0 = S0 and v_0 = v0 >= 0:
 *   z1 = draw n of Philox stream 0,  z2 = draw n of Philox stream 1    (as above: block n >> 2, element n & 3)
 *   u  = (word (n & 3) of block (n >> 2) of Philox stream 3 + 0.5) * 2^-32      in (0, 1)
 *        (stream 2 belongs to the branching-process kernels)
 *   m  = theta + (v_n - theta) E                      kappa == 0: m = v_n
 *   s2 = v_n c1 + c2
 *   psi = s2 / m^2
 *   m == 0          : v' = 0
 *   psi <= psi_c    : q = 2/psi;  b2 = q - 1 + sqrt(q) sqrt(q - 1);  v' = m/(1 + b2) * (sqrt(b2) + z2)^2
 *   psi >  psi_c    : p = (psi - 1)/(psi + 1);  beta = (1 - p)/m;  v' = 0 if u <= p else ln((1 - p)/(1 - u)) / beta
 *   S_{n+1} = S_n * exp(r dt + K0 + K1 v_n + K2 v' + sqrt(K3 v_n + K4 v') z1)
 *   v_{n+1} = v'
 * u is used only where psi > psi_c; a path's result does not depend on whether its neighbours needed theirs.
 * Everything else is the contract of mcg_paths_heston*: row n of *out is S_n; var_out may be NULL, otherwise row n of *var_out
 * is v_n, which is never negative here; ownership, the `generated` mark of the price matrix (mcg_greeks_european with
 * sigma <= 0: price, delta, rho and dual delta), shard and repeat bit-identity, an odd path_begin, the sums the _payoff form
 * leaves (all-reduced on a ctx with a collective) and the accounting under MCG_K_HESTON are the same.
 * MCG_ERR_INVALID with a message: everything mcg_paths_heston rejects, and sigma_v <= 0 (the K's divide by it: use
 * mcg_paths_heston there).  kappa = 0, theta = 0, v0 = 0 and |rho| = 1 are valid and give finite matrices. */
int mcg_paths_heston_qe(mcg_ctx* ctx, uint64_t seed, double S0, double r, double v0, double kappa, double theta,
                        double sigma_v, double rho, double dt, int n_steps, uint64_t path_begin, int64_t n_paths,
                        mcg_paths** out, mcg_paths** var_out);
int mcg_paths_heston_qe_payoff(mcg_ctx* ctx, uint64_t seed, double S0, double r, double v0, double kappa, double theta,
                               double sigma_v, double rho, double dt, int n_steps, uint64_t path_begin, int64_t n_paths,
                               double K, int is_call, mcg_paths** out, mcg_paths** var_out);

/* Bates: Heston plus compound-Poisson log-normal jumps in the price (Merton's jumps; with kappa = sigma_v = rho = 0 and
 * v0 = theta = sigma^2 under MCG_HESTON_EULER the model is Merton's jump-diffusion).  The jump component is applied per step
 * on top of either variance scheme above and is exact in law: a compound-Poisson increment is independent of the diffusion,
 * so the only time-stepping bias is the base scheme's.  Constants, computed once on the host in binary64:
 *   L     = lambda * dt                       (required: 0 <= L <= 1)
 *   kbar  = exp(mu_J + sigma_J^2 / 2) - 1
 *   comp  = -lambda * kbar * dt               (martingale compensator, per step)
 *   t_0 = exp(-L);  t_j = t_{j-1} * L / j;  c_k = c_{k-1} + t_k   (c_0 = t_0),  k = 0..15     Poisson CDF, summed in this order
 * For step n = 0 .. n_steps-1 (block n >> 2, element n & 3, the RNG contract of DESIGN.md):
 *   uN = (word (n & 3) of block (n >> 2) of Philox stream 4 + 0.5) * 2^-32
 *   N  = #{ k in 0..15 : uN > c_k }                                         number of jumps in the step
 *   z3 = draw n of Philox stream 5  (two Box-Muller pairs per block, exactly as streams 0 and 1 are turned into normals)
 *   J  = comp + N mu_J + sigma_J sqrt(N) z3
 *   S_{n+1} = S_n * exp( <the base scheme's exponent of this step> + J )    one exponential
 *   v_{n+1}   as the base scheme gives it (jumps do not touch the variance)
 * z3 is used only where N > 0; a path's result never depends on whether its neighbours jumped.  Streams 0, 1 and 3 are used
 * exactly as by the base scheme; stream 2 stays the branching-process kernels'.  With L <= 1, 1 - c_15 < 2^-33: no uniform
 * lies above c_15 and the count never reaches a cap.  (The device decides uN > c_k as word > floor(c_k 2^32 - 1/2), which is
 * the same statement: c_k 2^32 - 1/2 is exact in binary64.)  Both are tested: the equivalence on the words next to every
 * threshold and the last threshold at L = 1 in tests/test_bates_reference.py; on the device, words exactly on a threshold
 * through mcg_paths_bates and every threshold, every count up to the largest (12 at L = 1) and the word 2^32 - 1 through the
 * hook of include/mcgpu_debug.h (fn 9), in tests/test_gpu_bates.py.
 * scheme: MCG_HESTON_EULER, the step of mcg_paths_heston*, or MCG_HESTON_QE, that of mcg_paths_heston_qe*.
 * Everything else is the contract of mcg_paths_heston*: row n of *out is S_n; var_out may be NULL, otherwise row n of *var_out
 * is v_n; ownership, an odd path_begin, shard and repeat bit-identity, the sums the _payoff form leaves (all-reduced on a ctx
 * with a collective), the accounting under MCG_K_HESTON and the `generated` mark of the price matrix (S_T is still proportional
 * to e^{rT} and to S0: mcg_greeks_european with sigma <= 0 fills price, delta, rho and dual delta) are the same.
 * lambda = 0 reproduces mcg_paths_heston* / mcg_paths_heston_qe* bit for bit, both matrices and the sums (comp is then a zero and
 * every N is 0).  lambda = 0, sigma_j = 0 and mu_j = 0 are valid and give finite matrices.
 * MCG_ERR_INVALID with a message: everything the chosen base scheme rejects (sigma_v <= 0 for QE); a non-finite lambda, mu_j or
 * sigma_j; lambda < 0; sigma_j < 0; lambda * dt > 1 (use more steps); |mu_j| > 1 or sigma_j > 1 (log-jump sizes far beyond any
 * calibrated equity model; within the range a step's |J| stays below 50, and the summed exponent inside the domain of the
 * device's exponential, which is any finite argument); a scheme that is neither value.
 * Out of scope: jumps in the variance (SVJJ); double-exponential (Kou) jump sizes; sensitivities to the jump parameters; jumps
 * in the rBergomi generator; Bates in the batch rows, the coalescing layer and the drop-in classes. */
enum mcg_heston_scheme { MCG_HESTON_EULER = 0, MCG_HESTON_QE = 1 };
int mcg_paths_bates(mcg_ctx* ctx, uint64_t seed, double S0, double r, double v0, double kappa, double theta, double sigma_v,
                    double rho, double lambda, double mu_j, double sigma_j, double dt, int n_steps, uint64_t path_begin,
                    int64_t n_paths, int scheme, mcg_paths** out, mcg_paths** var_out);
int mcg_paths_bates_payoff(mcg_ctx* ctx, uint64_t seed, double S0, double r, double v0, double kappa, double theta,
                           double sigma_v, double rho, double lambda, double mu_j, double sigma_j, double dt, int n_steps,
                           uint64_t path_begin, int64_t n_paths, int scheme, double K, int is_call, mcg_paths** out,
                           mcg_paths** var_out);

/* Multi-asset GBM: n_assets correlated geometric Brownian motions per path, and the reduction of the n_assets matrices to one
 * -- a basket (negative weights: a spread), the best or the worst of the weighted assets (rainbows; weights 1 / S0_a give
 * performance options).  Every pricer takes the combined matrix as it takes any other: European, the exotics book, LSM,
 * LSM2 (paths = best-of, state = worst-of), Greeks, sharded prices.
 *
 * mcg_cholesky_corr (host only, no ctx): the lower Cholesky factor L of the correlation matrix `corr`, both row-major n x n;
 * the part of L above the diagonal is written as 0.  Cholesky-Banachiewicz order, in binary64 with no fused multiply-add:
 * for j = 0 .. n-1
 *   d_j  = C_jj - sum_{k<j} L_jk^2                       (the sum from 0, in increasing k, then one subtraction)
 *   L_jj = sqrt(d_j)
 *   L_ij = (C_ij - sum_{k<j} L_ik L_jk) / L_jj   for i > j  (likewise)
 * MCG_ERR_INVALID with a message: NULL corr or L; n outside [1, 8]; a non-finite entry; C_jj != 1; C_ij != C_ji; |C_ij| > 1;
 * some d_j <= 1e-10 ("not positive definite": perfectly correlated assets are out of scope).
 *
 * mcg_paths_gbm_multi.  Constants, computed once on the host in binary64 (L = mcg_cholesky_corr(corr)):
 *   drift_a = (r - q_a - sigma_a^2 / 2) dt                  q: dividend yields, NULL = zeros
 *   A_ab    = sigma_a sqrt(dt) L_ab,  b <= a
 * For step n = 0 .. n_steps-1, S^a_0 = S0_a:
 *   z_b = draw n of Philox stream s(b) of (seed, global path id): block n >> 2, element n & 3, two Box-Muller pairs per block
 *         (the RNG contract of DESIGN.md);  s(0) = 0, the price driver;  s(b) = 15 + b for b >= 1: streams 16..22.  Streams
 *         1..5 stay with the Heston, QE, branching-process and Bates kernels.
 *   e_a = drift_a + sum_{b<=a} A_ab z_b                     (added in increasing b; the device fuses each multiply-add)
 *   S^a_{n+1} = S^a_n * exp(e_a)                            one exponential per asset and step
 * Combined row, every row including row 0, with x_a = w_a S^a_n (weights NULL: all 1):
 *   MCG_C_BASKET    acc = x_0, then acc = fma(w_a, S^a_n, acc) for a = 1 .. in asset order
 *   MCG_C_BEST_OF   max_a x_a
 *   MCG_C_WORST_OF  min_a x_a
 * assets_out: an array of n_assets handles (row n of assets_out[a] is S^a_n), or NULL; combined_out: one handle of the same
 * shape, or NULL -- not both NULL; a non-NULL combined_out needs combine != MCG_C_NONE (and weights are unused for
 * MCG_C_NONE).  With assets_out NULL the d prices of a path never leave the registers: 8 B per path-step are stored however
 * many assets there are.  The combined matrix of the fused call equals mcg_paths_combine of the asset matrices bit for bit, and
 * the asset matrices have the same bits whether or not a combination was asked for.  A path depends on (seed, global path id)
 * only: any split into shards reproduces the one-call matrices bit for bit, repeated calls are bit-identical, path_begin may
 * be odd, n_paths = 0 gives empty matrices.  Asset a depends on S0, q and sigma of the assets 0 .. a and on the leading
 * (a + 1) x (a + 1) block of corr only, bit for bit, whatever n_assets is: row a of the Banachiewicz loop reads nothing beyond
 * that block, and e_a sums the drivers b <= a in one fixed order -- the first d asset matrices of a call are the matrices of
 * the d-asset call on the leading block (tests/test_gpu_gbm_multi.py: test_asset_prefixes_are_bit_identical, d = 1 .. 8;
 * tests/test_gbm_multi_reference.py for the factor and for the scheme).  n_assets = 1 is valid: the asset matrix is then the law of mcg_paths_gbm, from the
 * same stream (not its bits: that kernel folds sigma into the logarithm).  Asset matrices are marked `generated`; a combined
 * matrix is `generated` iff all its inputs are, for both entry points: dS_T/dr = T S_T holds for sums, max and min
 * (mcg_greeks_european's rho).  One launch, booked under MCG_K_MULTI.
 * On any error every output handle is NULL (the n_assets entries of assets_out where n_assets is in range) and nothing stays
 * allocated.
 * MCG_ERR_INVALID with a message: NULL ctx, S0, sigma or corr; both outputs NULL; n_assets outside [1, 8]; a non-finite S0_a,
 * r, q_a, sigma_a, dt, weight or correlation; S0_a <= 0; sigma_a < 0 (0 is valid); dt <= 0; n_steps < 1; n_paths < 0; everything
 * mcg_cholesky_corr rejects; a combine that is none of the four values, or MCG_C_NONE with combined_out; a weight <= 0 for
 * best-of / worst-of.  combine and weights are checked whenever combine != MCG_C_NONE, also where combined_out is NULL and
 * nothing uses them.
 *
 * mcg_paths_combine: *out = the combination `kind` of n_assets matrices of this ctx with equal n_paths and n_steps -- from any
 * generator (Heston, rBergomi, ...) or uploaded.  One launch of a streaming kernel ((n_assets + 1) * 8 B per path-step), booked
 * under MCG_K_MULTI.  MCG_ERR_INVALID with a message: NULL ctx, assets, an assets[a] or out; n_assets outside [1, 8]; a kind
 * other than the three combinations; a non-finite weight, or one <= 0 for best-of / worst-of; a matrix of another ctx; mismatched
 * shapes.  *out is NULL on error.
 *
 * Out of scope: fused terminal payoff sums; correlated Heston or rBergomi assets; perfectly correlated (semi-definite)
 * matrices; more than 8 assets; Greeks with respect to individual spots or correlations; multi-asset rows in the batch rows,
 * the coalescing layer and the drop-in classes. */
enum mcg_combine_kind { MCG_C_NONE = -1, MCG_C_BASKET = 0, MCG_C_BEST_OF = 1, MCG_C_WORST_OF = 2 };
int mcg_cholesky_corr(const double* corr, int n, double* L);
int mcg_paths_gbm_multi(mcg_ctx* ctx, uint64_t seed, int n_assets, const double* S0, double r, const double* q,
                        const double* sigma, const double* corr, double dt, int n_steps, uint64_t path_begin, int64_t n_paths,
                        int combine, const double* weights, mcg_paths** assets_out, mcg_paths** combined_out);
int mcg_paths_combine(mcg_ctx* ctx, const mcg_paths* const* assets, int n_assets, int kind, const double* weights,
                      mcg_paths** out);

/* Local volatility (Dupire): dS = (r - q) S dt + sigma(t, S) S dW, with sigma given on a rectangular grid in time and spot
 * log-moneyness x = ln(S / S0) -- the model that prices barriers, Asians and lookbacks consistently with a quoted smile.
 *
 * The surface: n_t time knots times[0] < ... < times[n_t - 1], n_t in [1, 64]; n_x equidistant nodes
 * x_j = x_min + j (x_max - x_min) / (n_x - 1), n_x in [2, 128]; values sigma[i * n_x + j] >= 0 at (times[i], x_j).  Bilinear in
 * (t, x), flat beyond the first and the last knot and outside [x_min, x_max].
 *
 * mcg_localvol_table (host only, no ctx): the surface as the steps read it, in binary64 with no fused multiply-add.
 *   n_slices = 1 if n_t == 1, else n_steps
 *   slice n belongs to step n at t = (double)n * dt -- the left end of the step decides:
 *     t <= times[0]: row 0;   t >= times[n_t - 1]: the last row;   otherwise the i with times[i] <= t < times[i + 1],
 *     g = (t - times[i]) / (times[i + 1] - times[i]),  sigma_{n,j} = sigma_{i,j} + g * (sigma_{i+1,j} - sigma_{i,j})
 *   a_{n,j} = sigma_{n,j} * sqrt(dt)
 *   d_{n,j} = a_{n,j+1} - a_{n,j},  j = 0 .. n_x - 2
 *   table_out[(n * (n_x - 1) + j) * 2 + {0, 1}] = {a_{n,j}, d_{n,j}}       n_slices * (n_x - 1) * 2 doubles: one 16-byte entry
 *                                                                          holds all a path-step needs of the surface
 * Further constants of the generator, likewise:  inv_dx = (n_x - 1) / (x_max - x_min),  u0 = -x_min * inv_dx,  m = (r - q) * dt.
 *
 * mcg_paths_localvol.  For step n = 0 .. n_steps-1, with S_0 = S0 and X_0 = 0:
 *   z = draw n of Philox stream 0 of (seed, global path id): block n >> 2, element n & 3   (the RNG contract of DESIGN.md)
 *   u = min(max(fma(X_n, inv_dx, u0), 0), n_x - 1)
 *   j = min((int)u, n_x - 2);  f = u - j
 *   a = fma(f, d_{s,j}, a_{s,j})                      s = n, or 0 when n_slices == 1
 *   e = fma(a, z, fma(-0.5 a, a, m))
 *   X_{n+1} = X_n + e
 *   S_{n+1} = S_n * exp(e)                            one exponential
 * Row n of *out is S_n.  X is the path's own running log-moneyness, never recomputed from S.  a is continuous in X, so a
 * last-bit difference in u at a node moves the result by a last bit only.  A flat surface gives the law of mcg_paths_gbm (and
 * of mcg_paths_gbm_multi with one asset and the same q) from the same stream -- not its bits: the exponent is grouped
 * differently.
 * A path depends on (seed, global path id) only: any split into shards reproduces the one-call matrix bit for bit, repeated
 * calls are bit-identical, path_begin may be odd, n_paths = 0 gives an empty matrix.
 * The matrix is NOT marked as generated: S_T is homogeneous in S0 but not proportional to e^{rT}, so for mcg_greeks_european
 * it is a plain matrix (rho NaN).
 * The _payoff form also leaves {sum payoff, sum payoff^2, n} for mcg_price_european, as mcg_paths_gbm_payoff does (all-reduced
 * on a ctx with a collective).  One launch per call, booked under MCG_K_LOCALVOL, behind the upload of the table on the ctx's
 * stream.
 * MCG_ERR_INVALID with a message, *out NULL and nothing left allocated: a NULL ctx, out, times, sigma (or table_out); n_t outside
 * [1, 64]; n_x outside [2, 128]; times that are not finite or not strictly increasing; a non-finite or negative sigma (zero is
 * valid); a non-finite S0, r, q, dt, x_min, x_max (or K); S0 <= 0; dt <= 0; x_min >= x_max; n_steps < 1; n_paths < 0.
 * Out of scope: building the surface from implied volatilities (Dupire's formula); term structures of r and q; interpolation
 * other than bilinear in (t, x); stochastic-local-volatility; local volatility in the multi-asset generator, the batch rows,
 * the coalescing layer and the drop-in classes; sensitivities to surface nodes. */
int mcg_localvol_table(const double* times, int n_t, int n_x, const double* sigma, double dt, int n_steps, double* table_out);
int mcg_paths_localvol(mcg_ctx* ctx, uint64_t seed, double S0, double r, double q, const double* times, int n_t, double x_min,
                       double x_max, int n_x, const double* sigma, double dt, int n_steps, uint64_t path_begin, int64_t n_paths,
                       mcg_paths** out);
int mcg_paths_localvol_payoff(mcg_ctx* ctx, uint64_t seed, double S0, double r, double q, const double* times, int n_t,
                              double x_min, double x_max, int n_x, const double* sigma, double dt, int n_steps,
                              uint64_t path_begin, int64_t n_paths, double K, int is_call, mcg_paths** out);

/* Randomised quasi-Monte Carlo: Sobol' paths with a Brownian bridge, for GBM and local volatility.
 *
 * Path `i` (its global id, path_begin + column) is point i of a Sobol' sequence, step by step a pure function of
 * (table, i) as a Philox draw is one of (seed, i): repeated calls are bit-identical, any split into shards (odd path_begin
 * included) reproduces the one-call matrix bit for bit, and the matrix is the plain step-major one every pricer takes.
 * mcg_price_european's std_err on such a matrix is the iid formula and is NOT an error bar of a Sobol' estimate: generate a
 * few replicates (same seed, replicate = 0, 1, ...), price each, and hand the prices to mcg_rqmc_combine.
 *
 * The point set (mcg_sobol_table; host only, no ctx).  Direction numbers: Joe and Kuo's new-joe-kuo-6, the first
 * MCG_SOBOL_MAX_DIMS dimensions, 32 bits, V[d][b] with its leading digit in bit 31 (b = 0 .. 31).  Point i, dimension d:
 *     g = i ^ (i >> 1);   x = shift[d] ^ XOR over the set bits b of g of V'[d][b]
 * With MCG_SOBOL_PLAIN (V' = V, shift = 0) x is scipy's Sobol(d, scramble=False, bits=32) point i times 2^32.
 * Random words of a scramble: the high 32 bits of successive outputs of ONE SplitMix64 stream per (seed, replicate),
 *     next(s):  s += 0x9E3779B97F4A7C15;  z = s;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *               z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)                  (all mod 2^64)
 *     h(x) = the output of next() on the state x;      the stream starts from the state  s = h(h(seed) ^ (uint64_t)replicate)
 * For d = 0 .. n_dims-1 in turn the stream yields 33 words (under MCG_SOBOL_SHIFT too, which uses the first only, so that
 * both scrambles of a (seed, replicate) share their shifts): shift[d] first, then w_0 .. w_31.
 *   MCG_SOBOL_SHIFT      V' = V, the digital shift shift[d].
 *   MCG_SOBOL_LMS_SHIFT  Matousek's linear matrix scramble ahead of the shift: M_j = ((w_j >> (31 - j)) | 1) << (31 - j), i.e.
 *                        bit 31-j set, random bits above it, zeros below;  bit (31 - j) of V'[d][b] = parity(M_j & V[d][b]).
 * v_out: n_dims * 32 words, V'[d][b] at v_out[d * 32 + b];  shift_out: n_dims words.
 *
 * The normal: u = (x + 0.5) * 2^-32 in (0, 1) and z = Phi^-1(u) by Wichura's AS241 (PPND16) in binary64: with q = u - 0.5,
 * |q| <= 0.425 takes its central rational in r = 0.180625 - q q times q; otherwise r = sqrt(-log(min(u, 1 - u))) (<= 4.8, so
 * only the branch r <= 5 exists) takes its rational in r - 1.6, negated for q < 0.  Each polynomial by Horner's rule.
 *
 * The bridge (mcg_sobol_bridge; host only): the schedule in dimension order, entry d = {t, l, r, wl, wr, sd} meaning
 *     B(t) = wl * B(l) + (wr * B(r) + sd * z_d)          B in units of sqrt(dt), B(0) = 0
 *   bridge = 1: entry 0 is the endpoint {n, 0, 0, 0, 0, sqrt(n)}; then the tree bridge(0, n), where bridge(l, r) stops if
 *     r - l < 2 and otherwise has the node m = (l + r) / 2 (integer) with parents l and r, wl = (r - m) / (r - l),
 *     wr = (m - l) / (r - l), sd = sqrt((m - l) (r - m) / (r - l)), and the children bridge(l, m), bridge(m, r).  The nodes
 *     take the dimensions 1, 2, ... breadth first: level by level, left to right.
 *   bridge = 0: the identity, entry d = {d + 1, d, d, 1, 0, 1}.
 * The increment of step t is z_t = B(t + 1) - B(t) under bridge = 1 and z_t itself (dimension t) under bridge = 0.  In units of
 * sqrt(dt) the map from the n normals to the n increments is orthogonal, so the law of the paths is that of the Philox
 * generators: only the assignment of the dimensions changes.
 *
 * mcg_paths_gbm_sobol: S_{t+1} = S_t * exp(m + s z_t), m = (r - sigma^2 / 2) dt, s = sigma sqrt(dt), the exponent as one fma.
 * mcg_paths_localvol_sobol: the step of mcg_paths_localvol with z = z_t.  Marks, sums of the _payoff forms and rejections are
 * those of the Philox namesakes; one launch per call, booked under MCG_K_SOBOL.
 * Limits (MCG_ERR_INVALID with a message, no launch, *out untouched): a NULL sobol; n_steps outside [1, 1024]; path_begin +
 * n_paths > 2^32; scramble outside {0, 1, 2}; bridge outside {0, 1}.
 * Out of scope: the Heston family (how two or three driver streams per step interleave under a bridge is a decision of its
 * own), the rBergomi, multi-asset and in-register twin generators.
 *
 * mcg_rqmc_combine: the mean of n replicate estimates and std(ddof = 1) / sqrt(n); n < 2 (or a NULL argument) is
 * MCG_ERR_INVALID. */
#define MCG_SOBOL_MAX_DIMS 1024
enum mcg_sobol_scramble { MCG_SOBOL_PLAIN = 0, MCG_SOBOL_SHIFT = 1, MCG_SOBOL_LMS_SHIFT = 2 };
typedef struct {
    uint64_t seed;
    uint32_t replicate;
    int scramble; /* enum mcg_sobol_scramble */
    int bridge;   /* 0: dimensions in time order, 1: Brownian bridge */
} mcg_sobol;
typedef struct {
    int t, l, r;       /* time index of the node and of its parents */
    double wl, wr, sd; /* B(t) = wl B(l) + (wr B(r) + sd z) */
} mcg_bridge_node;
int mcg_sobol_table(const mcg_sobol* sobol, int n_dims, uint32_t* v_out, uint32_t* shift_out);
int mcg_sobol_bridge(int n_steps, int bridge, mcg_bridge_node* out /* [n_steps] */);
int mcg_rqmc_combine(const double* estimates, int n, double* mean, double* std_err);
int mcg_paths_gbm_sobol(mcg_ctx* ctx, const mcg_sobol* sobol, double S0, double r, double sigma, double dt, int n_steps,
                        uint64_t path_begin, int64_t n_paths, mcg_paths** out);
int mcg_paths_gbm_sobol_payoff(mcg_ctx* ctx, const mcg_sobol* sobol, double S0, double r, double sigma, double dt, int n_steps,
                               uint64_t path_begin, int64_t n_paths, double K, int is_call, mcg_paths** out);
int mcg_paths_localvol_sobol(mcg_ctx* ctx, const mcg_sobol* sobol, double S0, double r, double q, const double* times, int n_t,
                             double x_min, double x_max, int n_x, const double* sigma, double dt, int n_steps, uint64_t path_begin,
                             int64_t n_paths, mcg_paths** out);
int mcg_paths_localvol_sobol_payoff(mcg_ctx* ctx, const mcg_sobol* sobol, double S0, double r, double q, const double* times,
                                    int n_t, double x_min, double x_max, int n_x, const double* sigma, double dt, int n_steps,
                                    uint64_t path_begin, int64_t n_paths, double K, int is_call, mcg_paths** out);

/* Upload a host matrix in the reference's layout: row_major[p*n_cols + j], n_cols = n_steps+1. */
int mcg_paths_from_host(mcg_ctx* ctx, const double* row_major, int64_t n_paths, int n_cols,
                        mcg_paths** out);
/* Download into the reference's layout (path-major, what GenerateStockPricePaths returns). */
int mcg_paths_to_host(const mcg_paths* paths, double* row_major_out);
/* Download as stored: out[j*n_paths + p]. */
int mcg_paths_to_host_step_major(const mcg_paths* paths, double* step_major_out);
int mcg_paths_info(const mcg_paths* paths, int64_t* n_paths, int* n_steps, int64_t* ld,
                   void** device_ptr);
int mcg_paths_free(mcg_paths* paths);

/* ---- pricing ---------------------------------------------------------------------------- */
/* e^{-rT} * mean(PayoffFunction(S_T)) (include/core/common.h:8-14 on the last column) and its
 * Monte Carlo standard error.  sums3 (optional) receives {sum, sum^2, n} before discounting. */
int mcg_price_european(mcg_ctx* ctx, const mcg_paths* paths, double K, double r, double T,
                       int is_call, double* mean, double* std_err);

/* LSM::PredictOptionPrice (src/models/LSMPricer.cpp:19-102) on a device-resident matrix.
 * Returns mean_i V[i][0]; std_err is an addition (the reference returns a bare mean).
 * poly_order in [0, 15] (orders above 8 take one launch per exercise date whatever the path count). */
int mcg_price_lsm(mcg_ctx* ctx, const mcg_paths* paths, double r, double K, double maturity,
                  double dt, int is_call, int poly_order, double* mean, double* std_err);

/* LSM with TWO regressors: the continuation value is fitted on (S_j, F_j), F = `state`, any per-path state of the same
 * shape as the price matrix (the variance matrix of mcg_paths_heston* / mcg_paths_heston_qe*: under stochastic volatility
 * the continuation value depends on both).  The sweep, the exercise rule and its constants are mcg_price_lsm's: terminal
 * payoff at row n_steps; dates with j dt > maturity only discount; a path whose payoff exceeds 1e-14, on a date with at
 * least one such path, gets V = max(payoff, fit); a path with payoff < 1e-14 gets V e^{-r dt}, any other 0; the price is
 * mean(V_0), std_err as mcg_price_lsm computes it.  Only the fit differs.  At a date with the in-the-money set I, |I| >= 1:
 *   1. standardise: for u = S_j and for u = F_j over I:  mu = mean(u), m2 = mean(u^2), var = max(m2 - mu^2, 0);
 *        the regressor is constant on this date iff !(var > 1e-12 m2): then z = 0 for every path;
 *        otherwise z = (u - mu)/sqrt(var).
 *      K does not enter; the fit is invariant under affine changes of either regressor.
 *   2. basis: the monomials zx^a zw^b, a + b <= poly_order, by total degree and within a degree by descending a:
 *        1; zx, zw; zx^2, zx zw, zw^2; zx^3, zx^2 zw, zx zw^2, zw^3      (poly_order in [0, 3]: nb = 1, 3, 6, 10)
 *   3. moments: the power sums sum zx^a zw^b, a + b <= 2 poly_order (28 at order 3), and the nb cross sums
 *        sum phi_k e^{-r dt} V, over I in a fixed order.
 *   4. solve: the Gram matrix G from the power sums; d_k = G_kk^-1/2 (0 where G_kk <= 0); LDL^T of d G d in basis order:
 *        a column whose d_k is 0, or whose pivot (in these equilibrated units) is <= 1e-8, is DROPPED: its coefficient
 *        is 0 and it takes no part in later columns.  The fit is the kept columns' combination.
 * *n_dropped (may be NULL) receives the number of dropped columns over all dates that had an in-the-money path; a date
 * with none fits nothing and drops nothing.  The one rule covers date 0 (both regressors constant: the fit is the mean),
 * a state that is constant or collinear with S, and fewer in-the-money paths than basis functions.
 * Repeated calls are bit-identical (fixed-order reductions, no floating-point atomics).  One launch sequence queued by the
 * host, four launches per exercise date, no read-back before the final sums; booked under MCG_K_LSM_SWEEP.
 * MCG_ERR_INVALID with a message: a NULL ctx, paths, state or mean; a state whose n_paths or n_steps differ from the
 * paths'; either matrix of another ctx; poly_order outside [0, 3]; a non-finite r, K, maturity or dt; K <= 0; dt <= 0;
 * a ctx that holds a collective.  An empty matrix is MCG_ERR_EMPTY_PATHS.
 * Out of scope: collectives (sharded matrices); the one-launch sweeps; Greeks; the batch rows, the coalescing layer and
 * the drop-in classes; more than one extra state; orders above 3. */
int mcg_price_lsm2(mcg_ctx* ctx, const mcg_paths* paths, const mcg_paths* state, double r, double K, double maturity,
                   double dt, int is_call, int poly_order, double* mean, double* std_err, int64_t* n_dropped);

/* ---- LSM exercise policies: fit on one path set, apply out of sample ------------------------ */
/* mcg_price_lsm's number is mean(V_0) of a sweep that sets V = max(payoff, FITTED continuation) on the paths it was fitted
 * on: neither a lower nor an upper bound on the American value.  A POLICY is the fitted exercise rule as plain host data;
 * applied to independent paths (stop at the first date the rule says exercise, take the discounted payoff there) it prices
 * a stopping time, and the value of any stopping time is a lower bound.
 *
 * A policy is a header and (n_steps + 1) rows of MCG_LSM_POLICY_STRIDE = 20 doubles, owned by the caller (no handle, no
 * lifetime).  Row j:
 *   [0..15]  c_t, the coefficients of y^t, y = (S/K - 1) - centre; entries above poly_order are 0
 *   [16]     the number of regression rows (in-the-money paths) at the fit
 *   [17]     the centre: 0 unless the date was re-fitted about the mean of its regressor
 *   [18]     the kind (enum mcg_lsm_policy_kind, as a double)          [19]  0
 * The continuation value of an EXERCISE_RULE row at price S is Horner in y with fused multiply-adds, x = fma(S, 1/K, -1),
 * y = x - centre, cont = c_p; cont = fma(cont, y, c_t) for t = p-1 .. 0: the arithmetic the sweep itself evaluates a fit with.
 *
 * mcg_lsm_fit: mcg_price_lsm's estimator (mean, std_err) on the per-date route whatever the path count (as mcg_greeks_lsm:
 * equal to mcg_price_lsm up to the summation order of the regression moments), and for every date the coefficient block
 * that date's update actually used -- after the re-fit where there was one.  Kinds: row n_steps is TERMINAL; a date with
 * j dt > maturity (the sweep only discounts there) is CONTINUE; a date with no in-the-money path at the fit is CONTINUE; every
 * other date is EXERCISE_RULE.  hdr_out receives the arguments, coef_out (n_steps + 1) * 20 doubles.  poly_order in [0, 15].
 *
 * mcg_lsm_apply: for each path of `paths`, tau = the first j < n_steps whose row is EXERCISE_RULE with payoff(S_j) > 1e-14
 * and !(continuation_j(S_j) > payoff(S_j)), else n_steps; v = payoff(S_tau) exp(-r dt tau) (the table exp(-r dt j) is formed
 * on the host in binary64); mean = sum v / n, std_err from {sum v, sum v^2, n} as mcg_price_lsm forms it.  sums3 (may be NULL)
 * receives {sum v, sum v^2, n}, tau_hist (may be NULL; n_steps + 1 counts) the number of paths with tau = j.  is_call, r, K
 * and dt are the header's; its maturity is not read (the kinds carry it).  One forward pass over the matrix, booked under
 * MCG_K_LSM_APPLY: 8 B per path and date at most -- a wavefront whose paths have all exercised stops reading.  Repeated calls
 * are bit-identical (fixed-order sums, integer counts).  Sharded matrices are combined by hand: add the shards' sums3 and
 * tau_hist.
 *
 * mcg_lsm_policy_continuation: host only, no ctx.  cont_out[i] = the continuation value of row `date` at S[i] for an
 * EXERCISE_RULE row, +infinity for a CONTINUE row (the rule never exercises there), 0 for the TERMINAL row.  It checks the
 * whole policy first, so it also serves as a policy's validator.
 *
 * MCG_ERR_INVALID with a message: a NULL ctx, paths, hdr, coef or mean (fit: hdr_out, coef_out); paths of another ctx;
 * hdr.n_steps different from the matrix's; poly_order outside [0, 15]; a non-finite r, K, maturity or dt; K <= 0; dt <= 0;
 * a kind outside {0, 1, 2}; row n_steps not TERMINAL, or another row TERMINAL; a non-finite coefficient or centre in an
 * EXERCISE_RULE row; (continuation) a date outside [0, n_steps], n < 0, a NULL S or cont_out with n > 0; a ctx that holds a
 * collective, for fit and apply alike.  An empty matrix is MCG_ERR_EMPTY_PATHS.
 * Out of scope: two-regressor policies (mcg_price_lsm2); upper bounds other than mcg_lsm_dual_upper's (below: the one-regressor
 * policy under a GBM inner model); collectives; the one-launch sweeps; the batch rows, the coalescing layer and the drop-in
 * classes; Greeks under a fixed policy. */
#define MCG_LSM_POLICY_STRIDE 20
enum mcg_lsm_policy_kind { MCG_POL_CONTINUE = 0, MCG_POL_EXERCISE_RULE = 1, MCG_POL_TERMINAL = 2 };
typedef struct mcg_lsm_policy_hdr {
    int n_steps, poly_order, is_call, reserved;
    double r, K, maturity, dt;
} mcg_lsm_policy_hdr;

int mcg_lsm_fit(mcg_ctx* ctx, const mcg_paths* paths, double r, double K, double maturity, double dt, int is_call,
                int poly_order, double* mean, double* std_err, mcg_lsm_policy_hdr* hdr_out, double* coef_out);
int mcg_lsm_apply(mcg_ctx* ctx, const mcg_lsm_policy_hdr* hdr, const double* coef, const mcg_paths* paths, double* mean,
                  double* std_err, double* sums3, int64_t* tau_hist);
int mcg_lsm_policy_continuation(const mcg_lsm_policy_hdr* hdr, const double* coef, int date, const double* S, int64_t n,
                                double* cont_out);

/* ---- Dual upper bounds for LSM exercise policies by nested simulation ------------------------- */
/* mcg_lsm_apply prices a stopping time: a lower bound.  mcg_lsm_dual_upper is the other side, the Andersen-Broadie (2004)
 * dual: along each outer path it builds the martingale part of the policy's own value process, with every conditional
 * expectation estimated by n_inner inner paths started from the outer path's price, and takes the pathwise maximum of the
 * discounted payoff less that martingale.
 *
 * Inputs: a checked policy (hdr, coef), n = hdr.n_steps; the outer matrix `paths` of n + 1 rows; the inner model: GBM with
 * model.sigma >= 0, dividend yield model.q and the header's r and dt; model.n_inner in [1, 65536]; the inner seed and
 * path_begin.  Per outer path i, global id g = path_begin + i, prices S_0 .. S_n:
 *   h_j = payoff(S_j) disc_j, disc_j = exp(-r dt j) formed on the host in binary64 (mcg_lsm_apply's table).
 *   e_j = mcg_lsm_apply's stop decision at (j, S_j), bit for the same rule: row j is EXERCISE_RULE, payoff(S_j) > 1e-14 and
 *         !(continuation_j(S_j) > payoff(S_j)), Horner fused in y = fma(S, 1/K, -1) - centre; e_n is true.
 *   C_j (j < n) = (sum over k < n_inner of v_{j,k}) / n_inner, the sum in ascending k within a slice of consecutive k and
 *         the slices in ascending order (the slices depend on n_inner and n only).  v_{j,k} is what mcg_lsm_apply returns for
 *         inner path k: it starts at S_j on date j, visits the dates j+1 .. n and stops at the first date l >= j+1 at which
 *         the rule stops (row n always), with v = payoff(S_l) disc_l.  An inner step is the in-register twin's
 *         (mcg_gbm_twin_stats): X = 0 at date j, X += fma(a, z, m), a = sigma sqrt(dt), m = (r - q - sigma^2/2) dt,
 *         S_l = S_j exp(X).
 *   L_j = e_j ? h_j : C_j (j < n), L_n = h_n;  Mt_0 = 0, Mt_{j+1} = Mt_j + L_{j+1} - C_j.
 *   D_i = max over the exercisable dates of (h_j - Mt_j): every j < n with !((double)j * dt > hdr.maturity), the expression
 *         the fit uses, and j = n.
 * upper = mean(D); std_err from {sum D, sum D^2, n} as mcg_lsm_apply forms its own.
 * Inner draws (the RNG contract of csrc/philox.hpp, extended): key = model.seed; counter = (g_lo, g_hi, (j << 12) | b,
 * 0x10000 + k); the step from date l - 1 to l, relative step s = l - j - 1, uses block b = s >> 2, element s & 3.  Hence
 * n_steps <= 16384.  Stream numbers >= 0x10000 are no generator's, so the inner seed may equal the outer one.
 *
 * For ANY policy E[D] is an upper bound on the value of the option exercisable on those dates, and the noise of the inner means
 * biases it upwards, never downwards (D is a maximum of terms linear in them: Jensen).  It is the caller's bound only if
 * the outer paths follow the same GBM (r, q, sigma, dt) as the inner ones: the library cannot check that.
 *
 * Outputs: sums3 (may be NULL) = {sum D, sum D^2, n}; cont_out (may be NULL; host, [n_steps][n_paths]) = C_j of every outer
 * path; d_out (may be NULL; host, n_paths) = D_i; inner_steps (may be NULL) = the sum over every inner path of the steps it
 * took, an integer count.  No floating-point atomics: repeated calls are bit-identical, and D_i and the C_j of outer path i
 * depend on that path alone, so any split of the outer paths into shards gives the same d_out and cont_out, bit for bit.
 * Sharded sets are combined by hand: give each shard its path_begin and add the shards' sums3 and inner_steps.  inner_steps
 * then equals the whole set's exactly; the added sums3 equal the whole set's to the rounding of the partial sums (floating-point
 * sums of other groupings), not bit for bit.  Booked under MCG_K_LSM_DUAL.
 * MCG_ERR_INVALID with a message: a NULL hdr, coef, model, ctx, paths or upper; n_inner outside [1, 65536]; a negative or
 * non-finite sigma; a non-finite q; hdr.n_steps above 16384; anything mcg_lsm_policy_continuation's validator rejects (these
 * are answered before the ctx is looked at); paths of another ctx; hdr.n_steps different from the matrix's; a ctx that holds a
 * collective.  An empty matrix is MCG_ERR_EMPTY_PATHS.
 * Out of scope: two-regressor policies; inner models other than GBM; collectives; compaction of stopped lanes and variance
 * reduction of the inner means; the drop-in classes. */
#define MCG_LSM_DUAL_MAX_INNER 65536
#define MCG_LSM_DUAL_MAX_STEPS 16384
typedef struct mcg_lsm_dual_model {
    uint64_t seed;
    double sigma, q;
    uint64_t path_begin;
    int n_inner;
    int reserved;
} mcg_lsm_dual_model;
int mcg_lsm_dual_upper(mcg_ctx* ctx, const mcg_lsm_policy_hdr* hdr, const double* coef, const mcg_paths* paths,
                       const mcg_lsm_dual_model* model, double* upper, double* std_err,
                       double* sums3 /* may be NULL: {sum D, sum D^2, n} */,
                       double* cont_out /* may be NULL: host, [n_steps][n_paths], C_j of every outer path */,
                       double* d_out /* may be NULL: host, n_paths, D_i */,
                       int64_t* inner_steps /* may be NULL: sum over every inner path of the steps it took */);

/* ---- Greeks ----------------------------------------------------------------------------- */
/* Price sensitivities with Monte Carlo standard errors.  Every field an entry point does not fill is NaN, and so is its
 * std error.  dual_delta = dP/dK.  Repeated calls on the same matrix are bit-identical (fixed-order reductions).
 * Neither call changes mcg_lsm_one_launch_enabled or anything mcg_price_* reads.
 * Errors: a ctx with a collective (mcg_set_allreduce, RCCL, shm) -> MCG_ERR_INVALID (sharded Greeks are not supported
 * yet); an empty matrix -> MCG_ERR_EMPTY_PATHS.
 * Out of scope: sharded Greeks; Greeks through the one-launch LSM sweeps or the batch rows; LSM gamma, vega and rho;
 * rBergomi vega (in xi or eta); Greeks of MartingaleOptimization, BranchingProcesses and AsymptoticAnalysis; anything in
 * the drop-in classes. */
typedef struct mcg_greeks {
    double price, delta, gamma, vega, rho, dual_delta;                    /* dual_delta = dP/dK */
    double price_se, delta_se, gamma_se, vega_se, rho_se, dual_delta_se;  /* MC std errors      */
} mcg_greeks;

/* European Greeks from row 0 (S0) and row n_steps (S_T) only, in one pass.  f' = 1{S_T > K} (call), -1{S_T < K} (put),
 * D = e^{-rT}, W_T = (ln(S_T/S0) - (r - sigma^2/2) T) / sigma.
 *   price      D mean(payoff)                                  always (== mcg_price_european up to summation order)
 *   dual_delta -D mean(f')                                     always
 *   delta      D mean(f' S_T / S0)                             when row 0 is one positive constant
 *   rho        -T price + D mean(f' T S_T)                     when the matrix came from a generator (mcg_paths_gbm* / _rbergomi* / _heston*)
 *                                                              (S_T proportional to e^{rT}); NaN for mcg_paths_from_host
 *   vega       D mean(f' S_T (W_T - sigma T))                  when sigma > 0: the caller asserts GBM with that sigma,
 *   gamma      D K / (S0^2 sigma T) mean(1{S_T > K} W_T)       generated over horizon T at rate r (gamma: mixed pathwise /
 *                                                              likelihood ratio, the same estimator for puts by parity)
 * sigma <= 0 (e.g. rBergomi paths): gamma and vega are NaN. */
int mcg_greeks_european(mcg_ctx* ctx, const mcg_paths* paths, double K, double r, double T, int is_call, double sigma,
                        mcg_greeks* out);

/* LSM (mcg_price_lsm's estimator) with its K-tangent carried through the sweep on the per-date route (one launch per
 * exercise date whatever the path count; exercise decisions held fixed):
 *   price      the LSM price (equal to mcg_price_lsm up to the summation order of the regression moments)
 *   dual_delta mean(dV_0/dK)                                   always
 *   delta      (price - K dual_delta) / S0                     when row 0 is one positive constant (the estimator is
 *                                                              homogeneous of degree 1 in (S0, K): both generators scale
 *                                                              with S0 and the regression is in S/K - 1)
 * Std errors from the per-path V_0, dV_0 and (V_0 - K dV_0) / S0.  gamma, vega and rho are NaN: for fixed decisions the
 * estimator is piecewise linear in K (a pathwise gamma is zero almost everywhere), and rho / vega need terms of the
 * regression matrix's derivative that are not moments of the sweep -- out of scope.  poly_order in [0, 8] (else
 * MCG_ERR_INVALID). */
int mcg_greeks_lsm(mcg_ctx* ctx, const mcg_paths* paths, double r, double K, double maturity, double dt, int is_call,
                   int poly_order, mcg_greeks* out);

/* ---- path-dependent European payoffs: Asian, lookback, barrier -------------------------------- */
/* One pass over the matrix reduces every path to five statistics over the monitoring dates, rows first_row .. n_steps
 * inclusive (0 <= first_row <= n_steps; first_row = 1 leaves S0 out):
 *   S_T = row n_steps,  A = arithmetic mean,  G = exp(mean of ln S),  m = min,  M = max.
 * A book of contracts is then priced on those statistics.  Undiscounted payoff per path (X is A or G):
 *   Asian, fixed strike       call max(X - K, 0)           put max(K - X, 0)
 *   Asian, floating strike    call max(S_T - X, 0)         put max(X - S_T, 0)          (K ignored)
 *   lookback, fixed strike    call max(M - K, 0)           put max(K - m, 0)
 *   lookback, floating strike call S_T - m                 put M - S_T                  (K ignored)
 *   barrier                   an up barrier is hit when M >= barrier, a down barrier when m <= barrier (discrete
 *                             monitoring on the dates above, plain comparisons of the stored doubles); an "out" contract
 *                             pays the vanilla payoff of S_T (max(S_T - K, 0) / max(K - S_T, 0)) when the barrier is
 *                             not hit, else `rebate`; an "in" contract pays it when the barrier is hit, else `rebate`.
 *                             The rebate is paid at T.
 * price[c] = e^{-rT} mean(payoff of contract c), std_err[c] its Monte Carlo standard error.
 * Rules: 1 <= n_contracts <= 1024; kind in range; K, barrier and rebate finite where the kind reads them (K: fixed
 * strikes and barriers; barrier, rebate: barriers); the paths belong to the ctx -- anything else is MCG_ERR_INVALID with a
 * message.  An empty matrix on a ctx without a collective is MCG_ERR_EMPTY_PATHS.  Repeated calls are bit-identical
 * (fixed-order reductions, no floating-point atomics), and a contract's result does not depend on what else is in the
 * book or where in the book it stands.  Matrices holding non-finite values are outside the contract.
 * Collectives: on a ctx with a collective (mcg_set_allreduce, RCCL, shm) the 2 n_contracts + 1 sums are all-reduced in one
 * call (the node-local shm collective carries 62 doubles a call: there in pieces of 62) and every rank returns the GLOBAL
 * prices, like mcg_price_european; `sums` lets a caller combine shards by hand.
 * Greeks of these payoffs: mcg_greeks_exotics, below.
 * Out of scope: early exercise; fusing the statistics into the generators; the batched driver rows; the drop-in classes.
 * Barriers here are monitored on the stored dates only; continuously monitored barriers are priced by
 * mcg_price_barriers_bridge, below. */
enum mcg_exotic_kind {
    MCG_X_ASIAN_ARITH_FIXED = 0, MCG_X_ASIAN_ARITH_FLOAT = 1,
    MCG_X_ASIAN_GEO_FIXED   = 2, MCG_X_ASIAN_GEO_FLOAT   = 3,
    MCG_X_LOOKBACK_FIXED    = 4, MCG_X_LOOKBACK_FLOAT    = 5,
    MCG_X_BARRIER_UP_OUT = 6, MCG_X_BARRIER_UP_IN = 7, MCG_X_BARRIER_DOWN_OUT = 8, MCG_X_BARRIER_DOWN_IN = 9
};
typedef struct mcg_exotic { int kind; int is_call; double K, barrier, rebate; } mcg_exotic;

/* per-path statistics over the monitoring rows first_row .. n_steps: out5[q*n_paths + p], q = 0 S_T, 1 A, 2 G, 3 min, 4 max */
int mcg_path_stats(mcg_ctx* ctx, const mcg_paths* paths, int first_row, double* host_out5);
int mcg_price_exotics(mcg_ctx* ctx, const mcg_paths* paths, double r, double T, int first_row,
                      const mcg_exotic* book, int n_contracts,
                      double* price, double* std_err /* may be NULL */, double* sums /* may be NULL: {sum, sum^2} per contract, then n */);

/* ---- Greeks of the exotics book ----------------------------------------------------------------- */
/* mcg_greeks_exotics returns one mcg_greeks per contract of a book of mcg_price_exotics.  One streaming pass over the matrix
 * reduces every path to ten statistics (mcg_path_tangent_stats), the book is then evaluated on those and on rows 0 and 1
 * (row 1 for the first step's normal Z_1).  Fields that are undefined are NaN, under the rules of mcg_greeks_european.
 *
 * Statistics, out10[q*n_paths + p]; j is the absolute row index, the monitoring rows are first_row .. n_steps, N of them:
 *   q = 0-4  S_T, A, G, min, max: bit for bit what mcg_path_stats returns
 *   q = 5    L = mean over the monitoring rows of S_j ln S_j
 *   q = 6    J = mean over the monitoring rows of j S_j
 *   q = 7, 8 row index (as a double) of the first minimum and of the first maximum on the monitoring rows (ties resolve to
 *            the lowest row index)
 *   q = 9    Q = sum_{i=1..n_steps} (ln S_i - ln S_{i-1})^2, over ALL steps, including rows before first_row
 * with_logs = 0 (what mcg_greeks_exotics takes when sigma <= 0) skips the one logarithm per element that L and Q need and
 * writes NaN there; the pass then costs what mcg_path_stats costs.  A path that holds a value below the smallest normal
 * double keeps mcg_path_stats' rescan rule for G; L, Q and every Greek that reads them are then unspecified: matrices holding
 * non-positive values are outside the contract for vega.
 *
 * Notation: D = e^{-rT}; dt = T / n_steps, t_j = j dt; s0 the path's own row-0 value; c = r - q + sigma^2/2;
 * mu = (r - q - sigma^2/2) dt; jbar = (first_row + n_steps) / 2; Z_1 = (ln(S_1/s0) - mu) / (sigma sqrt(dt));
 * W_T = (ln(S_T/s0) - (r - q - sigma^2/2) T) / sigma; f the undiscounted payoff above.  df/dX uses the strict comparisons of
 * mcg_greeks_european: call 1{X > K}, put -1{X < K}.  For floating strikes the call has df/dS_T = 1{S_T > X} and
 * df/dX = -1{S_T > X}.
 * Tangents of the statistics under GBM:
 *   statistic X   tau_sigma(X) = dX/dsigma                        tau_r(X) = dX/dr
 *   S_T           S_T (ln(S_T/s0) - c T) / sigma                  T S_T
 *   A             (L - A ln s0 - c dt J) / sigma                  dt J
 *   G             G (ln(G/s0) - c dt jbar) / sigma                G dt jbar
 *   m             m (ln(m/s0) - c dt j_m) / sigma                 dt j_m m
 *   M             M (ln(M/s0) - c dt j_M) / sigma                 dt j_M M
 * Kinds 0-5 (Asian, lookback; Lipschitz payoffs): pathwise estimators.
 *   price       D mean f, always.
 *   dual_delta  D mean(df/dK), always.  It is exactly 0 with standard error 0 for the floating kinds.
 *   delta       mean of D (f - K df/dK) / s0.  This uses homogeneity of degree 1 in (S0, K), as mcg_greeks_lsm does.  It is
 *               filled when row 0 is one positive constant, for every generator.
 *   rho         mean of D (-T f + sum_X df/dX tau_r(X)).  It is filled when the matrix carries the `generated` mark.
 *   vega        mean of D sum_X df/dX tau_sigma(X).  It is filled when sigma > 0; the caller asserts GBM with that sigma, r, q
 *               and T, as for mcg_greeks_european.
 *   gamma       floating kinds: exactly 0 with standard error 0 whenever delta is defined.
 *               fixed-strike kinds: D K / (s0^2 sigma sqrt(dt)) mean(1{X > K} Z_1).  X is the statistic the contract reads: A,
 *               G, M for the lookback call, m for the lookback put.  Calls and puts use the same estimator, by parity.  It is
 *               filled when sigma > 0, delta is defined and first_row >= 1.  At n_steps = 1 it is mcg_greeks_european's
 *               gamma.  Its variance grows as 1/dt.
 * Kinds 6-9 (barriers; discontinuous payoffs): likelihood-ratio estimators.
 *   price and dual_delta as above.  df/dK acts on the vanilla leg only; the indicator does not depend on K.
 *   The remaining four are filled when sigma > 0, row 0 is one positive constant and first_row >= 1:
 *   delta       D f Z_1 / (s0 sigma sqrt(dt))
 *   gamma       D f [(Z_1^2 - 1) / (s0^2 sigma^2 dt) - Z_1 / (s0^2 sigma sqrt(dt))]
 *   vega        D f [(sum Z_i^2 - n_steps) / sigma - sqrt(dt) sum Z_i], with
 *               sum Z_i = (ln(S_T/s0) - n_steps mu) / (sigma sqrt(dt)),
 *               sum Z_i^2 = (Q - 2 mu ln(S_T/s0) + n_steps mu^2) / (sigma^2 dt)
 *   rho         D f (W_T/sigma - T)
 *   The rebate is part of f.  The variance of the vega estimator grows with n_steps.
 * Every standard error is that of the per-path samples above.  Rules (MCG_ERR_INVALID with a message): everything
 * mcg_price_exotics rejects; non-finite r, q, sigma or T; T <= 0; a matrix without a step (n_steps < 1); a ctx with a
 * collective (mcg_set_allreduce, RCCL, shm), like the other Greeks calls.  An empty matrix is MCG_ERR_EMPTY_PATHS.  Repeated
 * calls are bit-identical (fixed-order reductions, no floating-point atomics), and a contract's result does not depend on
 * what else is in the book or where in the book it stands.  The launches are booked under MCG_K_EXOTIC.
 * Out of scope: sharded Greeks; Greeks with control variates; vega or likelihood-ratio Greeks under models other than GBM;
 * first_row = 0 for the likelihood-ratio fields; Greeks of continuously monitored barriers (mcg_price_barriers_bridge, below,
 * returns prices only). */
int mcg_path_tangent_stats(mcg_ctx* ctx, const mcg_paths* paths, int first_row, int with_logs, double* host_out10);
int mcg_greeks_exotics(mcg_ctx* ctx, const mcg_paths* paths, double r, double q, double sigma, double T, int first_row,
                       const mcg_exotic* book, int n_contracts, mcg_greeks* out /* [n_contracts] */);

/* ---- continuously monitored barriers: Brownian-bridge survival probabilities -------------------- */
/* mcg_price_barriers_bridge prices the barrier contracts of an mcg_price_exotics book under CONTINUOUS monitoring: between two
 * stored dates a path that is on the safe side of the barrier at both still crosses it with the probability of a Brownian bridge
 * in ln S, and the indicator "not hit" of mcg_price_exotics becomes the path's survival probability P.  Under GBM the estimator
 * is exact in law at any step count; under Heston, Bates and local volatility it is the first-order correction with the step's
 * variance frozen.  One streaming pass over the matrix (and the variance matrix, if given) computes P.
 *
 * Definitions.  A level is a pair (B, up) with B > 0 finite.  l_j = ln S_j: the device logarithm of the stored double;
 * h = ln B: computed on the host in binary64 and handed to the kernel; d_j = l_j - h.  Row j is SAFE when S_j > B (down level)
 * or S_j < B (up level): plain comparisons of the stored doubles, the complement of mcg_price_exotics' hit rule.
 * Monitoring window: rows first_row .. n_steps and every interval [j, j+1] with first_row <= j < n_steps
 * (0 <= first_row <= n_steps; continuous monitoring from t = 0 is first_row = 0).
 * Step variance w_j of the interval [j, j+1]: the scalar route, var == NULL, w = (sigma sigma) dt with sigma >= 0 finite; or the
 * matrix route, w_j = max(v_j, 0) dt, with `var` a matrix of this ctx and of the paths' shape whose row j holds v_j -- what
 * mcg_paths_heston* / mcg_paths_bates* return in var_out, or anything passed through mcg_paths_from_host (sigma is then not read).
 * Survival of a path for a level:
 *   P = 0 if any monitored row is not safe; otherwise
 *   P = prod_j (1 - exp(x_j)) over the intervals, x_j = -2 max(d_j d_{j+1}, 0) / w_j (evaluated as max(d_j d_{j+1}, 0) times the
 *   rounded quotient -2 / w_j, which every level shares); an interval with w_j = 0 contributes the factor 1.
 * The max keeps the factor in [0, 1) when a logarithm rounds d to 0 or to the wrong sign.  The product runs over the intervals
 * in ascending order.  A path's P for a level depends on that path's column and that level only (not on the other levels, the
 * other paths, the shard or the route: the scalar route equals the matrix route on a constant matrix of sigma sigma bit for bit).
 * With first_row = n_steps there is no interval and P is the safe indicator of the last row.  The kernel leaves an exponential
 * out where x_j <= -38 on every lane of a wave: there 1 - exp(x_j) rounds to 1, so this changes no bit.
 * Sample per contract: only kinds MCG_X_BARRIER_UP_OUT .. MCG_X_BARRIER_DOWN_IN are accepted (anything else: MCG_ERR_INVALID).
 * With f the vanilla payoff on S_T = row n_steps (max(S_T - K, 0) / max(K - S_T, 0)):
 *   out: Y = f P + rebate (1 - P);      in: Y = f (1 - P) + rebate P.
 * The rebate is paid at T, as in mcg_price_exotics.  price[c] = e^{-rT} mean Y, std_err[c] from {sum Y, sum Y^2}; dt = T / n_steps.
 * sums = {sum Y, sum Y^2} per contract in book order, then n.
 * The book's levels: duplicates (B and the direction compared bitwise) are computed once and their contracts share P; the
 * distinct levels are walked in groups of MCG_BRIDGE_L_MAX, the matrix is read once per group, and the workspace stays at
 * MCG_BRIDGE_L_MAX n_paths doubles whatever the book holds.
 * mcg_barrier_survival returns P itself, host_out[l*n_paths + p] for the levels (barriers[l], is_up[l]), 1 <= n_levels <= 1024
 * (no duplicates are removed); it takes dt itself.
 * Rules (MCG_ERR_INVALID with a message): everything mcg_price_exotics rejects for these kinds; a barrier that is not positive;
 * sigma negative or not finite (scalar route); r or T not finite, T <= 0; dt <= 0 or not finite; a matrix without a step
 * (n_steps < 1); var of another ctx or another shape; first_row outside [0, n_steps].  An empty matrix on a ctx without a
 * collective is MCG_ERR_EMPTY_PATHS.  Repeated calls are bit-identical (fixed-order reductions, no floating-point atomics), and a
 * contract's result does not depend on what else is in the book or where in the book it stands.  Matrices holding non-positive
 * or non-finite values are outside the contract.  The launches are booked under MCG_K_EXOTIC.
 * Collectives: as mcg_price_exotics -- the 2 n_contracts + 1 sums are all-reduced (the node-local shm collective: in pieces of
 * 62), every rank returns the global prices, an empty shard still takes part.
 * Out of scope: Greeks of the bridge estimator; control variates on it; double barriers; a local-volatility sigma(t, S)
 * evaluated in the kernel (hand a variance matrix instead); jump crossings under Bates (the bridge sees the diffusion only);
 * the batched driver rows, the coalescing layer and the drop-in classes. */
#define MCG_BRIDGE_L_MAX 8   /* levels one pass over the matrix keeps in registers */
#define MCG_BRIDGE_ROWS  4   /* rows one lane loads ahead of their logarithms */
int mcg_barrier_survival(mcg_ctx* ctx, const mcg_paths* paths, const mcg_paths* var /* NULL: the scalar route */, double sigma,
                         double dt, int first_row, const double* barriers, const int* is_up, int n_levels,
                         double* host_out /* [n_levels * n_paths] */);
int mcg_price_barriers_bridge(mcg_ctx* ctx, const mcg_paths* paths, const mcg_paths* var /* NULL: the scalar route */, double sigma,
                              double r, double T, int first_row, const mcg_exotic* book, int n_contracts,
                              double* price, double* std_err /* may be NULL */, double* sums /* may be NULL: {sum, sum^2} per contract, then n */);

/* ---- control variates for the exotics book ---------------------------------------------------- */
/* mcg_price_exotics_cv prices the book of mcg_price_exotics with up to two control variates a contract, in the SAME one
 * pass: the statistics, then one book kernel that keeps nine sums per contract, then host arithmetic on those sums.
 * A control is a function of a path's five statistics (the paths' own, or a TWIN's: another matrix of the same shape, or a
 * GBM path computed in registers from the same (seed, path id)) whose undiscounted expectation `mean` the caller knows:
 *   MCG_CV_PAYOFF   exotic_payoff(x) as above          MCG_CV_VANILLA  max(S_T - x.K, 0) / max(x.K - S_T, 0) by x.is_call
 *   MCG_CV_ST / MCG_CV_A / MCG_CV_G                     the statistic itself
 * The estimator.  For contract c with payoff Y and its m in {0, 1, 2} controls a = controls[ctrl[2c]], b = controls[ctrl[2c+1]],
 * centred on their means (d = C - mean), the nine sums over the paths, taken in a fixed order with no floating-point atomics,
 *   sums[9c + k] = {sum Y, sum Y^2, sum d_a, sum d_a^2, sum Y d_a, sum d_b, sum d_b^2, sum Y d_b, sum d_a d_b}   (unused: 0)
 *   sums[9 n_contracts] = n
 * go through mcg_exotics_cv_from_sums (host only; this arithmetic and nothing else):
 *   Ybar = sum Y / n, dbar = sum d / n;  S_yy = sum Y^2 - n Ybar^2, S_aa = sum d_a^2 - n dbar_a^2, S_ya = sum Y d_a - n Ybar dbar_a,
 *   S_ab = sum d_a d_b - n dbar_a dbar_b (S_bb, S_yb alike).
 *   Control a is kept iff S_aa > 1e-12 sum d_a^2 (a control that is constant on the sample is dropped), b alike.  With both kept,
 *   rho = S_ab / sqrt(S_aa S_bb), and b is dropped if 1 - rho^2 <= 1e-8.  If a was dropped and b kept, b takes a's place in the
 *   formulas (its beta is still reported in b's slot).  If n - 1 - (number kept) < 1, every control is dropped.
 *   beta solves the kept normal equations in equilibrated units: u_a = S_ya / sqrt(S_aa), u_b = S_yb / sqrt(S_bb),
 *   g_b = (u_b - rho u_a) / (1 - rho^2), g_a = u_a - rho g_b, beta = g / sqrt(S); one control: beta_a = S_ya / S_aa.
 *   price = e^{-rT} (Ybar - sum beta dbar);  RSS = max(S_yy - sum g u, 0);  std_err = e^{-rT} sqrt(RSS / (n - 1 - kept) / n)
 *   (0 when n - 1 - kept < 1: one path).  beta[2c], beta[2c+1]: a dropped or absent control reports 0.
 *   plain_price, plain_se: what mcg_price_exotics computes from sum Y and sum Y^2.  n < 1 is MCG_ERR_EMPTY_PATHS.
 * beta is estimated on the sample it corrects: the usual O(1/n) bias, far below the std error at the path counts of this
 * library.  A contract's nine sums do not depend on the rest of the book, on where it stands, or on what else `controls` holds.
 * The GBM twin (mcg_gbm_twin): a = sigma sqrt(dt), m = (r - q - sigma^2/2) dt; z_n = draw n of Philox stream 0 of
 * (seed, path_begin + p) (block n >> 2, element n & 3, the usual Box-Muller pairs); X_{n+1} = X_n + fma(a, z_n, m), X_0 = 0,
 * S_n = S0 exp(X_n); over rows first_row .. n_steps: S_T = S0 exp(X_{n_steps}), A = mean S_n, G = S0 exp(mean X_n),
 * min = S0 exp(min X_n), max = S0 exp(max X_n).  No matrix is stored.  The twin is GBM in law from the generators' own price
 * stream -- every generator draws its price driver from stream 0 of (seed, global path id), so it is strongly correlated with a
 * local-volatility path of that seed -- but it is NOT mcg_paths_gbm's bits (another step formula and exponential).  A path
 * depends on (seed, global path id) only: shards and repeats are bit-identical; odd path_begin and ids >= 2^32 are valid.
 * Under Heston / Bates the price driver is rho z2 + sqrt(1 - rho^2) z1 with z1 from stream 0: a twin correlates with the path
 * at most sqrt(1 - rho^2), so the gain there is modest (variance ratio <= 1 / rho^2).
 * mcg_gbm_expectation (host only, binary64): the closed-form mean of a control under GBM on the dates t_j = j dt,
 * j = first_row .. n_steps (N of them): MCG_CV_ST S0 e^{(r-q) n_steps dt}; MCG_CV_A (S0 / N) sum e^{(r-q) t_j} (both model-free:
 * they hold for every generator here with that r and q; sigma is not read); ln G ~ N(mu_G, v_G), mu_G = ln S0 +
 * (r - q - sigma^2/2) mean(t_j), v_G = sigma^2 sum_{j,k} min(t_j, t_k) / N^2: MCG_CV_G e^{mu_G + v_G/2}; MCG_CV_PAYOFF with
 * MCG_X_ASIAN_GEO_FIXED Black's formula on (mu_G, v_G); MCG_CV_VANILLA Black-Scholes without the discount factor.  A zero
 * variance (sigma = 0) or a strike <= 0 returns the deterministic payoff.  Any other payoff is MCG_ERR_INVALID, "no closed
 * form".  It fills *mean and leaves c->mean alone.
 * Rules (MCG_ERR_INVALID with a message): everything mcg_price_exotics rejects; both twins given; a control with on_twin and
 * no twin; a twin matrix of another ctx or another shape; non-finite twin parameters or a non-finite mean; twin S0 <= 0,
 * dt <= 0 or sigma < 0; a form out of range; a control whose payoff fields fail the book's own rules (MCG_CV_PAYOFF: as a
 * contract; MCG_CV_VANILLA: K finite); n_controls outside [0, 1024]; a ctrl index outside [-1, n_controls);
 * ctrl[2c+1] >= 0 with ctrl[2c] < 0.
 * Collectives: as mcg_price_exotics -- the 9 n_contracts + 1 sums are all-reduced in one call (the node-local shm collective:
 * in pieces of 62), every rank returns the global answer, an empty shard still takes part; a sharded in-register twin takes
 * the shard's path_begin.  Timed under MCG_K_EXOTIC: 3 launches without a twin, 4 with either.
 * Out of scope: antithetic or quasi-random paths; control variates for LSM and the other American pricers; more than two
 * controls a contract; a Heston or rBergomi twin; fusing the statistics into the existing generators; the batched driver
 * rows, the coalescing layer and the drop-in classes. */
enum mcg_control_form { MCG_CV_PAYOFF = 0,   /* exotic_payoff(x) on the statistics            */
                        MCG_CV_VANILLA = 1,  /* max(S_T - x.K, 0) / max(x.K - S_T, 0) by x.is_call */
                        MCG_CV_ST = 2, MCG_CV_A = 3, MCG_CV_G = 4 };  /* the statistic itself  */
typedef struct mcg_control { int form; int on_twin; mcg_exotic x; double mean; } mcg_control;
/* mean: the control's known UNDISCOUNTED expectation.
   on_twin: evaluate on the twin's statistics instead of the paths'. */
typedef struct mcg_gbm_twin { uint64_t seed; double S0, r, q, sigma, dt; uint64_t path_begin; } mcg_gbm_twin;

int mcg_price_exotics_cv(mcg_ctx* ctx, const mcg_paths* paths,
        const mcg_paths* twin_paths /* NULL, or any matrix of this ctx and the same shape */,
        const mcg_gbm_twin* gbm_twin /* NULL, or a twin computed in registers; not both */,
        double r, double T, int first_row, const mcg_exotic* book, int n_contracts,
        const mcg_control* controls, int n_controls /* 0..1024 */,
        const int* ctrl /* [2*n_contracts]: indices into controls, -1 = none; ctrl[2c+1] >= 0 needs ctrl[2c] >= 0 */,
        double* price, double* std_err, double* beta /* [2*n_contracts], may be NULL */,
        double* plain_price, double* plain_se /* may be NULL */, double* sums /* may be NULL: 9 per contract, then n */);
/* host only: only whether a ctrl entry is >= 0 is read; std_err, beta, plain_price, plain_se may be NULL */
int mcg_exotics_cv_from_sums(const double* sums, int n_contracts, const int* ctrl, double r, double T,
        double* price, double* std_err, double* beta, double* plain_price, double* plain_se);
/* the twin's statistics alone, out5[q*n_paths + p] as mcg_path_stats; n_steps >= 1, 0 <= first_row <= n_steps, n_paths >= 1 */
int mcg_gbm_twin_stats(mcg_ctx* ctx, const mcg_gbm_twin* twin, int n_steps, int first_row, int64_t n_paths, double* host_out5);
/* host only */
int mcg_gbm_expectation(const mcg_control* c, double S0, double r, double q, double sigma, double dt,
        int n_steps, int first_row, double* mean);

/* ---- multilevel Monte Carlo for local volatility ------------------------------------------------ */
/* Multilevel Monte Carlo (Giles 2008) trades steps against paths: E P_L = E P_0 + sum_{l=1..L} E (P_l - P_{l-1}), each difference
 * taken on a fine and a coarse path built from the SAME Brownian path, so that its variance falls with the step and nearly all
 * paths run on the coarsest grids.  mcg_mlmc_localvol_level is one level in one launch: both paths in registers, reduced to
 * the five statistics of mcg_path_stats, the book of mcg_price_exotics on them.  No matrix is stored.
 *
 * The fine path is mcg_paths_localvol's at (dt_f = T / n_fine, n_fine), step for step: the table mcg_localvol_table(dt_f,
 * n_fine), the same step, z_n = draw n of Philox stream 0 of (seed, path_begin + p).
 * The coarse path (has_coarse; n_fine even): n_coarse = n_fine / 2, dt_c = 2 * dt_f, m_c = (r - q) * dt_c, X_0 = 0, S_0 = S0;
 * its table is mcg_localvol_table(dt_c, n_coarse), slice k at t = k * dt_c; its draw k is (z_{2k} + z_{2k+1}) * sqrt(0.5) -- that
 * one addition and one multiplication -- and the step is mcg_paths_localvol's.
 * Monitoring: the fine rows k * stride_fine and the coarse rows k * stride_coarse, k = first_obs (0 or 1) .. n / stride.
 * stride_fine = 2 * stride_coarse monitors the same dates on both grids; stride_fine = stride_coarse = 1 each grid's own rows
 * (the continuous limit).  Per grid, over its monitored rows, in mcg_path_stats' layout and meaning: S_T; A = mean S summed in
 * row order; G = S0 exp(mean X) as the GBM twin computes it; min and max as fmin / fmax of the S values themselves.
 *   stats10[q * n_paths + p], q = 0..4 the fine grid's, q = 5..9 the coarse one's; without a coarse path five rows.
 * The book: P_f and P_c are a contract's payoff (mcg_price_exotics) on the fine and the coarse statistics, Y = P_f - P_c;
 * without a coarse path P_c = 0 and Y = P_f.  Taken in a fixed order with no floating-point atomics:
 *   sums[6c + k] = {sum Y, sum Y^2, sum P_f, sum P_f^2, sum P_c, sum P_c^2},   sums[6 n_contracts] = n_paths
 * A contract's sums do not depend on the rest of the book or on where it stands.  A path depends on (seed, path_begin + p)
 * only: the stats10 of shards are the one-call matrix's columns bit for bit, repeated calls are bit-identical, path_begin may be
 * odd or beyond 2^32.  Sums of shards ADD UP to the one-call sums (to rounding); no all-reduce takes place inside the call, also
 * on a ctx with a collective.  Three launches: the level kernel booked under MCG_K_LOCALVOL, the book kernel and its reduction
 * under MCG_K_EXOTIC.
 * MCG_ERR_INVALID with a message and nothing left allocated: everything mcg_paths_localvol (at dt_f, n_fine) and
 * mcg_price_exotics reject; a NULL lv, book or sums; a non-finite T or T <= 0; n_fine < 1; a coarse path with an odd n_fine; a
 * stride < 1 or one that does not divide its grid (stride_coarse is not read without a coarse path); first_obs outside {0, 1}.
 * n_paths < 1 is MCG_ERR_EMPTY_PATHS.
 *
 * mcg_mlmc_combine (host only, binary64, no fused multiply-add), levels l = 0 .. n_levels - 1 in this order:
 *   m_l = sum_y[l] / n[l];   V_l = max((sum_y2[l] - n[l] * m_l * m_l) / (n[l] - 1), 0), and 0 at n[l] = 1
 *   price = e^{-rT} sum_l m_l;   std_err = e^{-rT} sqrt(sum_l V_l / n[l])
 * mcg_mlmc_plan (host only, likewise), from per-level n, mean = m_l, var = V_l, cost C_l (path-steps a path: n_fine + n_coarse)
 * and a target eps:
 *   n_opt[l] = ceil((2 / (eps * eps)) * sqrt(V_l / C_l) * sum_k sqrt(V_k * C_k))                              (Giles' rule)
 *   alpha = minus the least-squares slope of log2 |m_l| on l over the levels l >= 1 with m_l != 0, clamped to [0.5, 2];
 *           1 where fewer than two such levels exist
 *   bias = max(|m_L|, |m_{L-1}| / 2^alpha) / (2^alpha - 1), L = n_levels - 1; the second term only for L >= 2 (level 0 is no
 *          difference); infinite for n_levels = 1
 *   converged = bias < eps / sqrt(2)
 * Rules (MCG_ERR_INVALID): a NULL array; n_levels outside [1, MCG_MLMC_MAX_LEVELS]; an n[l] < 1; a non-finite r, T, mean or eps;
 * eps <= 0; a negative or non-finite var; a cost that is not positive and finite.
 * Out of scope: Heston, Bates, rBergomi and multi-asset levels; Sobol' levels; antithetic couplings (the bridge coupling for
 * barriers is mcg_mlmc_localvol_level_ex below); Greeks; an all-reduce inside the call; the batched rows, the coalescing layer
 * and the drop-in classes. */
#define MCG_MLMC_MAX_LEVELS 32
typedef struct mcg_mlmc_level { uint64_t seed; int n_fine; int has_coarse; int stride_fine, stride_coarse; int first_obs;
                                uint64_t path_begin; int64_t n_paths; } mcg_mlmc_level;

int mcg_mlmc_localvol_level(mcg_ctx* ctx, double S0, double r, double q, const double* times, int n_t, double x_min, double x_max,
                            int n_x, const double* sigma, double T, const mcg_mlmc_level* lv, const mcg_exotic* book,
                            int n_contracts /* 1..1024 */, double* sums /* 6 n_contracts + 1: then n_paths */,
                            double* host_stats10 /* NULL, or [10 or 5][n_paths] */);
/* host only; std_err may be NULL */
int mcg_mlmc_combine(const double* sum_y, const double* sum_y2, const double* n, int n_levels, double r, double T,
                     double* price, double* std_err);
/* host only; alpha, bias, converged may be NULL */
int mcg_mlmc_plan(const double* n, const double* mean, const double* var, const double* cost, int n_levels, double eps,
                  double* n_opt /* [n_levels] */, double* alpha, double* bias, int* converged);

/* ---- multilevel barriers: Milstein levels with a Brownian-bridge coupling ------------------------- */
/* mcg_mlmc_localvol_level_ex is mcg_mlmc_localvol_level with two switches.  scheme = MCG_MLMC_LOG_EULER and bridge = 0 is that
 * call: the same kernels, sums and stats10 bit for bit.  A discretely monitored barrier's level variance falls at rate 1/2
 * only, and a scheme of strong order 1/2 keeps that rate under any coupling (Giles 2008, the Milstein paper); the two switches
 * together lift it above 1, and level 0 with bridge = 1 is the plain continuously monitored barrier estimator under sigma(t, S)
 * with no price or variance matrix stored.
 *
 * scheme = MCG_MLMC_MILSTEIN.  The lookup is mcg_paths_localvol's: u, j, f, {a_j, d_j}, s = fma(f, d_j, a_j).  Then
 *   uu = fma(X, inv_dx, u0);   g = (uu > 0 && uu < n_x - 1) ? d_j * inv_dx : 0        (the surface is flat outside the grid)
 *   e  = fma(s, z, fma(-0.5 * s, s, m));   e' = fma((0.5 * s) * g, fma(z, z, -1.0), e);   X += e';   S = scaled_exp(S, e')
 * on the fine grid, and on the coarse one with its own table, drift and summed draw.  Where g = 0 (a flat surface) the path is
 * the log-Euler path bit for bit.
 *
 * bridge = 1.  A level is (B, up) of a barrier contract of the book, compared bitwise, in the order of first appearance
 * (mcg_mlmc_bridge_levels lists them); contracts with the same level share it; at most MCG_MLMC_BRIDGE_L_MAX a call.  A down
 * barrier at exactly 0 is never touched: P = 1 by rule, no level (the EURO idiom: a down-and-out contract with B = 0 is the
 * vanilla payoff).  Any other barrier <= 0 is rejected.  h = log(B / S0) is formed on the host in binary64; d = X - h.
 * Survival along a grid: monitoring is continuous over [0, T] on EVERY step of the grid, whatever the strides and first_obs
 * are (they govern the five statistics only).  A row is safe when d > 0 (down) or d < 0 (up); row 0 has X = 0.  P = 0 if a row
 * is unsafe; otherwise P is the product, in ascending order, over the sub-intervals (a, b) of
 *   1 - exp(max(d_a * d_b, 0) * (-2 / w)),            a sub-interval with w = 0 contributes 1
 * Fine step n (and every step of a level without a coarse path): one sub-interval (X_n, X_n+1), w = s_n * s_n.
 * Coarse step k, s_c its step volatility: the midpoint xm = fma(0.5 * s_c, (z_2k - z_2k+1) * sqrt(0.5), 0.5 * (X_k + X_k+1))
 * is a row of its own (on the wrong side: P = 0), and the two sub-intervals (X_k, xm) and (xm, X_k+1) have w = 0.5 * (s_c * s_c)
 * each.  z_2k - z_2k+1 is independent of the coarse increment z_2k + z_2k+1, so xm is a draw of the Brownian bridge between the
 * coarse step's ends under its frozen volatility, and the conditional expectation of the two factors given the ends is the
 * one-step factor 1 - exp(-2 d_k d_k+1 / (s_c * s_c)): E P_c(level l) = E P_f(level l - 1), the telescoping sum stays exact.
 * Samples, f the vanilla payoff on the grid's own S_T: out contracts f P + rebate (1 - P), in contracts f (1 - P) + rebate P,
 * as mcg_price_barriers_bridge forms them; a contract of another kind as mcg_mlmc_localvol_level; with bridge = 0 barrier
 * contracts too.
 *   surv[(g * n_levels + l) * n_paths + p]: P of level l on the fine grid (g = 0) and, with a coarse path, the coarse one (g = 1)
 * Kept: a path depends on (seed, path_begin + p) only -- shards, repeats, an odd path_begin or one beyond 2^32 are bit-identical;
 * a contract's sums do not depend on the rest of the book, a level's P not on the other levels.  An exponential is skipped
 * where its argument is <= -38 on every lane of a wavefront: 1 - exp(x) is 1.0 there, no bit changes.  No float atomics.
 * MCG_ERR_INVALID with a message: everything mcg_mlmc_localvol_level rejects; a scheme or a bridge flag outside {0, 1}; with
 * bridge = 1 an up barrier <= 0, a down barrier < 0, more than MCG_MLMC_BRIDGE_L_MAX distinct levels.
 * Out of scope: bridge-sampled minima and maxima for lookbacks; Asian couplings; double barriers; more levels a call. */
#define MCG_MLMC_BRIDGE_L_MAX 4
enum mcg_mlmc_scheme { MCG_MLMC_LOG_EULER = 0, MCG_MLMC_MILSTEIN = 1 };
int mcg_mlmc_localvol_level_ex(mcg_ctx* ctx, double S0, double r, double q, const double* times, int n_t, double x_min, double x_max,
                               int n_x, const double* sigma, double T, const mcg_mlmc_level* lv, int scheme, int bridge,
                               const mcg_exotic* book, int n_contracts /* 1..1024 */, double* sums /* 6 n_contracts + 1 */,
                               double* host_stats10 /* NULL, or [10 or 5][n_paths] */,
                               double* host_surv /* NULL, or [(1 or 2) * n_levels][n_paths]: fine levels, then coarse */);
/* host only: the distinct levels of a book in the order the kernel holds them; barriers and is_up hold MCG_MLMC_BRIDGE_L_MAX */
int mcg_mlmc_bridge_levels(const mcg_exotic* book, int n_contracts, double* barriers, int* is_up, int* n_levels);

/* ---- notes on an observation schedule: autocallables and cliquets ------------------------------ */
/* mcg_price_scheduled prices a book of structured notes whose payoff is a small state machine walked over a few dates of the
 * matrix ("called yet?", "coupons missed so far", "knocked in?", "last reset level"): no function of the five statistics above.
 * One kernel reads only the scheduled rows of the step-major matrix (no statistics pass, no workspace per path), and a
 * wavefront whose paths have all been called stops reading: the pass is bounded by the bytes actually needed.
 *
 * Schedule: ONE per call, shared by the book.  obs[k].row is strictly increasing in 0 .. n_steps; 1 <= n_obs <= n_steps + 1;
 * t_k = obs[k].row dt; disc_k = exp(-r (row_k dt)), formed on the host in binary64.  obs[k].flags: any of MCG_OBS_COUPON,
 * MCG_OBS_CALL, MCG_OBS_KI (autocallables read these) and MCG_OBS_RESET (cliquets read this one).
 * Per path: s0 is the path's own row-0 value, X_k = S[row_k] / s0 (one IEEE division), and every level test is a plain
 * comparison of X_k.  Y is the path's PRESENT value: price = mean Y, std_err its Monte Carlo standard error; nothing further
 * is discounted.  stop is the index of the observation at which the note ended, n_obs at maturity.
 *
 * MCG_S_AUTOCALL.  State alive = true, missed = 0, ki = false, Y = 0.  For k = 0 .. n_obs - 1, while alive, in this order:
 *   1. if flags & KI and X_k <= ki_level: ki = true;
 *   2. if flags & COUPON: if X_k >= coupon_level, Y += coupon (1 + (memory ? missed : 0)) disc_k and missed = 0;
 *      else missed += 1;
 *   3. if flags & CALL and X_k >= call_level: Y += disc_k, alive = false, stop = k.
 * A path still alive after the last observation takes the maturity leg: R = (ki && X_last < put_strike) ? X_last / put_strike
 * : 1; Y += R disc_last; stop = n_obs.  ki_level = 0 means no knock-in; call_level = +inf means never called.
 * MCG_S_CLIQUET.  The dates flagged RESET are t_0 < ... < t_m; the first only sets the reference.  r_i = S(t_i) / S(t_{i-1}) - 1,
 * c_i = fmin(local_cap, fmax(local_floor, r_i)), added in sequence from i = 1; Y = fmin(global_cap, fmax(global_floor, sum))
 * disc(t_m); stop = n_obs.  +-inf is allowed in the four bounds.  With RESET on {t_1, T}, floor 0 and no caps this is the
 * at-the-money forward-start call on the return.
 *
 * sums = {sum Y, sum Y^2} per contract in book order, then n.  stop_hist[c * (n_obs + 1) + k] counts the paths of contract c
 * with stop == k: exact, integer atomics only.  mcg_sched_path_values returns Y itself, host_values[c * n_paths + p], and
 * stop likewise: the same device function.
 * Rules (MCG_ERR_INVALID with a message): a NULL ctx, paths, obs, book or price (host_values); paths of another ctx;
 * n_contracts outside [1, 1024]; n_obs out of range; rows not strictly increasing or outside the matrix; flags outside the
 * mask; a kind out of range; a non-finite r; dt <= 0 or not finite; autocall: put_strike <= 0, a non-finite coupon,
 * coupon_level or ki_level, a NaN call_level; cliquet: fewer than two RESET dates in the schedule, a NaN bound, a floor above
 * its cap; stop_hist on a ctx with a collective (counts of shards add by hand).  An empty matrix on a ctx without a collective
 * is MCG_ERR_EMPTY_PATHS.  Matrices holding non-positive or non-finite values are outside the contract.
 * Repeated calls are bit-identical (fixed-order reductions, no floating-point atomics), and a contract's sums, values and
 * counts do not depend on what else is in the book or where in the book it stands.  The launches are booked under MCG_K_EXOTIC.
 * Collectives: as mcg_price_exotics -- the 2 n_contracts + 1 sums are all-reduced (the node-local shm collective: in pieces of
 * 62), every rank returns the global prices, an empty shard still takes part.
 * Out of scope: per-contract schedules; a knock-in between observation dates (a Brownian bridge); Greeks; control variates;
 * fusing the walk into the generators; the batched driver rows, the coalescing layer and the drop-in classes. */
enum mcg_obs_flag   { MCG_OBS_COUPON = 1, MCG_OBS_CALL = 2, MCG_OBS_KI = 4, MCG_OBS_RESET = 8 };
typedef struct mcg_obs   { int row; int flags; } mcg_obs;
enum mcg_sched_kind { MCG_S_AUTOCALL = 0, MCG_S_CLIQUET = 1 };
typedef struct mcg_sched { int kind; int memory;
                           double call_level, coupon_level, coupon, ki_level, put_strike;   /* autocall */
                           double local_floor, local_cap, global_floor, global_cap;         /* cliquet  */ } mcg_sched;

int mcg_price_scheduled(mcg_ctx* ctx, const mcg_paths* paths, double r, double dt, const mcg_obs* obs, int n_obs,
        const mcg_sched* book, int n_contracts, double* price, double* std_err /* may be NULL */,
        double* sums /* may be NULL: {sum Y, sum Y^2} per contract, then n */,
        int64_t* stop_hist /* may be NULL: [n_contracts][n_obs + 1] */);
int mcg_sched_path_values(mcg_ctx* ctx, const mcg_paths* paths, double r, double dt, const mcg_obs* obs, int n_obs,
        const mcg_sched* book, int n_contracts, double* host_values /* [c * n_paths + p] */,
        int32_t* host_stop /* may be NULL, same layout */);

/* Whether this ctx currently uses the one-launch LSM sweep (one launch per price up to 8.37M paths per GPU, order <= 4):
 * it is switched off for the next eight LSM prices when the in-kernel hand-shake between workgroups times out
 * (another process holding part of the GPU); mcg_price_lsm answers those -- and the call that timed out -- from the
 * per-date kernels (one launch per exercise date). */
int mcg_lsm_one_launch_enabled(mcg_ctx* ctx, int* enabled);
/* Allow the one-launch sweep again at once (after a time-out it comes back by itself eight LSM prices later).
 * Sharded over mcg_comm_init_shm: call it on every rank or on none. */
int mcg_lsm_one_launch_reset(mcg_ctx* ctx);

/* AsymptoticAnalysis::PredictOptionPrice (src/models/AsymptoticAnalysisPricer.cpp:38-113) on a
 * device-resident matrix: mean over paths of the best discounted payoff among the dates (t <= maturity)
 * at which S lies beyond the short-time exercise boundary.  sigma <= 0 is MCG_ERR_INVALID with the
 * reference's message "AsymptoticAnalysis: Volatility must be positive."   */
int mcg_price_asymptotic(mcg_ctx* ctx, const mcg_paths* paths, double r, double K, double maturity,
                         double dt, int is_call, double sigma, double dividend, double* price);

/* MartingaleOptimization::PredictOptionPrice (src/models/MartingaleOptimizationPricer.cpp:21-189):
 * 0.5 * (primal + dual) after max_iterations iterations; lower/upper (optional) receive the two bounds.
 * poly_order in [0, 15]; max_iterations <= 0 is MCG_ERR_INVALID with the reference's message.
 *  */
int mcg_price_martingale(mcg_ctx* ctx, const mcg_paths* paths, double r, double K, double maturity,
                         double dt, int is_call, int poly_order, int max_iterations, double* price,
                         double* lower, double* upper);

/* BranchingProcesses::PredictOptionPrice (src/models/BranchingProcessPricer.cpp:12-134): midpoint of the
 * first-positive-payoff lower bound and the resampled-branch upper bound.  exercise_times are column indices
 * (the reference's driver passes 0..steps-1, PredictionGen.cpp:780-783).  The reference resamples with an
 * unseeded mt19937; here the resampling is Philox stream 2 of `seed`, so a call is reproducible.
 * Error messages are the reference's.   */
int mcg_price_branching(mcg_ctx* ctx, const mcg_paths* paths, double r, double K, double maturity,
                        double dt, int is_call, int num_branches, const int* exercise_times,
                        int n_exercise_times, uint64_t seed, double* price, double* lower, double* upper);

/* ---- batched driver rows ------------------------------------------- */
/* One option row of the reference's production caller (src/core/PredictionGen.cpp:566-791): path-engine
 * parameters (mcg_estimate_params of the row's spot history), contract terms and AsymptoticAnalysis inputs. */
typedef struct mcg_row {
    double S0, xi, H, eta, rho;                  /* RoughVolatility.cpp:327-331                          */
    double strike, maturity, sigma, dividend;    /* PredictionGen.cpp:701-709                            */
    int n_steps;                                 /* floor(maturity*252), :718                            */
    int is_call;
} mcg_row;

/* Prices n_rows option rows in six launches per chunk of rows (one chunk unless the rows' workspace exceeds the memory
 * budget, see below): n_paths (the driver uses 250) rBergomi paths per row,
 * then AsymptoticAnalysis, BranchingProcesses(num_branches, exercise dates 0..n_steps-1), LSM(poly_order) and
 * MartingaleOptimization(poly_order, max_iterations) on them.  out[4*i + {0,1,2,3}] = the four prices of row i
 * in the driver's column order (asymPrice, branchPrice, lsmPriceVal, martinPrice, :809-814).  Rows the driver
 * would answer with zeros (no steps, degenerate estimates, sigma <= 0, strike <= 0, an inf / nan among the row's generated
 * paths: :739-777 -- the row kernels scan every row's block for it, rows priced singly are scanned by a pass of their own) get zeros; every other row gets what its pricers
 * returned, finite or not (:809-816).
 * Row i uses Philox path ids (i << 32) + p of `seed`: its prices equal the single-contract entry points
 * called with path_begin = i << 32 -- and a row of more than 1020 steps (four years of trading days) IS priced through
 * them, after the batch, one row at a time -- as is every row of a call with n_paths > 256 or poly_order > 4 (the row
 * kernels' limits).  poly_order in [0, 15]. */
int mcg_batch_price_rows(mcg_ctx* ctx, const mcg_row* rows, int64_t n_rows, int n_paths, double r, double dt,
                         int num_branches, int poly_order, int max_iterations, uint64_t seed, double* out);
/* Any number of rows: the rows are processed in chunks whose workspace (every row's own (n_steps+1) x 256 block of the
 * path matrix, its amplitudes and compensator -- nothing is padded to the longest row) stays under a quarter of the
 * device memory that is free at the call; a row's Philox ids, and therefore its prices, do not depend on the chunking. */

/* The driver's two remaining feature columns (src/core/PredictionGen.cpp:313-347, compute20DayVolAndMomentum): annualised
 * standard deviation and sum of the last 20 log returns of the spot history; {0, 0} for fewer than 21 prices.
 * twenty_day_vol is also the `sigma` the driver hands to AsymptoticAnalysis (:706). */
int mcg_row_features(const double* hist, size_t n, double* twenty_day_vol, double* twenty_day_momentum);

/* One driver row from the driver's own inputs (PredictionGen.cpp:664-719): the spot history fetched for the row (the
 * driver appends underlying_last when it holds fewer than two prices, :671-673 -- so does this), the CSV fields
 * underlying_last, dte, strike_dist_pct, option_type (1 = call), dividend.  Fills *row (path-engine parameters by
 * mcg_estimate_params, strike = underlying_last (1 - strike_dist_pct), maturity = dte / 365, sigma = twenty_day_vol,
 * n_steps = floor(maturity 252)) and features2 = {twenty_day_vol, twenty_day_momentum}.  A row the driver answers with
 * ",0,0,0,0,0,0" (empty or non-finite history, inputs it rejects at :612-620) comes back with n_steps = 0 and zero
 * features, status MCG_OK: mcg_batch_price_rows* prices it to zeros like the driver. */
int mcg_row_build(const double* hist, size_t n, double underlying_last, double dte, double strike_dist_pct,
                  int option_type, double dividend, mcg_row* row, double features2[2]);

/* mcg_batch_price_rows with the driver's SIX output columns (:471-477, :809-816): out6[6*i + {0..3}] = the four model
 * prices, out6[6*i + {4,5}] = features2 of row i (mcg_row_build; NULL: zeros) -- except that a row whose pricing the
 * driver skips (n_steps < 1) keeps all six at zero, as the driver writes it. */
int mcg_batch_price_rows6(mcg_ctx* ctx, const mcg_row* rows, const double* features2, int64_t n_rows, int n_paths,
                          double r, double dt, int num_branches, int poly_order, int max_iterations, uint64_t seed,
                          double* out6);

/* ---- host-side pieces of the class-level API (a2/a3 of SURVEY.md section 8) --------------- */
/* RoughVolatility.cpp:324-331: out5 = {xi, H, eta, rho, S0}. */
int mcg_estimate_params(const double* hist, size_t n, double out5[5]);
/* Spectral amplitudes amp[0..Mz) and compensator comp[0..n_steps) staged in LDS by the rBergomi kernels
 * (DESIGN.md); Mz = nextpow2(n_steps). */
int mcg_rbergomi_spectrum(double H, double eta, double dt, int n_steps, double* amp, double* comp,
                          int* Mz);

/* The reference's class API through the C ABI (what the C++ shims in include/models call):
 * GenerateStockPricePaths(hist, steps, paths) -> out[paths][steps+1], and
 * LSM::PredictOptionPrice(pricePaths, r, strike, maturity, dt, isCall, polyOrder).
 * Both use a lazily created per-thread ctx on device 0 (MCG_DEVICE overrides). */
int mcg_compat_set_seed(uint64_t seed, int enabled); /* default: std::random_device per call */
/* Calls of the class API that arrive from DIFFERENT host threads while a round of them is on the device are answered
 * together: one launch per kind of call over all of them (the row kernels of mcg_batch_price_rows, one workgroup per
 * matrix), the reference's driver unchanged (src/core/PredictionGen.cpp:542-570, :736-737, :788-791: one row per OpenMP
 * thread, five calls per row).  Shapes the row kernels serve -- at most 256 paths, 1 .. 1020 steps, polynomial order <= 4,
 * BranchingProcesses with the driver's exercise dates 0 .. steps - 1; anything else, or everything after
 * mcg_compat_set_coalescing(0), runs on the calling thread's own context as before.  Mode 1 (the default) also PREFETCHES: the
 * first pricer call on a matrix the library already holds on the device queues the driver's other three pricers with the driver's
 * arguments (:788-791: the same r, strike, maturity, dt, isCall; 10 branches, order 2, 5 iterations), each in the lane of its kind,
 * so that the four run side by side; a later call is answered from that only if it asks for exactly what was computed on exactly
 * that matrix.  Mode 2: coalescing without the prefetch.  A lone caller is a round of one.  mcg_stats counts rounds, calls,
 * prefetches, hits and fall-backs.
 * Resources: the first class-API call that takes this route creates five contexts on device MCG_DEVICE (default 0) and starts
 * five service threads inside the library (one per kind of call; they sleep while nothing is queued and are joined by an atexit
 * handler before the HIP runtime shuts down); every calling thread gets a 2 MB slot of device memory (allocated 32 slots at a
 * time) and a pinned host buffer of its matrix's size, both released when the thread ends.  A process that forks must do so
 * before its first call, like any user of the HIP runtime. */
int mcg_compat_set_coalescing(int mode);
int mcg_compat_generate_paths(const double* hist, size_t n, int forward_steps, int path_num,
                              double* row_major_out);
int mcg_compat_lsm_price(const double* row_major, int64_t n_paths, int n_cols, double r,
                         double strike, double maturity, double dt, int is_call, int poly_order,
                         double* price);
/* AsymptoticAnalysis::PredictOptionPrice(pricePaths, r, strike, maturity, dt, isCall, sigma, dividend);
 * like the reference, empty or ragged input prices to 0.0 (status MCG_OK). */
/* MartingaleOptimization::PredictOptionPrice(pricePaths, r, strike, maturity, dt, isCall, polyOrder, maxIterations) */
int mcg_compat_martingale_price(const double* row_major, int64_t n_paths, int n_cols, double r,
                                double strike, double maturity, double dt, int is_call, int poly_order,
                                int max_iterations, double* price);
/* BranchingProcesses::PredictOptionPrice(pricePaths, r, strike, maturity, dt, isCall, numBranches, exerciseTimes) */
int mcg_compat_branching_price(const double* row_major, int64_t n_paths, int n_cols, double r,
                               double strike, double maturity, double dt, int is_call, int num_branches,
                               const int* exercise_times, int n_exercise_times, double* price);
int mcg_compat_asymptotic_price(const double* row_major, int64_t n_paths, int n_cols, double r,
                                double strike, double maturity, double dt, int is_call, double sigma,
                                double dividend, double* price);

/* ---- measurement ------------------------------------------------------------------------ */
/* When enabled, every kernel launch is bracketed by HIP events on the ctx stream. */
int mcg_timing_enable(mcg_ctx* ctx, int on);
/* Which kernels are bracketed while timing is enabled: bit k = enum mcg_kernel k (default: all).  An event pair costs
 * several microseconds on the stream, so a measurement of one kernel's duration inside a timed loop selects that one. */
int mcg_timing_select(mcg_ctx* ctx, unsigned mask);
int mcg_timing_reset(mcg_ctx* ctx);
int mcg_timing_get(mcg_ctx* ctx, int kernel /* enum mcg_kernel */, double* total_ms,
                   int64_t* launches);

/* What this board writes right now with the path matrix's store pattern and NO arithmetic: `reps` timed launches (after
 * two untimed ones) of a kernel that stores an n_paths x (n_steps+1) fp64 matrix exactly as the GBM generator does (two
 * adjacent paths per lane, one nontemporal 16-byte store per step, rows n_paths apart).  The ceiling the generator's
 * achieved GB/s is set against, measured in the same process on the same board (boards differ by ~10 %). */
int mcg_probe_write_ceiling(mcg_ctx* ctx, int64_t n_paths, int n_steps, int reps, double* gb_per_s, double* ms_per_launch);
/* Shader clock of a GBM generator launch, stamped inside the kernel by a few workgroups spread over the grid (s_memtime /
 * s_memrealtime around each one's whole life).  A measurement aid, OFF by default: mcg_generator_clock_arm(ctx, 1) makes the
 * NEXT launches of the GBM generator on this ctx stamp (one memset of the 1 KiB stamp buffer ahead of each, a few scalar
 * reads in ~40 workgroups), ..._arm(ctx, 0) ends it; launches that are not armed pass no stamp buffer and queue nothing
 * extra.  mcg_generator_clock returns the median in GHz, the number of stamps (0: the last launch was not armed, or too
 * small to stamp) and the lowest / highest.  The generator is power-limited; its clock under load is what separates boards. */
int mcg_generator_clock_arm(mcg_ctx* ctx, int on);
int mcg_generator_clock(mcg_ctx* ctx, double* ghz_median, int* n_stamps, double* ghz_min, double* ghz_max);

/* Process-wide event counters (all contexts, all threads): what ran and what fell back. */
typedef struct mcg_stats_t {
    int64_t lsm_one_launch_sweeps;     /* LSM prices answered by ONE launch (k_lsm_coop / k_lsm_big)                      */
    int64_t lsm_one_launch_timeouts;   /* one-launch sweeps whose hand-shake gave up: discarded, re-run on the per-date route */
    int64_t lsm_per_date_sweeps;       /* LSM prices answered by the per-date route                                       */
    int64_t lsm_per_date_launches;     /* k_lsm_date launches queued for them (one per column + one per re-fitted date)   */
    int64_t lsm_per_date_refits;       /* ... of which second launches of a re-fitted date                                */
    int64_t lsm_per_date_faults;       /* per-date sweeps ended because partial moments did not arrive (MCG_ERR_HIP)      */
    int64_t shm_barrier_failures;      /* barriers of the node segment that timed out or found it poisoned                */
    int64_t peer_mailbox_enabled;      /* mcg_comm_shm_peer_mailbox calls that ended with the mailbox in peer memory      */
    int64_t peer_mailbox_refused;      /* ... that left all ranks on the host mailbox (export, open or ping failed)       */
    int64_t batch_calls, batch_chunks; /* mcg_batch_price_rows*: calls, and the chunks they were processed in             */
    int64_t batch_rows;                /* rows priced by the row kernels                                                   */
    int64_t batch_rows_singly;         /* rows priced one by one through the single-contract entry points                 */
    int64_t batch_peak_workspace_bytes;/* largest device workspace a chunk has used                                        */
    int64_t peer_mailbox_kept;         /* peer-memory mailboxes left at release to the last same-process rank thread that held them (it frees them) */
    int64_t coalesced_rounds;          /* class-API calls of several host threads answered together: rounds (one set of launches each) */
    int64_t coalesced_calls;           /* ... and the calls they answered                                                  */
    int64_t coalesced_peak_calls_per_round; /* most calls one round has answered                                           */
    int64_t coalesced_fallbacks;       /* class-API calls that took the calling thread's own context instead (shape beyond the row kernels, coalescing off) */
    int64_t coalesced_round_us;        /* wall time of the rounds, summed (packing + upload + launches + synchronisation), microseconds */
    int64_t coalesced_device_wait_us;  /* ... of which inside hipStreamSynchronize                                          */
    int64_t coalesced_wake_us;         /* time the lanes' service threads spent waking the callers they had answered         */
    int64_t coalesced_prefetched;      /* pricer calls made ahead of the caller asking (the other pricers of a row, with the driver's arguments) */
    int64_t coalesced_prefetch_hits;   /* ... whose answer the caller then took (its call matched): no device round trip of its own */
} mcg_stats_t;
int mcg_stats(mcg_stats_t* out, int reset);

/* (Test hooks -- mcg_debug_* -- are declared in mcgpu_debug.h; nothing a caller of the product needs.) */

#ifdef __cplusplus
}
#endif
#endif /* MCGPU_H */
