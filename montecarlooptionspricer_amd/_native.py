"""ctypes binding of libmcgpu.so (the C ABI declared in include/mcgpu.h)."""
from __future__ import annotations

import ctypes as C
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.environ.get("MCG_LIB") or os.path.join(_HERE, "lib", "libmcgpu.so")  # MCG_LIB: A/B experiments with another build

MCG_OK = 0
K_GBM, K_RBERGOMI, K_PAYOFF, K_LSM_SWEEP, K_LSM_SOLVE, K_TRANSPOSE, K_ASYM, K_MARTINGALE, K_BRANCHING, K_BATCH, K_EXOTIC, K_HESTON, K_MULTI, K_LOCALVOL = range(14)
KERNEL_NAMES = {K_GBM: "gbm", K_RBERGOMI: "rbergomi", K_PAYOFF: "payoff", K_LSM_SWEEP: "lsm_sweep",
                K_LSM_SOLVE: "lsm_solve", K_TRANSPOSE: "transpose", K_ASYM: "asymptotic", K_MARTINGALE: "martingale", K_BRANCHING: "branching", K_BATCH: "batch_rows",
                K_EXOTIC: "exotic", K_HESTON: "heston", K_MULTI: "multi", K_LOCALVOL: "localvol"}
K_LSM_APPLY = 14  # mcg_lsm_apply's forward pass (KERNEL_NAMES stays the table of the fourteen spans the bench tools tabulate)
K_LSM_DUAL = 15   # mcg_lsm_dual_upper's nested simulation and martingale recursion
K_SOBOL = 16      # the Sobol' generators (mcg_paths_gbm_sobol*, mcg_paths_localvol_sobol*)
LSM_DUAL_MAX_INNER, LSM_DUAL_MAX_STEPS = 65536, 16384

# Sobol' point sets (include/mcgpu.h): enum mcg_sobol_scramble and the limits
SOBOL_PLAIN, SOBOL_SHIFT, SOBOL_LMS_SHIFT = range(3)
SOBOL_SCRAMBLES = {"plain": SOBOL_PLAIN, "shift": SOBOL_SHIFT, "lms": SOBOL_LMS_SHIFT}
SOBOL_MAX_DIMS = 1024

# LSM exercise policies (include/mcgpu.h): a row is LSM_POLICY_STRIDE doubles, slot 18 its kind
LSM_POLICY_STRIDE = 20
POL_CONTINUE, POL_EXERCISE_RULE, POL_TERMINAL = range(3)

# enum mcg_exotic_kind (include/mcgpu.h)
(X_ASIAN_ARITH_FIXED, X_ASIAN_ARITH_FLOAT, X_ASIAN_GEO_FIXED, X_ASIAN_GEO_FLOAT, X_LOOKBACK_FIXED, X_LOOKBACK_FLOAT,
 X_BARRIER_UP_OUT, X_BARRIER_UP_IN, X_BARRIER_DOWN_OUT, X_BARRIER_DOWN_IN) = range(10)
EXOTIC_KINDS = {"asian_arith_fixed": X_ASIAN_ARITH_FIXED, "asian_arith_float": X_ASIAN_ARITH_FLOAT,
                "asian_geo_fixed": X_ASIAN_GEO_FIXED, "asian_geo_float": X_ASIAN_GEO_FLOAT,
                "lookback_fixed": X_LOOKBACK_FIXED, "lookback_float": X_LOOKBACK_FLOAT,
                "barrier_up_out": X_BARRIER_UP_OUT, "barrier_up_in": X_BARRIER_UP_IN,
                "barrier_down_out": X_BARRIER_DOWN_OUT, "barrier_down_in": X_BARRIER_DOWN_IN}
# MCG_BRIDGE_L_MAX, MCG_BRIDGE_ROWS (include/mcgpu.h): the levels one pass of the bridge survival kernel keeps in registers,
# and the rows of one of its load groups
BRIDGE_L_MAX, BRIDGE_ROWS = 8, 4
# the rows of mcg_path_tangent_stats' out10 (include/mcgpu.h), in order
TANGENT_STATS = ("S_T", "A", "G", "min", "max", "L", "J", "j_min", "j_max", "Q")

# enum mcg_control_form (include/mcgpu.h)
CV_PAYOFF, CV_VANILLA, CV_ST, CV_A, CV_G = range(5)
CONTROL_FORMS = {"payoff": CV_PAYOFF, "vanilla": CV_VANILLA, "st": CV_ST, "a": CV_A, "g": CV_G}

# enum mcg_obs_flag and enum mcg_sched_kind (include/mcgpu.h): the observation schedule of mcg_price_scheduled
OBS_COUPON, OBS_CALL, OBS_KI, OBS_RESET = 1, 2, 4, 8
OBS_FLAGS = {"coupon": OBS_COUPON, "call": OBS_CALL, "ki": OBS_KI, "reset": OBS_RESET}
S_AUTOCALL, S_CLIQUET = range(2)

# enum mcg_combine_kind (include/mcgpu.h)
C_NONE, C_BASKET, C_BEST_OF, C_WORST_OF = -1, 0, 1, 2
COMBINE_KINDS = {"basket": C_BASKET, "best_of": C_BEST_OF, "worst_of": C_WORST_OF}

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)


class SobolSpec(C.Structure):
    """mcg_sobol (include/mcgpu.h): which scramble of the Sobol' sequence, and whether the dimensions go through a bridge."""
    _fields_ = [("seed", C.c_uint64), ("replicate", C.c_uint32), ("scramble", C.c_int), ("bridge", C.c_int)]


class BridgeNode(C.Structure):
    """mcg_bridge_node (include/mcgpu.h): one entry of the bridge schedule."""
    _fields_ = [("t", C.c_int), ("l", C.c_int), ("r", C.c_int), ("wl", C.c_double), ("wr", C.c_double), ("sd", C.c_double)]


class Row(C.Structure):
    """mcg_row (include/mcgpu.h): one option row of the reference's driver."""
    _fields_ = [("S0", C.c_double), ("xi", C.c_double), ("H", C.c_double), ("eta", C.c_double), ("rho", C.c_double),
                ("strike", C.c_double), ("maturity", C.c_double), ("sigma", C.c_double), ("dividend", C.c_double),
                ("n_steps", C.c_int), ("is_call", C.c_int)]


class Stats(C.Structure):
    """mcg_stats_t (include/mcgpu.h): process-wide event counters."""
    _fields_ = [(k, C.c_int64) for k in (
        "lsm_one_launch_sweeps", "lsm_one_launch_timeouts", "lsm_per_date_sweeps", "lsm_per_date_launches",
        "lsm_per_date_refits", "lsm_per_date_faults", "shm_barrier_failures", "peer_mailbox_enabled", "peer_mailbox_refused",
        "batch_calls", "batch_chunks", "batch_rows", "batch_rows_singly", "batch_peak_workspace_bytes",
        "peer_mailbox_kept", "coalesced_rounds", "coalesced_calls", "coalesced_peak_calls_per_round", "coalesced_fallbacks",
        "coalesced_round_us", "coalesced_device_wait_us", "coalesced_wake_us", "coalesced_prefetched",
        "coalesced_prefetch_hits")]


class Greeks(C.Structure):
    """mcg_greeks (include/mcgpu.h): price sensitivities and their Monte Carlo std errors; NaN where not computed."""
    FIELDS = ("price", "delta", "gamma", "vega", "rho", "dual_delta")
    _fields_ = [(k, C.c_double) for k in FIELDS] + [(k + "_se", C.c_double) for k in FIELDS]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class LsmPolicyHdr(C.Structure):
    """mcg_lsm_policy_hdr (include/mcgpu.h): what an LSM exercise policy was fitted with."""
    _fields_ = [("n_steps", C.c_int), ("poly_order", C.c_int), ("is_call", C.c_int), ("reserved", C.c_int),
                ("r", C.c_double), ("K", C.c_double), ("maturity", C.c_double), ("dt", C.c_double)]


class LsmDualModel(C.Structure):
    """mcg_lsm_dual_model (include/mcgpu.h): the inner GBM of mcg_lsm_dual_upper (r and dt are the policy header's)."""
    _fields_ = [("seed", C.c_uint64), ("sigma", C.c_double), ("q", C.c_double), ("path_begin", C.c_uint64), ("n_inner", C.c_int),
                ("reserved", C.c_int)]


class Exotic(C.Structure):
    """mcg_exotic (include/mcgpu.h): one path-dependent European contract."""
    _fields_ = [("kind", C.c_int), ("is_call", C.c_int), ("K", C.c_double), ("barrier", C.c_double), ("rebate", C.c_double)]


class Control(C.Structure):
    """mcg_control (include/mcgpu.h): one control variate of mcg_price_exotics_cv."""
    _fields_ = [("form", C.c_int), ("on_twin", C.c_int), ("x", Exotic), ("mean", C.c_double)]


class GbmTwin(C.Structure):
    """mcg_gbm_twin (include/mcgpu.h): the GBM path computed in registers from the generators' own price stream."""
    _fields_ = [("seed", C.c_uint64), ("S0", C.c_double), ("r", C.c_double), ("q", C.c_double), ("sigma", C.c_double),
                ("dt", C.c_double), ("path_begin", C.c_uint64)]


MLMC_MAX_LEVELS = 32  # MCG_MLMC_MAX_LEVELS
MLMC_BRIDGE_L_MAX = 4  # MCG_MLMC_BRIDGE_L_MAX
MLMC_SCHEMES = {"euler": 0, "milstein": 1}  # mcg_mlmc_scheme


class MlmcLevel(C.Structure):
    """mcg_mlmc_level (include/mcgpu.h): the shape, the monitoring and the paths of one multilevel level."""
    _fields_ = [("seed", C.c_uint64), ("n_fine", C.c_int), ("has_coarse", C.c_int), ("stride_fine", C.c_int), ("stride_coarse", C.c_int),
                ("first_obs", C.c_int), ("path_begin", C.c_uint64), ("n_paths", C.c_int64)]


class Obs(C.Structure):
    """mcg_obs (include/mcgpu.h): one date of an observation schedule."""
    _fields_ = [("row", C.c_int), ("flags", C.c_int)]


class Sched(C.Structure):
    """mcg_sched (include/mcgpu.h): one autocallable or cliquet of a mcg_price_scheduled book."""
    _fields_ = [("kind", C.c_int), ("memory", C.c_int)] + [(k, C.c_double) for k in (
        "call_level", "coupon_level", "coupon", "ki_level", "put_strike", "local_floor", "local_cap", "global_floor", "global_cap")]


class McgError(RuntimeError):
    """A non-zero status from libmcgpu (message = mcg_last_error()) or a missing library."""

    def __init__(self, msg: str, status: int = -1):
        super().__init__(msg)
        self.status = status


_lib = None


def lib_path() -> str:
    return _LIB


def load_library():
    """Load libmcgpu.so; fail loudly if it has not been built (no fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise McgError(f"{_LIB} not found: build it with `make lib` (or __graft_entry__.build()); "
                       "this package has no CPU fallback")
    # One process can host only ONE HIP runtime.  torch wheels bundle their own libamdhip64 (same
    # SONAME as /opt/rocm's): if torch is imported first, libmcgpu binds to that copy and both
    # coexist; the other order gives torch "No HIP GPUs are available".  So when torch is
    # installed, import it before dlopen'ing libmcgpu (MCG_NO_TORCH_PRELOAD=1 skips this).
    if "torch" not in sys.modules and not os.environ.get("MCG_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(_LIB)
    dp = C.POINTER(C.c_double)
    vp = C.c_void_p
    L.mcg_last_error.restype = C.c_char_p
    L.mcg_version.restype = C.c_char_p
    L.mcg_device_count.argtypes = [C.POINTER(C.c_int)]
    L.mcg_init.argtypes = [C.POINTER(vp), C.c_int]
    L.mcg_init_on_stream.argtypes = [C.POINTER(vp), C.c_int, vp]
    L.mcg_finalize.argtypes = [vp]
    L.mcg_synchronize.argtypes = [vp]
    L.mcg_trim.argtypes = [vp]
    L.mcg_set_allreduce.argtypes = [vp, ALLREDUCE_FN, vp]
    L.mcg_comm_unique_id.argtypes = [C.c_char_p]
    L.mcg_comm_init_rank.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
    L.mcg_comm_init_shm.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]

    def newer(name, argtypes):
        """Entry points added after round 2: an older build loaded through MCG_LIB for an A/B run lacks them."""
        try:
            getattr(L, name).argtypes = argtypes
        except AttributeError:
            if not os.environ.get("MCG_LIB"):
                raise

    newer("mcg_comm_shm_peer_mailbox", [vp, C.c_int, C.POINTER(C.c_int)])
    newer("mcg_debug_shm_attach", [C.c_char_p, C.c_int, C.c_int, C.c_double, C.POINTER(vp)])
    newer("mcg_debug_shm_barrier", [vp])
    newer("mcg_debug_shm_poison", [vp])
    newer("mcg_debug_shm_detach", [vp])
    newer("mcg_lsm_one_launch_reset", [vp])
    newer("mcg_debug_lsm_hooks", [vp, C.c_longlong, C.c_int])
    newer("mcg_comm_info", [vp] + [C.POINTER(C.c_int)] * 4)
    newer("mcg_timing_select", [vp, C.c_uint])
    # round 4
    newer("mcg_stats", [C.POINTER(Stats), C.c_int])
    newer("mcg_debug_lsm_date_fault", [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong])
    newer("mcg_debug_batch_budget", [vp, C.c_size_t])
    newer("mcg_debug_peer_decision", [C.c_int] * 4)
    newer("mcg_probe_write_ceiling", [vp, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)])
    newer("mcg_generator_clock_arm", [vp, C.c_int])
    newer("mcg_generator_clock", [vp, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)])
    newer("mcg_row_features", [C.POINTER(C.c_double), C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double)])
    newer("mcg_row_build", [C.POINTER(C.c_double), C.c_size_t, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double,
                            C.POINTER(Row), C.POINTER(C.c_double)])
    newer("mcg_batch_price_rows6", [vp, C.POINTER(Row), C.POINTER(C.c_double), C.c_int64, C.c_int, C.c_double, C.c_double, C.c_int,
                                    C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_double)])
    newer("mcg_debug_sincos2_tables", [dp, dp])
    newer("mcg_debug_gbm_route", [vp, C.c_int, C.POINTER(C.c_int)])
    newer("mcg_debug_branch_route", [vp, C.c_int, C.c_int, C.POINTER(C.c_int)])
    newer("mcg_debug_eval_v", [vp, C.c_int, dp, C.c_int, dp, C.c_int, dp, C.c_int64])
    newer("mcg_debug_bates_constants", [C.c_double] * 4 + [C.POINTER(C.c_uint32), dp])
    newer("mcg_debug_lsm_solve", [vp, C.c_int, C.c_int, dp, C.c_int, dp, dp, C.c_int64])
    newer("mcg_debug_batch_row_dump", [vp, C.POINTER(Row), C.c_int64, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int,
                                       C.c_uint64, dp, C.c_int64, dp, dp, dp])
    L.mcg_paths_gbm.argtypes = [vp, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int,
                                C.c_uint64, C.c_int64, C.POINTER(vp)]
    L.mcg_paths_gbm_payoff.argtypes = [vp, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int,
                                       C.c_uint64, C.c_int64, C.c_double, C.c_int, C.POINTER(vp)]
    L.mcg_paths_rbergomi.argtypes = [vp, C.c_uint64] + [C.c_double] * 7 + [C.c_int, C.c_uint64, C.c_int64,
                                                                          C.POINTER(vp)]
    L.mcg_paths_rbergomi_payoff.argtypes = [vp, C.c_uint64] + [C.c_double] * 7 + [C.c_int, C.c_uint64, C.c_int64,
                                                                                 C.c_double, C.c_int, C.POINTER(vp)]
    L.mcg_paths_heston.argtypes = [vp, C.c_uint64] + [C.c_double] * 8 + [C.c_int, C.c_uint64, C.c_int64, C.POINTER(vp), C.POINTER(vp)]
    L.mcg_paths_heston_payoff.argtypes = [vp, C.c_uint64] + [C.c_double] * 8 + [C.c_int, C.c_uint64, C.c_int64, C.c_double, C.c_int,
                                          C.POINTER(vp), C.POINTER(vp)]
    L.mcg_paths_heston_qe.argtypes = L.mcg_paths_heston.argtypes
    L.mcg_paths_heston_qe_payoff.argtypes = L.mcg_paths_heston_payoff.argtypes
    L.mcg_paths_bates.argtypes = [vp, C.c_uint64] + [C.c_double] * 11 + [C.c_int, C.c_uint64, C.c_int64, C.c_int, C.POINTER(vp),
                                                                          C.POINTER(vp)]
    L.mcg_paths_bates_payoff.argtypes = [vp, C.c_uint64] + [C.c_double] * 11 + [C.c_int, C.c_uint64, C.c_int64, C.c_int, C.c_double,
                                                                                 C.c_int, C.POINTER(vp), C.POINTER(vp)]
    L.mcg_cholesky_corr.argtypes = [dp, C.c_int, dp]
    L.mcg_paths_gbm_multi.argtypes = [vp, C.c_uint64, C.c_int, dp, C.c_double, dp, dp, dp, C.c_double, C.c_int, C.c_uint64, C.c_int64,
                                      C.c_int, dp, C.POINTER(vp), C.POINTER(vp)]
    L.mcg_paths_combine.argtypes = [vp, C.POINTER(vp), C.c_int, C.c_int, dp, C.POINTER(vp)]
    lv = [vp, C.c_uint64, C.c_double, C.c_double, C.c_double, dp, C.c_int, C.c_double, C.c_double, C.c_int, dp, C.c_double, C.c_int,
          C.c_uint64, C.c_int64]
    L.mcg_localvol_table.argtypes = [dp, C.c_int, C.c_int, dp, C.c_double, C.c_int, dp]
    L.mcg_paths_localvol.argtypes = lv + [C.POINTER(vp)]
    L.mcg_paths_localvol_payoff.argtypes = lv + [C.c_double, C.c_int, C.POINTER(vp)]
    up = C.POINTER(C.c_uint32)
    sb = C.POINTER(SobolSpec)
    L.mcg_sobol_table.argtypes = [sb, C.c_int, up, up]
    L.mcg_sobol_bridge.argtypes = [C.c_int, C.c_int, C.POINTER(BridgeNode)]
    L.mcg_rqmc_combine.argtypes = [dp, C.c_int, dp, dp]
    L.mcg_paths_gbm_sobol.argtypes = [vp, sb, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_uint64, C.c_int64, C.POINTER(vp)]
    L.mcg_paths_gbm_sobol_payoff.argtypes = L.mcg_paths_gbm_sobol.argtypes[:-1] + [C.c_double, C.c_int, C.POINTER(vp)]
    L.mcg_paths_localvol_sobol.argtypes = [vp, sb] + lv[2:] + [C.POINTER(vp)]
    L.mcg_paths_localvol_sobol_payoff.argtypes = [vp, sb] + lv[2:] + [C.c_double, C.c_int, C.POINTER(vp)]
    L.mcg_paths_from_host.argtypes = [vp, dp, C.c_int64, C.c_int, C.POINTER(vp)]
    L.mcg_paths_to_host.argtypes = [vp, dp]
    L.mcg_paths_to_host_step_major.argtypes = [vp, dp]
    L.mcg_paths_info.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(vp)]
    L.mcg_paths_free.argtypes = [vp]
    L.mcg_price_european.argtypes = [vp, vp, C.c_double, C.c_double, C.c_double, C.c_int, dp, dp]
    L.mcg_price_lsm.argtypes = [vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, dp, dp]
    L.mcg_price_lsm2.argtypes = [vp, vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, dp, dp,
                                 C.POINTER(C.c_int64)]
    L.mcg_lsm_one_launch_enabled.argtypes = [vp, C.POINTER(C.c_int)]
    L.mcg_greeks_european.argtypes = [vp, vp, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.POINTER(Greeks)]
    L.mcg_greeks_lsm.argtypes = [vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(Greeks)]
    newer("mcg_lsm_fit", [vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, dp, dp, C.POINTER(LsmPolicyHdr), dp])
    newer("mcg_lsm_apply", [vp, C.POINTER(LsmPolicyHdr), dp, vp, dp, dp, dp, C.POINTER(C.c_int64)])
    newer("mcg_lsm_policy_continuation", [C.POINTER(LsmPolicyHdr), dp, C.c_int, dp, C.c_int64, dp])
    newer("mcg_lsm_dual_upper", [vp, C.POINTER(LsmPolicyHdr), dp, vp, C.POINTER(LsmDualModel), dp, dp, dp, dp, dp, C.POINTER(C.c_int64)])
    newer("mcg_debug_lsm_dual_executed", [vp, C.POINTER(C.c_int64)])
    newer("mcg_debug_lsm_dual_workspace", [vp, C.c_size_t])
    newer("mcg_path_stats", [vp, vp, C.c_int, dp])
    newer("mcg_price_exotics", [vp, vp, C.c_double, C.c_double, C.c_int, C.POINTER(Exotic), C.c_int, dp, dp, dp])
    newer("mcg_price_exotics_cv", [vp, vp, vp, C.POINTER(GbmTwin), C.c_double, C.c_double, C.c_int, C.POINTER(Exotic), C.c_int,
                                   C.POINTER(Control), C.c_int, C.POINTER(C.c_int), dp, dp, dp, dp, dp, dp])
    newer("mcg_exotics_cv_from_sums", [dp, C.c_int, C.POINTER(C.c_int), C.c_double, C.c_double, dp, dp, dp, dp, dp])
    newer("mcg_path_tangent_stats", [vp, vp, C.c_int, C.c_int, dp])
    newer("mcg_greeks_exotics", [vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.POINTER(Exotic), C.c_int,
                                 C.POINTER(Greeks)])
    newer("mcg_barrier_survival", [vp, vp, vp, C.c_double, C.c_double, C.c_int, dp, C.POINTER(C.c_int), C.c_int, dp])
    newer("mcg_price_barriers_bridge", [vp, vp, vp, C.c_double, C.c_double, C.c_double, C.c_int, C.POINTER(Exotic), C.c_int, dp, dp, dp])
    newer("mcg_price_scheduled", [vp, vp, C.c_double, C.c_double, C.POINTER(Obs), C.c_int, C.POINTER(Sched), C.c_int, dp, dp, dp,
                                  C.POINTER(C.c_int64)])
    newer("mcg_sched_path_values", [vp, vp, C.c_double, C.c_double, C.POINTER(Obs), C.c_int, C.POINTER(Sched), C.c_int, dp,
                                    C.POINTER(C.c_int32)])
    newer("mcg_gbm_twin_stats",[vp, C.POINTER(GbmTwin), C.c_int, C.c_int, C.c_int64, dp])
    newer("mcg_gbm_expectation", [C.POINTER(Control)] + [C.c_double] * 5 + [C.c_int, C.c_int, dp])
    newer("mcg_mlmc_localvol_level", [vp, C.c_double, C.c_double, C.c_double, dp, C.c_int, C.c_double, C.c_double, C.c_int, dp, C.c_double,
                                      C.POINTER(MlmcLevel), C.POINTER(Exotic), C.c_int, dp, dp])
    newer("mcg_mlmc_localvol_level_ex", [vp, C.c_double, C.c_double, C.c_double, dp, C.c_int, C.c_double, C.c_double, C.c_int, dp, C.c_double,
                                         C.POINTER(MlmcLevel), C.c_int, C.c_int, C.POINTER(Exotic), C.c_int, dp, dp, dp])
    newer("mcg_mlmc_bridge_levels", [C.POINTER(Exotic), C.c_int, dp, C.POINTER(C.c_int), C.POINTER(C.c_int)])
    newer("mcg_mlmc_combine", [dp, dp, dp, C.c_int, C.c_double, C.c_double, dp, dp])
    newer("mcg_mlmc_plan", [dp, dp, dp, dp, C.c_int, C.c_double, dp, dp, dp, C.POINTER(C.c_int)])
    L.mcg_price_asymptotic.argtypes = [vp, vp] + [C.c_double] * 4 + [C.c_int, C.c_double, C.c_double, dp]
    L.mcg_compat_asymptotic_price.argtypes = [dp, C.c_int64, C.c_int] + [C.c_double] * 4 + [C.c_int, C.c_double, C.c_double, dp]
    L.mcg_price_martingale.argtypes = [vp, vp] + [C.c_double] * 4 + [C.c_int, C.c_int, C.c_int, dp, dp, dp]
    L.mcg_compat_martingale_price.argtypes = [dp, C.c_int64, C.c_int] + [C.c_double] * 4 + [C.c_int, C.c_int, C.c_int, dp]
    ip = C.POINTER(C.c_int)
    L.mcg_price_branching.argtypes = [vp, vp] + [C.c_double] * 4 + [C.c_int, C.c_int, ip, C.c_int, C.c_uint64, dp, dp, dp]
    L.mcg_compat_branching_price.argtypes = [dp, C.c_int64, C.c_int] + [C.c_double] * 4 + [C.c_int, C.c_int, ip, C.c_int, dp]
    L.mcg_batch_price_rows.argtypes = [vp, C.POINTER(Row), C.c_int64, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                                       C.c_int, C.c_uint64, dp]
    L.mcg_estimate_params.argtypes = [dp, C.c_size_t, dp]
    L.mcg_rbergomi_spectrum.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, dp, dp, C.POINTER(C.c_int)]
    L.mcg_compat_set_seed.argtypes = [C.c_uint64, C.c_int]
    L.mcg_compat_set_coalescing.argtypes = [C.c_int]
    L.mcg_debug_coalesce_slots.argtypes = [C.c_int]
    L.mcg_debug_coalesce_selftest.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.mcg_compat_generate_paths.argtypes = [dp, C.c_size_t, C.c_int, C.c_int, dp]
    L.mcg_compat_lsm_price.argtypes = [dp, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                       C.c_int, C.c_int, dp]
    L.mcg_debug_eval.argtypes = [vp, C.c_int, dp, dp, C.c_int64]
    L.mcg_timing_enable.argtypes = [vp, C.c_int]
    L.mcg_timing_reset.argtypes = [vp]
    L.mcg_timing_get.argtypes = [vp, C.c_int, dp, C.POINTER(C.c_int64)]
    _lib = L
    return L


def check(status: int) -> None:
    if status != MCG_OK:
        msg = load_library().mcg_last_error()
        raise McgError(msg.decode() if msg else f"libmcgpu status {status}", status)
