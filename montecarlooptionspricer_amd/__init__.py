"""montecarlooptionspricer_amd -- MI355X-native Monte Carlo path engine.

Host-side mirror (Python) of the reference's pricing-method interface for the hot path of
bcosm/MonteCarloOptionsPricer, over the C ABI in include/mcgpu.h (libmcgpu.so: hand-written HIP for
gfx950).  There is no CPU fallback: importing works anywhere, but every compute entry point raises
McgError when the library or a GPU is missing.

    from montecarlooptionspricer_amd import PathEngine, RoughVolatility, LSM
"""
from ._native import McgError, lib_path, load_library  # noqa: F401
from ._native import (X_ASIAN_ARITH_FIXED, X_ASIAN_ARITH_FLOAT, X_ASIAN_GEO_FIXED, X_ASIAN_GEO_FLOAT, X_BARRIER_DOWN_IN,  # noqa: F401
                      X_BARRIER_DOWN_OUT, X_BARRIER_UP_IN, X_BARRIER_UP_OUT, X_LOOKBACK_FIXED, X_LOOKBACK_FLOAT)
from ._native import CV_A, CV_G, CV_PAYOFF, CV_ST, CV_VANILLA  # noqa: F401
from ._native import TANGENT_STATS  # noqa: F401
from ._native import BRIDGE_L_MAX, BRIDGE_ROWS  # noqa: F401
from .engine import CvResult, control, exotics_cv_from_sums, gbm_expectation  # noqa: F401
from ._native import POL_CONTINUE, POL_EXERCISE_RULE, POL_TERMINAL  # noqa: F401
from .engine import DualResult, LsmPolicy  # noqa: F401
from .engine import LocalVolSurface, PathEngine, PathMatrix, cholesky_corr, estimate_params, exotic, local_vol_table, make_rows, rbergomi_spectrum, row_build, row_features, stats  # noqa: F401
from .engine import MlmcResult, mlmc_bridge_levels, mlmc_combine, mlmc_plan  # noqa: F401
from .engine import Sobol, rqmc_combine, sobol_bridge, sobol_table  # noqa: F401
from ._native import OBS_CALL, OBS_COUPON, OBS_KI, OBS_RESET, S_AUTOCALL, S_CLIQUET  # noqa: F401
from .engine import autocall, cliquet, make_sched_book, schedule  # noqa: F401
from .compat import LSM, AsymptoticAnalysis, BranchingProcesses, MartingaleOptimization, PayoffFunction, RoughVolatility, set_compat_coalescing, set_compat_seed  # noqa: F401
from .sharding import combine_sums, price_from_sums, shard_range  # noqa: F401

__all__ = ["McgError", "PathEngine", "PathMatrix", "RoughVolatility", "LSM", "AsymptoticAnalysis", "MartingaleOptimization", "BranchingProcesses",
           "PayoffFunction", "estimate_params", "rbergomi_spectrum", "make_rows", "row_build", "row_features", "stats",
           "set_compat_seed", "set_compat_coalescing", "shard_range", "combine_sums", "price_from_sums", "load_library", "lib_path",
           "exotic", "cholesky_corr", "LocalVolSurface", "local_vol_table", "X_ASIAN_ARITH_FIXED", "X_ASIAN_ARITH_FLOAT", "X_ASIAN_GEO_FIXED", "X_ASIAN_GEO_FLOAT", "X_LOOKBACK_FIXED",
           "X_LOOKBACK_FLOAT", "X_BARRIER_UP_OUT", "X_BARRIER_UP_IN", "X_BARRIER_DOWN_OUT", "X_BARRIER_DOWN_IN",
           "control", "gbm_expectation", "exotics_cv_from_sums", "CvResult", "LsmPolicy", "DualResult", "POL_CONTINUE", "POL_EXERCISE_RULE", "POL_TERMINAL", "CV_PAYOFF", "CV_VANILLA", "CV_ST", "CV_A", "CV_G",
           "Sobol", "sobol_table", "sobol_bridge", "rqmc_combine", "TANGENT_STATS", "BRIDGE_L_MAX", "BRIDGE_ROWS",
           "schedule", "autocall", "cliquet", "make_sched_book", "OBS_COUPON", "OBS_CALL", "OBS_KI", "OBS_RESET", "S_AUTOCALL", "S_CLIQUET",
           "MlmcResult", "mlmc_plan", "mlmc_combine", "mlmc_bridge_levels"]
