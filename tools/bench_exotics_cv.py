#!/usr/bin/env python3
"""Device ms of the control-variate pricer on ONE GPU (dev tool; the judged number comes from bench.py), on the 10M x 252 GBM
matrix of bench.py's C2 arguments, for a book of 1 and of 64 contracts:
  * price_exotics (the yardstick, unchanged) -- for one contract both without and with the geometric mean, which the control needs;
  * price_exotics_cv with a control on the paths themselves (no twin: no extra byte is moved);
  * ... with a control on a STORED GBM twin matrix, its generation included (mcg_paths_gbm + a second k_path_stats);
  * ... with a control on the twin computed in registers (k_gbm_twin_stats: no matrix);
  * k_gbm_twin_stats alone against mcg_paths_gbm + mcg_path_stats, the two ways to the twin's statistics;
  * the achieved variance ratio (plain_se / std_err)^2 of the one-contract cases.
HIP events around every launch (timing_select of K_EXOTIC and K_GBM); the measurements alternate in one process on one
matrix; medians of --reps rounds after a ramp.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlooptionspricer_amd as mc  # noqa: E402
from montecarlooptionspricer_amd import _native as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11, help="timed rounds (>= 10)")
ap.add_argument("--ramp", type=int, default=3, help="untimed rounds first")
ap.add_argument("--scale", type=float, default=1.0, help="scale the path count")
args = ap.parse_args()

SEED, S0, R, SIGMA, DT, T = 20251031, 100.0, 0.04, 0.2, 1.0 / 252.0, 1.0
n, steps = int(10_000_000 * args.scale), 252
eng = mc.PathEngine(0)
P = eng.gbm(SEED, S0, R, SIGMA, DT, steps, n, payoff=(100.0, True))
TWIN = dict(seed=SEED, S0=S0, r=R, q=0.0, sigma=SIGMA, dt=DT, path_begin=0)
eng.timing_enable(True)


def book(count):
    """Kinds in turn, geometric ones included; barriers and strikes spread around the money (tools/bench_exotics.py's)."""
    return [mc.exotic(i % 10, (i // 10) % 2 == 0, 80.0 + 40.0 * i / count, (110.0 if i % 10 in (6, 7) else 90.0) + 10.0 * i / count, 1.0)
            for i in range(count)]


def geo_control(K, on_twin):
    return mc.gbm_expectation(mc.control("payoff", on_twin=on_twin, kind="asian_geo_fixed", is_call=True, K=K), S0, R, SIGMA, DT, steps)


def device_ms(fn):
    eng.timing_select([N.K_EXOTIC, N.K_GBM])
    eng.timing_reset()
    out = fn()
    return eng.timing_get(N.K_EXOTIC)[0] + eng.timing_get(N.K_GBM)[0], out


def stored_twin(fn):
    """fn(twin matrix) with the twin generated first and freed afterwards: what a caller without the in-register twin pays.
    (Under GBM the twin of the same seed is the path matrix once more; what is measured is its cost.)"""
    Q = eng.gbm(SEED, S0, R, SIGMA, DT, steps, n)
    try:
        return fn(Q)
    finally:
        Q.free()


ARITH = [mc.exotic("asian_arith_fixed", True, 100.0)]
GEO = [mc.exotic("asian_geo_fixed", True, 100.0)]
B64 = book(64)
C64_OWN, C64_TWIN = [geo_control(c[2], False) for c in B64], [geo_control(c[2], True) for c in B64]
I64 = list(range(64))
cases = {
    "price_exotics, 1 contract (arithmetic Asian: no G)": lambda: eng.price_exotics(P, R, T, ARITH),
    "price_exotics, 1 contract (geometric Asian: with G)": lambda: eng.price_exotics(P, R, T, GEO),
    "price_exotics_cv, 1 contract, control on the paths (with G)": lambda: eng.price_exotics_cv(P, R, T, ARITH, [geo_control(100.0, False)], [0]),
    "price_exotics_cv, 1 contract, stored GBM twin (generation included)":
        lambda: stored_twin(lambda Q: eng.price_exotics_cv(P, R, T, ARITH, [geo_control(100.0, True)], [0], twin=Q)),
    "price_exotics_cv, 1 contract, in-register twin": lambda: eng.price_exotics_cv(P, R, T, ARITH, [geo_control(100.0, True)], [0], twin=TWIN),
    "price_exotics, 64 contracts": lambda: eng.price_exotics(P, R, T, B64),
    "price_exotics_cv, 64 contracts, control on the paths": lambda: eng.price_exotics_cv(P, R, T, B64, C64_OWN, I64),
    "price_exotics_cv, 64 contracts, stored GBM twin (generation included)":
        lambda: stored_twin(lambda Q: eng.price_exotics_cv(P, R, T, B64, C64_TWIN, I64, twin=Q)),
    "price_exotics_cv, 64 contracts, in-register twin": lambda: eng.price_exotics_cv(P, R, T, B64, C64_TWIN, I64, twin=TWIN),
    "k_gbm_twin_stats alone": lambda: eng.gbm_twin_stats(TWIN, steps, n),
    "mcg_paths_gbm + mcg_path_stats": lambda: stored_twin(lambda Q: eng.path_stats(Q)),
}
ms = {k: [] for k in cases}
last = {}
for rnd in range(args.ramp + max(10, args.reps)):
    for name, fn in cases.items():
        t, out = device_ms(fn)
        last[name] = out
        if rnd >= args.ramp:
            ms[name].append(t)
med = {k: statistics.median(v) for k, v in ms.items()}
for name in cases:
    line = {"what": name, "paths": n, "steps": steps, "ms_median": round(med[name], 3), "ms_min": round(min(ms[name]), 3),
            "ms_max": round(max(ms[name]), 3), "rounds": len(ms[name])}
    out = last[name]
    if isinstance(out, mc.CvResult) and len(out.price) == 1:
        line.update(price=round(float(out.price[0]), 6), std_err=float(out.std_err[0]), plain_se=float(out.plain_se[0]),
                    variance_ratio=round(float(out.variance_ratio[0]), 1))
    print(json.dumps(line), flush=True)
y1, y64 = med["price_exotics, 1 contract (geometric Asian: with G)"], med["price_exotics, 64 contracts"]
print(json.dumps({"what": "ratios to price_exotics of the same run",
                  "cv_no_twin_1": round(med["price_exotics_cv, 1 contract, control on the paths (with G)"] / y1, 3),
                  "cv_stored_twin_1": round(med["price_exotics_cv, 1 contract, stored GBM twin (generation included)"] / y1, 3),
                  "cv_register_twin_1": round(med["price_exotics_cv, 1 contract, in-register twin"] / y1, 3),
                  "cv_no_twin_64": round(med["price_exotics_cv, 64 contracts, control on the paths"] / y64, 3),
                  "cv_stored_twin_64": round(med["price_exotics_cv, 64 contracts, stored GBM twin (generation included)"] / y64, 3),
                  "cv_register_twin_64": round(med["price_exotics_cv, 64 contracts, in-register twin"] / y64, 3),
                  "twin_stats_over_gbm_plus_path_stats": round(med["k_gbm_twin_stats alone"] / med["mcg_paths_gbm + mcg_path_stats"], 3)}), flush=True)
P.free()
eng.close()
