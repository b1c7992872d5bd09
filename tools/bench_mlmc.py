#!/usr/bin/env python3
"""Multilevel Monte Carlo under local volatility on ONE GPU (dev tool; the judged number comes from bench.py), in one process, in
the manner of tools/bench_localvol.py: HIP events around the launches (timing_select), untimed ramp launches of every case
first, then alternating rounds, medians of --reps rounds.
  level kernel   k_mlmc_localvol_level at 10M paths x 256 fine steps (128 coarse) on the CEV surface (one slice) and on a 12-knot
                 surface (staged slices), against the route it replaces: local_vol + path_stats at 256 steps plus the same at 128
                 (generator under K_LOCALVOL, statistics under K_EXOTIC; the download of the statistics lies outside the events).
                 Both times and their ratio.
  estimator      mlmc_local_vol with the finest grid at 256 steps against the plain estimator (local_vol + price_exotics at
                 10M x 256), at the eps at which the plain estimator needs those 10M paths (its std error = eps / sqrt 2), for
                 the floating lookback call and the down-and-out put (B = 85): wall time and path-steps of both.
Prints ONE JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import montecarlooptionspricer_amd as mc  # noqa: E402
from montecarlooptionspricer_amd import _native as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11, help="timed rounds (>= 10)")
ap.add_argument("--ramp", type=int, default=3, help="untimed launches of each case first")
ap.add_argument("--scale", type=float, default=1.0, help="scale the path count")
args = ap.parse_args()

seed, steps, T, r, q, S0 = 20251031, 256, 1.0, 0.04, 0.01, 100.0
n = int(10_000_000 * args.scale)
cev = mc.LocalVolSurface.cev(0.2, 0.5, -1.5, 1.5, 64)
x = [-1.5 + 3.0 * j / 63 for j in range(64)]
knots = [T * i / 11 for i in range(12)]
surface = mc.LocalVolSurface(knots, -1.5, 1.5, [[(0.18 + 0.04 * t) * math.exp(-(0.5 - 0.2 * t) * xj) for xj in x] for t in knots])
book = [mc.exotic("lookback_float", True), mc.exotic("barrier_down_out", False, 100.0, 85.0)]
eng = mc.PathEngine(0)


def level(s):
    return lambda: eng.mlmc_level(seed, S0, r, s, T, book, steps, n, q=q)


def route(s):
    def run():
        for m in (steps, steps // 2):
            P = eng.local_vol(seed, S0, r, s, T / m, m, n, q=q)
            eng.path_stats(P)
            P.free()
    return run


cases = {"level_cev": level(cev), "route_cev": route(cev), "level_surface": level(surface), "route_surface": route(surface)}
for fn in cases.values():
    for _ in range(args.ramp):
        fn()
eng.synchronize()
eng.timing_enable(True)
eng.timing_select([N.K_LOCALVOL, N.K_EXOTIC])
ms = {k: [] for k in cases}
book_ms = {k: [] for k in cases}
for rnd in range(max(10, args.reps)):
    for name, fn in cases.items():
        eng.timing_reset()
        fn()
        gen, rest = eng.timing_get(N.K_LOCALVOL)[0], eng.timing_get(N.K_EXOTIC)[0]
        ms[name].append(gen if name.startswith("level") else gen + rest)   # the level kernel alone; generators + statistics
        book_ms[name].append(rest)
eng.timing_enable(False)
med = {k: statistics.median(v) for k, v in ms.items()}
out = {"what": "multilevel level kernel against local_vol + path_stats at both grids", "paths": n, "fine_steps": steps,
       "rounds": max(10, args.reps)}
for k, v in ms.items():
    out[k] = {"ms_median": round(med[k], 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}
    if k.startswith("level"):
        out[k]["book_and_reduce_ms_median"] = round(statistics.median(book_ms[k]), 3)
for s in ("cev", "surface"):
    out["route_over_level_" + s] = round(med["route_" + s] / med["level_" + s], 2)

# ---- the estimator against the plain one, contract by contract ----------------------------------------------------------------
est = {}
for name, contract in zip(("lookback_float_call", "down_and_out_put"), book):
    t0 = time.perf_counter()
    P = eng.local_vol(seed + 1, S0, r, cev, T / steps, steps, n, q=q)
    price, se = eng.price_exotics(P, r, T, [contract])
    P.free()
    t_plain = time.perf_counter() - t0
    eps = math.sqrt(2.0) * float(se[0]) * math.sqrt(args.scale)            # what the plain estimator reaches with 10M paths
    t0 = time.perf_counter()
    res = eng.mlmc_local_vol(seed, S0, r, cev, T, [contract], eps, q=q, l_min=6, l_max=6)
    t_mlmc = time.perf_counter() - t0
    est[name] = {"eps": eps, "plain": {"price": float(price[0]), "std_err": float(se[0]), "ms": round(1e3 * t_plain, 1), "path_steps": n * steps},
                 "mlmc": {"price": float(res.price[0]), "std_err": float(res.std_err[0]), "ms": round(1e3 * t_mlmc, 1), "path_steps": res.cost,
                          "paths_per_level": [lv["paths"] for lv in res.levels], "bias_estimate": float(res.bias_estimate[0])},
                 "path_steps_ratio": round(n * steps / res.cost, 2), "time_ratio": round(t_plain / t_mlmc, 2)}
out["estimator"] = est
print(json.dumps(out), flush=True)
eng.close()
