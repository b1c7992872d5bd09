#!/usr/bin/env python3
"""Device ms of the local-volatility generator on ONE GPU (dev tool; the judged number comes from bench.py), in one process, in
the manner of tools/bench_gbm_multi.py: HIP events around the launches (timing_select), 12 untimed ramp launches of every case
first, then alternating rounds, medians of --reps rounds.  At 10M x 252:
  cev         the CEV surface (beta = 1/2, 64 nodes, no time axis): the one-slice kernel, the slice staged once
  surface     12 knots x 64 nodes: the multi-slice kernel, four slices staged per Philox block
  gbm         mcg_paths_gbm at the same shape in the same rounds
The table upload that precedes a local-volatility launch on the stream lies outside the events.  Prints ONE JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import montecarlooptionspricer_amd as mc  # noqa: E402
from montecarlooptionspricer_amd import _native as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11, help="timed rounds (>= 10)")
ap.add_argument("--ramp", type=int, default=12, help="untimed launches of each case first")
ap.add_argument("--scale", type=float, default=1.0, help="scale the path count")
args = ap.parse_args()

seed, steps, T, r, q, S0 = 20251031, 252, 1.0, 0.04, 0.01, 100.0
n = int(10_000_000 * args.scale)
cev = mc.LocalVolSurface.cev(0.2, 0.5, -1.5, 1.5, 64)
x = [-1.5 + 3.0 * j / 63 for j in range(64)]
knots = [T * i / 11 for i in range(12)]
surface = mc.LocalVolSurface(knots, -1.5, 1.5, [[(0.18 + 0.04 * t) * math.exp(-(0.5 - 0.2 * t) * xj) for xj in x] for t in knots])
eng = mc.PathEngine(0)


def local_vol(s):
    return lambda: eng.local_vol(seed, S0, r, s, T / steps, steps, n, q=q).free()


cases = {"cev": (N.K_LOCALVOL, local_vol(cev)), "surface": (N.K_LOCALVOL, local_vol(surface)),
         "gbm": (N.K_GBM, lambda: eng.gbm(seed, S0, r, 0.2, T / steps, steps, n).free())}
for _, fn in cases.values():
    for _ in range(args.ramp):
        fn()
eng.synchronize()
eng.timing_enable(True)
eng.timing_select([N.K_LOCALVOL, N.K_GBM])
ms = {k: [] for k in cases}
for rnd in range(max(10, args.reps)):
    for name, (kernel, fn) in cases.items():
        eng.timing_reset()
        fn()
        ms[name].append(eng.timing_get(kernel)[0])
eng.timing_enable(False)
med = {k: statistics.median(v) for k, v in ms.items()}
out = {"what": "local volatility against gbm", "paths": n, "steps": steps, "rounds": max(10, args.reps)}
for k, v in ms.items():
    out[k] = {"ms_median": round(med[k], 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3),
              "Mpaths_per_s": round(n / med[k] / 1e3, 1), "TB_per_s_written": round(8 * n * (steps + 1) / med[k] / 1e9, 3),
              "over_gbm_time": round(med[k] / med["gbm"], 3)}
print(json.dumps(out), flush=True)
eng.close()
