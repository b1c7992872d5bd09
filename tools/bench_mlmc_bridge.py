#!/usr/bin/env python3
"""The multilevel level kernel with the Milstein step and bridge levels on ONE GPU (dev tool; the judged number comes from
bench.py), in one process, in the manner of tools/bench_mlmc.py: HIP events around the launches (timing_select), untimed ramp
launches of every case first, then alternating rounds, medians of --reps rounds.
  level kernel   k_mlmc_localvol_level at 10M paths x 256 fine steps (128 coarse) on the CEV surface (one slice) and on a 12-knot
                 surface (staged slices): the kernel of mcg_mlmc_localvol_level ("plain"), and both schemes with 0, 1 and 4 bridge
                 levels (barriers 85 down, 120 up, 80 down, 125 up), each against "plain".
  route          what a continuous barrier price under local volatility took before: local_vol at 256 steps (a 20 GB matrix)
                 and price_barriers_bridge on it.  local_vol stores no variance matrix, so the bridge pass runs on its scalar
                 route (8 B an element read) -- a LOWER bound of the variance-matrix route (16 B an element, and a second matrix
                 to generate).  Generator under K_LOCALVOL, bridge pass under K_EXOTIC.
  estimator      mlmc_local_vol(scheme="milstein", bridge=True) for the down-and-out put (100, 85) with the finest grid at 128
                 steps against the plain bridge estimator (one level without a coarse path at 128 steps) at the same std error:
                 path-steps of both.
Prints ONE JSON line."""
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
ap.add_argument("--ramp", type=int, default=3, help="untimed launches of each case first")
ap.add_argument("--scale", type=float, default=1.0, help="scale the path count")
args = ap.parse_args()

seed, steps, T, r, q, S0 = 20251031, 256, 1.0, 0.04, 0.01, 100.0
n = int(10_000_000 * args.scale)
cev = mc.LocalVolSurface.cev(0.2, 0.5, -1.5, 1.5, 64)
x = [-1.5 + 3.0 * j / 63 for j in range(64)]
knots = [T * i / 11 for i in range(12)]
surface = mc.LocalVolSurface(knots, -1.5, 1.5, [[(0.18 + 0.04 * t) * math.exp(-(0.5 - 0.2 * t) * xj) for xj in x] for t in knots])
barriers = [mc.exotic("barrier_down_out", False, 100.0, 85.0), mc.exotic("barrier_up_out", True, 100.0, 120.0),
            mc.exotic("barrier_down_out", False, 100.0, 80.0), mc.exotic("barrier_up_out", True, 100.0, 125.0)]
euro = [mc.exotic("barrier_down_out", True, 100.0, 0.0)]
eng = mc.PathEngine(0)


def level(s, scheme, n_levels):
    book = barriers[:n_levels] if n_levels else euro
    return lambda: eng.mlmc_level(seed, S0, r, s, T, book, steps, n, q=q, scheme=scheme, bridge=n_levels > 0)


def route(s):
    def run():
        P = eng.local_vol(seed, S0, r, s, T / steps, steps, n, q=q)
        eng.price_barriers_bridge(P, r, T, barriers[:1], sigma=0.2)
        P.free()
    return run


cases = {}
for tag, s in (("cev", cev), ("surface", surface)):
    cases[f"plain_{tag}"] = level(s, "euler", 0)
    for scheme in ("euler", "milstein"):
        for n_levels in (0, 1, 4):
            if scheme == "euler" and n_levels == 0:
                continue
            cases[f"{scheme}_{n_levels}_{tag}"] = level(s, scheme, n_levels)
    cases[f"route_{tag}"] = route(s)
for fn in cases.values():
    for _ in range(args.ramp):
        fn()
eng.synchronize()
eng.timing_enable(True)
eng.timing_select([N.K_LOCALVOL, N.K_EXOTIC])
ms = {k: [] for k in cases}
for rnd in range(max(10, args.reps)):
    for name, fn in cases.items():
        eng.timing_reset()
        fn()
        gen, rest = eng.timing_get(N.K_LOCALVOL)[0], eng.timing_get(N.K_EXOTIC)[0]
        ms[name].append(gen + rest if name.startswith("route") else gen)       # the level kernel alone; generator + bridge pass
eng.timing_enable(False)
med = {k: statistics.median(v) for k, v in ms.items()}
out = {"what": "multilevel level kernel with Milstein and bridge levels against the plain level kernel and the matrix route",
       "paths": n, "fine_steps": steps, "rounds": max(10, args.reps)}
for k, v in ms.items():
    tag = k.rsplit("_", 1)[1]
    out[k] = {"ms_median": round(med[k], 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3),
              "over_plain": round(med[k] / med["plain_" + tag], 3)}

# ---- the estimator against the plain bridge estimator -------------------------------------------------------------------------
book = barriers[:1]
n_plain = int(2_000_000 * args.scale)
s = eng.mlmc_level(seed + 1, S0, r, cev, T, book, 128, n_plain, has_coarse=False, q=q, scheme="milstein", bridge=True)
disc = math.exp(-r * T)
var = (s[3] - n_plain * (s[2] / n_plain) ** 2) / (n_plain - 1.0)
eps = math.sqrt(2.0) * disc * math.sqrt(var / n_plain)                         # what the plain estimator reaches with these paths
res = eng.mlmc_local_vol(seed, S0, r, cev, T, book, eps, q=q, l_min=5, l_max=5, scheme="milstein", bridge=True)
plain_steps = 128 * var * disc * disc / float(res.std_err[0]) ** 2
out["estimator"] = {"eps": eps, "plain": {"price": disc * s[2] / n_plain, "std_err": disc * math.sqrt(var / n_plain), "paths": n_plain},
                    "mlmc": {"price": float(res.price[0]), "std_err": float(res.std_err[0]), "path_steps": res.cost,
                             "paths_per_level": [lv["paths"] for lv in res.levels], "var_per_level": [float(lv["var_y"][0]) for lv in res.levels],
                             "bias_estimate": float(res.bias_estimate[0])},
                    "plain_path_steps_at_the_same_std_err": plain_steps, "path_steps_ratio": round(plain_steps / res.cost, 2)}
print(json.dumps(out), flush=True)
eng.close()
