#!/usr/bin/env python3
"""Device ms of the multi-asset GBM generator on ONE GPU (dev tool; the judged number comes from bench.py), in one process, in
the manner of tools/bench_bates.py: HIP events around the launches (timing_select), 12 untimed ramp launches of every case
first, then alternating rounds, medians of --reps rounds.  For D = 2, 4, 8 assets at 10M x 252 (D = 8: 4M paths, so that its
eight asset matrices and the combined one fit beside the pool), worst-of with weights 1 / S0:
  fused       mcg_paths_gbm_multi, combined matrix only: 8 B stored per path-step
  two-step    mcg_paths_gbm_multi, asset matrices only, then mcg_paths_combine: (2 D + 1) * 8 B moved per path-step
  combine     the mcg_paths_combine launch of the two-step route alone, in TB/s of the (D + 1) * 8 B per path-step it moves, beside
              mcg_probe_write_ceiling of the same process
  gbm         mcg_paths_gbm at the same shape in the same rounds
Prints ONE JSON line."""
import argparse
import json
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
ap.add_argument("--scale", type=float, default=1.0, help="scale the path counts")
ap.add_argument("--assets", type=int, nargs="+", default=[2, 4, 8])
args = ap.parse_args()

seed, steps, T, r = 20251031, 252, 1.0, 0.04
eng = mc.PathEngine(0)
ceiling_gbs, _ = eng.probe_write_ceiling(int(10_000_000 * args.scale), steps, 5)
eng.trim()
rows = []
for D in args.assets:
    n = int((4_000_000 if D >= 8 else 10_000_000) * args.scale)
    S0 = [100.0 + 10.0 * a for a in range(D)]
    sigma = [0.15 + 0.03 * a for a in range(D)]
    corr = [[0.5 ** abs(i - j) for j in range(D)] for i in range(D)]
    w = [1.0 / s for s in S0]
    gen = dict(seed=seed, S0=S0, r=r, sigma=sigma, corr=corr, dt=T / steps, n_steps=steps, n_paths=n)
    split = {"combine": 0.0}

    def fused():
        eng.gbm_multi(combine="worst_of", weights=w, want_assets=False, **gen)[1].free()

    def two_step():
        assets, _ = eng.gbm_multi(**gen)
        generated = eng.timing_get(N.K_MULTI)[0]      # (0 while timing is off; waits for the launch)
        eng.combine(assets, "worst_of", w).free()
        split["combine"] = eng.timing_get(N.K_MULTI)[0] - generated
        for a in assets:
            a.free()

    def gbm():
        eng.gbm(seed, S0[0], r, sigma[0], T / steps, steps, n).free()

    cases = {"fused": (N.K_MULTI, fused), "two-step": (N.K_MULTI, two_step), "gbm": (N.K_GBM, gbm)}
    for _, fn in cases.values():
        for _ in range(args.ramp):
            fn()
    eng.synchronize()
    eng.timing_enable(True)
    eng.timing_select([N.K_MULTI, N.K_GBM])
    ms = {k: [] for k in list(cases) + ["combine"]}
    for rnd in range(max(10, args.reps)):
        for name, (kernel, fn) in cases.items():
            eng.timing_reset()
            fn()
            ms[name].append(eng.timing_get(kernel)[0])
            if name == "two-step":
                ms["combine"].append(split["combine"])
    eng.timing_enable(False)
    med = {k: statistics.median(v) for k, v in ms.items()}
    cells = n * (steps + 1)
    row = {"assets": D, "paths": n}
    for k, v in ms.items():
        row[k] = {"ms_median": round(med[k], 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}
    row["fused"]["Mpaths_per_s"] = round(n / med["fused"] / 1e3, 1)
    row["fused_over_two_step_time"] = round(med["fused"] / med["two-step"], 3)
    row["fused_over_gbm_time"] = round(med["fused"] / med["gbm"], 3)
    row["combine"]["TB_per_s"] = round((D + 1) * 8 * cells / med["combine"] / 1e9, 3)
    row["combine"]["share_of_write_ceiling"] = round((D + 1) * 8 * cells / med["combine"] / 1e6 / ceiling_gbs, 3)
    rows.append(row)
    eng.trim()
print(json.dumps({"what": "multi-asset gbm: fused against two-step", "steps": steps, "rounds": max(10, args.reps),
                  "write_ceiling_TB_per_s": round(ceiling_gbs / 1e3, 3), "cases": rows}), flush=True)
eng.close()
