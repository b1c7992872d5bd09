#!/usr/bin/env python3
"""Device ms of the dual upper bound (mcg_lsm_dual_upper) on ONE GPU (dev tool; the judged number comes from bench.py): the
Longstaff-Schwartz put (S0 = 36, K = 40, sigma = 0.2, r = 0.06, T = 1, 50 dates), 4096 outer paths x {256, 4096} inner paths,
  * with the order-3 policy fit_lsm fits on 200 003 paths: inner paths stop where the rule exercises, lanes of a wavefront at
    different dates -- live lane-steps (inner_steps) over executed ones (mcg_debug_lsm_dual_executed) is the share of the
    wavefronts' work that was of use;
  * with an all-CONTINUE policy: no inner path stops early, every lane-step is live (and no date asks for a price: the step is
    Philox, Box-Muller and the fused add, one exponential per path at the last date);
  * beside mcg_gbm_twin_stats (MCG_K_EXOTIC) at a path and step count giving the all-CONTINUE run's number of path-steps: the
    same draws and step with an exponential every step, no policy and no ballot -- the yardstick.
The measurements alternate in one process; medians of --reps rounds after --ramp untimed ones.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlooptionspricer_amd as mc  # noqa: E402
from montecarlooptionspricer_amd import _native as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11, help="timed rounds")
ap.add_argument("--ramp", type=int, default=3, help="untimed rounds first")
ap.add_argument("--outer", type=int, default=4096)
ap.add_argument("--inner", type=int, nargs="+", default=[256, 4096])
ap.add_argument("--order", type=int, default=3)
args = ap.parse_args()

S0, K, SIGMA, R, T, STEPS = 36.0, 40.0, 0.2, 0.06, 1.0, 50
dt = T / STEPS
eng = mc.PathEngine(0)
eng.timing_enable(True)


def device_ms(kernel, fn):
    eng.timing_select([kernel])
    eng.timing_reset()
    out = fn()
    return eng.timing_get(kernel)[0], out


F = eng.gbm(20240607, S0, R, SIGMA, dt, STEPS, 200003)
_, _, policy = eng.fit_lsm(F, R, K, T, dt, False, args.order)
F.free()
nothing = mc.LsmPolicy.from_arrays(STEPS, args.order, False, R, K, T, dt, kinds=[N.POL_CONTINUE] * STEPS + [N.POL_TERMINAL])
P = eng.gbm(20240608, S0, R, SIGMA, dt, STEPS, args.outer)
lower, lower_se = eng.apply_lsm(policy, P)
twin = dict(seed=5, S0=S0, r=R, q=0.0, sigma=SIGMA, dt=dt, path_begin=0)

for n_inner in args.inner:
    all_steps = args.outer * n_inner * STEPS * (STEPS + 1) // 2
    twin_steps = STEPS * (STEPS + 1) // 2 * 4                      # 5100 steps x (outer * inner / 4) paths: the same path-steps
    twin_paths = max(args.outer * n_inner // 4, 1)
    cases = {
        "dual_upper_lsm, fitted policy": (N.K_LSM_DUAL, lambda: eng.dual_upper_lsm(policy, P, SIGMA, n_inner, seed=77)),
        "dual_upper_lsm, all-CONTINUE policy": (N.K_LSM_DUAL, lambda: eng.dual_upper_lsm(nothing, P, SIGMA, n_inner, seed=77)),
        "mcg_gbm_twin_stats": (N.K_EXOTIC, lambda: eng.gbm_twin_stats(twin, twin_steps, twin_paths)[0, :1]),
    }
    ms = {k: [] for k in cases}
    last, executed = {}, {}
    for rnd in range(args.ramp + args.reps):
        for name, (kernel, fn) in cases.items():
            t, out = device_ms(kernel, fn)
            last[name] = out
            if kernel == N.K_LSM_DUAL:
                executed[name] = eng.debug_lsm_dual_executed()
            if rnd >= args.ramp:
                ms[name].append(t)
    med = {k: statistics.median(v) for k, v in ms.items()}
    twin_rate = float(twin_steps) * twin_paths / med["mcg_gbm_twin_stats"] / 1e-3
    for name in cases:
        line = {"what": name, "outer": args.outer, "inner": n_inner, "dates": STEPS, "ms_median": round(med[name], 3),
                "ms_min": round(min(ms[name]), 3), "ms_max": round(max(ms[name]), 3), "rounds": len(ms[name])}
        if name == "mcg_gbm_twin_stats":
            line.update(paths=twin_paths, steps=twin_steps, path_steps=twin_steps * twin_paths, path_steps_per_s=float(f"{twin_rate:.4g}"))
        else:
            res = last[name]
            rate = res.inner_steps / med[name] / 1e-3
            line.update(upper=round(res.upper, 5), std_err=round(res.std_err, 5), inner_steps=res.inner_steps,
                        executed_steps=executed[name], live_over_executed=round(res.inner_steps / executed[name], 4),
                        inner_path_steps_per_s=float(f"{rate:.4g}"), ratio_to_twin=round(rate / twin_rate, 3),
                        executed_ratio_to_twin=round(executed[name] / med[name] / 1e-3 / twin_rate, 3))
        print(json.dumps(line), flush=True)
    assert last["dual_upper_lsm, all-CONTINUE policy"].inner_steps == all_steps
print(json.dumps({"what": "bracket", "lower": round(lower, 5), "lower_se": round(lower_se, 5), "outer": args.outer}), flush=True)
P.free()
eng.close()
