#!/usr/bin/env python3
"""Device ms of the LSM exercise policies on ONE GPU (dev tool; the judged number comes from bench.py), on 10M x 50 and
10M x 252 GBM matrices, at-the-money put (S0 = K = 100), order 2:
  * fit_lsm (the exporting per-date sweep) beside price_lsm forced onto the per-date route by an identity all-reduce on a
    second engine holding the same matrix (HIP events around the queued launch sequence, MCG_K_LSM_SWEEP);
  * apply_lsm with an all-CONTINUE policy (every row of every path is read) beside mcg_path_stats on the same matrix -- the
    same 8 B per path and date (MCG_K_LSM_APPLY against MCG_K_EXOTIC);
  * apply_lsm with the fitted policy: a wavefront stops reading once all its paths have exercised, so TB/s is given by the
    bytes actually needed, 8 B x sum over the paths of (tau + 1), from the call's own tau_hist.
The measurements alternate in one process; medians of --reps rounds after --ramp untimed ones.  One JSON line per
measurement."""
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
ap.add_argument("--scale", type=float, default=1.0, help="scale the path count")
ap.add_argument("--order", type=int, default=2)
args = ap.parse_args()

HBM_PEAK_GBS = 8000.0
R, K, SIGMA, T = 0.04, 100.0, 0.2, 1.0
n = int(10_000_000 * args.scale)
eng, routed = mc.PathEngine(0), mc.PathEngine(0)
routed.set_allreduce(lambda ptr, count, stream: None)
for e in (eng, routed):
    e.timing_enable(True)


def device_ms(e, kernel, fn):
    e.timing_select([kernel])
    e.timing_reset()
    fn()
    return e.timing_get(kernel)[0]


for steps in (50, 252):
    dt = T / steps
    P = eng.gbm(20251031, 100.0, R, SIGMA, dt, steps, n)
    Q = routed.gbm(20251031, 100.0, R, SIGMA, dt, steps, n)
    lsm = (R, K, T, dt, False, args.order)
    price, se, policy = eng.fit_lsm(P, *lsm)
    nothing = mc.LsmPolicy.from_arrays(steps, args.order, False, R, K, T, dt, kinds=[N.POL_CONTINUE] * steps + [N.POL_TERMINAL])
    out_price, out_se, hist = eng.apply_lsm(policy, P, return_hist=True)
    rows_needed = float(sum(int(c) * (j + 1) for j, c in enumerate(hist)))   # rows read if nothing were requested in vain
    cases = {
        "fit_lsm": (eng, N.K_LSM_SWEEP, lambda: eng.fit_lsm(P, *lsm), None),
        "price_lsm, per-date route": (routed, N.K_LSM_SWEEP, lambda: routed.price_lsm(Q, *lsm), None),
        "apply_lsm, all-CONTINUE policy": (eng, N.K_LSM_APPLY, lambda: eng.apply_lsm(nothing, P, return_hist=True), float(n) * (steps + 1)),
        "mcg_path_stats": (eng, N.K_EXOTIC, lambda: eng.path_stats(P, first_row=0), float(n) * (steps + 1)),
        "apply_lsm, fitted policy": (eng, N.K_LSM_APPLY, lambda: eng.apply_lsm(policy, P, return_hist=True), rows_needed),
    }
    ms = {k: [] for k in cases}
    for rnd in range(args.ramp + args.reps):
        for name, (e, kernel, fn, _) in cases.items():
            t = device_ms(e, kernel, fn)
            if rnd >= args.ramp:
                ms[name].append(t)
    med = {k: statistics.median(v) for k, v in ms.items()}
    for name, (_, _, _, elements) in cases.items():
        line = {"what": name, "paths": n, "steps": steps, "order": args.order, "ms_median": round(med[name], 3),
                "ms_min": round(min(ms[name]), 3), "ms_max": round(max(ms[name]), 3), "rounds": len(ms[name])}
        if elements is not None:
            gbs = 8.0 * elements / med[name] / 1e6
            line.update(GB_read=round(8.0 * elements / 1e9, 3), TB_per_s=round(gbs / 1e3, 3), share_of_8TBps_peak=round(gbs / HBM_PEAK_GBS, 3))
        print(json.dumps(line), flush=True)
    print(json.dumps({"what": "ratios", "steps": steps,
                      "fit_lsm / price_lsm per-date": round(med["fit_lsm"] / med["price_lsm, per-date route"], 3),
                      "apply all-CONTINUE / path_stats": round(med["apply_lsm, all-CONTINUE policy"] / med["mcg_path_stats"], 3),
                      "apply fitted / apply all-CONTINUE": round(med["apply_lsm, fitted policy"] / med["apply_lsm, all-CONTINUE policy"], 3),
                      "share of path-dates needed": round(rows_needed / (float(n) * (steps + 1)), 4),
                      "in-sample price": round(price, 5), "policy on its own paths": round(out_price, 5), "std_err": round(out_se, 5)}),
          flush=True)
    P.free()
    Q.free()
eng.close()
routed.close()
