#!/usr/bin/env python3
"""Device ms of the Heston generator on ONE GPU (dev tool; the judged number comes from bench.py), at the 10M x 252 shape of
bench.py's C2 arguments, in one process:
  * mcg_paths_heston, prices only;
  * mcg_paths_heston with the variance matrix (twice the bytes);
  * mcg_paths_gbm of the same shape, the yardstick for the arithmetic;
  * mcg_probe_write_ceiling: what this board writes with the generator's store pattern and no arithmetic.
HIP events around the one generator launch (timing_select).  Each generator first gets the 12 untimed ramp launches that
precede bench.py's headline (an idle MI355X needs them to settle at its clock under load); the measurements then alternate,
medians of --reps rounds.  GB/s written = 8 B x paths x (steps + 1) x matrices over the kernel time.  One JSON line per
measurement, then the ratios to the GBM time and to the write ceiling."""
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
ap.add_argument("--ramp", type=int, default=12, help="untimed launches of each generator first")
ap.add_argument("--scale", type=float, default=1.0, help="scale the path count")
args = ap.parse_args()

n, steps, dt, seed = int(10_000_000 * args.scale), 252, 1.0 / 252.0, 20251031
H = dict(S0=100.0, r=0.04, v0=0.04, kappa=2.0, theta=0.04, sigma_v=0.3, rho=-0.7)
eng = mc.PathEngine(0)


def heston(want_variance):
    got = eng.heston(seed, dt=dt, n_steps=steps, n_paths=n, want_variance=want_variance, **H)
    for M in (got if want_variance else (got,)):
        M.free()


cases = {
    "heston, prices only": (N.K_HESTON, lambda: heston(False), 1),
    "heston, prices + variances": (N.K_HESTON, lambda: heston(True), 2),
    "gbm": (N.K_GBM, lambda: eng.gbm(seed, 100.0, 0.04, 0.2, dt, steps, n).free(), 1),
}
for _, fn, _ in cases.values():
    for _ in range(args.ramp):
        fn()
eng.synchronize()
eng.timing_enable(True)
ms = {k: [] for k in cases}
for rnd in range(max(10, args.reps)):
    for name, (kernel, fn, _) in cases.items():
        eng.timing_select([kernel])
        eng.timing_reset()
        fn()
        ms[name].append(eng.timing_get(kernel)[0])
eng.timing_enable(False)
ceiling_gbs, ceiling_ms = eng.probe_write_ceiling(n, steps, 5)
med = {k: statistics.median(v) for k, v in ms.items()}
for name, (_, _, matrices) in cases.items():
    gbs = 8.0 * n * (steps + 1) * matrices / med[name] / 1e6
    print(json.dumps({"what": name, "paths": n, "steps": steps, "ms_median": round(med[name], 3), "ms_min": round(min(ms[name]), 3),
                      "ms_max": round(max(ms[name]), 3), "rounds": len(ms[name]), "Mpaths_per_s": round(n / med[name] / 1e3, 1),
                      "GB_per_s_written": round(gbs, 1), "ratio_to_gbm_time": round(med[name] / med["gbm"], 3),
                      "share_of_write_ceiling": round(gbs / ceiling_gbs, 3)}), flush=True)
print(json.dumps({"what": "mcg_probe_write_ceiling", "paths": n, "steps": steps, "GB_per_s": round(ceiling_gbs, 1),
                  "ms_per_launch": round(ceiling_ms, 3)}), flush=True)
eng.close()
