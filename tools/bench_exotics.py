#!/usr/bin/env python3
"""Device ms of the path-dependent payoffs on ONE GPU (dev tool; the judged number comes from bench.py), on the 10M x 252 GBM
matrix of bench.py's C2 arguments:
  * k_path_stats alone (path_stats: all five statistics; HIP events around the one launch, timing_select(K_EXOTIC));
  * price_exotics with a book of 1, 64 and 1024 contracts (statistics + book + reduction, the same events);
  * k_asym_scan (price_asymptotic), the existing kernel that streams the same 8 B per path and date, as the yardstick.
The measurements alternate in one process on one matrix; medians of --reps rounds after a ramp.  GB/s = 8 B x paths x
monitored rows over the kernel time, against the 8 TB/s HBM peak.  One JSON line per measurement."""
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

HBM_PEAK_GBS = 8000.0
n, steps = int(10_000_000 * args.scale), 252
eng = mc.PathEngine(0)
P = eng.gbm(20251031, 100.0, 0.04, 0.2, 1.0 / 252.0, steps, n, payoff=(100.0, True))
eng.timing_enable(True)


def book(count):
    """Kinds in turn, geometric ones included; barriers and strikes spread around the money."""
    return [mc.exotic(i % 10, (i // 10) % 2 == 0, 80.0 + 40.0 * i / count, (110.0 if i % 10 in (6, 7) else 90.0) + 10.0 * i / count, 1.0)
            for i in range(count)]


def device_ms(kernel, fn):
    eng.timing_select([kernel])
    eng.timing_reset()
    fn()
    return eng.timing_get(kernel)[0]


cases = {
    "k_path_stats (5 statistics)": (N.K_EXOTIC, lambda: eng.path_stats(P), steps),
    "price_exotics, 1 contract (arithmetic Asian: no G)": (N.K_EXOTIC, lambda b=book(1): eng.price_exotics(P, 0.04, 1.0, b), steps),
    "price_exotics, 64 contracts": (N.K_EXOTIC, lambda b=book(64): eng.price_exotics(P, 0.04, 1.0, b), steps),
    "price_exotics, 1024 contracts": (N.K_EXOTIC, lambda b=book(1024): eng.price_exotics(P, 0.04, 1.0, b), steps),
    "k_asym_scan (price_asymptotic)": (N.K_ASYM, lambda: eng.price_asymptotic(P, 0.04, 100.0, 1.0, 1.0 / 252.0, False, 0.2, 0.0), steps + 1),
}
ms = {k: [] for k in cases}
for rnd in range(args.ramp + max(10, args.reps)):
    for name, (kernel, fn, _) in cases.items():
        t = device_ms(kernel, fn)
        if rnd >= args.ramp:
            ms[name].append(t)
for name, (_, _, rows) in cases.items():
    med = statistics.median(ms[name])
    gbs = 8.0 * n * rows / med / 1e6
    print(json.dumps({"what": name, "paths": n, "rows_read": rows, "ms_median": round(med, 3), "ms_min": round(min(ms[name]), 3),
                      "ms_max": round(max(ms[name]), 3), "rounds": len(ms[name]), "matrix_GB_per_s": round(gbs, 1),
                      "share_of_8TBps_peak": round(gbs / HBM_PEAK_GBS, 3)}), flush=True)
a, s = statistics.median(ms["k_asym_scan (price_asymptotic)"]), statistics.median(ms["k_path_stats (5 statistics)"])
print(json.dumps({"what": "k_path_stats / k_asym_scan, per row read", "ratio": round((s / steps) / (a / (steps + 1)), 3)}), flush=True)
P.free()
eng.close()
