#!/usr/bin/env python3
"""Device ms of the notes on an observation schedule (price_scheduled) on ONE GPU (dev tool; the judged number comes from
bench.py), on the 10M x 252 GBM matrix of bench.py's C2 arguments, by the method of tools/bench_exotics.py: one process, ramp
rounds, then medians of --reps alternating rounds, with k_path_stats in the same rounds and mcg_probe_write_ceiling beside them.
  1. every row scheduled, a never-called book of 8 autocallables: the upper bound on the cost per row read (ms, GB/s of matrix
     read, the ratio to k_path_stats per row);
  2. quarterly COUPON|CALL with daily KI, 8 autocallables: the bytes actually needed are the rows up to each wavefront's
     (128 adjacent paths) last live path, counted from mcg_sched_path_values' stop on the same matrix;
  3. the quarterly schedule alone, 4 rows;
  4. case 2's schedule with books of 1, 64 and 1024 contracts (the rows are re-read once per chunk of 8).
One JSON line per measurement; nothing here is a pass/fail number."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlooptionspricer_amd as mc  # noqa: E402
from montecarlooptionspricer_amd import _native as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11, help="timed rounds (>= 10)")
ap.add_argument("--ramp", type=int, default=3, help="untimed rounds first")
ap.add_argument("--scale", type=float, default=1.0, help="scale the path count")
args = ap.parse_args()

n, steps, r, dt = int(10_000_000 * args.scale), 252, 0.04, 1.0 / 252.0
CC, KI = N.OBS_COUPON | N.OBS_CALL, N.OBS_KI
eng = mc.PathEngine(0)
P = eng.gbm(20251031, 100.0, r, 0.2, dt, steps, n, payoff=(100.0, True))
eng.timing_enable(True)


def notes(count, never_called=False):
    """Autocallables with call levels around the money, memory coupons on every other one, a 70% knock-in put."""
    return [mc.autocall(math.inf if never_called else 0.95 + 0.15 * (i % 8) / 8.0, 0.02, 0.8, 0.7, 1.0, memory=i % 2 == 0) for i in range(count)]


every_row = [(j, CC | KI) for j in range(steps + 1)]
daily_ki = [(j, KI | (CC if j % 63 == 0 else 0)) for j in range(1, steps + 1)]
quarterly = [(j, CC | (KI if j == steps else 0)) for j in range(63, steps + 1, 63)]


def needed_bytes(sched, book):
    """8 B x the scheduled rows up to the last live path of each wavefront's 128 adjacent paths (and row 0), summed."""
    _, stop = eng.sched_path_values(P, r, dt, sched, book)
    last = np.minimum(stop.max(axis=0), len(sched) - 1).astype(np.int64)          # the last observation any contract looks at
    pad = (-len(last)) % 128
    waves = np.concatenate([last, np.zeros(pad, dtype=np.int64)]).reshape(-1, 128).max(axis=1)
    return float(8 * 128 * (waves + 2).sum())                                     # observations 0 .. last, and row 0


def device_ms(fn):
    eng.timing_select([N.K_EXOTIC])
    eng.timing_reset()
    fn()
    return eng.timing_get(N.K_EXOTIC)[0]


def case(sched, book):
    return lambda: eng.price_scheduled(P, r, dt, sched, book)


matrix = lambda rows: 8.0 * n * rows  # noqa: E731
cases = {
    "k_path_stats (5 statistics)": (lambda: eng.path_stats(P), matrix(steps)),
    "1. every row, 8 never-called notes": (case(every_row, notes(8, True)), matrix(steps + 1)),
    "2. quarterly calls, daily KI, 8 notes": (case(daily_ki, notes(8)), needed_bytes(daily_ki, notes(8))),
    "3. quarterly schedule alone (4 rows), 8 notes": (case(quarterly, notes(8)), matrix(len(quarterly) + 1)),
    "4. schedule of 2, 1 note": (case(daily_ki, notes(1)), needed_bytes(daily_ki, notes(1))),
    "4. schedule of 2, 64 notes": (case(daily_ki, notes(64)), None),
    "4. schedule of 2, 1024 notes": (case(daily_ki, notes(1024)), None),
}
ms = {k: [] for k in cases}
for rnd in range(args.ramp + max(10, args.reps)):
    for name, (fn, _) in cases.items():
        t = device_ms(fn)
        if rnd >= args.ramp:
            ms[name].append(t)
for name, (_, nbytes) in cases.items():
    med = statistics.median(ms[name])
    row = {"what": name, "paths": n, "ms_median": round(med, 3), "ms_min": round(min(ms[name]), 3), "ms_max": round(max(ms[name]), 3),
           "rounds": len(ms[name])}
    if nbytes is not None:
        row.update({"GB_needed": round(nbytes / 1e9, 3), "GB_per_s": round(nbytes / med / 1e6, 1)})
    print(json.dumps(row), flush=True)
stats_ms, all_ms = statistics.median(ms["k_path_stats (5 statistics)"]), statistics.median(ms["1. every row, 8 never-called notes"])
print(json.dumps({"what": "case 1 / k_path_stats, per row read", "ratio": round((all_ms / (steps + 1)) / (stats_ms / steps), 3)}), flush=True)
gbs, ceiling_ms = eng.probe_write_ceiling(n, steps, 5)
print(json.dumps({"what": "mcg_probe_write_ceiling", "paths": n, "steps": steps, "GB_per_s": round(gbs, 1), "ms_per_launch": round(ceiling_ms, 3)}), flush=True)
price, se, hist = eng.price_scheduled(P, r, dt, quarterly, notes(1), return_hist=True)
print(json.dumps({"what": "quarterly note, call level 0.95", "price": round(float(price[0]), 6), "std_err": round(float(se[0]), 6),
                  "stop_share": [round(float(x), 4) for x in hist[0] / n]}), flush=True)
P.free()
eng.close()
