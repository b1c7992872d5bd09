#!/usr/bin/env python3
"""Device ms of the Greeks of the exotics book on ONE GPU (dev tool; the judged number comes from bench.py), on the 10M x 252
GBM matrix of bench.py's C2 arguments, for a book of 1 and of 64 contracts:
  * price_exotics (the yardstick, unchanged): k_path_stats + book + reduction;
  * greeks_exotics with sigma > 0: k_path_tangent_stats<LOGS> (one fp64 logarithm per element) + Greeks book + reduction;
  * greeks_exotics with sigma = 0: k_path_tangent_stats without the logarithms -- the stream of k_path_stats with J and the two
    row indices on top;
  * path_stats and path_tangent_stats (with and without the logarithms) alone, download excluded: the two streaming kernels.
HIP events around every launch (timing_select of K_EXOTIC); the measurements alternate in one process on one matrix; medians of
--reps rounds after a ramp.  TB/s = 8 B x paths x rows read over the time of the whole call.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlooptionspricer_amd as mc  # noqa: E402
from montecarlooptionspricer_amd import _native as N  # noqa: E402
from tools.bench_common import DT, HBM_PEAK_GBS, SEED  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11, help="timed rounds")
ap.add_argument("--ramp", type=int, default=3, help="untimed rounds first")
ap.add_argument("--scale", type=float, default=1.0, help="scale the path count")
args = ap.parse_args()

S0, R, SIGMA, T = 100.0, 0.04, 0.2, 1.0
n, steps = int(10_000_000 * args.scale), 252
eng = mc.PathEngine(0)
P = eng.gbm(SEED, S0, R, SIGMA, DT, steps, n, payoff=(100.0, True))
eng.timing_enable(True)


def book(count):
    """Kinds in turn, geometric ones included; barriers and strikes spread around the money (tools/bench_exotics.py's)."""
    return [mc.exotic(i % 10, (i // 10) % 2 == 0, 80.0 + 40.0 * i / count, (110.0 if i % 10 in (6, 7) else 90.0) + 10.0 * i / count, 1.0)
            for i in range(count)]


def device_ms(fn):
    eng.timing_select([N.K_EXOTIC])
    eng.timing_reset()
    fn()
    return eng.timing_get(N.K_EXOTIC)[0]


B1, B64 = book(1), book(64)
# rows of the matrix a call reads: the monitoring rows; with the logarithms row 0 once more for Q; the Greeks book rows 0 and 1
cases = {
    "path_stats (k_path_stats)": (lambda: eng.path_stats(P), steps),
    "path_tangent_stats, with_logs=False": (lambda: eng.path_tangent_stats(P, with_logs=False), steps),
    "path_tangent_stats, with_logs=True": (lambda: eng.path_tangent_stats(P), steps + 1),
    "price_exotics, 1 contract": (lambda: eng.price_exotics(P, R, T, B1), steps),
    "greeks_exotics, 1 contract, sigma = 0": (lambda: eng.greeks_exotics(P, R, T, B1), steps + 2),
    "greeks_exotics, 1 contract, sigma > 0": (lambda: eng.greeks_exotics(P, R, T, B1, sigma=SIGMA), steps + 3),
    "price_exotics, 64 contracts": (lambda: eng.price_exotics(P, R, T, B64), steps),
    "greeks_exotics, 64 contracts, sigma = 0": (lambda: eng.greeks_exotics(P, R, T, B64), steps + 2),
    "greeks_exotics, 64 contracts, sigma > 0": (lambda: eng.greeks_exotics(P, R, T, B64, sigma=SIGMA), steps + 3),
}
ms = {k: [] for k in cases}
for rnd in range(args.ramp + args.reps):
    for name, (fn, _) in cases.items():
        t = device_ms(fn)
        if rnd >= args.ramp:
            ms[name].append(t)
med = {k: statistics.median(v) for k, v in ms.items()}
for name, (_, rows) in cases.items():
    tbs = 8.0 * n * rows / med[name] / 1e9
    print(json.dumps({"what": name, "paths": n, "rows_read": rows, "ms_median": round(med[name], 3), "ms_min": round(min(ms[name]), 3),
                      "ms_max": round(max(ms[name]), 3), "rounds": len(ms[name]), "matrix_TB_per_s": round(tbs, 3),
                      "share_of_8TBps_peak": round(1e3 * tbs / HBM_PEAK_GBS, 3)}), flush=True)
print(json.dumps({"what": "ratios within this run",
                  "tangent_stats_no_logs / path_stats": round(med["path_tangent_stats, with_logs=False"] / med["path_stats (k_path_stats)"], 3),
                  "tangent_stats_logs / path_stats": round(med["path_tangent_stats, with_logs=True"] / med["path_stats (k_path_stats)"], 3),
                  "greeks_1_sigma0 / price_1": round(med["greeks_exotics, 1 contract, sigma = 0"] / med["price_exotics, 1 contract"], 3),
                  "greeks_1_sigma / price_1": round(med["greeks_exotics, 1 contract, sigma > 0"] / med["price_exotics, 1 contract"], 3),
                  "greeks_64_sigma0 / price_64": round(med["greeks_exotics, 64 contracts, sigma = 0"] / med["price_exotics, 64 contracts"], 3),
                  "greeks_64_sigma / price_64": round(med["greeks_exotics, 64 contracts, sigma > 0"] / med["price_exotics, 64 contracts"], 3)}),
      flush=True)
P.free()
eng.close()
