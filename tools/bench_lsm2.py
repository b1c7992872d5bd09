#!/usr/bin/env python3
"""Device ms of the two-regressor LSM price on ONE GPU (dev tool; the judged number comes from bench.py): mcg_price_lsm2 at
1M x 50 and 8M x 50, orders 1-3, on QE Heston paths (prices + variances), against mcg_price_lsm at the same order forced
onto its per-date route on the same price matrix -- a second context with an identity all-reduce, as the tests do, because
mcg_price_lsm2 refuses a context that holds a collective; the same seed gives it the same matrix.
HIP events around the queued launch sequence (MCG_K_LSM_SWEEP).  Every case first gets --ramp untimed calls (an idle MI355X
needs them to settle at its clock under load); the measurements then alternate in one process, medians of --reps rounds.
TB/s by the bytes the launches move per path and exercise date: 64 B for the two-regressor sweep (centre pass 16, update
pass 48), 32 B for the per-date route.  One JSON line per measurement, the ratio of the two times in the two-regressor line."""
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
ap.add_argument("--ramp", type=int, default=6, help="untimed calls of each case first")
ap.add_argument("--scale", type=float, default=1.0, help="scale the path counts")
ap.add_argument("--paths", type=int, nargs="*", default=[1_000_000, 8_000_000])
args = ap.parse_args()

steps, dt, seed, r, K = 50, 0.02, 20251031, 0.04, 100.0
H = dict(S0=100.0, r=r, v0=0.04, kappa=1.5, theta=0.04, sigma_v=0.9, rho=-0.7)
BYTES = {"lsm2": 64, "per-date lsm": 32}
eng, per_date = mc.PathEngine(0), mc.PathEngine(0)
per_date.set_allreduce(lambda ptr, count, stream: None)

for n in (int(p * args.scale) for p in args.paths):
    P, V = eng.heston(seed, dt=dt, n_steps=steps, n_paths=n, want_variance=True, scheme="qe", **H)
    Q = per_date.heston(seed, dt=dt, n_steps=steps, n_paths=n, scheme="qe", **H)
    cases = {}
    for order in (1, 2, 3):
        cases[("lsm2", order)] = (eng, lambda o=order: eng.price_lsm2(P, V, r, K, 1.0, dt, False, o))
        cases[("per-date lsm", order)] = (per_date, lambda o=order: per_date.price_lsm(Q, r, K, 1.0, dt, False, o))
    for _, fn in cases.values():
        for _ in range(args.ramp):
            fn()
    ms, price = {k: [] for k in cases}, {}
    for e in (eng, per_date):
        e.synchronize()
        e.timing_enable(True)
        e.timing_select([N.K_LSM_SWEEP])
    for rnd in range(max(10, args.reps)):
        for key, (e, fn) in cases.items():
            e.timing_reset()
            price[key] = fn()
            ms[key].append(e.timing_get(N.K_LSM_SWEEP)[0])
    for e in (eng, per_date):
        e.timing_enable(False)
    med = {k: statistics.median(v) for k, v in ms.items()}
    for (what, order), v in ms.items():
        line = {"what": what, "order": order, "paths": n, "dates": steps, "ms_median": round(med[(what, order)], 3),
                "ms_min": round(min(v), 3), "ms_max": round(max(v), 3), "rounds": len(v),
                "TB_per_s": round(BYTES[what] * n * steps / med[(what, order)] / 1e9, 3),
                "price": round(price[(what, order)][0], 6), "std_err": round(price[(what, order)][1], 6)}
        if what == "lsm2":
            line["ratio_to_per_date_lsm"] = round(med[(what, order)] / med[("per-date lsm", order)], 3)
        print(json.dumps(line), flush=True)
    for M in (P, V, Q):
        M.free()
eng.close()
per_date.close()
