#!/usr/bin/env python3
"""Device ms of the QE Heston generator beside the Euler one on ONE GPU (dev tool; the judged number comes from bench.py), in
one process, in the manner of tools/bench_heston.py: HIP events around the one generator launch (timing_select), 12 untimed
ramp launches of every case first, then alternating rounds, medians of --reps rounds.
  * per step: QE and Euler at 10M x 252, prices only and with the variance matrix, on the "feller" set (no lane ever takes
    the exponential branch) and on the Feller-violating set (lanes of one wave disagree, stream-3 blocks are drawn: the
    kernel's worst case) -- ms, Mpaths/s, the ratio to Euler in the same run, the share of mcg_probe_write_ceiling;
  * the point of the scheme: QE at 10M x 8 over T = 1 against Euler at 10M x 252 on the Feller-violating set, each one's time
    beside its distance from the closed form, in std errors, on the K = 110 call.
Prints ONE JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # the parameter sets and the closed form have one home
import montecarlooptionspricer_amd as mc  # noqa: E402
from montecarlooptionspricer_amd import _native as N  # noqa: E402
from test_heston_reference import FELLER_VIOLATING, PARAMS, R, S0, STAT_SEED, heston_closed_form  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11, help="timed rounds (>= 10)")
ap.add_argument("--ramp", type=int, default=12, help="untimed launches of each case first")
ap.add_argument("--scale", type=float, default=1.0, help="scale the path count")
args = ap.parse_args()

n, seed = int(10_000_000 * args.scale), 20251031
SETS = {"feller": PARAMS["feller"], "feller-violating": FELLER_VIOLATING}
K, T = 110.0, 1.0
eng = mc.PathEngine(0)


def run(p, scheme, steps, want_variance, seed=seed, price=False):
    got = eng.heston(seed, S0, R, dt=T / steps, n_steps=steps, n_paths=n, want_variance=want_variance, scheme=scheme, **p)
    out = eng.price_european(got, K, R, T, True) if price else None
    for M in (got if want_variance else (got,)):
        M.free()
    return out


# name -> (launch, steps, matrices)
cases = {}
for sname, p in SETS.items():
    for scheme in ("euler", "qe"):
        for want_variance in (False, True):
            cases[(sname, scheme, 252, want_variance)] = (lambda p=p, s=scheme, w=want_variance: run(p, s, 252, w), 252, 1 + want_variance)
cases[("feller-violating", "qe", 8, False)] = (lambda: run(FELLER_VIOLATING, "qe", 8, False), 8, 1)

for fn, _, _ in cases.values():
    for _ in range(args.ramp):
        fn()
eng.synchronize()
eng.timing_enable(True)
eng.timing_select([N.K_HESTON])
ms = {k: [] for k in cases}
for rnd in range(max(10, args.reps)):
    for name, (fn, _, _) in cases.items():
        eng.timing_reset()
        fn()
        ms[name].append(eng.timing_get(N.K_HESTON)[0])
eng.timing_enable(False)
ceiling_gbs, ceiling_ms = eng.probe_write_ceiling(n, 252, 5)
med = {k: statistics.median(v) for k, v in ms.items()}

rows = []
for (sname, scheme, steps, want_variance), (_, _, matrices) in cases.items():
    m = med[(sname, scheme, steps, want_variance)]
    gbs = 8.0 * n * (steps + 1) * matrices / m / 1e6
    row = {"set": sname, "scheme": scheme, "steps": steps, "matrices": matrices, "ms_median": round(m, 3),
           "ms_min": round(min(ms[(sname, scheme, steps, want_variance)]), 3),
           "ms_max": round(max(ms[(sname, scheme, steps, want_variance)]), 3), "Mpaths_per_s": round(n / m / 1e3, 1),
           "ns_per_path_step": round(m * 1e6 / (n * steps), 4), "GB_per_s_written": round(gbs, 1)}
    if steps == 252:
        row["ratio_to_euler_time"] = round(m / med[(sname, "euler", 252, want_variance)], 3)
        row["share_of_write_ceiling"] = round(gbs / ceiling_gbs, 3)
    rows.append(row)

# the point: the same contract, priced from eight steps and from 252
want = heston_closed_form(S0, K, R, T, is_call=True, **FELLER_VIOLATING)
point = []
for scheme, steps in (("euler", 252), ("qe", 8), ("euler", 8)):
    price, se = run(FELLER_VIOLATING, scheme, steps, False, seed=STAT_SEED, price=True)
    key = ("feller-violating", scheme, steps, False)
    point.append({"scheme": scheme, "steps": steps, "ms_median": round(med[key], 3) if key in med else None, "price": round(price, 5),
                  "std_error": round(se, 5), "closed_form": round(want, 5), "std_errors_from_closed_form": round(abs(price - want) / se, 2)})
print(json.dumps({"what": "heston qe against euler", "paths": n, "rounds": len(next(iter(ms.values()))), "generators": rows,
                  "K110_call_T1_feller_violating": point,
                  "write_ceiling": {"GB_per_s": round(ceiling_gbs, 1), "ms_per_launch": round(ceiling_ms, 3)}}), flush=True)
eng.close()
