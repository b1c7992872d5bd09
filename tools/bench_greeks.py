#!/usr/bin/env python3
"""ms per call of the Greeks entry points on ONE GPU (dev tool; the judged number comes from bench.py):
  * greeks_lsm against price_lsm at C3's arguments (1M x 50, order 2, put): the default price route (one launch), the
    per-date price route (forced on a second engine through an identity set_allreduce: one process, nothing to sum),
    and greeks_lsm (always the per-date route, with the K-tangent: ~48 instead of ~32 B per path and date);
  * greeks_european against price_european at 10M x 252 (reads rows 0 and 252 only).
One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlooptionspricer_amd as mc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--scale", type=float, default=1.0, help="scale path counts")
args = ap.parse_args()


def timed(eng, fn):
    fn()
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        res = fn()
    eng.synchronize()
    return (time.perf_counter() - t0) / args.reps * 1e3, res


def emit(name, ms, res, base_ms=None):
    out = {"what": name, "ms_per_call": round(ms, 3), "result": res}
    if base_ms:
        out["x_per_date_price"] = round(ms / base_ms, 2)
    print(json.dumps(out), flush=True)


eng = mc.PathEngine(0)
per_date = mc.PathEngine(0)
per_date.set_allreduce(lambda ptr, count, stream: None)  # identity: forces the per-date route on one GPU

n3 = int(1_000_000 * args.scale)
P = eng.gbm(20251031, 100.0, 0.04, 0.2, 0.02, 50, n3)
Q = per_date.gbm(20251031, 100.0, 0.04, 0.2, 0.02, 50, n3)
lsm = (0.04, 100.0, 1.0, 0.02, False, 2)
ms_default, r_default = timed(eng, lambda: eng.price_lsm(P, *lsm))
ms_dates, r_dates = timed(per_date, lambda: per_date.price_lsm(Q, *lsm))
ms_greeks, g = timed(eng, lambda: eng.greeks_lsm(P, *lsm))
emit(f"C3 price_lsm, default route ({n3} x 50, order 2, put)", ms_default, r_default)
emit("C3 price_lsm, per-date route", ms_dates, r_dates)
emit("C3 greeks_lsm (per-date route + K-tangent)", ms_greeks,
     {k: g[k] for k in ("price", "delta", "dual_delta", "price_se", "delta_se", "dual_delta_se")}, ms_dates)
P.free()
Q.free()

n2 = int(10_000_000 * args.scale)
E = eng.gbm(20251031, 100.0, 0.04, 0.2, 1.0 / 252.0, 252, n2)
ms_price, r_price = timed(eng, lambda: eng.price_european(E, 100.0, 0.04, 1.0, True))
ms_eg, ge = timed(eng, lambda: eng.greeks_european(E, 100.0, 0.04, 1.0, True, sigma=0.2))
emit(f"C2 price_european ({n2} x 252, call)", ms_price, r_price)
emit("C2 greeks_european", ms_eg, {k: ge[k] for k in ("price", "delta", "gamma", "vega", "rho", "dual_delta")})
E.free()
per_date.close()
eng.close()
