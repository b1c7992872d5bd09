#!/usr/bin/env python3
"""Device ms of the Brownian-bridge barrier pricer on ONE GPU (dev tool; the judged number comes from bench.py), on the
10M x 252 GBM matrix of bench.py's C2 arguments and on a Heston matrix of the same shape with its variance matrix:
  * path_stats and path_tangent_stats with logarithms (the natural comparison: one fp64 logarithm per element), same run;
  * barrier_survival (k_bridge_survival) with 1 and with BRIDGE_L_MAX levels, the levels near the spot (90 and 110 on
    S0 = 100, then outwards) and far from it (1e-3 S0 and 1e3 S0: every exponential skipped), on the scalar route and, on the
    Heston pair, on the matrix route;
  * whole calls: price_barriers_bridge beside price_exotics for books of 1 and 64 barrier contracts.
HIP events around every launch (timing_select of K_EXOTIC); the measurements alternate in one process; medians of --reps
rounds after a ramp.  TB/s = 8 B x paths x rows read (both matrices on the matrix route) over the device time of the call;
downloads are not inside the events.  One JSON line per measurement, then the kernels' resources from build/asm (written by
`make asmcheck`): VGPRs, LDS, the private segment size (which must be 0) and the VALU instructions of the main loop."""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import montecarlooptionspricer_amd as mc  # noqa: E402
from montecarlooptionspricer_amd import _native as N  # noqa: E402
from tools.bench_common import DT, HBM_PEAK_GBS, SEED  # noqa: E402


def kernel_resources(path=os.path.join(ROOT, "build", "asm", "kernels_barrier_bridge.hip.s")):
    """Per kernel of the assembly file: VGPRs, SGPRs, LDS and private segment bytes from the descriptor, and the VALU
    instruction count of its main loop: the innermost loop (a label up to a branch back to it, no other loop inside) that holds
    the most of them -- the unrolled row group, every exponential counted as if no wave skipped it."""
    if not os.path.exists(path):
        return None
    text = open(path).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        get = lambda k: int(re.search(r"\.amdhsa_" + k + r"\s+(\d+)", m.group(2)).group(1))  # noqa: E731
        out[m.group(1)] = {"vgprs": get("next_free_vgpr"), "sgprs": get("next_free_sgpr"), "lds_bytes": get("group_segment_fixed_size"),
                           "private_segment_bytes": get("private_segment_fixed_size")}
    for name in out:
        body = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M)
        lines = [l.split(";")[0].strip() for l in body.group(1).splitlines()] if body else []
        lines = [l for l in lines if l and not l.startswith(".") or re.match(r"\.LBB\d+_\d+:", l)]
        at = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
        loops = []
        for i, l in enumerate(lines):
            b = re.match(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)|s_branch\s+(\.LBB\d+_\d+)", l)
            target = b and (b.group(1) or b.group(2))
            if target in at and at[target] < i:
                loops.append((at[target], i))
        inner = [(a, b) for a, b in loops if not any((c, d) != (a, b) and a <= c and d <= b for c, d in loops)]
        out[name]["main_loop_valu"] = max([sum(1 for l in lines[a:b] if l.startswith("v_")) for a, b in inner], default=0)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11, help="timed rounds")
    ap.add_argument("--ramp", type=int, default=3, help="untimed rounds first")
    ap.add_argument("--scale", type=float, default=1.0, help="scale the path count")
    args = ap.parse_args()

    S0, R, SIGMA, T = 100.0, 0.04, 0.2, 1.0
    LM = mc.BRIDGE_L_MAX
    n, steps = int(10_000_000 * args.scale), 252
    eng = mc.PathEngine(0)
    P = eng.gbm(SEED, S0, R, SIGMA, DT, steps, n)
    H, V = eng.heston(SEED, S0, R, 0.04, 1.5, 0.04, 0.5, -0.7, DT, steps, n, want_variance=True, scheme="qe")
    eng.timing_enable(True)

    def near(count):
        return [(90.0 - 2.0 * (k // 2), False) if k % 2 == 0 else (110.0 + 2.0 * (k // 2), True) for k in range(count)]

    def far(count):
        return [(1e-3 * S0 / (1 + k // 2), False) if k % 2 == 0 else (1e3 * S0 * (1 + k // 2), True) for k in range(count)]

    def book(count):
        return [mc.exotic(6 + i % 4, (i // 4) % 2 == 0, 80.0 + 40.0 * i / count, (110.0 if i % 4 < 2 else 90.0) + (10.0 if i % 4 < 2 else -10.0) * i / count, 1.0)
                for i in range(count)]

    def device_ms(fn):
        eng.timing_select([N.K_EXOTIC])
        eng.timing_reset()
        fn()
        return eng.timing_get(N.K_EXOTIC)[0]

    B1, B64 = book(1), book(64)
    groups64 = -(-len({(c[3], c[0] in (6, 7)) for c in B64}) // LM)
    # rows of the matrices a call reads (the book kernels' row n_steps left aside)
    cases = {
        "path_stats (k_path_stats)": (lambda: eng.path_stats(P, 0), steps + 1),
        "path_tangent_stats, with_logs=True": (lambda: eng.path_tangent_stats(P, 0), steps + 2),
    }
    for tag, lv in (("near", near), ("far", far)):
        for count in (1, LM):
            cases[f"barrier_survival, scalar route, {count} levels {tag}"] = (lambda lv=lv, count=count: eng.barrier_survival(P, lv(count), DT, sigma=SIGMA), steps + 1)
            cases[f"barrier_survival, scalar route on the Heston matrix, {count} levels {tag}"] = (
                lambda lv=lv, count=count: eng.barrier_survival(H, lv(count), DT, sigma=SIGMA), steps + 1)
            cases[f"barrier_survival, matrix route, {count} levels {tag}"] = (lambda lv=lv, count=count: eng.barrier_survival(H, lv(count), DT, var=V), 2 * steps + 1)
    cases.update({
        "price_exotics, 1 contract": (lambda: eng.price_exotics(P, R, T, B1, first_row=0), steps + 1),
        "price_barriers_bridge, 1 contract": (lambda: eng.price_barriers_bridge(P, R, T, B1, sigma=SIGMA), steps + 1),
        "price_exotics, 64 contracts": (lambda: eng.price_exotics(P, R, T, B64, first_row=0), steps + 1),
        f"price_barriers_bridge, 64 contracts ({groups64} level groups)": (lambda: eng.price_barriers_bridge(P, R, T, B64, sigma=SIGMA), groups64 * (steps + 1)),
    })
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
    res = kernel_resources()
    if res is None:
        print(json.dumps({"what": "kernel resources", "note": "build/asm/kernels_barrier_bridge.hip.s not found: run `make asmcheck`"}))
    else:
        for name, r in sorted(res.items()):
            print(json.dumps({"what": "kernel resources", "kernel": name, **r}), flush=True)
        assert all(r["private_segment_bytes"] == 0 for r in res.values()), "a bridge kernel has a private segment"
    for M in (P, H, V):
        M.free()
    eng.close()
