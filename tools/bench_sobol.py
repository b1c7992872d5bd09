#!/usr/bin/env python3
"""Device ms of the Sobol' generators on ONE GPU (dev tool; the judged number comes from bench.py), in one process, in the manner
of tools/bench_localvol.py: HIP events around the launches (timing_select), 12 untimed ramp launches of every case first, then
alternating rounds, medians of --reps rounds.  At 10M x 252, matrix scramble + shift + bridge:
  gbm_sobol         against  gbm         (mcg_paths_gbm)
  local_vol_sobol   against  local_vol   (mcg_paths_localvol), the CEV surface (beta = 1/2, 64 nodes, no time axis)
The uploads that precede a launch on the stream (direction numbers, bridge program, table) lie outside the events.
With --asm FILE (the device assembly of csrc/kernels_sobol.hip: `make asmcheck` leaves build/asm/kernels_sobol.hip.s) it adds,
per kernel, from the code object's metadata and the disassembly: VGPRs, LDS, private segment, workgroups per CU, and the VALU
instructions of the main loop per 8 path-steps (the loop body as it stands, both branches of Phi^-1 and all four groups of
direction numbers counted; one pass of the loop is one dimension of two paths).  --asm-only skips the GPU.  Prints ONE JSON line."""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11, help="timed rounds (>= 10)")
ap.add_argument("--ramp", type=int, default=12, help="untimed launches of each case first")
ap.add_argument("--scale", type=float, default=1.0, help="scale the path count")
ap.add_argument("--asm", default=None, help="device assembly of kernels_sobol.hip")
ap.add_argument("--asm-only", action="store_true")
args = ap.parse_args()


def disassembly(path):
    """{kernel: {...}} of the k_sobol_paths instances in an assembly file."""
    text = open(path).read()
    meta = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or "k_sobol_paths" not in name.group(1):
            continue
        get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))  # noqa: E731
        meta[name.group(1)] = {"vgprs": get("vgpr_count"), "lds_bytes": get("group_segment_fixed_size"),
                               "private_segment_bytes": get("private_segment_fixed_size")}
    out = {}
    for name, m in meta.items():
        body = re.split(r"^" + re.escape(name) + r":", text, 1, flags=re.M)[1].split(".Lfunc_end", 1)[0].splitlines()
        # hipcc annotates every block of a loop with its header; the main loop is the one of depth 1
        valu, inside = 0, False
        for line in body:
            if re.match(r"\.LBB\d+_\d+:", line):
                inside = "Loop Header: Depth=1" in line or "in Loop: Header=" in line
            elif inside and re.match(r"\s+v_", line):
                valu += 1
        m2 = re.match(r"_ZN3mcg13k_sobol_pathsILb(\d)ELi(\d)ELb(\d)EEE", name)
        short = "payoff" * int(m2.group(1)) + ("gbm", "lv_one_slice", "lv_surface")[int(m2.group(2))] + ("", "_bridge")[int(m2.group(3))] if m2 else name
        waves = min(8, 512 // (8 * ((m["vgprs"] + 7) // 8)))
        by_lds = 163840 // m["lds_bytes"] if m["lds_bytes"] else 8
        out[short] = dict(m, workgroups_per_cu=min(waves, by_lds, 8), main_loop_valu_per_8_path_steps=4 * valu)
    return out


out = {"what": "sobol generators against their philox namesakes"}
if args.asm:
    out["kernels"] = disassembly(args.asm)
if not args.asm_only:
    import montecarlooptionspricer_amd as mc  # noqa: E402
    from montecarlooptionspricer_amd import _native as N  # noqa: E402
    seed, steps, T, r, q, S0 = 20251031, 252, 1.0, 0.04, 0.01, 100.0
    n = int(10_000_000 * args.scale)
    cev = mc.LocalVolSurface.cev(0.2, 0.5, -1.5, 1.5, 64)
    sobol = mc.Sobol(seed, 0, "lms", True)
    eng = mc.PathEngine(0)
    cases = {"gbm_sobol": (N.K_SOBOL, "gbm", lambda: eng.gbm_sobol(sobol, S0, r, 0.2, T / steps, steps, n).free()),
             "gbm": (N.K_GBM, "gbm", lambda: eng.gbm(seed, S0, r, 0.2, T / steps, steps, n).free()),
             "local_vol_sobol": (N.K_SOBOL, "local_vol", lambda: eng.local_vol_sobol(sobol, S0, r, cev, T / steps, steps, n, q=q).free()),
             "local_vol": (N.K_LOCALVOL, "local_vol", lambda: eng.local_vol(seed, S0, r, cev, T / steps, steps, n, q=q).free())}
    for _, _, fn in cases.values():
        for _ in range(args.ramp):
            fn()
    eng.synchronize()
    eng.timing_enable(True)
    eng.timing_select([N.K_SOBOL, N.K_LOCALVOL, N.K_GBM])
    ms = {k: [] for k in cases}
    for rnd in range(max(10, args.reps)):
        for name, (kernel, _, fn) in cases.items():
            eng.timing_reset()
            fn()
            ms[name].append(eng.timing_get(kernel)[0])
    eng.timing_enable(False)
    med = {k: statistics.median(v) for k, v in ms.items()}
    out.update(paths=n, steps=steps, rounds=max(10, args.reps))
    for k, v in ms.items():
        out[k] = {"ms_median": round(med[k], 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3),
                  "Mpaths_per_s": round(n / med[k] / 1e3, 1), "TB_per_s_written": round(8 * n * (steps + 1) / med[k] / 1e9, 3),
                  "over_philox_namesake": round(med[k] / med[cases[k][1]], 3)}
    eng.close()
print(json.dumps(out), flush=True)
