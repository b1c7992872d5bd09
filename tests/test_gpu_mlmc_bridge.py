"""One multilevel level with the Milstein step and the Brownian-bridge coupling on the GPU (mcg_mlmc_localvol_level_ex;
PathEngine.mlmc_level(scheme=, bridge=)) against the numpy restatement of tests/test_mlmc_bridge_reference.py on the same (seed,
path ids): the statistics, the survival probabilities and the sums; the exact values and the bit identities of the contract; the
driver PathEngine.mlmc_local_vol(scheme="milstein", bridge=True) against a plain continuous-barrier estimate; the refusals.

The cases (tests/test_mlmc_bridge_reference.py: CASES): the surfaces cev (one slice), skew-term (staged slices), narrow and
two-nodes (both clamps: the Milstein slope is zero outside the grid) and wide-128; with a coarse path n_fine in {2 .. 14},
without one in {1, 2, 3, 4, 5, 7}, and 252 x 1300; 1, 257, 513 and 1000 paths; path_begin 0, 12345 and 2^33 + 1; both schemes;
books on 1, 2 and 4 levels, up and down mixed, a duplicated level, the EURO idiom, in and out contracts, rebates.

Parity bounds: the statistics and the sums are compared relatively, as tests/test_gpu_mlmc.py does; P absolutely, since P lies in
[0, 1].  The device forms the exponent of a factor from its own X (rounding that accumulates over the steps, magnified by 2 |d| /
w, a few hundred on a daily step) and takes its own exponential (<= ~2 ulp).  Each bound is ten times the largest error observed
on an MI355X over all cases of this file, and none may exceed the 1e-11 the reference itself is held to (OWN_ERROR_BOUND)."""
import ctypes as C
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from test_heston_reference import OWN_ERROR_BOUND, SEED64
from test_localvol_reference import CEV, Q, R, S0, SURFACES
from test_mlmc_bridge_reference import (BAD_BRIDGES, BOOKS, BRIDGE_SURFACES, CASES, DOC_ABOVE, DOP, LOOK, UIC, UOP, book_sums_bridge_numpy,
                                        bridge_plan_python, raw_level_ex, reference, samples_numpy)
from test_mlmc_reference import EURO, case_T

pytestmark = pytest.mark.gpu

# on an MI355X: statistics 1.09e-14 on the 252-step case of "narrow" (5.8e-15 and below on the other 252-step cases, 1.2e-15 and
# below up to 14 steps); P 2.34e-14 on the 252-step case of "skew-term" (2.0e-14 to 2.1e-14 on the other 252-step cases, 5.5e-15
# and below up to 14 steps); the sums 2.87e-16 (7 steps x 513 paths of "two-nodes")
STATS_OBSERVED, SURV_OBSERVED, SUMS_OBSERVED = 1.09e-14, 2.34e-14, 2.87e-16
STATS_BOUND = min(10.0 * STATS_OBSERVED, OWN_ERROR_BOUND)
SURV_BOUND = min(10.0 * SURV_OBSERVED, OWN_ERROR_BOUND)
SUMS_BOUND = min(10.0 * SUMS_OBSERVED, OWN_ERROR_BOUND)
observed = {"statistics": 0.0, "P": 0.0, "sums": 0.0}
SCHEMES = ("euler", "milstein")


@pytest.fixture(scope="module")
def eng():
    with mc.PathEngine(0) as e:
        yield e


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest errors in this run: " + ", ".join(f"{k} {v:.2e}" for k, v in observed.items()))


def bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


def level(eng, name, case, book=None, surface=None, bridge=True, **over):
    """(sums, stats10, surv) of a case of tests/test_mlmc_bridge_reference.py"""
    n_fine, coarse, n_paths, begin, seed, scheme, book_name = case
    kw = dict(n_fine=n_fine, n_paths=n_paths, has_coarse=coarse, path_begin=begin, q=Q, return_stats=True, return_survival=True,
              scheme=SCHEMES[scheme], bridge=bridge)
    kw.update(over)
    return eng.mlmc_level(seed, S0, R, surface if surface is not None else SURFACES[name], case_T(n_fine), book if book is not None else BOOKS[book_name],
                          **kw)


def sums_error(sums, stats, surv, book, bridge=True):
    """Largest difference of the six sums of every contract from numpy's on the downloaded statistics and probabilities, relative
    to sum |P_f| + sum |P_c| (the sums of squares: to sum P_f^2 + sum P_c^2)."""
    want = book_sums_bridge_numpy(stats, surv, book, bridge)
    assert sums[-1] == want[-1] == stats.shape[1]
    pf, pc = samples_numpy(stats, surv, book, bridge)
    worst = 0.0
    for c in range(len(book)):
        s1, s2 = float(np.abs(pf[c]).sum() + np.abs(pc[c]).sum()), float((pf[c] * pf[c]).sum() + (pc[c] * pc[c]).sum())
        for k in range(6):
            d, scale = abs(sums[6 * c + k] - want[6 * c + k]), (s2 if k & 1 else s1)
            assert d == 0.0 or scale > 0.0, (c, k)
            worst = max(worst, d / scale if scale > 0.0 else 0.0)
    return worst


@pytest.mark.parametrize("name", BRIDGE_SURFACES)
def test_parity_with_numpy(eng, name):
    for case in CASES[name]:
        n_fine, coarse, n_paths, begin, seed, scheme, book_name = case
        book = BOOKS[book_name]
        n_levels = len(bridge_plan_python(book)[0])
        want_st, want_sv, _ = reference(name, case)
        sums, st, sv = level(eng, name, case)
        assert st.shape == want_st.shape == (10 if coarse else 5, n_paths) and sv.shape == want_sv.shape == ((2 if coarse else 1) * n_levels, n_paths)
        e = float(np.abs(st / want_st - 1.0).max())
        ep = float(np.abs(sv - want_sv).max())
        # every safe decision falls as the restatement's: the cases are well conditioned (tests/test_mlmc_bridge_reference.py)
        assert ((sv == 0.0) == (want_sv == 0.0)).all() and ((sv >= 0.0) & (sv <= 1.0)).all(), (name, case)
        es = sums_error(sums, st, sv, book)
        for key, v in (("statistics", e), ("P", ep), ("sums", es)):
            observed[key] = max(observed[key], v)
        print(f"{name} {case}: statistics {e:.2e}, P {ep:.2e}, sums {es:.2e}")
        assert e <= STATS_BOUND and ep <= SURV_BOUND and es <= SUMS_BOUND, (name, case, e, ep, es)
        if not coarse:      # without a coarse path P_c = 0 and Y = P_f
            s = sums[:-1].reshape(-1, 6)
            assert bits(s[:, 0]) == bits(s[:, 2]) and bits(s[:, 1]) == bits(s[:, 3]) and (s[:, 4:] == 0.0).all()


def test_exact_values(eng):
    far = (N.X_BARRIER_DOWN_OUT, True, 100.37, 1.0, 3.0)                    # never within reach: every factor is 1.0
    for name in ("cev", "skew-term"):
        for case in ((14, True, 1000, 3, 7, 1, None), (7, False, 513, 2 ** 33 + 1, SEED64, 0, None), (252, True, 1300, 777, SEED64, 1, None)):
            book = [EURO(100.37), far, DOC_ABOVE, (N.X_BARRIER_DOWN_IN, True, 100.37, 1.0, 3.0)]
            sums, st, sv = level(eng, name, case, book=book)
            rows = 2 if case[1] else 1
            assert sv.shape == (2 * rows, case[2])
            assert (sv[0::2] == 1.0).all(), (name, case)                     # B = 1: P == 1.0 on every path and grid
            assert (sv[1::2] == 0.0).all(), (name, case)                     # a down barrier above S0: row 0 is unsafe
            s = sums[:-1].reshape(-1, 6)
            assert bits(s[1]) == bits(s[0]), (name, case)                    # the barrier contract is the EURO contract bit for bit
            assert (s[2] == 0.0).all()                                       # knocked out at once, no rebate
            assert s[3, 0] == (0.0 if case[1] else 3.0 * case[2]) and s[3, 2] == 3.0 * case[2]   # never knocked in: the rebate


def old_level(eng, name, case, book):
    """mcg_mlmc_localvol_level itself, through ctypes: (sums, stats10)"""
    n_fine, coarse, n_paths, begin, seed, _, _ = case
    surface = SURFACES[name]
    dp = C.POINTER(C.c_double)
    arr = mc.engine.make_book(book)
    lv = N.MlmcLevel(seed & 0xFFFFFFFFFFFFFFFF, n_fine, int(coarse), 1, 1, 1, begin, n_paths)
    sums, stats = np.empty(6 * len(arr) + 1), np.empty((10 if coarse else 5, n_paths))
    rc = eng._L.mcg_mlmc_localvol_level(eng._ctx, S0, R, Q, surface.times.ctypes.data_as(dp), surface.n_t, surface.x_min, surface.x_max, surface.n_x,
                                        surface.sigma.ctypes.data_as(dp), case_T(n_fine), C.byref(lv), arr, len(arr), sums.ctypes.data_as(dp),
                                        stats.ctypes.data_as(dp))
    assert rc == 0, eng._L.mcg_last_error()
    return sums, stats


def test_bit_identities(eng):
    four = BOOKS["four-levels"]
    for name in ("skew-term", "wide-128", "cev"):
        for scheme in (0, 1):
            case = (14, True, 1000, 2 ** 33 + 1, SEED64, scheme, "four-levels")
            sums, whole, surv = level(eng, name, case)
            # repeated, and after other work on the ctx
            level(eng, "two-nodes", (6, True, 700, 3, 7, 1 - scheme, "two-levels"))
            eng.local_vol(5, S0, R, SURFACES["skew-term"], 1.0 / 252.0, 9, 700).free()
            again = level(eng, name, case)
            assert bits(again[0]) == bits(sums) and bits(again[1]) == bits(whole) and bits(again[2]) == bits(surv), (name, scheme)
            # shards cut at columns 1, 256 and 511: the columns bit for bit, sums that add up
            parts, probs, total = [], [], np.zeros(len(sums))
            for first, count in ((0, 1), (1, 255), (256, 255), (511, 489)):
                s, st, sv = level(eng, name, case, n_paths=count, path_begin=case[3] + first)
                parts.append(st), probs.append(sv)
                total += s
            assert bits(np.concatenate(parts, axis=1)) == bits(whole) and bits(np.concatenate(probs, axis=1)) == bits(surv), (name, scheme)
            assert total[-1] == sums[-1] == 1000.0
            pf, pc = samples_numpy(whole, surv, four, True)
            for c in range(len(four)):
                s1, s2 = float(np.abs(pf[c]).sum() + np.abs(pc[c]).sum()), float((pf[c] * pf[c]).sum() + (pc[c] * pc[c]).sum())
                for k in range(6):
                    assert abs(total[6 * c + k] - sums[6 * c + k]) <= 2.0 * 1000 * 2.0 ** -53 * (s2 if k & 1 else s1), (name, c, k)
            # without the downloads: the same sums
            assert bits(level(eng, name, case, return_stats=False, return_survival=False)) == bits(sums)
            # a level held alone or among four; a contract alone and at positions 0, 3 and 1023 of a 1024-contract book on 4 levels
            levels = bridge_plan_python(four)[0]
            for x in (DOP, UIC, UOP, DOC_ABOVE, LOOK):
                alone = level(eng, name, case, book=[x])
                if x is not LOOK:
                    l = levels.index((x[3], x[0] in (N.X_BARRIER_UP_OUT, N.X_BARRIER_UP_IN)))
                    assert bits(alone[2]) == bits(surv[[l, 4 + l]]), (name, scheme, x)
                assert bits(alone[1]) == bits(whole)
                for pos in (0, 3, 1023):
                    book = [four[(k * 5 + pos) % len(four)] for k in range(1024)]
                    book[pos] = x
                    full = level(eng, name, case, book=book, return_stats=False, return_survival=False)
                    assert bits(full[6 * pos:6 * pos + 6]) == bits(alone[0][:6]), (name, scheme, x, pos)
                    assert full[-1] == 1000.0
        # scheme 0 without the bridge is the old entry point: sums and statistics bit for bit
        for case in CASES[name]:
            if case[2] > 1000:
                continue
            book = BOOKS[case[6]] + [LOOK, (N.X_ASIAN_ARITH_FIXED, True, 99.67, 0.0, 0.0)]
            want = old_level(eng, name, case, book)
            got = level(eng, name, case, book=book, scheme="euler", bridge=False)
            assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1]) and got[2].shape == (0, case[2]), (name, case)
            # the bridge changes no statistic and no contract of another kind; the Milstein statistics do not depend on it
            both = level(eng, name, case, book=book, scheme="euler", bridge=True)
            assert bits(both[1]) == bits(want[1])
            k = 6 * len(BOOKS[case[6]])
            assert bits(both[0][k:]) == bits(want[0][k:])
            m0, m1 = level(eng, name, case, book=book, scheme="milstein", bridge=False), level(eng, name, case, book=book, scheme="milstein", bridge=True)
            assert bits(m0[1]) == bits(m1[1]) and bits(m0[0][k:]) == bits(m1[0][k:])
    # on a flat surface the Milstein path is the log-Euler path
    flat = SURFACES["flat"]
    for case in CASES["cev"]:
        e = level(eng, None, case, surface=flat, scheme="euler")
        m = level(eng, None, case, surface=flat, scheme="milstein")
        assert all(bits(a) == bits(b) for a, b in zip(e, m)), case


def test_driver_on_cev(eng):
    T = 1.0
    book = [(N.X_BARRIER_DOWN_OUT, False, 100.0, 85.0, 0.0)]
    res = eng.mlmc_local_vol(20261021, S0, R, CEV, T, book, eps=0.01, q=Q, l_max=8, scheme="milstein", bridge=True)
    price, se = res
    n_fine = res.levels[-1]["n_fine"]
    for lv in res.levels:
        print(f"  n_fine {lv['n_fine']:5d}  paths {lv['paths']:9d}  mean Y {lv['mean_y']}  var Y {lv['var_y']}  mean P_f {lv['mean_pf']}")
    assert [lv["n_fine"] for lv in res.levels] == [4 << l for l in range(len(res.levels))] and 3 <= len(res.levels) <= 9
    assert res.cost == sum(lv["paths"] * lv["cost"] for lv in res.levels) and se[0] > 0.0
    # the plain bridge estimator: a level without a coarse path on the finest grid the run reached, on other seeds
    n_plain = 1_000_000
    s = eng.mlmc_level(977, S0, R, CEV, T, book, n_fine, n_plain, has_coarse=False, q=Q, scheme="milstein", bridge=True)
    disc = math.exp(-R * T)
    pm = disc * s[2] / n_plain
    var = (s[3] - n_plain * (s[2] / n_plain) ** 2) / (n_plain - 1.0)
    pse = disc * math.sqrt(var / n_plain)
    z = abs(price[0] - pm) / math.hypot(se[0], pse)
    plain_cost = n_fine * var * disc * disc / se[0] ** 2                  # path-steps of the plain estimator at the same std error
    print(f"mlmc_local_vol(milstein, bridge): {len(res.levels)} levels, finest grid {n_fine} steps, converged {res.converged}: "
          f"{price[0]:.4f} +- {se[0]:.4f}; plain bridge estimator {pm:.4f} +- {pse:.4f}: {z:.2f} combined std errors; "
          f"cost {res.cost:.3e} path-steps against {plain_cost:.3e}: {plain_cost / res.cost:.2f}x fewer")
    assert z <= 4.0, (price, se, pm, pse)
    assert res.cost < plain_cost
    # the result is a function of the arguments alone, and the defaults are the driver of tests/test_gpu_mlmc.py
    res2 = eng.mlmc_local_vol(20261021, S0, R, CEV, T, book, eps=0.01, q=Q, l_max=8, scheme="milstein", bridge=True)
    assert bits(res2.price) == bits(price) and bits(res2.std_err) == bits(se) and res2.cost == res.cost
    a = eng.mlmc_local_vol(5, S0, R, CEV, T, book, eps=0.05, q=Q, n_pilot=2000, l_max=3)
    b = eng.mlmc_local_vol(5, S0, R, CEV, T, book, eps=0.05, q=Q, n_pilot=2000, l_max=3, scheme="euler", bridge=False)
    assert bits(a.price) == bits(b.price) and a.cost == b.cost
    with pytest.raises(mc.McgError, match="scheme"):
        eng.mlmc_local_vol(5, S0, R, CEV, T, book, eps=0.05, scheme="heun")


def test_refusals(eng):
    for scheme in (0, 1):
        for bridge in (0, 1):
            rc, msg = raw_level_ex(scheme, bridge, ctx=eng._ctx)
            assert rc == 0, msg
    for change, message in BAD_BRIDGES:
        rc, msg = raw_level_ex(ctx=eng._ctx, **change)
        assert rc == 1 and message in msg, (change, rc, msg)
    with pytest.raises(mc.McgError, match="more than 4"):
        eng.mlmc_level(7, S0, R, CEV, 1.0, [(N.X_BARRIER_DOWN_OUT, False, 100.0, 80.0 + k, 0.0) for k in range(5)], 8, 100, bridge=True)
    # the ctx still works
    sums, sv = eng.mlmc_level(7, S0, R, CEV, 1.0, [EURO(100.0), DOP], 8, 100, bridge=True, scheme="milstein", return_survival=True)
    assert sums[-1] == 100.0 and sums[2] > 0.0 and sv.shape == (2, 100)
