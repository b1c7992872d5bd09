"""One multilevel level on the GPU (mcg_mlmc_localvol_level; PathEngine.mlmc_level) against the numpy restatement of
tests/test_mlmc_reference.py on the same (seed, path ids), against the local-volatility generator and mcg_path_stats, its sums
against numpy on its own statistics, the bit identities of the contract, the driver PathEngine.mlmc_local_vol against a plain
estimate and the CEV closed form, and the refusals.

Parity bounds: the statistics are compared relatively.  The device draws the same normals with its own logarithm, sine / cosine
and square root, forms the exponent with fused multiply-adds and takes its own exponentials (<= ~2 ulp each); the volatility is
continuous in the path's log-moneyness, so the difference from numpy is rounding that accumulates over the steps.  STATS_BOUND is
ten times the largest error observed on an MI355X over all surfaces and cases of this file, AG_BOUND ten times what A and G
showed against mcg_path_stats of the generator's matrix (another summation order for A; a product of mantissas and one
logarithm against a sum of log-moneyness for G), SUMS_BOUND ten times what the six sums showed against numpy's own summation of
the payoffs of the downloaded statistics, relative to sum |P_f| + sum |P_c| (their squares for the sums of squares).  None may
exceed the 1e-11 the reference itself is held to (OWN_ERROR_BOUND)."""
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from test_exotics_reference import payoff_numpy
from test_heston_reference import OWN_ERROR_BOUND, SEED64
from test_localvol_reference import CEV, DT, Q, R, S0, SURFACES, WIDE_128, Surface, cev_half_closed_form
from test_mlmc_reference import (BAD_LEVELS, CASES, EURO, MLMC_SURFACES, PARITY_BOOK, book_sums_numpy, case_T, raw_level, reference)

pytestmark = pytest.mark.gpu

# on an MI355X: statistics 9.99e-15 on the 252-step cases of "narrow" (5.8e-15 and below on the other 252-step cases, 1.4e-15 and
# below up to 14 steps); A and G against mcg_path_stats 2.44e-15; the sums 4.38e-16 (7 steps x 257 paths of "skew-term")
STATS_OBSERVED, AG_OBSERVED, SUMS_OBSERVED = 9.99e-15, 2.44e-15, 4.38e-16
STATS_BOUND = min(10.0 * STATS_OBSERVED, OWN_ERROR_BOUND)
AG_BOUND = min(10.0 * AG_OBSERVED, OWN_ERROR_BOUND)
SUMS_BOUND = min(10.0 * SUMS_OBSERVED, OWN_ERROR_BOUND)
observed = {"statistics": 0.0, "A and G against path_stats": 0.0, "sums": 0.0}


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


def level(eng, name, case, book=PARITY_BOOK, surface=None, **over):
    n_fine, coarse, sf, sc, first_obs, n_paths, begin, seed = case
    kw = dict(n_fine=n_fine, n_paths=n_paths, has_coarse=coarse, stride_fine=sf, stride_coarse=sc, first_obs=first_obs, path_begin=begin,
              q=Q, return_stats=True)
    kw.update(over)
    return eng.mlmc_level(seed, S0, R, surface if surface is not None else SURFACES[name], case_T(n_fine), book, **kw)


def sums_error(sums, stats, book):
    """Largest difference of the six sums of every contract from numpy's on `stats`, relative to sum |P_f| + sum |P_c| (the sums
    of squares: to sum P_f^2 + sum P_c^2); the payoffs themselves are numpy's on the very doubles the book kernel read."""
    want = book_sums_numpy(stats, book)
    assert sums[-1] == want[-1] == stats.shape[1]
    worst = 0.0
    for c, x in enumerate(book):
        pf = payoff_numpy(stats[:5], x)
        pc = payoff_numpy(stats[5:], x) if len(stats) == 10 else np.zeros_like(pf)
        s1, s2 = float(np.abs(pf).sum() + np.abs(pc).sum()), float((pf * pf).sum() + (pc * pc).sum())
        for k in range(6):
            d, scale = abs(sums[6 * c + k] - want[6 * c + k]), (s2 if k & 1 else s1)
            assert d == 0.0 or scale > 0.0, (c, k)
            worst = max(worst, d / scale if scale > 0.0 else 0.0)
    return worst


@pytest.mark.parametrize("name", MLMC_SURFACES)
def test_parity_with_numpy(eng, name):
    for case in CASES[name]:
        n_fine, coarse, sf, sc, first_obs, n_paths, begin, seed = case
        want = reference(name, case)
        sums, got = level(eng, name, case)
        assert got.shape == want.shape == (10 if coarse else 5, n_paths)
        e = float(np.abs(got / want - 1.0).max())
        observed["statistics"] = max(observed["statistics"], e)
        assert e <= STATS_BOUND, (name, case, e)
        # every payoff decision falls as the restatement's: the cases are well conditioned (tests/test_mlmc_reference.py)
        for x in PARITY_BOOK:
            for g, w in ((got[:5], want[:5]), (got[5:], want[5:])) if coarse else ((got, want),):
                assert float(np.abs(payoff_numpy(g, x) - payoff_numpy(w, x)).max()) <= 1e-9, (name, case, x)   # (a flipped barrier: >= 0.25)
        es = sums_error(sums, got, PARITY_BOOK)
        observed["sums"] = max(observed["sums"], es)
        print(f"{name} {case}: statistics {e:.2e}, sums {es:.2e}")
        assert es <= SUMS_BOUND, (name, case, es)
        if not coarse:      # without a coarse path P_c = 0 and Y = P_f
            s = sums[:-1].reshape(-1, 6)
            assert bits(s[:, 0]) == bits(s[:, 2]) and bits(s[:, 1]) == bits(s[:, 3]) and (s[:, 4:] == 0.0).all()


@pytest.mark.parametrize("name", MLMC_SURFACES)
def test_fine_statistics_against_the_generator(eng, name):
    for case in CASES[name]:
        n_fine, coarse, sf, sc, first_obs, n_paths, begin, seed = case
        if sf != 1:
            continue
        _, got = level(eng, name, case)
        P = eng.local_vol(seed, S0, R, SURFACES[name], case_T(n_fine) / n_fine, n_fine, n_paths, path_begin=begin, q=Q)
        want = eng.path_stats(P, first_row=first_obs)
        P.free()
        for q in (0, 3, 4):
            assert bits(got[q]) == bits(want[q]), (name, case, q)
        e = float(np.abs(got[1:3] / want[1:3] - 1.0).max())
        observed["A and G against path_stats"] = max(observed["A and G against path_stats"], e)
        assert e <= AG_BOUND, (name, case, e)


def test_bit_identities(eng):
    for name in ("skew-term", "wide-128", "cev"):
        case = (14, True, 2, 1, 0, 1000, 2 ** 33 + 1, SEED64)
        sums, whole = level(eng, name, case)
        # repeated, and after other work on the ctx
        eng.gbm(5, 100.0, R, 0.3, DT, 7, 3000).free()
        level(eng, "two-nodes", (6, True, 1, 1, 1, 700, 3, 7))
        eng.local_vol(5, S0, R, SURFACES["skew-term"], DT, 9, 700).free()
        again, stats = level(eng, name, case)
        assert bits(again) == bits(sums) and bits(stats) == bits(whole), name
        # shards cut at columns 1, 256 and 511: the columns bit for bit, sums that add up
        parts, total = [], np.zeros(len(sums))
        for first, count in ((0, 1), (1, 255), (256, 255), (511, 489)):
            s, st = level(eng, name, case, n_paths=count, path_begin=case[6] + first)
            parts.append(st)
            total += s
        assert bits(np.concatenate(parts, axis=1)) == bits(whole), name
        assert total[-1] == sums[-1] == 1000.0
        # each shard's sum is a rounding of the same terms: the totals differ by at most ~n 2^-53 of the sum of the absolute terms
        for c, x in enumerate(PARITY_BOOK):
            pf, pc = payoff_numpy(whole[:5], x), payoff_numpy(whole[5:], x)
            s1, s2 = float(np.abs(pf).sum() + np.abs(pc).sum()), float((pf * pf).sum() + (pc * pc).sum())
            for k in range(6):
                assert abs(total[6 * c + k] - sums[6 * c + k]) <= 2.0 * 1000 * 2.0 ** -53 * (s2 if k & 1 else s1), (name, c, k)
        # without the statistics' download: the same sums
        assert bits(level(eng, name, case, return_stats=False)) == bits(sums)
        # a contract alone and at positions 0, 3 and 1023 of a 1024-contract book
        for x in (PARITY_BOOK[7], PARITY_BOOK[1]):
            alone, _ = level(eng, name, case, book=[x])
            for pos in (0, 3, 1023):
                book = [PARITY_BOOK[(k * 7 + pos) % len(PARITY_BOOK)] for k in range(1024)]
                book[pos] = x
                full, _ = level(eng, name, case, book=book)
                assert bits(full[6 * pos:6 * pos + 6]) == bits(alone[:6]), (name, x, pos)
                assert full[-1] == 1000.0
    # a one-slice surface and the same values given as two identical rows: the same arithmetic through the other kernel
    for surface in (CEV, SURFACES["two-nodes"], Surface([0.0], -2.0, 2.0, [WIDE_128.sigma[0]])):
        twice = Surface([0.0, 1.0], surface.x_min, surface.x_max, [surface.sigma[0], surface.sigma[0]])
        for case in CASES["cev"]:
            if case[5] > 1000:
                continue
            one = level(eng, None, case, surface=surface)
            two = level(eng, None, case, surface=twice)
            assert bits(one[0]) == bits(two[0]) and bits(one[1]) == bits(two[1]), (surface.n_x, case)


def test_driver_on_cev(eng):
    T = 1.0
    book = [EURO(100.0), (N.X_BARRIER_DOWN_OUT, False, 100.0, 85.0, 0.0)]
    res = eng.mlmc_local_vol(20261021, S0, R, CEV, T, book, eps=0.02, q=Q, l_max=8)
    price, se = res
    n_fine = res.levels[-1]["n_fine"]
    print(f"mlmc_local_vol: {len(res.levels)} levels, finest grid {n_fine} steps, converged {res.converged}, cost {res.cost:.3e} path-steps "
          f"(a plain estimator at the same std errors on {n_fine} steps: "
          f"{n_fine * max(res.levels[0]['var_y'] * math.exp(-2 * R * T) / se ** 2):.3e})")
    for lv in res.levels:
        print(f"  n_fine {lv['n_fine']:5d}  paths {lv['paths']:9d}  mean Y {lv['mean_y']}  var Y {lv['var_y']}  mean P_f {lv['mean_pf']}")
    assert res.price is price and res.std_err is se and price.shape == se.shape == res.bias_estimate.shape == (2,)
    assert [lv["n_fine"] for lv in res.levels] == [4 << l for l in range(len(res.levels))] and 3 <= len(res.levels) <= 9
    assert res.cost == sum(lv["paths"] * lv["cost"] for lv in res.levels)
    assert (se > 0.0).all() and (se <= 0.02).all()             # Giles' rule aims at eps / sqrt(2)
    # the call against the closed form
    want = cev_half_closed_form(S0, 100.0, R, Q, T, 0.2, True)
    print(f"call: {price[0]:.4f} +- {se[0]:.4f} (bias estimate {res.bias_estimate[0]:.4f}), closed form {want:.4f}")
    assert abs(price[0] - want) <= 4.0 * se[0] + res.bias_estimate[0]
    # the barrier against a plain estimate on the finest level's grid
    P = eng.local_vol(977, S0, R, CEV, T / n_fine, n_fine, 1_000_000, q=Q)
    pp, pse = eng.price_exotics(P, R, T, [book[1]], first_row=1)
    P.free()
    print(f"down-and-out put: {price[1]:.4f} +- {se[1]:.4f} (bias estimate {res.bias_estimate[1]:.4f}), plain {pp[0]:.4f} +- {pse[0]:.4f}")
    assert abs(price[1] - pp[0]) <= 4.0 * math.hypot(se[1], pse[0]) + res.bias_estimate[1]
    # the result is a function of the arguments alone
    res2 = eng.mlmc_local_vol(20261021, S0, R, CEV, T, book, eps=0.02, q=Q, l_max=8)
    assert bits(res2.price) == bits(price) and bits(res2.std_err) == bits(se) and res2.cost == res.cost and res2.converged == res.converged
    # monitoring on fixed dates, and a level cap that is reached: no error
    res3 = eng.mlmc_local_vol(5, S0, R, CEV, T, [(N.X_LOOKBACK_FLOAT, True, 0.0, 0.0, 0.0)], eps=0.05, q=Q, n0=8, n_obs=4, l_min=1, l_max=1,
                              n_pilot=2000)
    assert len(res3.levels) == 2 and res3.converged in (True, False) and math.isfinite(res3.price[0])
    for bad in (dict(eps=0.0), dict(n0=3), dict(n0=8, n_obs=3), dict(l_min=3, l_max=2), dict(n_pilot=1)):
        with pytest.raises(mc.McgError):
            eng.mlmc_local_vol(5, S0, R, CEV, T, book, **dict(dict(eps=0.05), **bad))


def test_refusals(eng):
    rc, msg = raw_level(ctx=eng._ctx)
    assert rc == 0, msg
    for change, message, status in BAD_LEVELS:
        rc, msg = raw_level(ctx=eng._ctx, **change)
        assert rc == status and message in msg, (change, rc, msg)
    with pytest.raises(mc.McgError, match="even n_fine"):
        eng.mlmc_level(7, S0, R, CEV, 1.0, [EURO(100.0)], 7, 100)
    # the ctx still works
    sums = eng.mlmc_level(7, S0, R, CEV, 1.0, [EURO(100.0)], 8, 100)
    assert sums[-1] == 100.0 and sums[2] > 0.0
