"""The regression solves of the LSM sweeps on the GPU, elementwise (mcg_debug_lsm_solve: the routines of csrc/lsm_device.hpp as
the product runs them -- one workgroup per element, thread 0 solving, moments and workspace in LDS) against the 60-digit
references and on the cases of tests/test_lsm_solve_reference.py, and la_continuation at every order through mcg_lsm_apply.

Bounds.
  lsm_rcp, lsm_rsqrt        1 ulp, the header's claim.
  fast path (fn 0)          8 eps kappa on the error measure of the CPU file (the numpy restatement stays under 1 eps kappa; the
                            factor 8 is for the device's fused multiply-adds, the elimination order of its fma chains and the
                            1-ulp reciprocal and rsqrt in place of division).  Where 8 eps kappa > 1e-3 (provisional coefficients
                            of badly conditioned, untrusted dates) accuracy is not asked; at most a quarter of the cases of any
                            nb, and no trusted one.  Every decision (COUNT, CENTER, REFINE, HINT, zeros) on every case.
  tangent forms, dispatch   the same bits.
  centred solve (fn 3)      per (nb, decade of spread) ten times the restatement's recorded error, at least 64 eps, at most 2e-5.
  threshold probe (fn 3)    probe_threshold() of the CPU file: two prices a few ulp apart at nb = 16 whose second singular value
                            (4.4 eps sigma_max) lies between Eigen's threshold min(count, nb) eps = 2 eps and the 16 eps of a
                            rule that forgot the count.  Fitted error <= 2e-5, the oracle solver's bound (the restatement: 1.4e-16;
                            the wrong threshold: 0.29); fn 4 gives the same bits.
  lsm_continuation (fn 6)   2 nb eps sum |c_t| |y|^t against Horner in 60 digits.
  la_continuation           the stop histogram exact; price 1e-12, std error by se_error (tests/test_gpu_lsm_policy.py).

Observed on an MI355X: see the report this module prints at its end and DESIGN.md ("The regression solves, elementwise")."""
import ctypes as C
import functools

import mpmath as mp
import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from test_gpu_lsm_policy import YARDSTICK_BOUND, check_apply
from test_lsm_policy_reference import RULE, TERM, lsm_apply_numpy, undecided
from test_lsm_solve_reference import (C_CENTER, C_COUNT, C_HINT, C_REFINE, CENTRED_NB, COEF_STRIDE, DPS, EPS, FAST_NB, FN_CENTRED,
                                      FN_CENTRED_TAN, FN_CONTINUATION, FN_NB, FN_NB_TAN, FN_ONE, FN_RCP_RSQRT, MAX_NB, SKIP_ABOVE,
                                      as_tangent_rhs, centred_bound, centred_cases, continuation_cases, continuation_reference,
                                      fast_cases, fitted_error, poly_error, probe_threshold, rcp_rsqrt_inputs, rcp_rsqrt_reference, ulp_errors)

pytestmark = pytest.mark.gpu

report_lines = []


@pytest.fixture(scope="module")
def eng():
    with mc.PathEngine(0) as e:
        yield e


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst cases in this run:\n  " + "\n  ".join(report_lines))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def fast_inputs(nb, tangent=False):
    cs = fast_cases(nb)
    width = 4 * nb - 1 if tangent else 3 * nb - 1
    return cs, np.array([c["moments"][:width] for c in cs]), np.array([[c["min_count"], c["K_param"], 0.0] for c in cs])


def centred_inputs(nb, tangent=False):
    cs = centred_cases(nb)
    width = 4 * nb - 1 if tangent else 3 * nb - 1
    return cs, np.array([c["moments"][:width] for c in cs]), np.array([[1.0, c["K"], c["mu"]] for c in cs])


# ---- lsm_rcp, lsm_rsqrt ------------------------------------------------------------------------------------------------------------
def test_rcp_and_rsqrt_within_one_ulp(eng):
    x = rcp_rsqrt_inputs()
    y = eng.debug_lsm_solve(FN_RCP_RSQRT, 1, x)
    assert (y[:, 2:] == 0.0).all()
    want_rcp, want_rsq = rcp_rsqrt_reference(x)
    with mp.workdps(DPS):
        e_rcp, e_rsq = ulp_errors(y[:, 0], want_rcp), ulp_errors(y[:, 1], want_rsq)
    i, j = int(np.argmax(e_rcp)), int(np.argmax(e_rsq))
    line = (f"lsm_rcp {e_rcp[i]:.3f} ulp at x = {x[i]!r} ({float(x[i]).hex()}), lsm_rsqrt {e_rsq[j]:.3f} ulp at x = {x[j]!r} "
            f"({float(x[j]).hex()}); {len(x)} inputs, above 1/2 ulp: {int((e_rcp > 0.5).sum())} and {int((e_rsq > 0.5).sum())}")
    print(line)
    report_lines.append(line)
    assert e_rcp[i] <= 1.0 and e_rsq[j] <= 1.0


# ---- the fast path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", FAST_NB)
def test_fast_path_against_the_exact_solution(eng, nb):
    cs, m, p = fast_inputs(nb)
    out = eng.debug_lsm_solve(FN_NB, nb, m, p)
    assert np.isfinite(out).all() and (out[:, 20:] == 0.0).all() and (out[:, nb:MAX_NB] == 0.0).all()
    worst, worst_trusted, skipped, checked = (0.0, None), (0.0, None), 0, 0
    for c, row in zip(cs, out):
        assert row[C_COUNT] == len(c["S"]) and row[C_CENTER] == 0.0, c["id"]
        assert row[C_REFINE] == (1.0 if c["refine"] else 0.0), (c["id"], c["pivots"], c["est"])
        if c["K_param"] <= 0.0:
            assert row[C_REFINE] == 0.0, c["id"]
        if c["refine"]:
            want = c["moments"][1] / c["moments"][0]
            assert abs(row[C_HINT] - want) <= 2.0 * np.spacing(abs(want)), (c["id"], row[C_HINT], want)
        else:
            assert row[C_HINT] == 0.0 and bits(row[C_HINT]) == 0, c["id"]
        if c["zero"] or not c["ok"]:
            assert (bits(row[:MAX_NB]) == 0).all(), (c["id"], row[:MAX_NB])    # +0.0: nothing of the stand-in pivot leaks
            continue
        bound = 8.0 * EPS * c["kappa"]
        if not bound <= SKIP_ABOVE:
            assert not c["trusted"], c["id"]
            skipped += 1
            continue
        checked += 1
        e = poly_error(row[:nb], c["exact"], c["x"])
        if e / (EPS * c["kappa"]) > worst[0]:
            worst = (e / (EPS * c["kappa"]), c["id"], e, c["kappa"])
        if c["trusted"] and e > worst_trusted[0]:
            worst_trusted = (e, c["id"], c["kappa"], min(c["pivots"]))
        assert e <= bound, (c["id"], e, bound, c["kappa"], c["pivots"])
    line = (f"fast path nb {nb}: {checked} cases checked, worst {worst[0]:.3f} eps kappa at {worst[1:]}; largest error of a trusted "
            f"case {worst_trusted[0]:.2e} at {worst_trusted[1:]}; accuracy not asked (8 eps kappa > 1e-3): {skipped} of {len(cs)}")
    print(line)
    report_lines.append(line)
    assert 4 * skipped <= len(cs)


@pytest.mark.parametrize("nb", FAST_NB)
def test_tangent_and_dispatch_are_the_same_bits(eng, nb):
    cs, m4, p = fast_inputs(nb, tangent=True)
    price = eng.debug_lsm_solve(FN_NB, nb, m4[:, :3 * nb - 1], p)
    as_rhs = eng.debug_lsm_solve(FN_NB, nb, np.array([as_tangent_rhs(row, nb) for row in m4]), p)
    tan = eng.debug_lsm_solve(FN_NB_TAN, nb, m4, p)
    one = eng.debug_lsm_solve(FN_ONE, nb, m4[:, :3 * nb - 1], p)
    assert (bits(tan[:, :COEF_STRIDE]) == bits(price[:, :COEF_STRIDE])).all()
    assert (bits(tan[:, COEF_STRIDE:COEF_STRIDE + MAX_NB]) == bits(as_rhs[:, :MAX_NB])).all()
    assert (tan[:, COEF_STRIDE + MAX_NB:] == 0.0).all()
    assert (bits(one) == bits(price)).all()
    assert sum(1 for c, row in zip(cs, tan) if c["ok"] and not c["zero"] and (row[COEF_STRIDE:COEF_STRIDE + nb] != 0.0).all()) >= 5


# ---- the centred solve -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", CENTRED_NB)
def test_centred_solve_against_eigens_rule_in_exact_arithmetic(eng, nb):
    cs, m, p = centred_inputs(nb)
    out = eng.debug_lsm_solve(FN_CENTRED, nb, m, p)
    assert np.isfinite(out).all() and (out[:, 20:] == 0.0).all() and (out[:, nb:MAX_NB] == 0.0).all()
    worst, failed = (0.0, None), []
    for c, row in zip(cs, out):
        assert row[C_COUNT] == len(c["S"]) and row[C_CENTER] == c["mu"] and row[C_REFINE] == 0.0 and row[C_HINT] == 0.0, c["id"]
        e, bound = fitted_error(row, c["mu"], c), centred_bound(c["group"])
        if e / bound > worst[0]:
            worst = (e / bound, c["id"], e, bound, f"rank {c['rank']} of {min(len(c['S']), nb)}")
        if not e <= bound:
            failed.append((c["id"], e, bound, c["rank"]))
    line = f"centred solve nb {nb}: {len(cs)} cases, worst error / bound {worst[0]:.3f} at {worst[1:]}"
    print(line)
    report_lines.append(line)
    assert not failed, failed


@pytest.mark.parametrize("nb", CENTRED_NB)
def test_centred_tangent_is_the_same_bits(eng, nb):
    cs, m4, p = centred_inputs(nb, tangent=True)
    price = eng.debug_lsm_solve(FN_CENTRED, nb, m4[:, :3 * nb - 1], p)
    as_rhs = eng.debug_lsm_solve(FN_CENTRED, nb, np.array([as_tangent_rhs(row, nb) for row in m4]), p)
    tan = eng.debug_lsm_solve(FN_CENTRED_TAN, nb, m4, p)
    assert (bits(tan[:, :COEF_STRIDE]) == bits(price[:, :COEF_STRIDE])).all()
    assert (bits(tan[:, COEF_STRIDE:]) == bits(as_rhs[:, :COEF_STRIDE])).all()
    assert (tan[:, COEF_STRIDE:COEF_STRIDE + nb] != 0.0).any()


def test_threshold_probe_keeps_the_direction_eigen_keeps(eng):
    """The case that tells min(count, nb) eps sigma_max from nb eps sigma_max (tests/test_lsm_solve_reference.py:
    test_mutations_are_caught), on the device."""
    p = probe_threshold()
    nb, m4 = p["nb"], p["moments"][None, :]
    par = np.array([[1.0, p["K"], p["mu"]]])
    out = eng.debug_lsm_solve(FN_CENTRED, nb, m4[:, :3 * nb - 1], par)
    tan = eng.debug_lsm_solve(FN_CENTRED_TAN, nb, m4, par)
    as_rhs = eng.debug_lsm_solve(FN_CENTRED, nb, as_tangent_rhs(m4[0], nb)[None, :], par)
    assert np.isfinite(out).all() and out[0, C_COUNT] == 2.0 and out[0, C_CENTER] == p["mu"] and out[0, C_REFINE] == 0.0
    e = fitted_error(out[0], p["mu"], p)
    line = f"threshold probe (sigma_2 = {p['sv'][1] / EPS:.2f} eps sigma_max, two rows, nb 16): fitted error {e:.2e} (bound 2e-5)"
    print(line)
    report_lines.append(line)
    assert e <= 2e-5
    assert (bits(tan[:, :COEF_STRIDE]) == bits(out[:, :COEF_STRIDE])).all() and (bits(tan[:, COEF_STRIDE:]) == bits(as_rhs[:, :COEF_STRIDE])).all()


# ---- lsm_continuation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", FAST_NB)
def test_continuation_against_horner_in_60_digits(eng, nb):
    e = continuation_cases(nb)
    got = eng.debug_lsm_solve(FN_CONTINUATION, nb, e)
    assert (got[:, 1:] == 0.0).all()
    want, bound = continuation_reference(e, nb)
    with mp.workdps(DPS):
        err = np.array([float(abs(mp.mpf(float(g)) - w)) for g, w in zip(got[:, 0], want)])
    i = int(np.argmax(err / bound))
    line = f"lsm_continuation nb {nb}: worst error / bound {err[i] / bound[i]:.3f} (error {err[i]:.2e}, bound {bound[i]:.2e})"
    print(line)
    report_lines.append(line)
    assert (err <= bound).all()


# ---- la_continuation at every order, through the product ---------------------------------------------------------------------------------
LA_K, LA_R, LA_CENTRE, LA_Y = 100.0, 0.04, 0.01, 0.45
# c_t y^t = K beta_t (|y| / 0.45)^t for y < 0: every coefficient moves the exercise boundary (near y = -0.45) by a price unit or so
LA_COEF = [LA_K * (0.40 if t == 0 else 0.02 * (-1.0) ** t * (1.0 + 0.05 * t)) * (-1.0 / LA_Y) ** t for t in range(16)]


def la_policy(order):
    coefficients = np.zeros((2, 16))
    coefficients[0] = LA_COEF
    return mc.LsmPolicy.from_arrays(1, order, False, LA_R, LA_K, 1.0, 1.0, coefficients=coefficients, kinds=[RULE, TERM],
                                    centres=[LA_CENTRE, 0.0])


def la_boundaries(order):
    """The prices at which the continuation value of LA_COEF[0..order] crosses the put's payoff K - S, in 60 digits."""
    with mp.workdps(DPS):
        def g(S):
            y = (S / mp.mpf(LA_K) - 1) - mp.mpf(LA_CENTRE)
            v = mp.mpf(0)
            for t in range(order, -1, -1):
                v = v * y + mp.mpf(LA_COEF[t])
            return v - (mp.mpf(LA_K) - S)
        grid = [mp.mpf(40) + mp.mpf(k) / 20 for k in range(1201)]          # 40 .. 100 in steps of 0.05
        vals = [g(S) for S in grid]
        roots = []
        for a, b, va, vb in zip(grid, grid[1:], vals, vals[1:]):
            if va == 0:
                roots.append(a)
            elif va * vb < 0:
                roots.append(mp.findroot(g, (a, b), solver="illinois", tol=mp.mpf(10) ** -40))
        return [float(r) for r in roots]


@functools.lru_cache(maxsize=None)
def la_world():
    """One two-date matrix for all sixteen orders: paths on both sides of every crossing of every order's boundary, each at
    least 1e-6 K from all of them; and numpy's stop histogram and price per order."""
    roots = {order: la_boundaries(order) for order in range(16)}
    every = np.array(sorted(r for v in roots.values() for r in v))
    rs = np.random.RandomState(16)
    S0 = np.concatenate([rs.uniform(45.0, 99.9, 200), rs.uniform(100.1, 120.0, 20)] +
                        [[r - 1e-3, r - 2e-4, r + 2e-4, r + 1e-3] for r in every])
    S0 = S0[np.all(np.abs(S0[:, None] - every[None, :]) >= 1e-6 * LA_K, axis=1)]
    rows = np.stack([S0, S0 * rs.uniform(0.8, 1.1, len(S0))], axis=1)
    M = np.ascontiguousarray(rows.T)
    want = {order: lsm_apply_numpy(la_policy(order), M) for order in range(16)}
    return roots, rows, M, {order: w[2] for order, w in want.items()}, {order: w[0] for order, w in want.items()}


@pytest.mark.parametrize("order", range(16))
def test_la_continuation_at_every_order(eng, order):
    """A two-date matrix under an uploaded policy whose one exercise date carries sixteen distinct coefficients: the device must
    read exactly the first order + 1 of them.  Paths lie on both sides of every crossing of the exercise boundary (in 60
    digits) and at least 1e-6 K from it; reading any other number of coefficients gives another histogram or another price."""
    assert len(set(LA_COEF)) == 16
    roots, rows, M, hists, prices = la_world()
    policy, S0, hist = la_policy(order), rows[:, 0], hists[order]
    assert roots[order], order
    for r in roots[order]:
        assert (S0 < r).any() and (S0 > r).any() and 1e-6 * LA_K <= np.abs(S0 - r).min() <= 3e-4
    assert undecided(policy, M) == 0
    assert hist[0] >= 10 and hist[1] >= 10, hist                       # both decisions are taken
    assert all((hists[other] != hist).any() or abs(prices[other] - prices[order]) > 1e-6 * prices[order]
               for other in range(16) if other != order)
    P = eng.from_host(rows)
    check_apply(eng, policy, P, M, f"la_continuation order {order}")
    P.free()
    report_lines.append(f"la_continuation order {order}: {len(roots[order])} crossings at {np.round(roots[order], 3)}, {len(S0)} paths, "
                        f"{hist[0]} exercise at date 0; histogram exact, price within {YARDSTICK_BOUND:g}")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(eng):
    L, dp = eng._L, C.POINTER(C.c_double)
    Q = eng.gbm(7, 100.0, 0.04, 0.2, 0.02, 50, 4096)
    before = eng.price_lsm(Q, 0.04, 100.0, 1.0, 0.02, False, 2)
    m, p, out = np.ones((2, 63)), np.tile([1.0, 1.0, 0.0], (2, 1)), np.full((2, 48), 7.0)

    def call(ctx=eng._ctx, fn=FN_NB, nb=3, mom=m.ctypes.data_as(dp), n_moments=8, par=p.ctypes.data_as(dp), o=out.ctypes.data_as(dp), n=2):
        return L.mcg_debug_lsm_solve(ctx, fn, nb, mom, n_moments, par, o, n), L.mcg_last_error().decode()

    assert call()[0] == 0 and (out != 7.0).all()
    out[:] = 7.0
    bad = [dict(ctx=None), dict(mom=None), dict(par=None), dict(o=None), dict(n=-1), dict(n=2 ** 20 + 1), dict(fn=-1), dict(fn=7), dict(nb=0), dict(nb=10),
           dict(n_moments=7), dict(n_moments=11), dict(fn=FN_NB_TAN, n_moments=8), dict(fn=FN_NB_TAN, nb=10, n_moments=39),
           dict(fn=FN_ONE, nb=10, n_moments=29), dict(fn=FN_ONE, nb=0, n_moments=-1), dict(fn=FN_CENTRED, nb=17, n_moments=50),
           dict(fn=FN_CENTRED, nb=0, n_moments=-1), dict(fn=FN_CENTRED, nb=16, n_moments=63), dict(fn=FN_CENTRED_TAN, nb=17, n_moments=67),
           dict(fn=FN_CENTRED_TAN, nb=16, n_moments=47), dict(fn=FN_RCP_RSQRT, n_moments=2), dict(fn=FN_CONTINUATION, nb=10, n_moments=12),
           dict(fn=FN_CONTINUATION, nb=3, n_moments=8), dict(fn=FN_CONTINUATION, nb=0, n_moments=2)]
    for kw in bad:
        status, msg = call(**kw)
        assert status == 1 and msg, (kw, status, msg)
        assert (out == 7.0).all(), kw                                    # nothing was launched
    assert call(n=0)[0] == 0 and (out == 7.0).all()                      # n = 0: nothing to do
    for kw in (dict(fn=FN_CENTRED, nb=16, n_moments=47), dict(fn=FN_CENTRED_TAN, nb=16, n_moments=63), dict(fn=FN_RCP_RSQRT, n_moments=1),
               dict(fn=FN_CONTINUATION, nb=9, n_moments=11)):
        assert call(**kw)[0] == 0, kw
    assert eng.price_lsm(Q, 0.04, 100.0, 1.0, 0.02, False, 2) == before
    Q.free()
