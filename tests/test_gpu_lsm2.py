"""The two-regressor LSM price on the GPU (mcg_price_lsm2; PathEngine.price_lsm2) against lsm2_numpy of
tests/test_lsm2_reference.py on the matrices the library itself generated (PathEngine.heston(..., want_variance=True), both
schemes, downloaded), against mcg_price_lsm where the state carries no information, for repeatability, refusals and timing.

Parity bounds: the device sums the same moments in another order and with fused multiply-adds, solves the same equilibrated
LDL^T and takes the same drop decisions (asserted on every case: no pivot and no relative variance near its threshold), so
the price differs from numpy by rounding.  PRICE_BOUND is ten times the largest error observed on an MI355X over all cases of
this file (observed: price 1.61e-13, on the 1 000 003-path case; std error 6.57e-14), far inside the project's
LSM-on-identical-paths bound of 1e-8 it may not exceed; the std error keeps the issue's 1e-7."""
import ctypes as C
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from test_heston_reference import R, S0
from test_lsm2_reference import (LSM2_CASES, STRONG, assert_decision_distance, case_id, expected_drops_without_state, exponents,
                                 lsm2_numpy)

pytestmark = pytest.mark.gpu

PRICE_BOUND = 1.7e-12
SE_BOUND = 1e-7
# The library forms the std error as mcg_price_lsm does, from {sum V, sum V^2}: var = (sum2 - n mean^2) / (n - 1) carries the
# relative rounding SUMS_REL of the two sums times mean^2, whatever the spread of V_0 (tree sums over per-thread partials of a
# few terms: at most 64 roundings deep at the sizes of this file).  The issue's relative bound on the std error therefore
# has a meaning only where the spread resolves it, 1/2 SUMS_REL mean^2 / var <= SE_BOUND; below that (date 0 in the money:
# every path exercises there, or keeps the same mean, and V_0 is one value on all paths) the variances are compared on the
# scale the sums resolve.
SUMS_REL = 64.0 * np.finfo(float).eps
observed = {"price": 0.0, "std_err": 0.0}


@pytest.fixture(scope="module")
def eng():
    with mc.PathEngine(0) as e:
        yield e


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest errors against numpy in this run: " + ", ".join(f"{k} {v:.2e}" for k, v in observed.items()))


def generate(eng, c, **over):
    a = dict(seed=c["seed"], S0=S0, r=R, dt=c["dt"], n_steps=c["n_steps"], n_paths=c["n_paths"], scheme=c["scheme"],
             want_variance=True, **c["p"])
    a.update(over)
    return eng.heston(**a)


def price2(eng, c, P, F, poly):
    return eng.price_lsm2(P, F, R, c["K"], c["maturity"], c["dt"], c["is_call"], poly, return_dropped=True)


def price1(eng, c, P, poly):
    return eng.price_lsm(P, R, c["K"], c["maturity"], c["dt"], c["is_call"], poly)


def se_error(mean, got_se, want_se, n, where):
    """Relative error of the std error where V_0's spread resolves it (returned for the issue's bound); else asserts that the
    two variances agree to what the sums resolve, and returns 0."""
    if n * want_se ** 2 >= 0.5 * SUMS_REL * mean ** 2 / SE_BOUND:
        return rel(got_se, want_se)
    assert n * abs(got_se ** 2 - want_se ** 2) <= SUMS_REL * mean ** 2, (where, got_se, want_se)
    return 0.0


def rel(a, b):
    return abs(a - b) / abs(b) if b != 0.0 else abs(a)


@pytest.mark.parametrize("c", [c for c in LSM2_CASES if "feature" not in c["name"]], ids=case_id)
def test_parity_with_numpy(eng, c):
    P, V = generate(eng, c)
    S, v = P.to_host_step_major(), V.to_host_step_major()
    if c["name"] == "255":
        assert (v == 0.0).any()           # QE on the Feller-violating set: zeros in the state
    if c["name"] == "257":
        assert (v < 0.0).any()            # the Euler scheme on it: negative variances in the state
    for poly in c["orders"]:
        want, want_se, want_dropped, diag = lsm2_numpy(S, v, R, c["K"], c["maturity"], c["dt"], c["is_call"], poly)
        assert_decision_distance(diag, (c["name"], poly))
        got, got_se, dropped = price2(eng, c, P, V, poly)
        e = rel(got, want)
        e_se = se_error(got, got_se, want_se, c["n_paths"], (c["name"], poly))
        observed["price"], observed["std_err"] = max(observed["price"], e), max(observed["std_err"], e_se)
        print(f"{c['name']} order {poly}: price {e:.2e}, std error {e_se:.2e}, dropped {dropped}")
        assert e <= PRICE_BOUND, (c["name"], poly, got, want)
        assert e_se <= SE_BOUND, (c["name"], poly, got_se, want_se)
        assert dropped == want_dropped, (c["name"], poly, dropped, want_dropped)
        if c["n_paths"] == 1:
            nb = len(exponents(poly))
            assert dropped == (nb - 1) * sum(1 for j in range(c["n_steps"]) if S[j, 0] < c["K"]) and got_se == 0.0
    P.free()
    V.free()


WITHOUT_STATE = [c for c in LSM2_CASES if c["name"] in ("513", "513-short-maturity", "4099-put-110")]


@pytest.mark.parametrize("c", WITHOUT_STATE, ids=case_id)
def test_constant_variance_gives_the_one_regressor_price(eng, c):
    """sigma_v = 0 under the Euler scheme: the variance is the same bits on every path, so every column with zw is dropped
    and the price is mcg_price_lsm's on the same price matrix."""
    P, V = generate(eng, c, scheme="euler", sigma_v=0.0)
    S, v = P.to_host_step_major(), V.to_host_step_major()
    assert (v == v[:, :1]).all()
    for poly in c["orders"]:
        got, _, dropped = price2(eng, c, P, V, poly)
        want = price1(eng, c, P, poly)[0]
        print(f"{c['name']} order {poly}: against price_lsm {rel(got, want):.2e}, dropped {dropped}")
        assert rel(got, want) <= (1e-8 if poly <= 2 else 1e-6), (c["name"], poly, got, want)
        assert dropped == expected_drops_without_state(c, S, poly), (c["name"], poly, dropped)
    P.free()
    V.free()


@pytest.mark.parametrize("c", WITHOUT_STATE[:2], ids=case_id)
def test_uploaded_constant_and_collinear_states(eng, c):
    P, V = generate(eng, c)
    V.free()
    rows = P.to_host()
    S = np.ascontiguousarray(rows.T)
    states = {"constant": eng.from_host(np.full_like(rows, 0.04)), "collinear": eng.from_host(3.0 * rows + 2.0)}
    for poly in c["orders"]:
        want = price1(eng, c, P, poly)[0]
        for name, F in states.items():
            got, _, dropped = price2(eng, c, P, F, poly)
            assert rel(got, want) <= (1e-8 if poly <= 2 else 1e-6), (c["name"], name, poly, got, want)
            assert dropped == expected_drops_without_state(c, S, poly), (c["name"], name, poly, dropped)
    for F in states.values():
        F.free()
    P.free()


def test_repeatable_and_independent_of_other_calls(eng):
    c = next(c for c in LSM2_CASES if c["name"] == "20011")
    P, V = generate(eng, c)
    first = [price2(eng, c, P, V, poly) for poly in c["orders"]]
    assert [price2(eng, c, P, V, poly) for poly in c["orders"]] == first
    price1(eng, c, P, 2)                                      # the one-launch sweep
    price1(eng, c, P, 5)                                      # the per-date route: the same message slot and partials
    eng.price_exotics(P, R, 1.0, [mc.exotic("asian_arith_fixed", False, 100.0), mc.exotic("lookback_float", True)])
    assert [price2(eng, c, P, V, poly) for poly in c["orders"]] == first
    P.free()
    V.free()


def test_the_second_regressor_moves_the_price(eng):
    """200 003 QE paths x 20 dates, sigma_v = 0.9, rho = -0.7, at-the-money put, order 2: numpy alone shows 15 combined std
    errors on these draws (test_lsm2_reference.py); the library must show more than 4."""
    c = next(c for c in LSM2_CASES if c["name"] == "200003-feature")
    assert c["p"] is STRONG
    P, V = generate(eng, c)
    two, se2, _ = price2(eng, c, P, V, 2)
    one, se1 = price1(eng, c, P, 2)
    gap = (two - one) / math.hypot(se1, se2)
    print(f"two regressors {two:.4f} +- {se2:.4f}, one {one:.4f} +- {se1:.4f}: {gap:.1f} combined std errors")
    assert gap > 4.0
    P.free()
    V.free()


def test_refusals(eng):
    c = next(c for c in LSM2_CASES if c["name"] == "513")
    P, V = generate(eng, c)
    L, m = eng._L, C.c_double()

    def raw(ctx=eng._ctx, paths=P._h, state=V._h, r=R, K=100.0, maturity=1.0, dt=c["dt"], poly=2, mean=C.byref(m)):
        status = L.mcg_price_lsm2(ctx, paths, state, r, K, maturity, dt, 0, poly, mean, None, None)
        return status, L.mcg_last_error().decode()

    assert raw()[0] == 0                                       # (and a NULL std_err and n_dropped are fine)
    short = eng.gbm(5, 100.0, R, 0.2, c["dt"], c["n_steps"] - 1, c["n_paths"])
    narrow = eng.gbm(5, 100.0, R, 0.2, c["dt"], c["n_steps"], c["n_paths"] - 1)
    bad = [dict(ctx=None), dict(paths=None), dict(state=None), dict(mean=None), dict(state=short._h), dict(state=narrow._h),
           dict(poly=-1), dict(poly=4), dict(r=math.nan), dict(K=math.inf), dict(maturity=math.nan), dict(dt=math.inf),
           dict(K=0.0), dict(K=-1.0), dict(dt=0.0), dict(dt=-0.1)]
    with mc.PathEngine(0) as other:
        Q, W = generate(other, c)
        bad += [dict(paths=Q._h), dict(state=W._h)]
        for kw in bad:
            status, msg = raw(**kw)
            assert status == 1 and msg, (kw, status, msg)
        other.set_allreduce(lambda ptr, count, stream: None)
        status, msg = raw(ctx=other._ctx, paths=Q._h, state=W._h)
        assert status == 1 and "collective" in msg, (status, msg)
    empty, empty_state = eng.gbm(5, 100.0, R, 0.2, c["dt"], c["n_steps"], 0), eng.gbm(6, 100.0, R, 0.2, c["dt"], c["n_steps"], 0)
    status, msg = raw(paths=empty._h, state=empty_state._h)
    assert status == 6 and msg, (status, msg)
    with pytest.raises(mc.McgError) as e:
        eng.price_lsm2(P, V, R, 100.0, 1.0, c["dt"], False, 4)
    assert e.value.status == 1 and "poly_order" in str(e.value)
    for M in (short, narrow, empty, empty_state, P, V):
        M.free()


def test_device_time_is_booked_under_the_lsm_sweep(eng):
    c = next(c for c in LSM2_CASES if c["name"] == "20011")
    P, V = generate(eng, c)
    eng.timing_enable(True)
    eng.timing_reset()
    try:
        price2(eng, c, P, V, 2)
        ms, launches = eng.timing_get(N.K_LSM_SWEEP)
        assert ms > 0.0 and launches >= 4 * c["n_steps"]          # four launches per exercise date
        price2(eng, c, P, V, 2)
        ms2, launches2 = eng.timing_get(N.K_LSM_SWEEP)
        assert ms2 > ms and launches2 == 2 * launches
    finally:
        eng.timing_enable(False)
    P.free()
    V.free()
