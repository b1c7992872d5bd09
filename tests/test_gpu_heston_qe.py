"""The QE Heston generator on the GPU (mcg_paths_heston_qe, mcg_paths_heston_qe_payoff; PathEngine.heston(scheme="qe"))
against the numpy reference of tests/test_heston_qe_reference.py on the same (seed, path ids), against the closed form, and
through the consumers of a path matrix.

Parity bounds: S is compared relatively, v on the scale max(v0, theta).  The device evaluates the same scheme with its own
logarithm, sine / cosine, square root, reciprocal and exponential (<= ~2 ulp each) and with fused multiply-adds, so the
difference from numpy is rounding that accumulates over the steps.  S_BOUND and V_BOUND are ten times the largest error
observed on an MI355X over all cases of this file (observed: S 7.88e-14, v 5.74e-13, both on the 252-step
Feller-violating shape), far inside the 1e-9 they may not
exceed.  The cases are test_heston_qe_reference.QE_PARITY_SETS, where every draw keeps a distance of 1e-9 from both branch
decisions of the scheme and the reference's own rounding error is held to 1e-11.
The fused payoff, the consumers and the exotics keep the bounds of the Euler file (test_gpu_heston.py).

One step on its own (mcg_debug_eval_v fn 8: HestonQe::step as the kernels call it, two paths per lane) is compared with the step
of include/mcgpu.h in mpmath, test_heston_qe_reference.qe_step_mp, on the cases of step_cases.  Its three bars are 1.5 times the
largest error observed on an MI355X:
  STEP_V_BAR_IN_M  v' in units of m, the step's conditional mean: observed 1.912e-10 (theta = 0, v = 1.3e-8, psi = 5e5, u next
                   to p).  The exponential branch dominates it: v' = ln(1 / y) / beta with y = (1 - u) / (1 - p) rounded next
                   to 1, so an ulp of y is an ulp of 1 / beta = m (psi + 1) / 2, and psi has no upper end.  In the quadratic branch
                   and at psi of order one the cancellation in m = theta + (v - theta) E dominates (4.3e-13 at v = 5e-8,
                   theta = 0.04, daily steps: half an ulp of theta is 2e-14 of that m, doubled by ln(1 / m^2)).
  STEP_V_BAR       v' on the scale that takes both out (qe_step_mp: (m or 1 / beta, plus v') x max(1, theta / m)): observed
                   4.234e-16, two ulps -- the bar that would notice a lost Newton step or a wrong coefficient.
  STEP_S_BAR       S' relatively, in units of the size of its exponent's terms (1 + |drift| + |K1 v| + |K2 v'| + |sqrt z1|):
                   observed 8.966e-16 -- the 2 ulp of the exponential and an ulp per term; K2 times the error of v' is below
                   1e-16 in every case.
(Before HestonQe::constants took m = v at kappa = 0, that corner had v' off by 6.8e-5 m and S' by 2.2e-12 at v = 1.8e-8,
theta = 0.04.)"""
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from test_exotics_reference import stats_numpy
from test_gpu_exotics import check_prices, full_book
from test_heston_qe_reference import (QE_PARITY_SETS, STAT_PATHS, STAT_ROWS, STEP_BLOCK, STEP_ELEM, STEP_MARGIN, STEP_SEED,
                                      STEP_SETS, heston_qe_numpy, stat_cases, step_constants, step_reference)
from test_heston_reference import (FELLER_VIOLATING, PARAMS, R, S0, SEED64, STAT_SEED, STD_ERRORS, STRIKES,
                                   heston_closed_form)

pytestmark = pytest.mark.gpu

S_BOUND = 7.9e-13
V_BOUND = 5.8e-12
STEP_V_BAR_IN_M = 1.5 * 1.912e-10
STEP_V_BAR = 1.5 * 4.234e-16
STEP_S_BAR = 1.5 * 8.966e-16
V_QE_STEP = 8
DT = 1.0 / 252.0
observed = {"S": 0.0, "v": 0.0}


@pytest.fixture(scope="module")
def eng():
    with mc.PathEngine(0) as e:
        yield e


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest errors against numpy in this run: " + ", ".join(f"{k} {v:.2e}" for k, v in observed.items()))


def bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


def gen(p, dt, n_steps):
    return dict(S0=S0, r=R, dt=dt, n_steps=n_steps, scheme="qe", **p)


def reference(seed, p, dt, n_steps, n_paths, path_begin, cache={}):
    """One numpy run per case, shared by its four forms (never written to)."""
    key = (seed, tuple(sorted(p.items())), dt, n_steps, n_paths, path_begin)
    if key not in cache:
        cache[key] = heston_qe_numpy(seed, S0, R, dt=dt, n_steps=n_steps, n_paths=n_paths, path_begin=path_begin, **p)
    return cache[key]


def check_parity(eng, seed, p, dt, n_steps, n_paths, path_begin, want_variance, payoff, where):
    S, v = reference(seed, p, dt, n_steps, n_paths, path_begin)
    got = eng.heston(seed, n_paths=n_paths, path_begin=path_begin, payoff=payoff, want_variance=want_variance, **gen(p, dt, n_steps))
    P, V = got if want_variance else (got, None)
    assert (P.n_paths, P.n_steps) == (n_paths, n_steps)
    gs = P.to_host_step_major()
    es = float(np.abs(gs / S - 1.0).max())
    observed["S"] = max(observed["S"], es)
    print(f"{where}: S {es:.2e}", end="")
    assert es <= S_BOUND, (where, "S", es)
    gv = None
    if V is not None:
        assert (V.n_paths, V.n_steps) == (n_paths, n_steps)
        gv = V.to_host_step_major()
        ev = float(np.abs(gv - v).max()) / max(p["v0"], p["theta"])
        observed["v"] = max(observed["v"], ev)
        print(f", v {ev:.2e}", end="")
        assert ev <= V_BOUND, (where, "v", ev)
        assert (gv >= 0.0).all(), (where, "v < 0")
        assert np.array_equal(gv == 0.0, v == 0.0), (where, "the zeros of v")
        V.free()
    print()
    if payoff is not None:
        K, is_call = payoff
        T = n_steps * dt
        x = np.maximum(gs[-1] - K, 0.0) if is_call else np.maximum(K - gs[-1], 0.0)
        m, se = eng.price_european(P, K, R, T, is_call)
        D = math.exp(-R * T)
        assert abs(m - D * x.mean()) <= 1e-12 * max(D * x.mean(), 1e-300), (where, "fused price")
        if n_paths > 1 and x.std() > 0.0:
            # the library forms the std error from {sum, sum^2}: the relative error of the sums times (1/2 + mean^2 / variance),
            # which matters where nearly every path pays the same (a put after 21 years at 200 % volatility pays K)
            want_se = D * x.std(ddof=1) / math.sqrt(n_paths)
            cond = max(1.0, 0.5 + (x.mean() / x.std()) ** 2)
            assert abs(se - want_se) <= 1e-9 * cond * want_se, (where, "fused std error", se, want_se, cond)
    P.free()
    return gv


@pytest.mark.parametrize("name", list(QE_PARITY_SETS))
def test_parity_with_numpy(eng, name):
    p, dt, shapes = QE_PARITY_SETS[name]
    for k, (n_steps, n_paths, begin, seed) in enumerate(shapes):
        for want_variance in (False, True):
            for payoff in (None, (100.0, (k + want_variance) % 2 == 0)):
                gv = check_parity(eng, seed, p, dt, n_steps, n_paths, begin, want_variance, payoff,
                                  (name, n_steps, n_paths, begin, want_variance, payoff))
        if name == "feller-violating" and n_paths >= 257 and n_steps >= 8:
            assert (gv == 0.0).any()                     # the exponential branch and its mass at zero, in the short shapes too


def qe_step(eng, name, cases):
    """[n][3] (v', S', exponential?) of HestonQe::step on cases [n][>= 5] (v, z1, z2, S, path id) of one parameter set."""
    p, dt = STEP_SETS[name]
    params = step_constants(p, dt) + (STEP_SEED & 0xFFFFFFFF, STEP_SEED >> 32, STEP_BLOCK, STEP_ELEM)
    return eng.debug_eval_v(V_QE_STEP, np.ascontiguousarray(cases[:, :5]), params)[:, :3]


step_observed = {"v in m": 0.0, "v": 0.0, "S": 0.0}


@pytest.fixture(scope="module", autouse=True)
def report_steps():
    yield
    print("\nlargest errors of one step against mpmath in this run: " + ", ".join(f"{k} {v:.3e}" for k, v in step_observed.items()))


@pytest.mark.parametrize("name", list(STEP_SETS))
def test_one_step_against_mpmath(eng, name):
    import mpmath as mp
    cases, ref = step_reference(name)
    got = qe_step(eng, name, cases)
    assert np.isfinite(got).all() and (got[:, 0] >= 0.0).all() and (got[:, 1] > 0.0).all()        # (c): every case has m >= 0
    worst = {"v in m": 0.0, "v": 0.0, "S": 0.0}
    at = {}
    for row, (gv, gs, gflag), (vn, Sn, exponential, m, margin, v_scale, e_size) in zip(cases, got, ref):
        if margin < STEP_MARGIN:                           # (at most STEP_LEFT_OUT of all cases: asserted in the reference's file)
            continue
        assert bool(gflag) == exponential, row                                                      # (a)
        err = {"S": float(abs(mp.mpf(gs) / Sn - 1) / e_size)}
        if m == 0 or vn == 0:
            assert gv == 0.0, row
        else:
            dv = abs(mp.mpf(gv) - vn)
            err["v in m"], err["v"] = float(dv / m), float(dv / v_scale)
        for k, e in err.items():
            if e > worst[k]:
                worst[k], at[k] = e, (row[0], float(m), exponential)
    print(f"{name}: " + ", ".join(f"{k} {worst[k]:.3e} at (v, m, exponential) = {at.get(k)}" for k in worst))
    for k in worst:
        step_observed[k] = max(step_observed[k], worst[k])
    assert worst["v in m"] <= STEP_V_BAR_IN_M and worst["v"] <= STEP_V_BAR and worst["S"] <= STEP_S_BAR, (name, worst)   # (b)


def test_one_step_does_not_depend_on_the_wave(eng):
    """A wave enters the exponential branch when one of its lanes needs it.  Whole waves (128 elements: 64 lanes of two paths) of
    quadratic elements, of exponential elements, and the quadratic wave with a single exponential element: every element keeps
    its bits, the quadratic lane-mate of the exponential element included."""
    name = "violating-eighth"
    cases, ref = step_reference(name)
    clear = np.array([r[4] >= STEP_MARGIN for r in ref])
    expo = np.array([r[2] for r in ref])
    Q, X = cases[clear & ~expo][:128], cases[clear & expo][:128]
    assert len(Q) == len(X) == 128
    q, x = qe_step(eng, name, Q), qe_step(eng, name, X)
    assert (q[:, 2] == 0.0).all() and (x[:, 2] == 1.0).all()
    mixed = Q.copy()
    mixed[37] = X[0]
    want = q.copy()
    want[37] = x[0]
    assert bits(qe_step(eng, name, mixed)) == bits(want)
    assert bits(qe_step(eng, name, np.concatenate([Q, X, Q[:5]]))) == bits(np.concatenate([q, x, q[:5]]))
    everything = qe_step(eng, name, cases)
    assert bits(everything[clear & ~expo][:128]) == bits(q) and bits(everything[clear & expo][:128]) == bits(x)


def test_with_kappa_zero_the_level_does_not_enter(eng):
    """kappa = 0: no constant of the scheme depends on theta, and m = v exactly (HestonQe::constants) -- formed as theta + (v - theta)
    it would round at the size of theta and move S by 1e-12 a step where v << theta.  (v0 = 0.01: psi = 0.7 at the first step, so
    every path has a positive variance for that rounding to act on.)"""
    a = dict(S0=S0, r=R, dt=1.0 / 52.0, n_steps=9, scheme="qe", v0=0.01, kappa=0.0, sigma_v=0.6, rho=-0.7)
    out = []
    for theta in (0.0, 0.04, 4.0):
        P, V = eng.heston(SEED64, n_paths=1000, want_variance=True, theta=theta, **a)
        out.append((bits(P.to_host_step_major()), bits(V.to_host_step_major())))
        P.free()
        V.free()
    assert out[0] == out[1] == out[2]


def test_sharding_and_determinism(eng):
    n, a_cut = 5000, 1537
    for p, dt, _ in (QE_PARITY_SETS["feller-violating"], QE_PARITY_SETS["large-vol"]):
        a = gen(p, dt, 11)
        P, V = eng.heston(SEED64, n_paths=n, want_variance=True, **a)
        whole_s, whole_v = P.to_host_step_major(), V.to_host_step_major()
        Q, W = eng.heston(SEED64, n_paths=n, want_variance=True, **a)
        assert bits(Q.to_host_step_major()) == bits(whole_s) and bits(W.to_host_step_major()) == bits(whole_v)
        only_s = eng.heston(SEED64, n_paths=n, **a)
        assert bits(only_s.to_host_step_major()) == bits(whole_s)          # the variance matrix changes nothing in S
        A, VA = eng.heston(SEED64, n_paths=a_cut, want_variance=True, **a)
        B, VB = eng.heston(SEED64, n_paths=n - a_cut, path_begin=a_cut, want_variance=True, **a)
        assert bits(np.hstack([A.to_host_step_major(), B.to_host_step_major()])) == bits(whole_s)
        assert bits(np.hstack([VA.to_host_step_major(), VB.to_host_step_major()])) == bits(whole_v)
        f1 = eng.heston(SEED64, n_paths=n, payoff=(100.0, False), **a)
        f2 = eng.heston(SEED64, n_paths=n, payoff=(100.0, False), **a)
        assert bits(eng.price_european(f1, 100.0, R, 11 * dt, False)) == bits(eng.price_european(f2, 100.0, R, 11 * dt, False))
        assert bits(f1.to_host_step_major()) == bits(whole_s)
        for M in (P, V, Q, W, only_s, A, VA, B, VB, f1, f2):
            M.free()
    # the violating set at eight steps a year: lanes of one wave take both branches (half of the draws are exponential), and a
    # shard boundary regroups the paths into other waves -- a stream-3 block skipped for a wave that needed it would show here
    a = gen(FELLER_VIOLATING, 1.0 / 8.0, 8)
    P, V = eng.heston(SEED64, n_paths=n, want_variance=True, **a)
    whole_s, whole_v = P.to_host_step_major(), V.to_host_step_major()
    zero = (whole_v[1:, :4992] == 0.0).reshape(8, -1, 128)          # (a wave holds 128 adjacent paths)
    assert (zero.any(axis=2) & ~zero.all(axis=2)).any()
    for cut in (a_cut, 64, 4999):
        A, VA = eng.heston(SEED64, n_paths=cut, want_variance=True, **a)
        B, VB = eng.heston(SEED64, n_paths=n - cut, path_begin=cut, want_variance=True, **a)
        assert bits(np.hstack([A.to_host_step_major(), B.to_host_step_major()])) == bits(whole_s)
        assert bits(np.hstack([VA.to_host_step_major(), VB.to_host_step_major()])) == bits(whole_v)
        for M in (A, VA, B, VB):
            M.free()
    P.free()
    V.free()


@pytest.mark.parametrize("p, T, n_steps", stat_cases(STAT_ROWS))
def test_closed_form_and_martingale(eng, p, T, n_steps):
    a = gen(p, T / n_steps, n_steps)
    P = eng.heston(STAT_SEED, n_paths=STAT_PATHS, **a)
    fwd, fwd_se = eng.price_european(P, 0.0, R, T, True)
    print(f"martingale: e^-rT mean(S_T) = {fwd:.5f} +- {fwd_se:.5f}, {abs(fwd - S0) / fwd_se:.2f} std errors")
    assert fwd_se > 0.0 and abs(fwd - S0) <= STD_ERRORS * fwd_se
    for K in STRIKES:
        for is_call in (True, False):
            want = heston_closed_form(S0, K, R, T, is_call=is_call, **p)
            price, se = eng.price_european(P, K, R, T, is_call)
            print(f"K={K:g} call={is_call}: {price:.5f} +- {se:.5f}, closed form {want:.5f}, {abs(price - want) / se:.2f} std errors")
            assert se > 0.0 and abs(price - want) <= STD_ERRORS * se, (K, is_call, price, want, se)
            F = eng.heston(STAT_SEED, n_paths=STAT_PATHS, payoff=(K, is_call), **a)
            fused, fused_se = eng.price_european(F, K, R, T, is_call)
            F.free()
            assert abs(fused - price) <= 1e-12 * price and abs(fused_se - se) <= 1e-9 * se
            assert abs(fused - want) <= STD_ERRORS * fused_se
            g = eng.greeks_european(P, K, R, T, is_call, sigma=0.0)
            assert abs(g["price"] - want) <= STD_ERRORS * g["price_se"] and abs(g["price"] - price) <= 1e-12 * price
    P.free()


def test_the_advantage_over_euler_at_eight_steps_a_year(eng):
    T, n_steps, K = 1.0, 8, 110.0
    want = heston_closed_form(S0, K, R, T, is_call=True, **FELLER_VIOLATING)
    dist = {}
    for scheme in ("euler", "qe"):
        P = eng.heston(STAT_SEED, n_paths=STAT_PATHS, **dict(gen(FELLER_VIOLATING, T / n_steps, n_steps), scheme=scheme))
        price, se = eng.price_european(P, K, R, T, True)
        P.free()
        dist[scheme] = abs(price - want) / se
        print(f"{scheme}: {price:.5f} +- {se:.5f}, closed form {want:.5f}, {dist[scheme]:.2f} std errors")
    assert dist["euler"] > 10.0
    assert dist["qe"] <= STD_ERRORS


def test_consumers_accept_the_matrix(eng):
    p, n_steps, dt, n = PARAMS["feller"], 50, 0.02, 100_000
    T = n_steps * dt
    P = eng.heston(STAT_SEED, n_paths=n, **gen(p, dt, n_steps))
    put, put_se = eng.price_european(P, 100.0, R, T, False)
    lsm, lsm_se = eng.price_lsm(P, R, 100.0, T, dt, False, 2)
    print(f"European put {put:.4f} +- {put_se:.4f}, LSM put {lsm:.4f} +- {lsm_se:.4f}")
    assert lsm >= put - 3.0 * put_se
    for is_call in (True, False):
        g = eng.greeks_european(P, 100.0, R, T, is_call)
        assert all(math.isfinite(g[k]) and math.isfinite(g[k + "_se"]) for k in ("price", "delta", "rho", "dual_delta")), g
        assert math.isnan(g["gamma"]) and math.isnan(g["vega"])
        assert (g["delta"] > 0.0) == is_call
    X = P.to_host()
    for first_row in (0, 1):
        st5 = stats_numpy(X, first_row)
        book = full_book(st5, (90.0, 100.0, 110.0))
        price, se = eng.price_exotics(P, R, T, book, first_row=first_row)
        check_prices(price, se, book, st5, R, T, ("heston-qe", first_row))
    P.free()


def test_invalid_arguments(eng):
    L = mc.load_library()
    ok = dict(seed=1, S0=100.0, r=0.04, v0=0.04, kappa=2.0, theta=0.04, sigma_v=0.3, rho=-0.7, dt=DT, n_steps=8, n_paths=100,
              scheme="qe")
    eng.heston(**ok).free()
    nan, inf = float("nan"), float("inf")
    bad = [dict(S0=0.0), dict(S0=-1.0), dict(dt=0.0), dict(dt=-DT), dict(v0=-0.01), dict(kappa=-1.0), dict(theta=-0.04),
           dict(sigma_v=-0.3), dict(sigma_v=0.0), dict(rho=1.0001), dict(rho=-1.5), dict(n_steps=0), dict(n_paths=-1)]
    bad += [{k: x} for k in ("S0", "r", "v0", "kappa", "theta", "sigma_v", "rho", "dt") for x in (nan, inf, -inf)]
    for change in bad:
        for extra in (dict(), dict(payoff=(100.0, True)), dict(want_variance=True)):
            with pytest.raises(mc.McgError) as e:
                eng.heston(**dict(ok, **change), **extra)
            assert e.value.status == 1 and str(e.value) and L.mcg_last_error(), change
            if change == dict(sigma_v=0.0):
                assert "mcg_paths_heston" in str(e.value).replace("mcg_paths_heston_qe", "")
    with pytest.raises(mc.McgError) as e:
        eng.heston(**ok, payoff=(nan, True))
    assert e.value.status == 1
    with pytest.raises(ValueError):
        eng.heston(**dict(ok, scheme="nonsense"))
    # the edges of the valid set
    for change in (dict(rho=1.0), dict(rho=-1.0), dict(v0=0.0), dict(kappa=0.0), dict(theta=0.0), dict(theta=0.0, v0=0.0),
                   dict(kappa=0.0, v0=0.0), dict(n_paths=0)):
        M, V = eng.heston(**dict(ok, **change), want_variance=True)
        if M.n_paths:
            s, v = M.to_host_step_major(), V.to_host_step_major()
            assert np.isfinite(s).all() and np.isfinite(v).all() and (v >= 0.0).all() and (s > 0.0).all(), change
        M.free()
        V.free()


def test_launch_accounting(eng):
    eng.timing_enable(True)
    eng.timing_reset()
    P = eng.heston(1, n_paths=10_000, **gen(PARAMS["feller"], DT, 8))
    ms, launches = eng.timing_get(N.K_HESTON)
    assert launches == 1 and ms > 0.0 and eng.timing_get(N.K_GBM)[1] == 0 and eng.timing_get(N.K_PAYOFF)[1] == 0
    Q, V = eng.heston(1, n_paths=10_000, payoff=(100.0, True), want_variance=True, **gen(PARAMS["feller"], DT, 8))
    assert eng.timing_get(N.K_HESTON)[1] == 2 and eng.timing_get(N.K_GBM)[1] == 0 and eng.timing_get(N.K_PAYOFF)[1] > 0
    eng.timing_enable(False)
    for M in (P, Q, V):
        M.free()
