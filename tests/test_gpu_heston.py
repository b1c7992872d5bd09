"""The Heston generator on the GPU (mcg_paths_heston, mcg_paths_heston_payoff) against the numpy reference of
tests/test_heston_reference.py on the same (seed, path ids), against the closed form, and through the consumers of a
path matrix.

Parity bounds: S is compared relatively, v on the scale max(v0, theta).  The device evaluates the same scheme with its
own logarithm, sine / cosine, square root and exponential (<= ~2 ulp each, fastmath.hpp) and with fused multiply-adds, so
the difference from numpy is rounding that accumulates over the steps.  S_BOUND and V_BOUND are ten times the largest
error observed on an MI355X over all cases of this file (observed: S 1.92e-14, v 6.94e-15, both on the 252-step shapes),
far inside the 1e-9 they may not exceed.  The cases are those of test_heston_reference.PARITY_SETS, where the reference's own
rounding error is held to 1e-11 (the scheme is ill-conditioned where v passes closely above zero: see there).
The reduction to GBM, the fused payoff and the exotics keep the bounds of the tests they mirror (test_gpu_parity.py,
test_gpu_exotics.py)."""
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from test_exotics_reference import stats_numpy
from test_gpu_exotics import check_prices, full_book
from test_heston_reference import (PARAMS, PARITY_SETS, R, S0, SEED64, STAT_SEED, STD_ERRORS, STREAM_PRICE, STRIKES,
                                   heston_closed_form, heston_numpy, normal_quad, stat_cases)

pytestmark = pytest.mark.gpu

S_BOUND = 2e-13
V_BOUND = 7e-14
DT = 1.0 / 252.0
STAT_PATHS = 1_000_000
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
    return dict(S0=S0, r=R, dt=dt, n_steps=n_steps, **p)


def check_parity(eng, seed, p, dt, n_steps, n_paths, path_begin, want_variance, payoff, where):
    a = gen(p, dt, n_steps)
    S, v = heston_numpy(seed, n_paths=n_paths, path_begin=path_begin, **a)
    got = eng.heston(seed, n_paths=n_paths, path_begin=path_begin, payoff=payoff, want_variance=want_variance, **a)
    P, V = got if want_variance else (got, None)
    assert (P.n_paths, P.n_steps) == (n_paths, n_steps)
    gs = P.to_host_step_major()
    es = float(np.abs(gs / S - 1.0).max())
    observed["S"] = max(observed["S"], es)
    assert es <= S_BOUND, (where, "S", es)
    if V is not None:
        assert (V.n_paths, V.n_steps) == (n_paths, n_steps)
        ev = float(np.abs(V.to_host_step_major() - v).max()) / max(p["v0"], p["theta"])
        observed["v"] = max(observed["v"], ev)
        assert ev <= V_BOUND, (where, "v", ev)
        V.free()
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
    return S, v


@pytest.mark.parametrize("name", list(PARITY_SETS))
def test_parity_with_numpy(eng, name):
    p, dt, shapes = PARITY_SETS[name]
    for k, (n_steps, n_paths, begin, seed) in enumerate(shapes):
        for want_variance in (False, True):
            for payoff in (None, (100.0, (k + want_variance) % 2 == 0)):
                S, v = check_parity(eng, seed, p, dt, n_steps, n_paths, begin, want_variance, payoff,
                                    (name, n_steps, n_paths, begin, want_variance, payoff))
        if name == "feller-violating" and n_paths >= 257 and n_steps >= 8:
            assert (v < 0.0).any()                       # the reference really truncates, in the short shapes too
        if name == "large-vol" and n_steps == 252:
            assert np.abs(np.log(S[1:] / S[:-1])).max() > 0.34   # ... and really leaves the small-exponent shortcut


def test_reduction_to_gbm(eng):
    n_steps, n_paths, dt = 50, 3000, 0.02
    P, V = eng.heston(7, S0, R, 0.04, 2.0, 0.04, 0.0, 0.0, dt, n_steps, n_paths, path_begin=5, want_variance=True)
    G = eng.gbm(7, S0, R, 0.2, dt, n_steps, n_paths, path_begin=5)
    h, g = P.to_host_step_major(), G.to_host_step_major()
    assert (V.to_host_step_major() == 0.04).all()
    path = np.uint64(5) + np.arange(n_paths, dtype=np.uint64)
    z = np.stack([normal_quad(7, path, n >> 2, STREAM_PRICE)[n & 3] for n in range(n_steps)])
    want = S0 * np.exp(np.cumsum((R - 0.02) * dt + 0.2 * math.sqrt(dt) * z, axis=0))
    eh, eg, ehg = (float(np.abs(a[1:] / b - 1.0).max()) for a, b in ((h, want), (g, want), (h, g[1:])))
    print(f"Heston at sigma_v = 0 against the draws {eh:.2e}, GBM against them {eg:.2e}, one against the other {ehg:.2e}")
    assert eh <= 1e-11 and eg <= 1e-11 and ehg <= 2e-11
    assert (h[0] == S0).all()
    for M in (P, V, G):
        M.free()


def test_sharding_and_determinism(eng):
    n, a_cut = 5000, 1537
    for p, dt, _ in (PARITY_SETS["feller-violating"], PARITY_SETS["large-vol"]):
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


@pytest.mark.parametrize("p, T, n_steps", stat_cases())
def test_closed_form_and_martingale(eng, p, T, n_steps):
    a = gen(p, T / n_steps, n_steps)
    P = eng.heston(STAT_SEED, n_paths=STAT_PATHS, **a)
    fwd, fwd_se = eng.price_european(P, 0.0, R, T, True)
    print(f"martingale: e^-rT mean(S_T) = {fwd:.5f} +- {fwd_se:.5f}")
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
        check_prices(price, se, book, st5, R, T, ("heston", first_row))
    P.free()


def test_invalid_arguments(eng):
    L = mc.load_library()
    ok = dict(seed=1, S0=100.0, r=0.04, v0=0.04, kappa=2.0, theta=0.04, sigma_v=0.3, rho=-0.7, dt=DT, n_steps=8, n_paths=100)
    eng.heston(**ok).free()
    nan, inf = float("nan"), float("inf")
    bad = [dict(S0=0.0), dict(S0=-1.0), dict(dt=0.0), dict(dt=-DT), dict(v0=-0.01), dict(kappa=-1.0), dict(theta=-0.04),
           dict(sigma_v=-0.3), dict(rho=1.0001), dict(rho=-1.5), dict(n_steps=0), dict(n_paths=-1)]
    bad += [{k: x} for k in ("S0", "r", "v0", "kappa", "theta", "sigma_v", "rho", "dt") for x in (nan, inf, -inf)]
    for change in bad:
        for extra in (dict(), dict(payoff=(100.0, True)), dict(want_variance=True)):
            with pytest.raises(mc.McgError) as e:
                eng.heston(**dict(ok, **change), **extra)
            assert e.value.status == 1 and str(e.value) and L.mcg_last_error(), change
    with pytest.raises(mc.McgError) as e:
        eng.heston(**ok, payoff=(nan, True))
    assert e.value.status == 1
    # the edges of the valid set
    for change in (dict(rho=1.0), dict(rho=-1.0), dict(v0=0.0), dict(kappa=0.0), dict(theta=0.0), dict(sigma_v=0.0), dict(n_paths=0)):
        M = eng.heston(**dict(ok, **change))
        if M.n_paths:
            assert np.isfinite(M.to_host_step_major()).all(), change
        M.free()


def test_launch_accounting(eng):
    eng.timing_enable(True)
    eng.timing_reset()
    P = eng.heston(1, S0, R, dt=DT, n_steps=8, n_paths=10_000, **PARAMS["feller"])
    ms, launches = eng.timing_get(N.K_HESTON)
    assert launches == 1 and ms > 0.0 and eng.timing_get(N.K_GBM)[1] == 0 and eng.timing_get(N.K_PAYOFF)[1] == 0
    Q, V = eng.heston(1, S0, R, dt=DT, n_steps=8, n_paths=10_000, payoff=(100.0, True), want_variance=True, **PARAMS["feller"])
    assert eng.timing_get(N.K_HESTON)[1] == 2 and eng.timing_get(N.K_GBM)[1] == 0 and eng.timing_get(N.K_PAYOFF)[1] > 0
    eng.timing_enable(False)
    for M in (P, Q, V):
        M.free()


def test_launch_frame(eng):
    """One launch under the generator's kernel id with the variance matrix stored, the fused sums and their reuse
    (test_gpu_parity.check_launch_frame)."""
    from test_gpu_parity import FRAME_PATHS, FRAME_STEPS, check_launch_frame
    check_launch_frame(eng, N.K_HESTON, lambda payoff: eng.heston(1, 100.0, R, dt=DT, n_steps=FRAME_STEPS, n_paths=FRAME_PATHS, payoff=payoff,
                                                                  want_variance=True, **PARAMS["feller"]))
