"""The local-volatility generator on the GPU (mcg_paths_localvol, mcg_paths_localvol_payoff; PathEngine.local_vol) against the
numpy reference of tests/test_localvol_reference.py on the same (seed, path ids), for the bit identities of the contract, against
the GBM generators on a flat surface, through the consumers of a path matrix, for its refusals and against closed forms.

Parity bounds: S is compared relatively.  The device draws the same normals with its own logarithm, sine / cosine and square
root, forms the exponent with fused multiply-adds and takes its own exponential (<= ~2 ulp each); the volatility a is continuous
in the path's log-moneyness, so the difference from numpy is rounding that accumulates over the steps.  S_BOUND is ten times the
largest error observed on an MI355X over all surfaces and shapes of this file (S_OBSERVED, on a 252-step shape), GBM_BOUND ten
times what the flat surface showed against mcg_paths_gbm and against the one-asset mcg_paths_gbm_multi (GBM_OBSERVED); neither
may exceed the 1e-11 the reference itself is held to (OWN_ERROR_BOUND)."""
import ctypes as C
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from test_heston_reference import OWN_ERROR_BOUND, SEED64, STAT_SEED
from test_localvol_reference import (BAD_MODELS, BAD_SURFACES, CEV, DT, NARROW, Q, R, S0, SHAPES, STAT_STEPS, STAT_T, SURFACES, TERM_STAT,
                                     WIDE_128, Surface, check_cev_prices, check_term_prices, raw_paths, reference)

pytestmark = pytest.mark.gpu

# on an MI355X: 1.44e-14 on the 252-step shape of "narrow" (next: 1.0e-14 and below on the other 252-step shapes); the flat surface at
# sigma = 1.5 over 252 steps: 4.11e-15 against mcg_paths_gbm, 3.11e-15 against mcg_paths_gbm_multi with one asset at q = 0.02
S_OBSERVED, GBM_OBSERVED = 1.44e-14, 4.11e-15
S_BOUND = min(10.0 * S_OBSERVED, OWN_ERROR_BOUND)
GBM_BOUND = min(10.0 * GBM_OBSERVED, OWN_ERROR_BOUND)
STAT_PATHS = 1_000_000
observed = {"S": 0.0, "flat against gbm": 0.0, "flat against gbm_multi": 0.0}


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


def host(M):
    """The step-major matrix of M, which it frees."""
    out = M.to_host_step_major()
    M.free()
    return out


@pytest.mark.parametrize("name", sorted(SURFACES))
def test_parity_with_numpy(eng, name):
    surface = SURFACES[name]
    for k, shape in enumerate(SHAPES):
        n_steps, n_paths, begin, seed = shape
        want = reference(name, shape)
        P = eng.local_vol(seed, S0, R, surface, DT, n_steps, n_paths, path_begin=begin, q=Q)
        assert (P.n_paths, P.n_steps) == (n_paths, n_steps)
        got = host(P)
        e = float(np.abs(got / want - 1.0).max())
        observed["S"] = max(observed["S"], e)
        print(f"{name} {shape}: S {e:.2e}")
        assert (got[0] == S0).all()
        assert e <= S_BOUND, (name, shape, e)
        # the _payoff form: the same matrix, and the sums of its last row
        K, is_call = 100.0, k % 2 == 0
        F = eng.local_vol(seed, S0, R, surface, DT, n_steps, n_paths, path_begin=begin, q=Q, payoff=(K, is_call))
        m, se = eng.price_european(F, K, R, n_steps * DT, is_call)
        assert bits(host(F)) == bits(got), (name, shape, "payoff form")
        x = math.exp(-R * n_steps * DT) * (np.maximum(got[-1] - K, 0.0) if is_call else np.maximum(K - got[-1], 0.0))
        assert abs(m - x.mean()) <= 1e-12 * max(x.mean(), 1e-300), (name, shape, "fused price")
    if name == "narrow":      # most path-steps of the long shape sit on a clamp
        X = np.log(reference(name, SHAPES[-1])[1:] / S0)
        assert float(((X < NARROW.x_min) | (X > NARROW.x_max)).mean()) > 0.5


def test_bit_identities(eng):
    for name in ("skew-term", "wide-128", "cev"):
        surface = SURFACES[name]
        gen = dict(seed=SEED64, S0=S0, r=R, surface=surface, dt=DT, n_steps=27, q=Q)
        n, begin = 1301, 4097
        whole = host(eng.local_vol(n_paths=n, path_begin=begin, **gen))
        # three shards, an odd boundary and an empty one in the middle
        parts = []
        for first, count in ((0, 513), (513, 0), (513, 788)):
            part = eng.local_vol(n_paths=count, path_begin=begin + first, **gen)
            assert (part.n_paths, part.n_steps) == (count, 27)
            parts.append(host(part))
        assert bits(np.concatenate(parts, axis=1)) == bits(whole), name
        # again, after other work on the ctx, and in the _payoff form
        eng.gbm(5, 100.0, R, 0.3, DT, 7, 3000).free()
        eng.local_vol(5, S0, R, SURFACES["two-nodes"], DT, 9, 700).free()
        assert bits(host(eng.local_vol(n_paths=n, path_begin=begin, **gen))) == bits(whole), name
        assert bits(host(eng.local_vol(n_paths=n, path_begin=begin, payoff=(95.0, False), **gen))) == bits(whole), name
    # a one-slice surface and the same values given as two identical rows: the same arithmetic through the other kernel
    for surface in (CEV, SURFACES["two-nodes"], Surface([0.0], -2.0, 2.0, [WIDE_128.sigma[0]])):
        twice = Surface([0.0, 1.0], surface.x_min, surface.x_max, [surface.sigma[0], surface.sigma[0]])
        for n_steps, n_paths, begin, seed in SHAPES:
            one = host(eng.local_vol(seed, S0, R, surface, DT, n_steps, n_paths, path_begin=begin, q=Q))
            two = host(eng.local_vol(seed, S0, R, twice, DT, n_steps, n_paths, path_begin=begin, q=Q))
            assert bits(one) == bits(two), (surface.n_x, n_steps, n_paths)


def test_flat_surface_against_the_gbm_generators(eng):
    for n_steps, n_paths, begin, seed in SHAPES:
        for sigma in (0.2, 0.0, 1.5):    # (1.5 on daily steps: exponents beyond the exponential's small-argument shortcut)
            L = host(eng.local_vol(seed, S0, R, Surface.flat(sigma), DT, n_steps, n_paths, path_begin=begin))
            G = host(eng.gbm(seed, S0, R, sigma, DT, n_steps, n_paths, path_begin=begin))
            e = float(np.abs(L / G - 1.0).max())
            observed["flat against gbm"] = max(observed["flat against gbm"], e)
            Lq = host(eng.local_vol(seed, S0, R, Surface.flat(sigma), DT, n_steps, n_paths, path_begin=begin, q=0.02))
            assets, _ = eng.gbm_multi(seed, [S0], R, [sigma], [[1.0]], DT, n_steps, n_paths, path_begin=begin, q=[0.02])
            eq = float(np.abs(Lq / host(assets[0]) - 1.0).max())
            observed["flat against gbm_multi"] = max(observed["flat against gbm_multi"], eq)
            print(f"{n_steps} x {n_paths}, sigma {sigma}: against gbm {e:.2e}, against gbm_multi at q = 0.02 {eq:.2e}")
            assert e <= GBM_BOUND and eq <= GBM_BOUND, (n_steps, n_paths, sigma, e, eq)


def test_fused_sums(eng):
    n_steps, n_paths = 50, 100_003
    T = n_steps * 0.02
    gen = dict(seed=20251031, S0=S0, r=R, surface=SURFACES["skew-term"], dt=0.02, n_steps=n_steps, n_paths=n_paths, q=Q)
    P = eng.local_vol(**gen)
    for K, is_call in ((100.0, True), (100.0, False), (90.0, False)):
        want, want_se = eng.price_european(P, K, R, T, is_call)
        F = eng.local_vol(payoff=(K, is_call), **gen)
        got, got_se = eng.price_european(F, K, R, T, is_call)
        assert want > 0.0 and abs(got - want) <= 1e-12 * want and abs(got_se - want_se) <= 1e-9 * want_se, (K, is_call, got, want)
        assert bits(eng.price_european(F, K, R, T, is_call)) == bits((got, got_se))
        # the sums belong to their (K, is_call): any other payoff is summed afresh
        for K2, c2 in ((K, not is_call), (K + 5.0, is_call)):
            other, _ = eng.price_european(F, K2, R, T, c2)
            plain, _ = eng.price_european(P, K2, R, T, c2)
            assert other != got and abs(other - plain) <= 1e-12 * plain, (K, is_call, K2, c2)
        F.free()
    P.free()


def test_law_of_the_cev_surface(eng):
    P = eng.local_vol(STAT_SEED, S0, R, CEV, STAT_T / STAT_STEPS, STAT_STEPS, STAT_PATHS, q=Q)
    check_cev_prices(lambda K, is_call: eng.price_european(P, K, R, STAT_T, is_call), "MI355X, CEV")
    P.free()


def test_law_of_the_time_dependent_surface(eng):
    P = eng.local_vol(STAT_SEED, S0, R, TERM_STAT, STAT_T / STAT_STEPS, STAT_STEPS, STAT_PATHS, q=Q)
    check_term_prices(lambda K, is_call: eng.price_european(P, K, R, STAT_T, is_call), "MI355X, sigma(t)")
    P.free()


def test_consumers_and_launch_accounting(eng):
    n_steps, dt, n_paths = 50, 0.02, 100_003
    T = n_steps * dt
    eng.timing_enable(True)
    eng.timing_reset()
    P = eng.local_vol(20251031, S0, R, SURFACES["skew-term"], dt, n_steps, n_paths, q=Q)
    ms, launches = eng.timing_get(N.K_LOCALVOL)
    assert launches == 1 and ms > 0.0 and eng.timing_get(N.K_GBM)[1] == 0 and eng.timing_get(N.K_PAYOFF)[1] == 0
    eng.local_vol(20251031, S0, R, CEV, dt, n_steps, n_paths, q=Q, payoff=(100.0, False)).free()
    assert eng.timing_get(N.K_LOCALVOL)[1] == 2 and eng.timing_get(N.K_GBM)[1] == 0
    eng.timing_enable(False)
    X = P.to_host()
    assert (X[:, 0] == S0).all() and (X > 0.0).all()
    U = eng.from_host(X)
    book = [mc.exotic("barrier_down_out", False, 100.0, barrier=85.0), mc.exotic("asian_arith_fixed", True, 100.0)]
    (price, se), (uprice, use) = eng.price_exotics(P, R, T, book), eng.price_exotics(U, R, T, book)
    print(f"down-and-out put {price[0]:.4f} +- {se[0]:.4f}, arithmetic Asian call {price[1]:.4f} +- {se[1]:.4f}")
    assert (price > 0.0).all() and (np.abs(price - uprice) <= 1e-12 * uprice).all() and (np.abs(se - use) <= 1e-9 * use).all()
    lsm, ulsm = eng.price_lsm(P, R, 100.0, T, dt, False, 2), eng.price_lsm(U, R, 100.0, T, dt, False, 2)
    put, put_se = eng.price_european(P, 100.0, R, T, False)
    print(f"European put {put:.4f} +- {put_se:.4f}, LSM put {lsm[0]:.4f} +- {lsm[1]:.4f}")
    assert abs(lsm[0] - ulsm[0]) <= 1e-12 * ulsm[0] and lsm[0] >= put - 3.0 * put_se
    st, ust = eng.path_stats(P), eng.path_stats(U)
    assert (np.abs(st - ust) <= 1e-12 * np.abs(ust)).all()
    # a plain matrix for the Greeks: no rho (S_T is not proportional to e^{rT}), the rest as on any uploaded matrix
    g, ug = eng.greeks_european(P, 100.0, R, T, True), eng.greeks_european(U, 100.0, R, T, True)
    assert math.isnan(g["rho"]) and math.isnan(ug["rho"]) and abs(g["delta"] - ug["delta"]) <= 1e-12 * ug["delta"]
    P.free()
    U.free()


def test_empty_matrix_and_errors(eng):
    L = eng._L
    for payoff in (None, (100.0, True)):
        E = eng.local_vol(1, S0, R, SURFACES["skew-term"], DT, 8, 0, payoff=payoff)
        assert (E.n_paths, E.n_steps) == (0, 8) and E.to_host_step_major().shape == (9, 0)
        E.free()
        for change, message in BAD_SURFACES + BAD_MODELS:
            if "payoff" in change and payoff is None:
                continue
            rc, msg, h = raw_paths(eng._ctx, L, **dict(dict(payoff=payoff), **change))
            assert rc == 1 and message in msg and h is None, (change, rc, msg, h)
        rc, msg, _ = raw_paths(eng._ctx, L, payoff=payoff, with_out=False)
        assert rc == 1 and "out is NULL" in msg
        # ... and the ctx is as good as before
        rc, msg, h = raw_paths(eng._ctx, L, payoff=payoff)
        assert rc == 0 and h, msg
        L.mcg_paths_free(C.c_void_p(h))
    # the edges of the valid set: zero volatility (the forward, exactly in law), 64 knots, 128 nodes, one step
    Z = host(eng.local_vol(1, S0, R, Surface([0.0], -1.0, 1.0, [[0.0, 0.0]]), DT, 11, 700, q=Q))
    assert np.abs(Z[-1] / (S0 * math.exp((R - Q) * 11 * DT)) - 1.0).max() <= 1e-14
    many = Surface([0.001 * i for i in range(64)], -1.0, 1.0, [[0.2 + 0.001 * i] * 128 for i in range(64)])
    assert np.isfinite(host(eng.local_vol(1, S0, R, many, DT, 1, 513))).all()


def test_launch_frame(eng):
    """One launch under the generator's kernel id, the fused sums and their reuse (test_gpu_parity.check_launch_frame)."""
    from test_gpu_parity import FRAME_PATHS, FRAME_STEPS, check_launch_frame
    check_launch_frame(eng, N.K_LOCALVOL, lambda payoff: eng.local_vol(1, 100.0, R, CEV, DT, FRAME_STEPS, FRAME_PATHS, q=Q, payoff=payoff))
