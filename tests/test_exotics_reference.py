"""numpy reference of the path-dependent European payoffs (mcg_path_stats, mcg_price_exotics) -- the yardstick of
tests/test_gpu_exotics.py -- anchored on the discrete geometric Asian closed form and on exact identities, plus what the
library and the Python surface must answer without a GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N

GEO_KINDS = (N.X_ASIAN_GEO_FIXED, N.X_ASIAN_GEO_FLOAT)


def stats_numpy(X, first_row):
    """[5][n_paths] = S_T, A, G, min, max over the columns first_row .. n_steps of a path-major matrix X[n_paths][n_steps + 1]."""
    M = X[:, first_row:]
    return np.stack([X[:, -1], M.mean(axis=1), np.exp(np.log(M).mean(axis=1)), M.min(axis=1), M.max(axis=1)])


def payoff_numpy(st5, c):
    """Undiscounted per-path payoff of contract c = (kind, is_call, K, barrier, rebate): the definitions of include/mcgpu.h."""
    kind, call, K, barrier, rebate = c
    st, A, G, lo, hi = st5
    vanilla = np.maximum(st - K, 0.0) if call else np.maximum(K - st, 0.0)
    if kind in (N.X_ASIAN_ARITH_FIXED, N.X_ASIAN_GEO_FIXED):
        X = A if kind == N.X_ASIAN_ARITH_FIXED else G
        return np.maximum(X - K, 0.0) if call else np.maximum(K - X, 0.0)
    if kind in (N.X_ASIAN_ARITH_FLOAT, N.X_ASIAN_GEO_FLOAT):
        X = A if kind == N.X_ASIAN_ARITH_FLOAT else G
        return np.maximum(st - X, 0.0) if call else np.maximum(X - st, 0.0)
    if kind == N.X_LOOKBACK_FIXED:
        return np.maximum(hi - K, 0.0) if call else np.maximum(K - lo, 0.0)
    if kind == N.X_LOOKBACK_FLOAT:
        return st - lo if call else hi - st
    up = kind in (N.X_BARRIER_UP_OUT, N.X_BARRIER_UP_IN)
    knock_in = kind in (N.X_BARRIER_UP_IN, N.X_BARRIER_DOWN_IN)
    assert up or kind in (N.X_BARRIER_DOWN_OUT, N.X_BARRIER_DOWN_IN), kind
    hit = hi >= barrier if up else lo <= barrier
    return np.where(hit == knock_in, vanilla, rebate)


def price_numpy(st5, c, r, T):
    """(price, std error) of contract c: e^{-rT} mean and e^{-rT} std(ddof 1) / sqrt n (0 for one path)."""
    x = payoff_numpy(st5, c)
    n = len(x)
    D = math.exp(-r * T)
    return D * float(x.mean()), D * float(x.std(ddof=1) / math.sqrt(n)) if n > 1 else 0.0


def geo_asian_closed_form(S0, K, r, sigma, dt, n_steps, first_row, is_call):
    """Discrete geometric Asian under GBM, monitored at t_j = j dt, j = first_row .. n_steps, paid at T = n_steps dt:
    ln G ~ N(ln S0 + (r - sigma^2 / 2) mean(t_j), sigma^2 sum_{j,k} min(t_j, t_k) / N^2), priced Black-style."""
    t = dt * np.arange(first_row, n_steps + 1)
    mu = math.log(S0) + (r - 0.5 * sigma * sigma) * float(t.mean())
    var = sigma * sigma * float(np.minimum.outer(t, t).sum()) / len(t) ** 2
    sd = math.sqrt(var)
    Nc = lambda x: 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))  # noqa: E731
    d2 = (mu - math.log(K)) / sd
    d1 = d2 + sd
    D, F = math.exp(-r * n_steps * dt), math.exp(mu + 0.5 * var)
    return D * (F * Nc(d1) - K * Nc(d2)) if is_call else D * (K * Nc(-d2) - F * Nc(-d1))


def gbm_numpy(seed, S0, r, sigma, dt, n_steps, n_paths):
    z = np.random.default_rng(seed).standard_normal((n_paths, n_steps))
    X = np.empty((n_paths, n_steps + 1))
    X[:, 0] = S0
    X[:, 1:] = S0 * np.exp(np.cumsum((r - 0.5 * sigma * sigma) * dt + sigma * math.sqrt(dt) * z, axis=1))
    return X


@pytest.fixture(scope="module")
def sample():
    return gbm_numpy(20251031, 100.0, 0.04, 0.2, 0.02, 50, 400_000)


@pytest.mark.parametrize("first_row", [0, 1])
@pytest.mark.parametrize("is_call", [True, False])
def test_reference_against_the_geometric_asian_closed_form(sample, is_call, first_row):
    st5 = stats_numpy(sample, first_row)
    price, se = price_numpy(st5, (N.X_ASIAN_GEO_FIXED, is_call, 100.0, 0.0, 0.0), 0.04, 1.0)
    want = geo_asian_closed_form(100.0, 100.0, 0.04, 0.2, 0.02, 50, first_row, is_call)
    print(f"geometric Asian call={is_call} first_row={first_row}: {price:.6f} +- {se:.6f}, closed form {want:.6f}, "
          f"{abs(price - want) / se:.2f} std errors")
    assert abs(price - want) <= 4.0 * se, (price, want, se)


def test_reference_identities(sample):
    X = sample[:50_000]
    n_steps = X.shape[1] - 1
    st5 = stats_numpy(X, 1)
    for is_call in (True, False):
        vanilla = np.maximum(X[:, -1] - 95.0, 0.0) if is_call else np.maximum(95.0 - X[:, -1], 0.0)
        for k_in, k_out, level in ((N.X_BARRIER_UP_IN, N.X_BARRIER_UP_OUT, 115.0), (N.X_BARRIER_DOWN_IN, N.X_BARRIER_DOWN_OUT, 90.0)):
            both = payoff_numpy(st5, (k_in, is_call, 95.0, level, 0.0)) + payoff_numpy(st5, (k_out, is_call, 95.0, level, 0.0))
            assert np.array_equal(both, vanilla)          # in + out = vanilla, exactly, for rebate 0
            hit = payoff_numpy(st5, (k_in, is_call, 95.0, level, -1.0)) != -1.0
            assert 0.05 < hit.mean() < 0.95               # (both branches are exercised)
        last = stats_numpy(X, n_steps)
        for kind in (N.X_ASIAN_ARITH_FIXED, N.X_ASIAN_GEO_FIXED):
            got = payoff_numpy(last, (kind, is_call, 95.0, 0.0, 0.0))
            if kind == N.X_ASIAN_ARITH_FIXED:
                assert np.array_equal(got, vanilla)       # first_row = n_steps: the mean of one value is the value
            else:
                assert np.allclose(got, vanilla, rtol=0.0, atol=1e-11)  # exp(log x) is x to a few ulp
    # monitoring row 0 matters: S0 = 100 is the minimum of a path that only rises
    up = np.array([[100.0, 101.0, 103.0]])
    assert stats_numpy(up, 0)[3, 0] == 100.0 and stats_numpy(up, 1)[3, 0] == 101.0


def test_library_exports_and_rejects_without_a_gpu():
    L = mc.load_library()
    assert hasattr(L, "mcg_price_exotics") and hasattr(L, "mcg_path_stats")
    out = (C.c_double * 5)()
    assert L.mcg_path_stats(None, None, 1, out) != 0
    assert L.mcg_last_error()
    book = (N.Exotic * 1)(N.Exotic(N.X_LOOKBACK_FLOAT, 1, 0.0, 0.0, 0.0))
    assert L.mcg_price_exotics(None, None, 0.04, 1.0, 1, book, 1, out, None, None) != 0
    assert L.mcg_last_error()
    assert N.K_EXOTIC == 10 and N.KERNEL_NAMES[N.K_EXOTIC] == "exotic"


def test_exotic_helper():
    assert mc.exotic("barrier_up_out", True, 100.0, 120.0, 1.5) == (mc.X_BARRIER_UP_OUT, True, 100.0, 120.0, 1.5)
    assert mc.exotic(mc.X_ASIAN_GEO_FLOAT, False) == (3, False, 0.0, 0.0, 0.0)
    assert sorted(N.EXOTIC_KINDS.values()) == list(range(10))
    for bad in (-1, 10, "asian"):
        with pytest.raises(mc.McgError, match="unknown exotic kind"):
            mc.exotic(bad, True)
