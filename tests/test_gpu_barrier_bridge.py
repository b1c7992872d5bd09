"""mcg_barrier_survival / mcg_price_barriers_bridge on the device against the numpy restatement of
tests/test_barrier_bridge_reference.py, on the matrices the device itself made (downloaded) and on crafted ones.

Bounds (ten times the largest value measured on an MI355X over every case of this file; the run prints what it observes):
  P_BOUND      max |P_gpu - P_numpy| / E_p, E_p the elementwise bound of the restatement (the first-order effect of one-ulp
               errors in the logarithms, ln B and x_j; l - h cancels, so a flat relative bound would be wrong).  Where the
               restatement has P = 0 (E_p = 0) or P = 1 the device value is equal bit for bit.
  SUM_BOUND    |sum Y - numpy's| / sum |Y| and |sum Y^2 - numpy's| / sum Y^2 on the downloaded P and S_T; also the price in
               units of e^{-rT} mean |Y|
  SE_BOUND     the std error, relative, in units of max(1, 1/2 + (mean / std)^2) (its cancellation), as test_gpu_exotics.py
Measured: P 0.418 E_p, sums 3.74e-16, price 3.85e-16, std error 4.11e-16.
k_bridge_survival with MCG_BRIDGE_L_MAX = 8 levels in registers takes 147 VGPRs on the matrix route and 131 on the scalar
route, no private segment; its row group is MCG_BRIDGE_ROWS = 4.  tools/bench_barrier_bridge.py at 10M x 252 on an MI355X:
the survival pass on the scalar route 11.14 ms with 1 level and 26.19 ms with 8 near the spot, 9.26 / 12.73 ms with every
exponential skipped; matrix route 13.47 / 29.35 and 11.64 / 16.23 ms; k_path_tangent_stats with logarithms 9.88 ms in that run.
"""
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from test_barrier_bridge_reference import (IN_OF, TABLE, barrier_out_closed_form, level_of, price_bridge_numpy, sample_numpy,
                                           survival_numpy)

pytestmark = pytest.mark.gpu

LM, G = mc.BRIDGE_L_MAX, mc.BRIDGE_ROWS
P_BOUND = 4.2
SUM_BOUND = 3.9e-15
SE_BOUND = 4.2e-15
S0, R, SIGMA, T = 100.0, 0.05, 0.2, 1.0
HESTON = dict(v0=0.04, kappa=1.5, theta=0.04, sigma_v=0.5, rho=-0.7)
PATHS = (1, 2, 63, 64, 65, 127, 129, 511, 1000, 1003)
STEPS = (1, 2, G - 1, G, G + 1, 2 * G + 1, 50, 252)
LEVEL_COUNTS = (1, LM - 1, LM, LM + 1, 2 * LM + 3)
observed = {"P": 0.0, "sums": 0.0, "price": 0.0, "se": 0.0}


@pytest.fixture(scope="module")
def eng():
    with mc.PathEngine(0) as e:
        yield e


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest values in this run: |P - P_numpy| / E_p %.3f, sums %.2e, price %.2e, std error %.2e"
          % (observed["P"], observed["sums"], observed["price"], observed["se"]))


def bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


def first_rows(steps):
    return sorted({0, min(1, steps), max(steps - 1, 0), steps})


def levels_of(count):
    """count distinct levels about S0 = 100, down and up mixed, from near the spot outwards."""
    return [(100.0 + 2.5 * (k // 2 + 1), True) if k % 2 else (100.0 - 2.5 * (k // 2 + 1), False) for k in range(count)]


def book_of(levels, rebate=0.75):
    """Four contracts a level (out / in, call / put, strikes about the spot), walked twice in different orders: duplicates of
    every level stand apart in the book."""
    book = []
    for rnd in range(2):
        for k, (B, up) in (enumerate(levels) if rnd == 0 else reversed(list(enumerate(levels)))):
            out = N.X_BARRIER_UP_OUT if up else N.X_BARRIER_DOWN_OUT
            book.append((out if rnd == 0 else IN_OF[out], (k + rnd) % 2 == 0, 95.0 + 5.0 * (k % 3), B, rebate if k % 2 else 0.0))
            book.append((IN_OF[out] if rnd == 0 else out, (k + rnd) % 2 == 1, 100.0, B, -rebate if k % 3 == 0 else rebate))
    return book


def check_survival(eng, PM, X, dt, levels, first_row, where, sigma=None, VM=None, V=None):
    got = eng.barrier_survival(PM, levels, dt, sigma=sigma, var=VM, first_row=first_row)
    P, E, fragile = survival_numpy(X, levels, dt, sigma=sigma, V=V, first_row=first_row, full=True)
    assert got.shape == P.shape, where
    assert not fragile.any(), where           # (no path of the random cases sits one ulp from a barrier)
    assert np.isfinite(got).all() and (got >= 0.0).all() and (got <= 1.0).all(), where
    fixed = (P == 0.0) | (P == 1.0)
    assert np.array_equal(got[fixed], P[fixed]), (where, "P = 0 and P = 1 are exact")
    live = E > 0.0
    if live.any():
        ratio = float((np.abs(got - P)[live] / E[live]).max())
        observed["P"] = max(observed["P"], ratio)
        assert ratio <= P_BOUND, (where, ratio)
    return got


def check_prices(eng, PM, X, r, T, book, first_row, where, sigma=None, VM=None):
    """price_barriers_bridge against price_bridge_numpy on the device's own P (barrier_survival) and the downloaded S_T."""
    price, se, sums = eng.price_barriers_bridge(PM, r, T, book, sigma=sigma, var=VM, first_row=first_row, return_sums=True)
    distinct = list(dict.fromkeys(level_of(c) for c in book))
    P = eng.barrier_survival(PM, distinct, T / PM.n_steps, sigma=sigma, var=VM, first_row=first_row)
    st, n, D = X[:, -1], X.shape[0], math.exp(-r * T)
    assert sums.shape == (2 * len(book) + 1,) and sums[-1] == n, where
    for i, c in enumerate(book):
        p = P[distinct.index(level_of(c))]
        want, want_se, s1, s2 = price_bridge_numpy(st, p, c, r, T)
        y = sample_numpy(st, p, c)
        a1, mean_abs = float(np.abs(y).sum()), float(np.abs(y).mean())
        errs = [abs(sums[2 * i] - s1) / a1 if a1 else abs(sums[2 * i]), abs(sums[2 * i + 1] - s2) / s2 if s2 else abs(sums[2 * i + 1])]
        observed["sums"] = max(observed["sums"], *errs)
        assert max(errs) <= SUM_BOUND, (where, i, c, "sums", errs)
        ep = abs(price[i] - want) / (D * mean_abs) if mean_abs else abs(price[i])
        observed["price"] = max(observed["price"], ep)
        assert ep <= SUM_BOUND, (where, i, c, "price", price[i], want)
        if want_se > 0.0:
            es = abs(se[i] - want_se) / want_se / max(1.0, 0.5 + (want / want_se) ** 2 / n)
            observed["se"] = max(observed["se"], es)
            assert es <= SE_BOUND, (where, i, c, "std error", se[i], want_se)
        else:   # one path, or a constant sample: what rounding leaves of sum Y^2 - n m^2 is at most a few ulp of n m^2
            assert 0.0 <= se[i] <= 1e-7 * D * mean_abs, (where, i, c, se[i])
    return price, se, sums


# ---- elementwise -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_paths", PATHS)
def test_survival_on_gbm_matrices(eng, n_paths):
    for si, steps in enumerate(STEPS):
        dt = T / steps
        PM = eng.gbm(20260401 + steps, S0, R, SIGMA, dt, steps, n_paths)
        X = PM.to_host()
        # every first_row, the level counts in rotation; at 2 G + 1 steps every level count for every first_row
        for fi, first_row in enumerate(first_rows(steps)):
            counts = LEVEL_COUNTS if steps == 2 * G + 1 else (LEVEL_COUNTS[(si + fi) % len(LEVEL_COUNTS)],)
            for count in counts:
                check_survival(eng, PM, X, dt, levels_of(count), first_row, (n_paths, steps, first_row, count), sigma=SIGMA)
        PM.free()


@pytest.mark.parametrize("scheme", ["euler", "qe"])
def test_survival_on_heston_matrices_with_their_variances(eng, scheme):
    seen_negative = False
    for n_paths in (1, 65, 1003):
        for si, steps in enumerate((1, G + 1, 2 * G + 1, 50)):
            dt = T / steps
            PM, VM = eng.heston(7 + steps, S0, R, dt=dt, n_steps=steps, n_paths=n_paths, want_variance=True, scheme=scheme, **HESTON)
            X, V = PM.to_host(), VM.to_host()
            seen_negative = seen_negative or bool((V < 0.0).any())
            for fi, first_row in enumerate(first_rows(steps)):
                count = LEVEL_COUNTS[(si + fi + 1) % len(LEVEL_COUNTS)]
                check_survival(eng, PM, X, dt, levels_of(count), first_row, (scheme, n_paths, steps, first_row, count), VM=VM, V=V)
            if n_paths == 1003 and steps == 50:
                check_prices(eng, PM, X, R, T, book_of(levels_of(LM + 1)), 0, (scheme, "book"), VM=VM)
            PM.free()
            VM.free()
    assert seen_negative == (scheme == "euler")        # (Euler's untruncated variances exercise max(v, 0))


@pytest.mark.parametrize("count", LEVEL_COUNTS)
def test_prices_against_numpy(eng, count):
    for n_paths, steps in ((1, 2), (129, G + 1), (1003, 50)):
        PM = eng.gbm(20260402, S0, R, SIGMA, T / steps, steps, n_paths)
        X = PM.to_host()
        for first_row in (0, steps):
            check_prices(eng, PM, X, R, T, book_of(levels_of(count)), first_row, (count, n_paths, steps, first_row), sigma=SIGMA)
        PM.free()


# ---- crafted matrices ----------------------------------------------------------------------------------------------------------
def crafted(n_paths=200, steps=2 * G + 1, seed=5):
    z = np.random.default_rng(seed).standard_normal((n_paths, steps))
    X = np.empty((n_paths, steps + 1))
    X[:, 0] = S0
    X[:, 1:] = S0 * np.exp(np.cumsum(0.02 * z, axis=1))
    return X


def test_a_row_on_the_barrier_kills_the_path(eng):
    X = crafted()
    steps = X.shape[1] - 1
    dt = T / steps
    X = np.clip(X, 92.0, 108.0)                        # every path safe for the two levels ...
    hit_down, hit_up = [3, 64, 199], [0, 65, 130]
    for k, p in enumerate(hit_down):
        X[p, (0, steps // 2, steps)[k]] = 90.0         # ... but for a row that equals the barrier: first, middle and last row
    for k, p in enumerate(hit_up):
        X[p, (0, steps // 2, steps)[k]] = 110.0
    PM = eng.from_host(X)
    got = check_survival(eng, PM, X, dt, [(90.0, False), (110.0, True)], 0, "on the barrier", sigma=SIGMA)
    assert (got[0, hit_down] == 0.0).all() and (got[1, hit_up] == 0.0).all()
    others = np.setdiff1d(np.arange(len(X)), hit_down + hit_up)
    assert (got[:, others] > 0.0).all()
    PM.free()


def test_a_start_beyond_the_barrier_and_the_unmonitored_first_interval(eng):
    X = crafted()
    steps = X.shape[1] - 1
    dt = T / steps
    X[:, 0] = 80.0                                     # below the down level 90, above nothing
    X[:, 1:] = np.clip(X[:, 1:], 92.0, 108.0)
    PM = eng.from_host(X)
    lv = [(90.0, False)]
    got0 = check_survival(eng, PM, X, dt, lv, 0, "start beyond, first_row 0", sigma=SIGMA)
    got1 = check_survival(eng, PM, X, dt, lv, 1, "start beyond, first_row 1", sigma=SIGMA)
    assert (got0 == 0.0).all() and (got1 > 0.0).all()
    # first_row = 1 does not read row 0 at all
    X2 = X.copy()
    X2[:, 0] = 1e6
    P2 = eng.from_host(X2)
    assert bits(eng.barrier_survival(P2, lv, dt, sigma=SIGMA, first_row=1)) == bits(got1)
    PM.free()
    P2.free()


def test_a_far_barrier_is_never_hit_and_the_price_is_the_european_one(eng):
    for steps in (1, G, 50):
        PM = eng.gbm(11, S0, R, SIGMA, T / steps, steps, 1003)
        far = [(1e-3 * S0, False), (1e3 * S0, True)]
        got = eng.barrier_survival(PM, far, T / steps, sigma=SIGMA)
        assert (got == 1.0).all()
        book = [(N.X_BARRIER_DOWN_OUT, True, 100.0, far[0][0], 0.0), (N.X_BARRIER_UP_OUT, False, 105.0, far[1][0], 3.0),
                (N.X_BARRIER_UP_OUT, True, 95.0, far[1][0], 0.0)]
        price, se = eng.price_barriers_bridge(PM, R, T, book, sigma=SIGMA)
        for i, (_, call, K, _, _) in enumerate(book):
            want, want_se = eng.price_european(PM, K, R, T, call)
            assert abs(price[i] - want) <= 1e-13 * want and abs(se[i] - want_se) <= 1e-13 * want_se, (steps, i, price[i], want, se[i], want_se)
        PM.free()


def test_variance_rows_at_or_below_zero_contribute_no_factor(eng):
    X = crafted()
    steps = X.shape[1] - 1
    dt = T / steps
    X = np.clip(X, 92.0, 108.0)
    V = np.full(X.shape, SIGMA * SIGMA)
    V[:, 1], V[:, 4], V[:, steps - 1] = 0.0, -0.3, -0.0
    V[::3, 2] = 0.0
    PM, VM = eng.from_host(X), eng.from_host(V)
    lv = [(90.0, False), (110.0, True)]
    got = check_survival(eng, PM, X, dt, lv, 0, "zero variances", VM=VM, V=V)
    # the same without those intervals: the product over the rest, by the restatement on a matrix whose dead intervals are far
    d = [np.log(X) - math.log(B) for B, _ in lv]
    for k in range(2):
        want = np.ones(len(X))
        for j in range(steps):
            f = 1.0 - np.exp(np.maximum(d[k][:, j] * d[k][:, j + 1], 0.0) * (-2.0 / (SIGMA * SIGMA * dt)))
            want = want * np.where(V[:, j] > 0.0, f, 1.0)
        assert np.allclose(got[k], want, rtol=1e-9, atol=0.0) and (got[k] > 0.0).all()
    # an all-zero variance matrix: the safe indicator
    Z = eng.from_host(np.zeros(X.shape))
    assert (eng.barrier_survival(PM, lv, dt, var=Z) == 1.0).all()
    for M in (PM, VM, Z):
        M.free()


def test_a_row_one_ulp_on_the_safe_side(eng):
    X = crafted()
    steps = X.shape[1] - 1
    X = np.clip(X, 92.0, 108.0)
    rows = (0, 1, steps // 2, steps)
    for k, j in enumerate(rows):
        X[k, j] = np.nextafter(90.0, 100.0)
        X[10 + k, j] = np.nextafter(110.0, 100.0)
    PM = eng.from_host(X)
    got = eng.barrier_survival(PM, [(90.0, False), (110.0, True)], T / steps, sigma=SIGMA)
    near = np.concatenate([got[0, :4], got[1, 10:14]])
    assert np.isfinite(near).all() and (near >= 0.0).all() and (near <= 1e-6).all(), near
    # every other path is within the bound (these eight are the only ones left out)
    P, E, fragile = survival_numpy(X, [(90.0, False), (110.0, True)], T / steps, sigma=SIGMA, full=True)
    keep = np.ones(P.shape, dtype=bool)
    keep[0, :4] = keep[1, 10:14] = False
    assert not fragile[keep].any() and (np.abs(got - P)[keep] <= P_BOUND * E[keep]).all()
    PM.free()


# ---- the skipped exponentials ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("column", [0, 37, 63])
def test_the_skip_changes_no_bit(eng, column):
    steps = 2 * G + 1
    dt = T / steps
    near = crafted(1, steps, seed=9)[0]                 # within a few per cent of the levels 97.5 and 102.5
    far_down, far_up = np.full(steps + 1, 1000.0), np.full(steps + 1, 10.0)
    lv = levels_of(LM)
    P1 = eng.from_host(near[None, :])
    alone = eng.barrier_survival(P1, lv, dt, sigma=SIGMA)[:, 0]
    assert ((alone > 0.0) & (alone < 1.0)).any()
    copies = eng.from_host(np.tile(near, (64, 1)))
    assert bits(eng.barrier_survival(copies, lv, dt, sigma=SIGMA)[:, column]) == bits(alone)
    for far, levels in ((far_down, [l for l in lv if not l[1]]), (far_up, [l for l in lv if l[1]])):
        M = np.tile(far, (64, 1))
        M[column] = near
        PM = eng.from_host(M)
        got = eng.barrier_survival(PM, levels, dt, sigma=SIGMA)
        want = alone[[lv.index(l) for l in levels]]
        assert bits(got[:, column]) == bits(want)
        rest = np.delete(got, column, axis=1)
        assert (rest == 1.0).all()                      # every exponential of the 63 far paths is beyond the threshold
        PM.free()
    P1.free()
    copies.free()


# ---- bit-identity ------------------------------------------------------------------------------------------------------------
def test_repeats_positions_and_groups_are_bit_identical(eng):
    steps, n = 50, 1003
    PM = eng.gbm(3, S0, R, SIGMA, T / steps, steps, n)
    lv = levels_of(2 * LM + 3)
    full = eng.barrier_survival(PM, lv, T / steps, sigma=SIGMA)
    assert bits(eng.barrier_survival(PM, lv, T / steps, sigma=SIGMA)) == bits(full)
    for k in (0, LM - 1, LM, 2 * LM + 2):               # a level alone, and at another slot of another group
        assert bits(eng.barrier_survival(PM, [lv[k]], T / steps, sigma=SIGMA)[0]) == bits(full[k])
        assert bits(eng.barrier_survival(PM, lv[:3] + [lv[k]], T / steps, sigma=SIGMA)[3]) == bits(full[k])
    book = book_of(lv)
    price, se, sums = eng.price_barriers_bridge(PM, R, T, book, sigma=SIGMA, return_sums=True)
    again = eng.price_barriers_bridge(PM, R, T, book, sigma=SIGMA, return_sums=True)
    assert all(bits(a) == bits(b) for a, b in zip(again, (price, se, sums)))
    for i in (0, 1, len(book) // 2, len(book) - 1):     # a contract alone and among 2 L_MAX + 3 levels
        p1, s1, u1 = eng.price_barriers_bridge(PM, R, T, [book[i]], sigma=SIGMA, return_sums=True)
        assert (p1[0], s1[0]) == (price[i], se[i]) and bits(u1[:2]) == bits(sums[2 * i:2 * i + 2]), i
    # any position in a 1024-contract book
    big = (book * (1024 // len(book) + 1))[:1024]
    c = (N.X_BARRIER_DOWN_OUT, False, 101.0, 93.25, 0.5)
    alone = eng.price_barriers_bridge(PM, R, T, [c], sigma=SIGMA, return_sums=True)
    for pos in (0, 7, 8, 500, 1023):
        bk = list(big)
        bk[pos] = c
        p, s, u = eng.price_barriers_bridge(PM, R, T, bk, sigma=SIGMA, return_sums=True)
        assert (p[pos], s[pos]) == (alone[0][0], alone[1][0]) and bits(u[2 * pos:2 * pos + 2]) == bits(alone[2][:2]), pos
        other = (pos + 1) % 1024
        assert p[other] == eng.price_barriers_bridge(PM, R, T, [bk[other]], sigma=SIGMA)[0][0]
    PM.free()


def test_the_scalar_route_is_the_matrix_route_on_a_constant_matrix(eng):
    for n, steps in ((129, G + 1), (1003, 50)):
        PM = eng.gbm(4, S0, R, SIGMA, T / steps, steps, n)
        VM = eng.from_host(np.full((n, steps + 1), SIGMA * SIGMA))
        lv = levels_of(LM + 1)
        for first_row in (0, 1):
            a = eng.barrier_survival(PM, lv, T / steps, sigma=SIGMA, first_row=first_row)
            b = eng.barrier_survival(PM, lv, T / steps, var=VM, first_row=first_row)
            assert bits(a) == bits(b) and ((a > 0.0) & (a < 1.0)).any()
        book = book_of(lv)
        assert all(bits(x) == bits(y) for x, y in zip(eng.price_barriers_bridge(PM, R, T, book, sigma=SIGMA, return_sums=True),
                                                      eng.price_barriers_bridge(PM, R, T, book, var=VM, return_sums=True)))
        PM.free()
        VM.free()


def test_shards_and_an_identity_collective(eng):
    steps, n = 50, 1003
    gen = (6, S0, R, SIGMA, T / steps, steps)
    lv = levels_of(LM + 1)
    book = book_of(lv)
    PM = eng.gbm(*gen, n)
    whole = eng.barrier_survival(PM, lv, T / steps, sigma=SIGMA)
    price, se, sums = eng.price_barriers_bridge(PM, R, T, book, sigma=SIGMA, return_sums=True)
    cuts = [0, 1, 256, 511, n]
    total = np.zeros_like(sums)
    for a, b in zip(cuts[:-1], cuts[1:]):
        S = eng.gbm(*gen, b - a, path_begin=a)
        assert bits(eng.barrier_survival(S, lv, T / steps, sigma=SIGMA)) == bits(whole[:, a:b]), (a, b)
        total += eng.price_barriers_bridge(S, R, T, book, sigma=SIGMA, return_sums=True)[2]
        S.free()
    assert total[-1] == n
    for i in range(len(book)):                          # (sum Y may cancel under a negative rebate: its scale is sqrt(n sum Y^2))
        assert abs(total[2 * i] - sums[2 * i]) <= 1e-13 * math.sqrt(n * sums[2 * i + 1]), i
        assert abs(total[2 * i + 1] - sums[2 * i + 1]) <= 1e-13 * sums[2 * i + 1], i
    calls = []
    with mc.PathEngine(0) as ident:
        ident.set_allreduce(lambda ptr, count, stream: calls.append(count))   # world size 1: the sum over ranks is the identity
        Q = ident.gbm(*gen, n)
        got = ident.price_barriers_bridge(Q, R, T, book, sigma=SIGMA, return_sums=True)
        assert calls == [2 * len(book) + 1]
        assert all(bits(x) == bits(y) for x, y in zip(got, (price, se, sums)))
        E = ident.gbm(*gen, 0)                          # an empty shard still takes part: the sums are all zero, n = 0
        with pytest.raises(mc.McgError) as e:
            ident.price_barriers_bridge(E, R, T, book, sigma=SIGMA)
        assert e.value.status == 6 and len(calls) == 2
    PM.free()


# ---- agreement with the existing pricers ---------------------------------------------------------------------------------------
def test_sigma_zero_is_the_discrete_pricer_and_the_bridge_only_removes_survivors(eng):
    steps, n = 12, 20_000
    PM = eng.gbm(8, S0, R, SIGMA, T / steps, steps, n)
    lv = levels_of(LM + 1)
    book = book_of(lv)
    for first_row in (0, 1, steps):
        want, want_se = eng.price_exotics(PM, R, T, book, first_row=first_row)
        got, got_se = eng.price_barriers_bridge(PM, R, T, book, sigma=0.0, first_row=first_row)
        assert (np.abs(got - want) <= 1e-13 * np.abs(want)).all() and (np.abs(got_se - want_se) <= 1e-13 * np.abs(want_se)).all(), first_row
    plain = [(k, call, K, B, 0.0) for k, call, K, B, _ in book]
    dis, _ = eng.price_exotics(PM, R, T, plain, first_row=0)
    bri, _ = eng.price_barriers_bridge(PM, R, T, plain, sigma=SIGMA)
    for i, c in enumerate(plain):
        if c[0] in (N.X_BARRIER_UP_OUT, N.X_BARRIER_DOWN_OUT):
            assert bri[i] <= dis[i], (i, c, bri[i], dis[i])
        else:
            assert bri[i] >= dis[i], (i, c, bri[i], dis[i])
    assert (bri != dis).any()
    PM.free()


# ---- statistics --------------------------------------------------------------------------------------------------------------
def test_closed_forms_at_twelve_steps(eng):
    steps, n = 12, 1_000_000
    PM = eng.gbm(20260403, S0, R, SIGMA, T / steps, steps, n)
    book = [(kind, call, K, B, 0.0) for kind, call, K, B, _ in TABLE]
    bri, bri_se = eng.price_barriers_bridge(PM, R, T, book, sigma=SIGMA)
    dis, dis_se = eng.price_exotics(PM, R, T, book, first_row=0)
    for i, (kind, call, K, B, _) in enumerate(TABLE):
        cf = barrier_out_closed_form(S0, K, B, R, SIGMA, T, call, kind == N.X_BARRIER_UP_OUT)
        print(f"out kind {kind} call={call} K={K} B={B}: closed form {cf:.4f}, bridge {bri[i]:.4f} ({(bri[i] - cf) / bri_se[i]:+.1f} se), "
              f"discrete {dis[i]:.4f} ({(dis[i] - cf) / dis_se[i]:+.1f} se)")
        assert abs(bri[i] - cf) <= 4.0 * bri_se[i], (i, bri[i], cf, bri_se[i])
        assert abs(dis[i] - cf) > 10.0 * dis_se[i], (i, dis[i], cf, dis_se[i])
    PM.free()


def test_heston_qe_down_and_out_put_by_step_count(eng):
    """Not asserted beyond finiteness: the figures quoted in README.md (the bridge price should move little with the step count,
    the discrete price sits above both)."""
    c = [(N.X_BARRIER_DOWN_OUT, False, 100.0, 85.0, 0.0)]
    out = {}
    for steps in (50, 400):
        PM, VM = eng.heston(20260404, S0, R, dt=T / steps, n_steps=steps, n_paths=400_000, want_variance=True, scheme="qe", **HESTON)
        out[steps] = eng.price_barriers_bridge(PM, R, T, c, var=VM)
        if steps == 50:
            out["discrete"] = eng.price_exotics(PM, R, T, c, first_row=0)
        PM.free()
        VM.free()
    print("Heston QE, rho = -0.7, down-and-out put K = 100, B = 85, 400 000 paths: " +
          ", ".join(f"{k}: {v[0][0]:.4f} +- {v[1][0]:.4f}" for k, v in (("bridge, 50 steps", out[50]), ("bridge, 400 steps", out[400]),
                                                                       ("discrete, 50 steps", out["discrete"]))))
    assert all(np.isfinite(v[0]).all() and np.isfinite(v[1]).all() for v in out.values())


# ---- errors and accounting -------------------------------------------------------------------------------------------------------
def test_errors(eng):
    steps = 4
    PM = eng.gbm(5, S0, R, SIGMA, T / steps, steps, 300)
    VM = eng.from_host(np.full((300, steps + 1), 0.04))
    one = [(N.X_BARRIER_DOWN_OUT, True, 100.0, 90.0, 0.0)]
    lv = [(90.0, False)]
    nan, inf = float("nan"), float("inf")
    flat = eng.from_host(np.full((300, 1), 100.0))                     # a matrix without a step
    bad_shapes = [eng.from_host(np.full((299, steps + 1), 0.04)), eng.from_host(np.full((300, steps), 0.04))]
    price = lambda **kw: eng.price_barriers_bridge(**{**dict(paths=PM, r=R, T=T, book=one, sigma=SIGMA), **kw})       # noqa: E731
    surv = lambda **kw: eng.barrier_survival(**{**dict(paths=PM, levels=lv, dt=T / steps, sigma=SIGMA), **kw})       # noqa: E731
    cases = [(lambda: price(book=[]), "n_contracts"), (lambda: price(book=one * 1025), "n_contracts"),
             (lambda: price(first_row=-1), "first_row"), (lambda: price(first_row=steps + 1), "first_row"),
             (lambda: surv(first_row=-1), "first_row"), (lambda: surv(first_row=steps + 1), "first_row"),
             (lambda: surv(levels=[]), "n_levels"), (lambda: surv(levels=lv * 1025), "n_levels"),
             (lambda: price(book=[(N.X_BARRIER_UP_IN, True, nan, 110.0, 0.0)]), "K must be finite"),
             (lambda: price(book=[(N.X_BARRIER_UP_IN, True, 100.0, nan, 0.0)]), "barrier must be finite"),
             (lambda: price(book=[(N.X_BARRIER_UP_IN, True, 100.0, inf, 0.0)]), "barrier must be finite"),
             (lambda: price(book=[(N.X_BARRIER_UP_IN, True, 100.0, 110.0, nan)]), "rebate must be finite"),
             (lambda: price(book=one + [(N.X_BARRIER_UP_IN, True, 100.0, 0.0, 0.0)]), "contract 1: barrier must be positive"),
             (lambda: price(book=[(N.X_BARRIER_DOWN_OUT, True, 100.0, -90.0, 0.0)]), "barrier must be positive"),
             (lambda: surv(levels=[(90.0, False), (0.0, True)]), "level 1: barrier must be positive"),
             (lambda: surv(levels=[(-1.0, False)]), "barrier must be positive"), (lambda: surv(levels=[(inf, True)]), "barrier must be finite"),
             (lambda: surv(levels=[(nan, True)]), "barrier must be finite"),
             (lambda: price(sigma=-0.1), "sigma must be finite and non-negative"), (lambda: price(sigma=nan), "sigma must be"),
             (lambda: price(sigma=inf), "sigma must be"), (lambda: surv(sigma=-0.1), "sigma must be"), (lambda: surv(sigma=nan), "sigma must be"),
             (lambda: price(r=nan), "r and T must be finite"), (lambda: price(T=inf), "r and T must be finite"),
             (lambda: price(T=0.0), "T must be positive"), (lambda: price(T=-1.0), "T must be positive"),
             (lambda: price(T=5e-324), "dt must be finite and positive"),
             (lambda: surv(dt=0.0), "dt must be"), (lambda: surv(dt=-0.01), "dt must be"), (lambda: surv(dt=nan), "dt must be"),
             (lambda: surv(dt=inf), "dt must be"), (lambda: surv(dt=0.0, sigma=None, var=VM), "dt must be"),
             (lambda: price(paths=flat), "at least one step"), (lambda: surv(paths=flat), "at least one step")]
    cases += [(lambda k=k: price(book=[(k, True, 100.0, 90.0, 0.0)]), "kind must be a barrier kind") for k in (-1, 0, 5, 10)]
    for V in bad_shapes:
        cases += [(lambda V=V: price(sigma=None, var=V), "var must have the shape"), (lambda V=V: surv(sigma=None, var=V), "var must have the shape")]
    for call, message in cases:
        with pytest.raises(mc.McgError, match=message) as e:
            call()
        assert e.value.status == 1, message
    with mc.PathEngine(0) as other:
        foreign = other.from_host(np.full((300, steps + 1), 0.04))
        for call in (lambda: price(sigma=None, var=foreign), lambda: surv(sigma=None, var=foreign)):
            with pytest.raises(mc.McgError, match="var belongs to a different ctx") as e:
                call()
            assert e.value.status == 1
        for call in (lambda: other.price_barriers_bridge(PM, R, T, one, sigma=SIGMA), lambda: other.barrier_survival(PM, lv, T / steps, sigma=SIGMA)):
            with pytest.raises(mc.McgError, match="different ctx"):
                call()
    E = eng.gbm(5, S0, R, SIGMA, T / steps, steps, 0)
    for call in (lambda: price(paths=E), lambda: surv(paths=E)):
        with pytest.raises(mc.McgError) as e:
            call()
        assert e.value.status == 6
    for call in (lambda: price(var=VM), lambda: price(sigma=None), lambda: surv(var=VM), lambda: surv(sigma=None),
                 lambda: price(sigma=None, var=np.zeros((300, steps + 1)))):
        with pytest.raises(ValueError):
            call()
    # the limits themselves are accepted; sigma is not read on the matrix route; with var the price is what sigma gives
    assert price(book=one * 1024)[0].shape == (1024,) and surv(levels=lv * 1024).shape == (1024, 300)
    assert bits(price(sigma=None, var=VM)[0]) == bits(price(sigma=0.2)[0])
    for M in [PM, VM, flat, E] + bad_shapes:
        M.free()


def test_launch_accounting(eng):
    steps = 4
    PM = eng.gbm(1, S0, R, SIGMA, T / steps, steps, 10_000)
    eng.timing_enable(True)
    eng.timing_reset()
    eng.price_barriers_bridge(PM, R, T, book_of(levels_of(1)), sigma=SIGMA)
    ms, launches = eng.timing_get(N.K_EXOTIC)
    assert launches == 3 and ms > 0.0                   # survival, book, reduction
    eng.timing_reset()
    eng.price_barriers_bridge(PM, R, T, book_of(levels_of(2 * LM + 3)), sigma=SIGMA)
    assert eng.timing_get(N.K_EXOTIC)[1] == 2 * 3 + 1   # three groups: survival and book each, one reduction
    eng.timing_reset()
    eng.barrier_survival(PM, levels_of(LM + 1), T / steps, sigma=SIGMA)
    assert eng.timing_get(N.K_EXOTIC)[1] == 2
    eng.timing_enable(False)
    PM.free()
