"""Greeks of the exotics book on the GPU (mcg_path_tangent_stats, mcg_greeks_exotics) against the numpy restatement of
tests/test_exotic_greeks_reference.py: the ten statistics against tangent_stats_np on the matrix downloaded from the device,
the Greeks against exotic_greeks_np fed the library's own statistics and rows 0 and 1, and the laws of the CPU file (closed
forms within 4 standard errors) through the library.

Bounds.  Statistics: S_T, A, G, min, max bit-identical to mcg_path_stats; the rows of the first minimum and maximum exact; L and
J within (N + 16) 2^-52 mean|term| over the N monitoring rows (N roundings of a sum and a logarithm good to a few ulp, twice
over for the two sides); Q within 8 2^-52 (max|ln S| sum|y_i| + n_steps Q) (each difference of logarithms carries two
roundings of size 2^-53 max|ln S|, the sum n_steps more).  Greeks: every field and standard error within 1e-12 mean|per-path
sample|, the bound the European Greeks carry; the price within 1e-13 relative of mcg_price_exotics.
mcg_paths_from_host pads every row to 256 columns on an aligned base, so no matrix it makes leaves the 16-byte route: that
route's one-path-per-lane sibling is the same scan at W = 1, which the lone last path of every odd count runs."""
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from test_exotic_greeks_reference import (FIELDS, black_scholes, check_against, differences_of, exotic_greeks_np, geo_price,
                                          tangent_stats_np, up_out_call_one_step)

pytestmark = pytest.mark.gpu

SEED = 20251031
U = 2.0 ** -52
S0, R, SIGMA, T = 100.0, 0.04, 0.2, 1.0
FIELD_BOUND = 1e-12
ALL_FIELDS = tuple(FIELDS) + tuple(k + "_se" for k in FIELDS)
observed = {"L": 0.0, "J": 0.0, "Q": 0.0, "field": 0.0}


@pytest.fixture(scope="module")
def eng():
    with mc.PathEngine(0) as e:
        yield e


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest error over its bound in this run: " + ", ".join(f"{k} {v:.3f}" for k, v in observed.items()))


def bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


def greeks_bits(gs):
    return bits([[g[k] for k in ALL_FIELDS] for g in gs])


def check_tangent_stats(eng, P, X, first_row, where):
    got = eng.path_tangent_stats(P, first_row)
    assert got.shape == (10, X.shape[0]), where
    assert bits(got[:5]) == bits(eng.path_stats(P, first_row)), where
    with np.errstate(divide="ignore", invalid="ignore"):
        want = tangent_stats_np(X, first_row)
        M, lnX = X[:, first_row:], np.log(X)
    n_rows, n_steps = M.shape[1], X.shape[1] - 1
    j = np.arange(first_row, n_steps + 1, dtype=np.float64)
    assert np.array_equal(got[7], want[7]) and np.array_equal(got[8], want[8]), where
    bound = {5: (n_rows + 16) * U * np.abs(M * lnX[:, first_row:]).mean(axis=1), 6: (n_rows + 16) * U * np.abs(j * M).mean(axis=1),
             9: 8 * U * (np.abs(lnX).max(axis=1) * np.abs(np.diff(lnX, axis=1)).sum(axis=1) + n_steps * want[9])}
    for q, name in ((5, "L"), (6, "J"), (9, "Q")):
        err = np.abs(got[q] - want[q])
        worst = float(np.max(np.where(err > 0.0, err / np.where(bound[q] > 0.0, bound[q], 1.0), 0.0)))
        print(f"{where}: {name} error / bound {worst:.3f}")
        observed[name] = max(observed[name], worst)
        assert (err <= bound[q]).all(), (where, name, worst)
    off = eng.path_tangent_stats(P, first_row, with_logs=False)
    assert np.isnan(off[5]).all() and np.isnan(off[9]).all(), where
    keep = [0, 1, 2, 3, 4, 6, 7, 8]
    assert bits(off[keep]) == bits(got[keep]), where


def first_rows(n_steps):
    return sorted({0, 1, (n_steps + 1) // 2, n_steps})


@pytest.mark.parametrize("n_paths", [1, 2, 63, 64, 65, 255, 257, 513, 1001])
def test_tangent_statistics_against_numpy(eng, n_paths):
    for n_steps in (1, 2, 7, 8, 9, 15, 16, 17, 33):
        for name, P in (("gbm", eng.gbm(SEED + n_steps, S0, R, SIGMA, T / n_steps, n_steps, n_paths)),
                        ("heston", eng.heston(SEED + n_steps, S0, R, 0.04, 1.5, 0.04, 0.5, -0.7, T / n_steps, n_steps, n_paths))):
            X = P.to_host()
            for first_row in first_rows(n_steps):
                check_tangent_stats(eng, P, X, first_row, (name, n_paths, n_steps, first_row))
            P.free()


def test_tangent_statistics_with_ties(eng):
    """Exact ties in the minimum and the maximum: paths that do not move (sigma = 0 rows) and paths over a handful of values."""
    rng = np.random.default_rng(7)
    for n_steps in (7, 17, 33):
        X = 10.0 * rng.integers(1, 5, size=(259, n_steps + 1)).astype(np.float64)
        X[::5] = X[::5, :1]                       # constant paths: every row ties
        X[1, :] = 20.0
        X[1, [3, n_steps]] = 40.0                 # the maximum twice, the second time in the last row
        X[2, :] = 30.0
        X[2, [2, 5]] = 10.0                       # the minimum twice within one group of rows
        P = eng.from_host(X)
        for first_row in first_rows(n_steps):
            check_tangent_stats(eng, P, X, first_row, ("ties", n_steps, first_row))
        got = eng.path_tangent_stats(P, 1)
        assert got[8, 1] == 3.0 and got[7, 2] == 2.0 and got[7, 0] == 1.0 and got[8, 0] == 1.0
        assert eng.path_tangent_stats(P, 4)[8, 1] == float(n_steps) and eng.path_tangent_stats(P, 3)[7, 2] == 5.0
        P.free()


def every_kind(st10, n_contracts):
    """n_contracts contracts, kinds and call / put in turn; strikes around the median of S_T, barriers that part of the paths hit."""
    k0 = float(np.median(st10[0]))
    up, down = np.quantile(st10[4], [0.3, 0.6, 0.9]), np.quantile(st10[3], [0.1, 0.4, 0.7])
    book = []
    for i in range(n_contracts):
        kind, call = i % 10, (i // 10) % 2 == 0
        f = ((i * 7919) % 997) / 997.0
        barrier = float(up[i % 3]) if kind in (N.X_BARRIER_UP_OUT, N.X_BARRIER_UP_IN) else float(down[i % 3])
        book.append((kind, call, k0 * (0.9 + 0.2 * f), barrier * (1.0 + 1e-3 * f), 0.25 + f))
    return book


def check_greeks(eng, P, book, r, q, sigma, T, first_row, where, X, generated=True):
    st10 = eng.path_tangent_stats(P, first_row, with_logs=sigma > 0.0)
    got = eng.greeks_exotics(P, r, T, book, sigma=sigma, q=q, first_row=first_row)
    price, _ = eng.price_exotics(P, r, T, book, first_row=first_row)
    assert len(got) == len(book)
    for i, c in enumerate(book):
        want, scale = exotic_greeks_np(st10, X[:, 0], X[:, 1], c, r, q, sigma, T, P.n_steps, first_row, generated=generated)
        for k in FIELDS:
            for kk in (k, k + "_se"):
                assert math.isnan(got[i][kk]) == math.isnan(want[kk]), (where, i, c, kk, got[i][kk], want[kk])
                if math.isnan(want[kk]):
                    continue
                err, tol = abs(got[i][kk] - want[kk]), FIELD_BOUND * scale[k]
                if err > 0.0:
                    observed["field"] = max(observed["field"], err / tol if tol > 0.0 else math.inf)
                assert err <= tol, (where, i, c, kk, got[i][kk], want[kk], err, tol)
        assert abs(got[i]["price"] - price[i]) <= 1e-13 * abs(price[i]), (where, i, c)
    return got


@pytest.mark.parametrize("n_contracts", [1, 7, 8, 9, 1024])
def test_every_kind_against_numpy(eng, n_contracts):
    P = eng.gbm(SEED, S0, R, SIGMA, T / 12, 12, 20_001)
    X = P.to_host()
    st10 = eng.path_tangent_stats(P, 1)
    if n_contracts >= 20:
        check_greeks(eng, P, every_kind(st10, n_contracts), R, 0.0, SIGMA, T, 1, ("book", n_contracts), X)
    else:  # every window of the twenty kind x call / put pairs at this book size
        twenty = every_kind(st10, 20)
        for at in range(0, 20, n_contracts):
            check_greeks(eng, P, (twenty + twenty)[at:at + n_contracts], R, 0.0, SIGMA, T, 1, ("book", n_contracts, at), X)
    P.free()


def nan_fields(g):
    return {k for k in ALL_FIELDS if math.isnan(g[k])}


def both(*names):
    return {k for n in names for k in (n, n + "_se")}


def test_nan_pattern(eng):
    asian, floating, barrier = (0, True, 100.0, 0.0, 0.0), (5, False, 0.0, 0.0, 0.0), (8, False, 100.0, 90.0, 1.0)
    book = [asian, floating, barrier]
    P = eng.gbm(SEED, S0, R, SIGMA, T / 9, 9, 5003)
    X = P.to_host()
    rest = both("delta", "gamma", "vega", "rho")
    for sigma, first_row, want in ((SIGMA, 1, [set(), set(), set()]),
                                   (0.0, 1, [both("gamma", "vega"), both("vega"), rest]),
                                   (-1.0, 1, [both("gamma", "vega"), both("vega"), rest]),
                                   (SIGMA, 0, [both("gamma"), set(), rest])):
        got = check_greeks(eng, P, book, R, 0.0, sigma, T, first_row, ("nan", sigma, first_row), X)
        assert [nan_fields(g) for g in got] == want, (sigma, first_row)
        assert got[1]["gamma"] == 0.0 and got[1]["gamma_se"] == 0.0 and got[1]["dual_delta"] == 0.0 and got[1]["dual_delta_se"] == 0.0
    P.free()
    H = eng.from_host(X)              # no `generated` mark: no pathwise rho
    got = check_greeks(eng, H, book, R, 0.0, SIGMA, T, 1, "from_host", X, generated=False)
    assert [nan_fields(g) for g in got] == [both("rho"), both("rho"), set()]
    H.free()
    Y = X.copy()
    Y[17, 0] = 99.0                   # row 0 is not one constant
    H = eng.from_host(Y)
    got = check_greeks(eng, H, book, R, 0.0, SIGMA, T, 1, "non-constant row 0", Y, generated=False)
    assert [nan_fields(g) for g in got] == [both("delta", "gamma", "rho"), both("delta", "gamma", "rho"), rest]
    H.free()


@pytest.mark.parametrize("is_call", [True, False])
def test_one_step_arithmetic_asian_is_the_european(eng, is_call):
    P = eng.gbm(SEED, S0, R, SIGMA, T, 1, 100_003)
    for K in (95.0, 100.0, 107.0):
        got = eng.greeks_exotics(P, R, T, [(N.X_ASIAN_ARITH_FIXED, is_call, K, 0.0, 0.0)], sigma=SIGMA)[0]
        want = eng.greeks_european(P, K, R, T, is_call, sigma=SIGMA)
        for k in ALL_FIELDS:
            assert math.isfinite(want[k]) and abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (K, k, got[k], want[k])
    P.free()


PICKS = (0, 1, 2, 3, 14, 25, 106, 339, 517, 1016, 1018, 1023)   # every kind, every slot of a chunk of the book kernel


def test_determinism_and_book_independence(eng):
    P = eng.gbm(SEED, S0, R, SIGMA, T / 12, 12, 20_001)
    book = every_kind(eng.path_tangent_stats(P, 1), 1024)
    got = eng.greeks_exotics(P, R, T, book, sigma=SIGMA)
    assert greeks_bits(eng.greeks_exotics(P, R, T, book, sigma=SIGMA)) == greeks_bits(got)
    assert greeks_bits(eng.greeks_exotics(P, R, T, book[::-1], sigma=SIGMA)[::-1]) == greeks_bits(got)
    for i in PICKS:
        assert greeks_bits(eng.greeks_exotics(P, R, T, [book[i]], sigma=SIGMA)) == greeks_bits(got[i:i + 1]), i
    assert {book[i][0] for i in PICKS} == set(range(10)) and {i % 4 for i in PICKS} == set(range(4))
    P.free()


def test_rejections(eng):
    P = eng.gbm(SEED, S0, R, SIGMA, T / 4, 4, 100)
    one = [(N.X_ASIAN_ARITH_FIXED, True, 100.0, 0.0, 0.0)]
    nan, inf = math.nan, math.inf
    for call, message in ((lambda: eng.greeks_exotics(P, R, T, one, first_row=5), "first_row"),
                          (lambda: eng.greeks_exotics(P, R, T, one, first_row=-1), "first_row"),
                          (lambda: eng.greeks_exotics(P, R, T, one * 1025), "n_contracts"),
                          (lambda: eng.greeks_exotics(P, R, T, [(10, True, 100.0, 0.0, 0.0)]), "kind"),
                          (lambda: eng.greeks_exotics(P, R, T, [(N.X_ASIAN_GEO_FIXED, True, nan, 0.0, 0.0)]), "K must be finite"),
                          (lambda: eng.greeks_exotics(P, R, T, [(N.X_BARRIER_UP_IN, True, 100.0, inf, 0.0)]), "barrier must be finite"),
                          (lambda: eng.greeks_exotics(P, nan, T, one), "finite"),
                          (lambda: eng.greeks_exotics(P, R, T, one, q=inf), "finite"),
                          (lambda: eng.greeks_exotics(P, R, T, one, sigma=nan), "finite"),
                          (lambda: eng.greeks_exotics(P, R, inf, one), "finite"),
                          (lambda: eng.greeks_exotics(P, R, 0.0, one), "T must be positive"),
                          (lambda: eng.greeks_exotics(P, R, -1.0, one), "T must be positive"),
                          (lambda: eng.path_tangent_stats(P, 5), "first_row")):
        with pytest.raises(mc.McgError, match=message) as e:
            call()
        assert e.value.status == 1
    E = eng.gbm(5, S0, R, SIGMA, T / 4, 4, 0)
    for call in (lambda: eng.greeks_exotics(E, R, T, one), lambda: eng.path_tangent_stats(E)):
        with pytest.raises(mc.McgError) as e:
            call()
        assert e.value.status == 6
    E.free()
    with mc.PathEngine(0) as other:
        with pytest.raises(mc.McgError, match="different ctx"):
            other.greeks_exotics(P, R, T, one)
    with mc.PathEngine(0) as sharded:
        sharded.set_allreduce(lambda ptr, count, stream: None)
        Q = sharded.gbm(5, S0, R, SIGMA, T / 4, 4, 3000)
        with pytest.raises(mc.McgError, match="sharded Greeks are not supported"):
            sharded.greeks_exotics(Q, R, T, one, sigma=SIGMA)
        Q.free()
    P.free()


@pytest.fixture(scope="module")
def law_matrix(eng):
    P = eng.gbm(SEED, S0, R, SIGMA, T / 12, 12, 200_003)
    yield P
    P.free()


@pytest.mark.parametrize("is_call", [True, False])
def test_law_geometric_asian(eng, law_matrix, is_call):
    K = 101.0
    g = eng.greeks_exotics(law_matrix, R, T, [(N.X_ASIAN_GEO_FIXED, is_call, K, 0.0, 0.0)], sigma=SIGMA)[0]
    price = lambda s, v, r: geo_price(is_call, K, s, r, 0.0, v, 12, 1)  # noqa: E731
    check_against(g, differences_of(price), f"geometric Asian call={is_call}")
    assert abs(g["price"] - price(S0, SIGMA, R)) <= 4.0 * g["price_se"]


@pytest.mark.parametrize("kind,barrier,is_call", [(N.X_BARRIER_UP_OUT, 1e9, True), (N.X_BARRIER_DOWN_OUT, 1e-9, False)])
def test_law_unreachable_barrier(eng, law_matrix, kind, barrier, is_call):
    K = 100.0
    g = eng.greeks_exotics(law_matrix, R, T, [(kind, is_call, K, barrier, 0.5)], sigma=SIGMA)[0]
    check_against(g, differences_of(lambda s, v, r: black_scholes(is_call, s, K, r, 0.0, v, T)), f"unreachable barrier kind {kind}")


def test_law_one_step_barrier(eng):
    K, B = 100.0, 120.0
    P = eng.gbm(SEED + 1, S0, R, SIGMA, T, 1, 200_003)
    g = eng.greeks_exotics(P, R, T, [(N.X_BARRIER_UP_OUT, True, K, B, 0.0)], sigma=SIGMA)[0]
    P.free()
    check_against(g, differences_of(lambda s, v, r: up_out_call_one_step(s, K, B, r, 0.0, v, T)), "one-step up-and-out call")
    assert abs(g["price"] - up_out_call_one_step(S0, K, B, R, 0.0, SIGMA, T)) <= 4.0 * g["price_se"]
