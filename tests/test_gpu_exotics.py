"""Asian, lookback and barrier prices on the GPU (mcg_path_stats, mcg_price_exotics) against the numpy reference of
tests/test_exotics_reference.py evaluated on the matrix downloaded from the device, and against closed forms.

Bounds: prices and std errors 1e-12 relative (the bound of the European Greeks tests for the same kind of sum); min, max
and S_T exact; A 1e-14.  What goes through G = exp(mean ln S) has bounds of its own, because the device takes ONE log per
path (of a product of mantissas) where numpy takes a log per element: ten times the largest relative error observed on an
MI355X over all cases of this file, G_BOUND for G itself and GEO_PRICE_BOUND for prices and std errors of the kinds that
use G (observed: G 1.98e-15, prices 1.57e-13, std errors 6.8e-15), both far inside the 1e-9 they may not
exceed.  Two places where a relative bound on the result says nothing get a stated scale instead:
  * geometric floating strike monitored on the last row only: the payoff is S_T - G with G == S_T up to rounding, a price
    of rounding noise around zero; it is compared on the scale of e^{-rT} mean(S_T), with G_BOUND;
  * std errors in the small-shape tests (a handful of paths, nearly equal payoffs): the library forms them from
    {sum, sum^2} (sums_to_mean_stderr), whose relative error is that of the sums times (1/2 + mean^2 / variance); those
    tests allow that factor where it exceeds 1.  The tests on large samples do not."""
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from test_exotics_reference import GEO_KINDS, geo_asian_closed_form, price_numpy, stats_numpy

pytestmark = pytest.mark.gpu

SEED = 20251031
DT = 1.0 / 252.0
RB = dict(xi=0.04, H=0.1, eta=1.9, rho=-0.9)
SUM_BOUND = 1e-12
A_BOUND = 1e-14
G_BOUND = 2e-14
GEO_PRICE_BOUND = 1.6e-12
REBATE = 0.75
ALL_KINDS = tuple(range(10))
observed = {"G": 0.0, "A": 0.0, "price": 0.0, "se": 0.0, "price_geo": 0.0, "se_geo": 0.0}


@pytest.fixture(scope="module")
def eng():
    with mc.PathEngine(0) as e:
        yield e


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest relative errors against numpy in this run: " + ", ".join(f"{k} {v:.2e}" for k, v in observed.items()))


def columns(P, begin, count):
    """Paths begin .. begin + count of a device matrix as a path-major host array, without downloading the rest."""
    import torch
    from montecarlooptionspricer_amd.engine import _DevView
    t = torch.as_tensor(_DevView(P.device_ptr, P.ld * (P.n_steps + 1)), device="cuda:0").view(P.n_steps + 1, P.ld)
    return np.ascontiguousarray(t[:, begin:begin + count].cpu().numpy().T)


def bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


def check_stats(got, want, where):
    assert got.shape == want.shape, where
    for q in (0, 3, 4):
        assert np.array_equal(got[q], want[q]), (where, q)
    with np.errstate(invalid="ignore", divide="ignore"):
        ea = np.abs(got[1] - want[1]) / np.abs(want[1])
        eg = np.where(got[2] == want[2], 0.0, np.abs(got[2] - want[2]) / np.abs(want[2]))
    observed["A"], observed["G"] = max(observed["A"], float(ea.max())), max(observed["G"], float(eg.max()))
    assert ea.max() <= A_BOUND, (where, ea.max())
    assert eg.max() <= G_BOUND, (where, eg.max())


def check_prices(price, se, book, st5, r, T, where, last_row_only=False, conditioned=False):
    D = math.exp(-r * T)
    for i, c in enumerate(book):
        want, want_se = price_numpy(st5, c, r, T)
        geo = c[0] in GEO_KINDS
        bound = GEO_PRICE_BOUND if geo else SUM_BOUND
        tol, tol_se = bound * abs(want), bound * abs(want_se)
        if geo and last_row_only and c[0] == N.X_ASIAN_GEO_FLOAT:
            tol = tol_se = G_BOUND * D * float(st5[0].mean())
        else:
            k = "_geo" if geo else ""
            if want != 0.0:
                observed["price" + k] = max(observed["price" + k], abs(price[i] - want) / abs(want))
            if want_se != 0.0 and not conditioned:
                observed["se" + k] = max(observed["se" + k], abs(se[i] - want_se) / abs(want_se))
            if conditioned and want_se != 0.0:
                tol_se *= max(1.0, 0.5 + (want / want_se) ** 2 / len(st5[0]))
        assert abs(price[i] - want) <= tol, (where, i, c, "price", price[i], want)
        assert abs(se[i] - want_se) <= tol_se, (where, i, c, "std error", se[i], want_se)


def level(values, fraction_hit, up):
    """A barrier that this fraction of the paths hits: one of the stored extremes itself, so that >= / <= decide a path."""
    s = np.sort(values)
    n = len(s)
    return float(s[min(n - 1, int((1.0 - fraction_hit) * n))] if up else s[max(0, int(fraction_hit * n) - 1)])


def full_book(st5, strikes):
    """Every kind x call / put x in-, at- and out-of-the-money strikes; barriers hit by about 1/10, 1/2 and 9/10 of the paths."""
    book = []
    for kind in ALL_KINDS:
        for call in (True, False):
            for K in strikes:
                if kind < N.X_BARRIER_UP_OUT:
                    book.append((kind, call, K, 0.0, 0.0))
                    continue
                up = kind in (N.X_BARRIER_UP_OUT, N.X_BARRIER_UP_IN)
                for f in (0.1, 0.5, 0.9):
                    book.append((kind, call, K, level(st5[4] if up else st5[3], f, up), REBATE))
    return book


def matrices(eng):
    yield "gbm", eng.gbm(SEED, 100.0, 0.04, 0.2, 0.02, 50, 200_000), 0.04, 1.0
    yield "rbergomi", eng.rbergomi(SEED, 100.0, 0.04, RB["xi"], RB["H"], RB["eta"], RB["rho"], DT, 64, 100_000), 0.04, 64 * DT


def test_every_kind_against_numpy(eng):
    for name, P, r, T in matrices(eng):
        X = P.to_host()
        for first_row in (0, 1, P.n_steps):
            where = (name, first_row)
            st5 = stats_numpy(X, first_row)
            check_stats(eng.path_stats(P, first_row), st5, where)
            book = full_book(st5, (90.0, 100.0, 110.0))
            for c in book:
                if c[0] >= N.X_BARRIER_UP_OUT and first_row != 0:      # (row 0 ties many extremes at S0)
                    up = c[0] in (N.X_BARRIER_UP_OUT, N.X_BARRIER_UP_IN)
                    hit = (st5[4] >= c[3]).mean() if up else (st5[3] <= c[3]).mean()
                    assert min(abs(hit - f) for f in (0.1, 0.5, 0.9)) < 0.01, (where, c, hit)
            assert len(book) == 6 * 2 * 3 + 4 * 2 * 3 * 3
            price, se = eng.price_exotics(P, r, T, book, first_row=first_row)
            check_prices(price, se, book, st5, r, T, where, last_row_only=first_row == P.n_steps)
        P.free()
    # default first_row is 1: S0 = 100 is left out of the extremes
    Q = eng.gbm(3, 100.0, 0.04, 0.2, 0.02, 50, 4096)
    assert np.array_equal(eng.path_stats(Q), eng.path_stats(Q, 1))
    assert (eng.path_stats(Q, 0)[3] <= 100.0).all() and (eng.path_stats(Q)[3] > 100.0).any()
    Q.free()


@pytest.mark.parametrize("is_call", [True, False])
def test_geometric_asian_closed_form(eng, is_call):
    P = eng.gbm(SEED, 100.0, 0.04, 0.2, DT, 252, 4_000_000)
    price, se = eng.price_exotics(P, 0.04, 1.0, [mc.exotic("asian_geo_fixed", is_call, K=100.0)])
    want = geo_asian_closed_form(100.0, 100.0, 0.04, 0.2, DT, 252, 1, is_call)
    print(f"geometric Asian call={is_call}: {price[0]:.6f} +- {se[0]:.6f}, closed form {want:.6f}")
    P.free()
    assert se[0] > 0.0 and abs(price[0] - want) <= 4.0 * se[0], (price[0], want, se[0])


def test_identities_on_the_device(eng):
    r, T, K = 0.04, 1.0, 100.0
    P = eng.gbm(SEED, 100.0, r, 0.2, 0.02, 50, 200_000)
    st5 = eng.path_stats(P)
    for call in (True, False):
        vanilla, _ = eng.price_european(P, K, r, T, call)
        book = [(N.X_BARRIER_UP_IN, call, K, level(st5[4], 0.5, True), 0.0), (N.X_BARRIER_UP_OUT, call, K, level(st5[4], 0.5, True), 0.0),
                (N.X_BARRIER_DOWN_IN, call, K, level(st5[3], 0.5, False), 0.0), (N.X_BARRIER_DOWN_OUT, call, K, level(st5[3], 0.5, False), 0.0),
                (N.X_BARRIER_UP_OUT, call, K, 1e300, REBATE), (N.X_LOOKBACK_FIXED, call, K, 0.0, 0.0), (N.X_ASIAN_ARITH_FIXED, call, K, 0.0, 0.0)]
        p, _ = eng.price_exotics(P, r, T, book)
        assert min(p[:4]) > 0.0
        assert abs(p[0] + p[1] - vanilla) <= 1e-12 * vanilla and abs(p[2] + p[3] - vanilla) <= 1e-12 * vanilla
        assert abs(p[4] - vanilla) <= 1e-12 * vanilla
        assert p[5] >= vanilla and p[6] <= p[5]      # hold path by path
        last, _ = eng.price_exotics(P, r, T, [(N.X_ASIAN_ARITH_FIXED, call, K, 0.0, 0.0), (N.X_ASIAN_GEO_FIXED, call, K, 0.0, 0.0)],
                                    first_row=P.n_steps)
        assert abs(last[0] - vanilla) <= 1e-13 * vanilla
        assert abs(last[1] - vanilla) <= G_BOUND * math.exp(-r * T) * float(st5[0].mean())
    P.free()


def mixed_book(n):
    """n contracts, kinds in turn; up barriers in [105, 130), down barriers in [75, 97): no payoff is one constant."""
    def barrier(i):
        f = ((i * 104729) % n) / n
        return 105.0 + 25.0 * f if i % 10 in (N.X_BARRIER_UP_OUT, N.X_BARRIER_UP_IN) else 75.0 + 22.0 * f
    return [(i % 10, (i // 10) % 2 == 0, 80.0 + 40.0 * ((i * 7919) % n) / n, barrier(i), 0.5 + i / n) for i in range(n)]


PICKS = (0, 1, 3, 7, 8, 12, 14, 25, 106, 339, 517, 1016, 1023)   # every kind, every slot of a chunk of the book kernel


def test_book_independence_and_determinism(eng):
    P = eng.gbm(SEED, 100.0, 0.04, 0.2, 0.02, 50, 200_001)
    book = mixed_book(1024)
    price, se = eng.price_exotics(P, 0.04, 1.0, book)
    again = eng.price_exotics(P, 0.04, 1.0, book)
    assert bits(price) == bits(again[0]) and bits(se) == bits(again[1])
    rev = eng.price_exotics(P, 0.04, 1.0, book[::-1])
    assert bits(rev[0][::-1]) == bits(price) and bits(rev[1][::-1]) == bits(se)
    for i in PICKS:
        alone = eng.price_exotics(P, 0.04, 1.0, [book[i]])
        assert bits(alone[0]) == bits(price[i:i + 1]) and bits(alone[1]) == bits(se[i:i + 1]), i
    assert {book[i][0] for i in PICKS} == set(ALL_KINDS) and {i % 8 for i in PICKS} == set(range(8))
    X = P.to_host()
    st5 = stats_numpy(X, 1)
    check_prices(price[:40], se[:40], book[:40], st5, 0.04, 1.0, "mixed book")
    P.free()


def small_book(st5):
    return full_book(st5, (float(np.median(st5[0])),))


@pytest.mark.parametrize("n_paths", [1, 2, 63, 65, 255, 257, 20_001])
def test_path_counts(eng, n_paths):
    for n_steps in (50, 1):
        P = eng.gbm(11, 100.0, 0.04, 0.3, 0.02, n_steps, n_paths)
        X = P.to_host()
        for first_row in (0, 1):
            st5 = stats_numpy(X, first_row)
            check_stats(eng.path_stats(P, first_row), st5, (n_paths, n_steps, first_row))
            book = small_book(st5)
            price, se = eng.price_exotics(P, 0.04, n_steps * 0.02, book, first_row=first_row)
            check_prices(price, se, book, st5, 0.04, n_steps * 0.02, (n_paths, n_steps, first_row), last_row_only=first_row == n_steps,
                         conditioned=True)
            if n_paths == 1:
                assert not se.any()
        P.free()


@pytest.mark.parametrize("n_paths", [1, 2, 257])           # the lone path, one full vector lane, an odd count over a block edge
@pytest.mark.parametrize("n_rows", [1, 2, 7, 8, 9, 15, 16, 17])
def test_scan_groups_and_tails(eng, n_rows, n_paths):
    """The scan's groups of 8 rows and its tail of up to 7, at every monitored row count around one and two groups, reached
    with first_row = 1 and (from two rows on) first_row = 0; the tangent statistics' first five are the same bits."""
    for first_row in (1, 0) if n_rows > 1 else (1,):
        n_steps = n_rows + first_row - 1
        where = (n_rows, n_paths, first_row)
        P = eng.gbm(17, 100.0, 0.04, 0.3, 0.02, n_steps, n_paths)
        X = P.to_host()
        assert X[:, first_row:].shape == (n_paths, n_rows)
        got = eng.path_stats(P, first_row)
        check_stats(got, stats_numpy(X, first_row), where)
        for with_logs in (True, False):
            t = eng.path_tangent_stats(P, first_row, with_logs=with_logs)
            assert t.shape == (10, n_paths) and bits(t[:5]) == bits(got), (where, with_logs)
            assert np.array_equal(t[7], first_row + np.argmin(X[:, first_row:], axis=1)), (where, with_logs)
            assert np.array_equal(t[8], first_row + np.argmax(X[:, first_row:], axis=1)), (where, with_logs)
        P.free()


def test_other_sources_of_a_matrix(eng):
    # uploaded from the host, with a zero among its values (numpy: log 0 = -inf, G = 0) ...
    rng = np.random.default_rng(5)
    X = 100.0 * np.exp(np.cumsum(0.05 * rng.standard_normal((37, 11)), axis=1))
    X[3, 4] = 0.0
    P = eng.from_host(X)
    for first_row in (0, 1, 10):
        with np.errstate(divide="ignore"):
            st5 = stats_numpy(X, first_row)
        check_stats(eng.path_stats(P, first_row), st5, ("from_host", first_row))
    assert eng.path_stats(P, 1)[2, 3] == 0.0
    book = small_book(stats_numpy(X, 5))
    price, se = eng.price_exotics(P, 0.04, 1.0, book, first_row=5)
    check_prices(price, se, book, stats_numpy(X, 5), 0.04, 1.0, "from_host", conditioned=True)
    P.free()
    # ... and with subnormal values: ln G is a sum of logs near -710, whose own rounding (2e-13) is what numpy's G is good to
    Y = X.copy()
    Y[3, 4], Y[20, 10], Y[21, 0] = 50.0, 1e-310, 3e-320
    P = eng.from_host(Y)
    got, want = eng.path_stats(P, 0), stats_numpy(Y, 0)
    for q in (0, 3, 4):
        assert np.array_equal(got[q], want[q])
    assert np.abs(got[2] / want[2] - 1.0).max() <= 1e-12 and np.abs(got[1] / want[1] - 1.0).max() <= A_BOUND
    P.free()
    # a shard that does not start at path 0, an odd count; the fused-payoff generators' matrices
    for P in (eng.gbm(SEED, 100.0, 0.04, 0.2, 0.02, 50, 1001, path_begin=1000),
              eng.gbm(SEED, 100.0, 0.04, 0.2, 0.02, 50, 3000, payoff=(100.0, True)),
              eng.rbergomi(SEED, 100.0, 0.04, RB["xi"], RB["H"], RB["eta"], RB["rho"], DT, 64, 3000, path_begin=2000, payoff=(100.0, False))):
        X = P.to_host()
        st5 = stats_numpy(X, 1)
        check_stats(eng.path_stats(P), st5, "generated")
        book = small_book(st5)
        price, se = eng.price_exotics(P, 0.04, 1.0, book)
        check_prices(price, se, book, st5, 0.04, 1.0, "generated")
        P.free()
    whole = eng.gbm(SEED, 100.0, 0.04, 0.2, 0.02, 50, 2001)
    shard = eng.gbm(SEED, 100.0, 0.04, 0.2, 0.02, 50, 1001, path_begin=1000)
    assert np.array_equal(eng.path_stats(whole)[:, 1000:], eng.path_stats(shard))
    whole.free()
    shard.free()


def test_the_timed_shape(eng):
    """10M x 252 GBM, the benchmark's C2 matrix: statistics of the first and last 4096 paths against numpy on those columns,
    and a 64-contract book against numpy evaluated on the full-width statistics."""
    n = 10_000_000
    P = eng.gbm(SEED, 100.0, 0.04, 0.2, DT, 252, n, payoff=(100.0, True))
    st5 = eng.path_stats(P)
    for begin in (0, n - 4096):
        check_stats(st5[:, begin:begin + 4096], stats_numpy(columns(P, begin, 4096), 1), ("10M", begin))
    book = full_book(st5[:, :200_000], (100.0,)) + full_book(st5[:, :200_000], (90.0,))[:24] + [(N.X_BARRIER_UP_OUT, True, 100.0, 1e300, 0.0), (N.X_LOOKBACK_FLOAT, True, 0.0, 0.0, 0.0),
                                                       (N.X_ASIAN_ARITH_FIXED, True, 100.0, 0.0, 0.0), (N.X_ASIAN_GEO_FIXED, False, 100.0, 0.0, 0.0)]
    assert len(book) == 64 and {c[0] for c in book} == set(ALL_KINDS)
    price, se = eng.price_exotics(P, 0.04, 1.0, book)
    check_prices(price, se, book, st5, 0.04, 1.0, "10M")
    vanilla, vanilla_se = eng.price_european(P, 100.0, 0.04, 1.0, True)
    assert abs(price[60] - vanilla) <= 1e-12 * vanilla and abs(se[60] - vanilla_se) <= 1e-10 * vanilla_se
    P.free()


def test_errors(eng):
    P = eng.gbm(1, 100.0, 0.04, 0.2, 0.02, 50, 1000)
    L = mc.load_library()
    ok = (N.X_ASIAN_ARITH_FIXED, True, 100.0, 0.0, 0.0)
    nan = float("nan")

    def refused(book, first_row=1, engine=eng):
        with pytest.raises(mc.McgError) as e:
            engine.price_exotics(P, 0.04, 1.0, book, first_row=first_row)
        assert e.value.status == 1 and str(e.value) and L.mcg_last_error(), book

    refused([])
    refused([ok] * 1025)
    eng.price_exotics(P, 0.04, 1.0, [ok] * 1024)
    refused([ok, (-1, True, 100.0, 0.0, 0.0)])
    refused([(10, True, 100.0, 0.0, 0.0), ok])
    refused([ok], first_row=-1)
    refused([ok], first_row=51)
    eng.price_exotics(P, 0.04, 1.0, [ok], first_row=50)
    for kind in (N.X_ASIAN_ARITH_FIXED, N.X_ASIAN_GEO_FIXED, N.X_LOOKBACK_FIXED) + tuple(range(6, 10)):
        refused([(kind, True, nan, 100.0, 0.0)])
        refused([(kind, False, float("inf"), 100.0, 0.0)])
    for kind in range(6, 10):
        refused([(kind, True, 100.0, nan, 0.0)])
        refused([(kind, True, 100.0, 100.0, nan)])
    # fields a kind does not read may hold anything
    p, _ = eng.price_exotics(P, 0.04, 1.0, [(N.X_ASIAN_ARITH_FLOAT, True, nan, nan, nan), (N.X_LOOKBACK_FLOAT, False, nan, nan, nan),
                                            (N.X_LOOKBACK_FIXED, True, 100.0, nan, nan)])
    assert np.isfinite(p).all()
    with mc.PathEngine(0) as other:
        refused([ok], engine=other)
        with pytest.raises(mc.McgError) as e:
            other.path_stats(P)
        assert e.value.status == 1
    for first_row in (-1, 51):
        with pytest.raises(mc.McgError) as e:
            eng.path_stats(P, first_row)
        assert e.value.status == 1 and L.mcg_last_error()
    P.free()


def from_sums(s, n, r, T):
    m = s[0] / n
    var = max(0.0, (s[1] - n * m * m) / (n - 1.0))
    return math.exp(-r * T) * m, math.exp(-r * T) * math.sqrt(var / n)


def test_sharding_on_one_gpu(eng):
    n, r, T = 200_000, 0.04, 1.0
    gen = (SEED, 100.0, r, 0.2, 0.02, 50)
    book = mixed_book(64)
    P = eng.gbm(*gen, n)
    price, se, sums = eng.price_exotics(P, r, T, book, return_sums=True)
    assert sums.shape == (129,) and sums[128] == n
    calls = []
    with mc.PathEngine(0) as ident:
        ident.set_allreduce(lambda ptr, count, stream: calls.append(count))   # world size 1: the sum over ranks is the identity
        Q = ident.gbm(*gen, n)
        got = ident.price_exotics(Q, r, T, book, return_sums=True)
        assert calls == [129]                                               # one collective call for the whole book
        assert bits(got[0]) == bits(price) and bits(got[1]) == bits(se) and bits(got[2]) == bits(sums)
    with mc.PathEngine(0) as a, mc.PathEngine(0) as b:
        A, B = a.gbm(*gen, n // 2), b.gbm(*gen, n - n // 2, path_begin=n // 2)
        sa, sb = a.price_exotics(A, r, T, book, return_sums=True)[2], b.price_exotics(B, r, T, book, return_sums=True)[2]
    both = sa + sb
    assert both[128] == n
    for c in range(64):
        p, s = from_sums(both[2 * c:2 * c + 2], n, r, T)
        assert abs(p - price[c]) <= 1e-12 * abs(price[c]) and abs(s - se[c]) <= 1e-12 * abs(se[c]), (c, book[c])
    P.free()


def test_launch_accounting(eng):
    P = eng.gbm(1, 100.0, 0.04, 0.2, 0.02, 50, 10_000)
    eng.timing_enable(True)
    eng.timing_reset()
    eng.price_european(P, 100.0, 0.04, 1.0, True)
    assert eng.timing_get(N.K_EXOTIC)[1] == 0 and eng.timing_get(N.K_PAYOFF)[1] > 0
    eng.price_exotics(P, 0.04, 1.0, [mc.exotic("lookback_float", True)])
    ms, launches = eng.timing_get(N.K_EXOTIC)
    assert launches == 3 and ms > 0.0            # statistics, book, reduction
    eng.path_stats(P)
    assert eng.timing_get(N.K_EXOTIC)[1] == 4
    eng.timing_enable(False)
    P.free()
