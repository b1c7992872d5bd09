"""Autocallables and cliquets on the GPU (mcg_price_scheduled, mcg_sched_path_values) against the numpy restatement of
tests/test_sched_reference.py evaluated on the matrix downloaded from the device, and against closed forms.

Bounds.  stop is exact on every path: the division X_k = S / s0 and the comparisons are IEEE on both sides.  An autocallable's
Y is a sum of at most n_obs + 1 non-negative terms, each with one rounding for disc_k, one for the product and one for the
add, and the compiler may contract a product and an add into an FMA: |Y - Y_np| <= (n_obs + 4) 2^-52 Y_np.  A cliquet's sum
has m terms of either sign: |Y - Y_np| <= (m + 4) 2^-52 (|Y_np| + sum |c_i| disc).  Prices and std errors: 1e-12 relative,
SUM_BOUND of tests/test_gpu_exotics.py, with that file's allowance where a std error is formed from {sum, sum^2} of nearly
equal payoffs: the relative error of the sums times (1/2 + mean^2 / variance), where that exceeds 1.  A note's payoffs sit
near 1 by construction, so this applies at every sample size; where numpy's own std error is zero up to rounding (one
constant payoff), the library's is held to |mean| sqrt(64 2^-52 / (n - 1)): 64 roundings of the two sums that the variance
subtracts.  The largest observed fraction of each bound is printed at the end of the run."""
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from test_sched_reference import CALL, COUPON, KI, RESET, discounts, forward_start_call, price_numpy, values_numpy

pytestmark = pytest.mark.gpu

SEED = 20260114
INF = math.inf
U = 2.0 ** -52
SUM_BOUND = 1e-12
R, DT = 0.04, 0.02
observed = {"autocall Y": 0.0, "cliquet Y": 0.0, "price": 0.0, "std error": 0.0}


@pytest.fixture(scope="module")
def eng():
    with mc.PathEngine(0) as e:
        yield e


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest fractions of the bounds against numpy in this run: " + ", ".join(f"{k} {v:.3f}" for k, v in observed.items()))


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def raw_obs(entries):
    """An mcg_obs array as it is: what the library itself has to check."""
    return (N.Obs * len(entries))(*[N.Obs(int(r), int(f)) for r, f in entries])


def mixed_book(n):
    """n contracts, two autocallables then a cliquet in turn; levels spread so that calls, missed coupons and knock-ins occur."""
    book = []
    for i in range(n):
        f = ((i * 7919) % 64) / 64.0
        if i % 3 == 2:
            book.append(mc.cliquet(*((0.0, INF, -INF, INF), (-0.03, 0.04, 0.0, 0.15 + 0.1 * f), (-INF, 0.02 + 0.02 * f, -0.05, INF),
                                    (-INF, INF, -INF, INF))[(i // 3) % 4]))
        else:
            call = (1.0, 1.03 + 0.05 * f, 0.97, INF, 1.1)[(i // 3) % 5]
            book.append(mc.autocall(call, 0.01 + 0.02 * f, 0.85 + 0.15 * f, (0.0, 0.8 + 0.1 * f, 0.95)[i % 3 + (i // 6) % 2],
                                    (1.0, 0.9)[(i // 2) % 2], memory=(i // 3) % 2 == 0))
    return book


def n_resets(sched):
    return sum(1 for _, f in sched if f & RESET)


def check_values(eng, P, X, r, dt, sched, book, where):
    vals, stop = eng.sched_path_values(P, r, dt, sched, book)
    assert vals.shape == stop.shape == (len(book), len(X)), where
    n_obs, m = len(sched), n_resets(sched) - 1
    want = []
    for i, c in enumerate(book):
        Y, st, scale = values_numpy(X, r, dt, sched, c)
        assert np.array_equal(stop[i], st), (where, i, c, np.flatnonzero(stop[i] != st)[:5])
        err = np.abs(vals[i] - Y)
        if c[0] == N.S_AUTOCALL:
            assert (Y >= 0.0).all()
            key, bound = "autocall Y", (n_obs + 4) * U * Y
        else:
            key, bound = "cliquet Y", (m + 4) * U * (np.abs(Y) + scale)
        with np.errstate(invalid="ignore", divide="ignore"):
            frac = np.where(err == 0.0, 0.0, err / bound)
        print(f"{where} contract {i}: largest |Y - Y_np| / bound {frac.max():.3f}")
        observed[key] = max(observed[key], float(frac.max()))
        assert (err <= bound).all(), (where, i, c, float(frac.max()))
        want.append((Y, st))
    return want


def check_prices(eng, P, r, dt, sched, book, want, where):
    price, se, sums, hist = eng.price_scheduled(P, r, dt, sched, book, return_sums=True, return_hist=True)
    n = len(want[0][0])
    assert sums.shape == (2 * len(book) + 1,) and sums[-1] == n and hist.shape == (len(book), len(sched) + 1), where
    for i, (Y, st) in enumerate(want):
        w, w_se = price_numpy(Y)
        tol, tol_se = SUM_BOUND * abs(w), SUM_BOUND * w_se
        if n > 1 and w_se <= SUM_BOUND * abs(w):
            tol_se = abs(w) * math.sqrt(64.0 * U / (n - 1))
        elif w_se != 0.0:
            tol_se *= max(1.0, 0.5 + (w / w_se) ** 2 / n)
            observed["std error"] = max(observed["std error"], abs(se[i] - w_se) / tol_se)
        if w != 0.0:
            observed["price"] = max(observed["price"], abs(price[i] - w) / tol)
        print(f"{where} contract {i}: price {price[i]:.12g} numpy {w:.12g}, std error {se[i]:.6g} numpy {w_se:.6g}")
        assert abs(price[i] - w) <= tol, (where, i, book[i], "price", price[i], w)
        assert abs(se[i] - w_se) <= tol_se, (where, i, book[i], "std error", se[i], w_se)
        assert np.array_equal(hist[i], np.bincount(st, minlength=len(sched) + 1)), (where, i, book[i])
    return price, se, sums, hist


def flag_mix(rows, mix):
    """0: KI on every date, COUPON|CALL on every third and the last; 1: a non-call period, coupons only in the first half;
    2: CALL without COUPON on every date, row 0 included.  RESET on the first, a middle and the last date."""
    n = len(rows)
    out = []
    for k, row in enumerate(rows):
        if mix == 0:
            f = KI | (COUPON | CALL if (k % 3 == 2 or k == n - 1) and row > 0 else 0)
        elif mix == 1:
            f = (COUPON if row > 0 else 0) | (CALL if k >= n // 2 and row > 0 else 0) | (KI if k == n - 1 else 0)
        else:
            f = CALL | (KI if k % 2 else 0)
        out.append((row, f | (RESET if k in (0, n // 2, n - 1) else 0)))
    return out


def schedules(n_steps):
    """Row sets: 1, 7, 8, 9 and 17 dates (the edges of the load groups of 8) where the matrix has so many, row 0 plus the last
    row, every row, the last row alone -- each under one of the three flag mixes in turn."""
    sets = []
    for count in (1, 7, 8, 9, 17):
        if count <= n_steps + 1:
            rows = sorted({int(round(v)) for v in np.linspace(1 if count <= n_steps else 0, n_steps, count)})
            assert len(rows) == count
            sets.append(rows)
    sets += [[0, n_steps], list(range(n_steps + 1)), [n_steps]]
    return [flag_mix(rows, i % 3) for i, rows in enumerate(sets)]


def book_for(sched, n):
    book = mixed_book(n)
    return book if n_resets(sched) >= 2 else [c for c in book if c[0] == N.S_AUTOCALL]


@pytest.mark.parametrize("n_paths", [1, 2, 63, 64, 65, 255, 256, 257, 511, 1003])
def test_shapes(eng, n_paths):
    for n_steps in (1, 7, 8, 9, 50):
        P = eng.gbm(SEED + n_steps, 100.0, R, 0.3, DT, n_steps, n_paths)
        X = P.to_host()
        for s, sched in enumerate(schedules(n_steps)):
            where = (n_paths, n_steps, s)
            book = book_for(sched, 9)
            want = check_values(eng, P, X, R, DT, sched, book, where)
            check_prices(eng, P, R, DT, sched, book, want, where)
            if n_paths == 1:
                assert not eng.price_scheduled(P, R, DT, sched, book)[1].any()
        P.free()


@pytest.mark.parametrize("n_contracts", [1, 7, 8, 9, 17])
def test_book_sizes(eng, n_contracts):
    P = eng.gbm(SEED, 100.0, R, 0.3, DT, 50, 1003)
    X = P.to_host()
    sched = flag_mix(list(range(51)), 0)
    book = mixed_book(n_contracts + 2)[2:] if n_contracts == 1 else mixed_book(n_contracts)   # (a cliquet alone; else both kinds)
    assert n_contracts == 1 or {c[0] for c in book} == {N.S_AUTOCALL, N.S_CLIQUET}
    want = check_values(eng, P, X, R, DT, sched, book[:n_contracts], n_contracts)
    check_prices(eng, P, R, DT, sched, book[:n_contracts], want, n_contracts)
    P.free()


def test_other_models(eng):
    quarterly = [(j, KI | (COUPON | CALL if j % 10 == 0 and j > 0 else 0) | (RESET if j % 20 == 0 else 0)) for j in range(0, 41)]
    H = eng.heston(SEED, 100.0, R, 0.04, 1.5, 0.04, 0.6, -0.7, DT, 40, 20_001, scheme="qe")
    assets, _ = eng.gbm_multi(SEED, [100.0, 40.0], R, [0.25, 0.35], [[1.0, 0.6], [0.6, 1.0]], DT, 40, 20_001)
    W = eng.combine(assets, "worst_of", weights=[1.0 / 100.0, 1.0 / 40.0])
    G = eng.gbm(SEED, 100.0, R, 0.2, DT, 40, 20_001)
    for name, P in (("gbm", G), ("heston qe", H), ("worst of two", W)):
        X = P.to_host()
        if name == "worst of two":
            assert (X[:, 0] == 1.0).all()
        book = mixed_book(9)
        want = check_values(eng, P, X, R, DT, quarterly, book, name)
        _, _, _, hist = check_prices(eng, P, R, DT, quarterly, book, want, name)
        assert (hist[0] > 0).sum() >= 3, (name, hist[0])           # called at several dates, and paths that reach maturity
        P.free()
    for A in assets:
        A.free()


def test_levels_met_exactly(eng):
    """Exactly representable values with X_k on a level: >= and <= decide as written."""
    s0 = 64.0
    up, dn = 2.0 ** -46, 2.0 ** -47                               # one ulp of 80 and of 48: X moves by one ulp of 1.25, of 0.75
    X = np.array([[s0, 80.0, 64.0, 64.0],                         # X == call_level: called at the first date
                  [s0, 80.0 - up, 64.0, 64.0],                    # one ulp below: not called, coupons paid (X == coupon_level pays)
                  [s0, 48.0, 60.0, 64.0],                         # X == ki_level: knocked in; X_last == put_strike: redeems at 1
                  [s0, 48.0 + dn, 60.0, 56.0],                    # one ulp above the knock-in level: not knocked in, redeems at 1
                  [s0, 48.0, 60.0, 56.0],                         # knocked in and below the strike: X_last / put_strike
                  [s0, 64.0 - 2.0 ** -47, 64.0, 64.0]])           # one ulp below the coupon level at the first date: a missed coupon
    assert (80.0 - up) / s0 == 1.25 - U and (48.0 + dn) / s0 == 0.75 + U / 2 and (64.0 - 2.0 ** -47) / s0 == 1.0 - U / 2
    sched = [(1, COUPON | CALL | KI), (2, COUPON | CALL | KI), (3, COUPON | CALL | KI)]
    book = [mc.autocall(1.25, 0.0625, 1.0, 0.75, 1.0, memory=True), mc.autocall(1.25, 0.0625, 1.0, 0.75, 1.0, memory=False)]
    P = eng.from_host(X)
    assert np.array_equal(P.to_host(), X)
    vals, stop = eng.sched_path_values(P, 0.0, 1.0, sched, book)
    want = check_values(eng, P, X, 0.0, 1.0, sched, book, "levels")
    check_prices(eng, P, 0.0, 1.0, sched, book, want, "levels")
    assert stop[0].tolist() == [0, 3, 3, 3, 3, 3]
    assert vals[0].tolist() == [1.0625, 1.1875, 1.1875, 1.0, 0.875, 1.1875]      # memory: the missed coupons are paid back
    assert vals[1].tolist() == [1.0625, 1.1875, 1.0625, 1.0, 0.875, 1.125] and stop[1].tolist() == stop[0].tolist()
    P.free()


def test_sums_prices_and_histogram(eng):
    P = eng.gbm(SEED, 100.0, R, 0.25, DT, 50, 200_001)
    X = P.to_host()
    sched = flag_mix(list(range(1, 51)), 0)
    book = mixed_book(17)
    want = [values_numpy(X, R, DT, sched, c)[:2] for c in book]
    price, se, sums, hist = check_prices(eng, P, R, DT, sched, book, want, "200001 x 50")
    assert (hist.sum(axis=1) == 200_001).all()
    again = eng.price_scheduled(P, R, DT, sched, book, return_sums=True, return_hist=True)
    assert all(bits(a) == bits(b) for a, b in zip(again, (price, se, sums, hist)))
    plain = eng.price_scheduled(P, R, DT, sched, book)
    assert len(plain) == 2 and bits(plain[0]) == bits(price) and bits(plain[1]) == bits(se)
    P.free()


def test_long_schedules_take_the_direct_histogram(eng):
    """8 contracts x (n_obs + 1) counters fit the workgroup's LDS up to 255 dates; 300 dates are added to global memory directly."""
    P = eng.gbm(SEED, 100.0, R, 0.3, 1.0 / 300.0, 300, 1003)
    X = P.to_host()
    for n_obs in (255, 256, 300):
        sched = [(j, COUPON | KI | (CALL if j % 7 == 0 else 0) | (RESET if j % 50 == 0 else 0)) for j in range(301 - n_obs, 301)]
        book = mixed_book(9)
        want = check_values(eng, P, X, R, 1.0 / 300.0, sched, book, n_obs)
        check_prices(eng, P, R, 1.0 / 300.0, sched, book, want, n_obs)
    P.free()


def test_position_in_the_book(eng):
    P = eng.gbm(SEED, 100.0, R, 0.3, DT, 50, 1003)
    sched = flag_mix(list(range(51)), 0)
    filler = mixed_book(1024)
    for c in (mixed_book(2)[0], mixed_book(3)[2]):
        alone = eng.price_scheduled(P, R, DT, sched, [c], return_sums=True, return_hist=True)
        alone_v = eng.sched_path_values(P, R, DT, sched, [c])
        for at in (0, 8, 1023):
            book = list(filler)
            book[at] = c
            price, se, sums, hist = eng.price_scheduled(P, R, DT, sched, book, return_sums=True, return_hist=True)
            assert bits(price[at:at + 1]) == bits(alone[0]) and bits(se[at:at + 1]) == bits(alone[1]), (c, at)
            assert bits(sums[2 * at:2 * at + 2]) == bits(alone[2][:2]) and bits(hist[at]) == bits(alone[3][0]), (c, at)
            vals, stop = eng.sched_path_values(P, R, DT, sched, book)
            assert bits(vals[at]) == bits(alone_v[0][0]) and bits(stop[at]) == bits(alone_v[1][0]), (c, at)
    P.free()


def from_sums(s, n):
    m = s[0] / n
    return m, math.sqrt(max(0.0, (s[1] - n * m * m) / (n - 1.0)) / n)


def test_collective_and_shards(eng):
    n = 1003
    gen = (SEED, 100.0, R, 0.3, DT, 50)
    sched = flag_mix(list(range(51)), 0)
    book = mixed_book(17)
    P = eng.gbm(*gen, n)
    price, se, sums, hist = eng.price_scheduled(P, R, DT, sched, book, return_sums=True, return_hist=True)
    calls = []
    with mc.PathEngine(0) as ident:
        ident.set_allreduce(lambda ptr, count, stream: calls.append(count))   # world size 1: the sum over ranks is the identity
        Q = ident.gbm(*gen, n)
        got = ident.price_scheduled(Q, R, DT, sched, book, return_sums=True)
        assert calls == [2 * len(book) + 1]
        assert bits(got[0]) == bits(price) and bits(got[1]) == bits(se) and bits(got[2]) == bits(sums)
        with pytest.raises(mc.McgError, match="collective") as e:
            ident.price_scheduled(Q, R, DT, sched, book, return_hist=True)
        assert e.value.status == 1 and len(calls) == 1
        E = ident.gbm(*gen, 0)                                    # an empty shard still takes part: the sums are all zero, n = 0
        with pytest.raises(mc.McgError) as e:
            ident.price_scheduled(E, R, DT, sched, book)
        assert e.value.status == 6 and len(calls) == 2
    for cut in (1, 256, 511):
        A, B = eng.gbm(*gen, cut), eng.gbm(*gen, n - cut, path_begin=cut)
        ra = eng.price_scheduled(A, R, DT, sched, book, return_sums=True, return_hist=True)
        rb = eng.price_scheduled(B, R, DT, sched, book, return_sums=True, return_hist=True)
        both = ra[2] + rb[2]
        assert both[-1] == n and np.array_equal(ra[3] + rb[3], hist), cut
        for c in range(len(book)):
            assert abs(both[2 * c] - sums[2 * c]) <= SUM_BOUND * abs(sums[2 * c]), (cut, c)
            assert abs(both[2 * c + 1] - sums[2 * c + 1]) <= SUM_BOUND * sums[2 * c + 1], (cut, c)
            p, s = from_sums(both[2 * c:2 * c + 2], n)
            assert abs(p - price[c]) <= SUM_BOUND * abs(price[c]), (cut, c)
            assert abs(s - se[c]) <= SUM_BOUND * se[c] * max(1.0, 0.5 + (price[c] / se[c]) ** 2 / n), (cut, c)
        A.free()
        B.free()
    P.free()


@pytest.mark.parametrize("count", [64, 130])
def test_the_early_exit_changes_no_bit(eng, count):
    """All paths but one are called at the first date and one lives to maturity: each path alone, all together, and as many
    copies of the live one -- a wave that stops reading against waves that cannot -- and the same with a cliquet in the chunk,
    where no wave may stop."""
    n_steps, live = 20, 37
    rng = np.random.default_rng(count)
    X = 100.0 * np.exp(np.cumsum(np.concatenate([np.zeros((count, 1)), 0.03 * rng.standard_normal((count, n_steps))], axis=1), axis=1))
    X[:, 1] = 100.0 * (1.02 + 0.1 * rng.random(count))                         # called at the first date ...
    X[live, 1:] = 100.0 * np.linspace(0.97, 0.55, n_steps)                     # ... but this one: never called, knocked in
    sched = [(j, COUPON | CALL | KI | (RESET if j in (1, 9, 20) else 0)) for j in range(1, n_steps + 1)]
    auto = [mc.autocall(1.0, 0.02, 0.8, 0.7, 1.0, memory=True), mc.autocall(1.01, 0.01, 0.9, 0.6, 0.9)]
    for book in (auto, auto + [mc.cliquet(-0.02, 0.03, 0.0, INF)]):
        P = eng.from_host(X)
        vals, stop = eng.sched_path_values(P, R, DT, sched, book)
        assert (np.delete(stop[:2], live, axis=1) == 0).all() and (stop[:2, live] == n_steps).all()
        assert (vals[:2, live] < 0.75).all()
        want = check_values(eng, P, X, R, DT, sched, book, ("early exit", count, len(book)))
        check_prices(eng, P, R, DT, sched, book, want, ("early exit", count, len(book)))
        P.free()
        for p in sorted({0, 1, live - 1, live, live + 1, count - 1}):
            Q = eng.from_host(X[p:p + 1])
            v1, s1 = eng.sched_path_values(Q, R, DT, sched, book)
            assert bits(v1[:, 0]) == bits(vals[:, p]) and bits(s1[:, 0]) == bits(stop[:, p]), p
            Q.free()
        C = eng.from_host(np.repeat(X[live:live + 1], count, axis=0))
        vc, sc = eng.sched_path_values(C, R, DT, sched, book)
        assert all(bits(vc[:, p]) == bits(vals[:, live]) and bits(sc[:, p]) == bits(stop[:, live]) for p in range(count))
        C.free()
        if len(book) == 2:
            without = vals
        else:
            assert bits(vals[:2]) == bits(without)                 # the autocallables' values, with the skip and without it


def test_rules(eng):
    P = eng.gbm(1, 100.0, R, 0.2, DT, 10, 300)
    L = mc.load_library()
    nan = math.nan
    ok_s = [(2, COUPON | CALL | RESET), (5, KI), (10, COUPON | CALL | RESET)]
    a_ok, c_ok = mc.autocall(1.0, 0.02, 0.8, 0.7, 1.0), mc.cliquet(0.0)

    def contract(base, **fields):
        d = dict(zip([k for k, _ in N.Sched._fields_], base))
        d.update(fields)
        return d

    def refused(sched=ok_s, book=(a_ok, c_ok), r=R, dt=DT, engine=eng, paths=P, status=1):
        for call in (engine.price_scheduled, engine.sched_path_values):
            with pytest.raises(mc.McgError) as e:
                call(paths, r, dt, raw_obs(sched), list(book))
            assert e.value.status == status and str(e.value) and L.mcg_last_error(), (sched, book, r, dt)

    eng.price_scheduled(P, R, DT, raw_obs(ok_s), [a_ok, c_ok])
    refused(book=[])
    refused(book=[a_ok] * 1025)
    eng.price_scheduled(P, R, DT, raw_obs(ok_s), [a_ok] * 1024)
    refused(sched=[])
    refused(sched=[(j, CALL) for j in range(12)])                 # n_obs > n_steps + 1
    eng.price_scheduled(P, R, DT, raw_obs([(j, CALL) for j in range(11)]), [a_ok])
    refused(sched=[(2, CALL), (2, CALL)])
    refused(sched=[(5, CALL), (2, CALL)])
    refused(sched=[(-1, CALL), (2, CALL)])
    refused(sched=[(2, CALL), (11, CALL)])
    refused(sched=[(2, 16)])
    refused(sched=[(2, -1)])
    refused(book=[contract(a_ok, kind=2)])
    refused(book=[a_ok, contract(a_ok, kind=-1)])
    for r in (nan, INF):
        refused(r=r)
    for dt in (0.0, -DT, nan, INF):
        refused(dt=dt)
    for bad in (dict(put_strike=0.0), dict(put_strike=-1.0), dict(put_strike=nan), dict(coupon=nan), dict(coupon=INF), dict(coupon_level=INF),
                dict(coupon_level=nan), dict(ki_level=nan), dict(ki_level=-INF), dict(call_level=nan)):
        refused(book=[a_ok, contract(a_ok, **bad)])
    refused(sched=[(2, CALL | RESET), (5, KI)], book=[c_ok])    # one RESET date
    refused(sched=[(2, CALL), (5, KI)], book=[a_ok, c_ok])      # none
    eng.price_scheduled(P, R, DT, raw_obs([(2, CALL), (5, KI)]), [a_ok])      # ... which autocallables do not need
    for bad in (dict(local_floor=nan), dict(local_cap=nan), dict(global_floor=nan), dict(global_cap=nan), dict(local_floor=0.1, local_cap=0.0),
                dict(global_floor=0.1, global_cap=0.0)):
        refused(book=[contract(c_ok, **bad)])
    # fields the other kind reads may hold anything; the bounds may be infinite, the call level too
    p, _ = eng.price_scheduled(P, R, DT, raw_obs(ok_s), [contract(a_ok, local_floor=nan, global_cap=nan, call_level=INF),
                                                          contract(c_ok, put_strike=nan, coupon=nan, call_level=nan, local_floor=-INF, global_cap=INF)])
    assert np.isfinite(p).all()
    with mc.PathEngine(0) as other:
        refused(engine=other)
    E = eng.gbm(1, 100.0, R, 0.2, DT, 10, 0)
    refused(paths=E, status=6)
    refused(paths=E, sched=[(2, 16)])                           # the arguments are checked first
    P.free()


def test_closed_forms(eng):
    n, steps, sigma = 200_000, 50, 0.2
    T = steps * DT
    P = eng.gbm(SEED, 100.0, R, sigma, DT, steps, n)
    # the deterministic note
    sched = [(10, COUPON | CALL), (25, COUPON | CALL | KI), (50, COUPON | CALL)]
    price, se = eng.price_scheduled(P, R, DT, sched, [mc.autocall(INF, 0.025, 0.0)])
    d = discounts(R, DT, sched)
    want = sum(0.025 * dk for dk in d) + d[-1]
    print(f"deterministic note: {price[0]:.16g} against {want:.16g}, std error {se[0]:.3g}")
    assert abs(price[0] - want) <= 1e-13
    # the European knock-in note is a bond less 1/K puts
    K = 0.9
    note, _ = eng.price_scheduled(P, R, DT, [(steps, KI)], [mc.autocall(INF, 0.0, 0.0, K, K)])
    put, _ = eng.price_european(P, K * 100.0, R, T, False)
    want = math.exp(-R * T) - put / (K * 100.0)
    print(f"European knock-in note: {note[0]:.16g} against {want:.16g}")
    assert abs(note[0] - want) <= 1e-12 * want
    # the forward-start call on the return, and a floor-0 cliquet of five periods
    fs, fs_se = eng.price_scheduled(P, R, DT, [(20, RESET), (steps, RESET)], [mc.cliquet(0.0)])
    want = forward_start_call(R, sigma, 20 * DT, T, T)
    print(f"forward-start call: {fs[0]:.6f} +- {fs_se[0]:.6f}, closed form {want:.6f}")
    assert fs_se[0] > 0.0 and abs(fs[0] - want) <= 4.0 * fs_se[0]
    resets = [0, 10, 20, 30, 40, 50]
    cq, cq_se = eng.price_scheduled(P, R, DT, [(j, RESET) for j in resets], [mc.cliquet(0.0)])
    want = sum(forward_start_call(R, sigma, a * DT, b * DT, T) for a, b in zip(resets, resets[1:]))
    print(f"floor-0 cliquet: {cq[0]:.6f} +- {cq_se[0]:.6f}, closed form {want:.6f}")
    assert abs(cq[0] - want) <= 4.0 * cq_se[0]
    P.free()


def test_launch_accounting(eng):
    P = eng.gbm(1, 100.0, R, 0.2, DT, 50, 10_000)
    sched = [(25, COUPON | CALL), (50, COUPON | CALL)]
    eng.timing_enable(True)
    eng.timing_reset()
    eng.price_scheduled(P, R, DT, sched, [mc.autocall(1.0, 0.02)], return_hist=True)
    ms, launches = eng.timing_get(N.K_EXOTIC)
    assert launches == 2 and ms > 0.0              # the book kernel and the reduction: no statistics pass
    eng.sched_path_values(P, R, DT, sched, [mc.autocall(1.0, 0.02)])
    assert eng.timing_get(N.K_EXOTIC)[1] == 3
    eng.timing_enable(False)
    P.free()
