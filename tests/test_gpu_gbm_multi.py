"""The multi-asset GBM generator and the combinations on the GPU (mcg_paths_gbm_multi, mcg_paths_combine;
PathEngine.gbm_multi, PathEngine.combine) against the numpy reference of tests/test_gbm_multi_reference.py on the same
(seed, path ids), against the one-asset GBM generator, for the bit identities of the contract, on matrices of other
generators, for its refusals, through the consumers of a path matrix and against closed forms.

Parity bounds: S is compared relatively.  The device draws the same normals with its own logarithm, sine / cosine and square
root, sums an exponent with fused multiply-adds and takes its own exponential (<= ~2 ulp each), so the difference from numpy
is rounding that accumulates over the steps.  S_BOUND is ten times the largest error observed on an MI355X over all cases of
this file (observed: 1.60e-14, on the 252-step shape of the "three" set), far inside the 1e-9 it may not exceed; GBM_BOUND, for
the one-asset matrix against mcg_paths_gbm, is ten times the 4.11e-15 observed there (252 steps, sigma = 1.5), inside the
project's GBM bound of 1e-11.  A best-of / worst-of matrix equals combine_numpy of the downloaded asset matrices bit for bit
(one rounded product per asset, then max / min); a basket differs from it by the fused additions only: (D + 1) 2^-52 on the
scale sum |w_a| S^a (observed: 2.67e-16).  The order-3 American max-call of test_american_max_call_through_lsm2 came out at
13.8977 +- 0.0156 beside the published 13.902."""
import ctypes as C
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from test_exotics_reference import stats_numpy
from test_gbm_multi_reference import (BASKET, BEST_OF, DT, KINDS, MULTI_SETS, R, STAT_SETS, STAT_STEPS, STAT_T, WORST_OF,
                                      check_statistics, combine_numpy, model_args, reference, shapes_of, stat_model)
from test_gpu_exotics import check_prices, full_book
from test_gpu_lsm2 import PRICE_BOUND as LSM2_PRICE_BOUND
from test_heston_reference import PARAMS, STAT_SEED
from test_lsm2_reference import lsm2_numpy

pytestmark = pytest.mark.gpu

S_OBSERVED, GBM_OBSERVED = 1.60e-14, 4.11e-15   # on an MI355X, both on the 252-step shape
S_BOUND = min(10.0 * S_OBSERVED, 1e-9)
GBM_BOUND = min(10.0 * GBM_OBSERVED, 1e-11)
EPS = 2.0 ** -52
STAT_PATHS = 1_000_000
observed = {"S": 0.0, "one asset against gbm": 0.0, "basket": 0.0}


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


def host(ms):
    """[n][n_steps + 1][n_paths] from a list of matrices, which it frees."""
    out = np.stack([m.to_host_step_major() for m in ms])
    for m in ms:
        m.free()
    return out


def inv(S0):
    return [1.0 / s for s in S0]


def weights_of(m, kind):
    return m["weights"] if kind == BASKET else inv(m["S0"])


def basket_error(got, assets, w):
    """|got - combine_numpy| on the scale sum |w_a| S^a."""
    scale = np.abs(np.asarray(w))[:, None, None] * np.abs(assets)
    return float((np.abs(got - combine_numpy(assets, BASKET, w)) / scale.sum(axis=0)).max())


@pytest.mark.parametrize("name", sorted(MULTI_SETS))
def test_parity_with_numpy(eng, name):
    m = MULTI_SETS[name]
    d = len(m["S0"])
    for k, shape in enumerate(shapes_of(name)):
        n_steps, n_paths, begin, seed = shape
        want = reference(name, shape)
        gen = dict(seed=seed, dt=DT, n_steps=n_steps, n_paths=n_paths, path_begin=begin, **model_args(m))
        # assets only
        assets, none = eng.gbm_multi(**gen)
        assert none is None and len(assets) == d and all((a.n_paths, a.n_steps) == (n_paths, n_steps) for a in assets)
        S = host(assets)
        e = float(np.abs(S / want - 1.0).max())
        observed["S"] = max(observed["S"], e)
        print(f"{name} {shape}: S {e:.2e}", end="")
        assert e <= S_BOUND, (name, shape, e)
        for kind in KINDS:
            w = weights_of(m, kind)
            # combined only
            none, comb = eng.gbm_multi(combine=kind, weights=w, want_assets=False, **gen)
            assert none is None and (comb.n_paths, comb.n_steps) == (n_paths, n_steps)
            c = host([comb])[0]
            # both: one kind per shape, in turn
            if KINDS[k % 3] == kind:
                assets, comb = eng.gbm_multi(combine=kind, weights=w, **gen)
                assert bits(host(assets)) == bits(S) and bits(host([comb])[0]) == bits(c), (name, shape, kind, "both")
            if kind == BASKET:
                eb = basket_error(c, S, w)
                observed["basket"] = max(observed["basket"], eb)
                assert eb <= (d + 1) * EPS, (name, shape, eb)
                scale = (np.abs(np.asarray(w))[:, None, None] * want).sum(axis=0)
                assert float((np.abs(c - combine_numpy(want, BASKET, w)) / scale).max()) <= S_BOUND + (d + 1) * EPS
            else:
                assert bits(c) == bits(combine_numpy(S, kind, w)), (name, shape, kind)
                assert float(np.abs(c / combine_numpy(want, kind, w) - 1.0).max()) <= S_BOUND + EPS
        print()


def test_one_asset_agrees_with_the_gbm_generator(eng):
    for n_steps, n_paths, begin, seed in shapes_of("three"):
        for sigma in (0.2, 0.0, 1.5):    # (1.5 on daily steps: beyond the GBM kernel's small-exponent modes)
            assets, _ = eng.gbm_multi(seed, [100.0], R, [sigma], [[1.0]], DT, n_steps, n_paths, path_begin=begin)
            P = eng.gbm(seed, 100.0, R, sigma, DT, n_steps, n_paths, path_begin=begin)
            e = float(np.abs(host(assets)[0] / host([P])[0] - 1.0).max())
            observed["one asset against gbm"] = max(observed["one asset against gbm"], e)
            print(f"{n_steps} x {n_paths}, sigma {sigma}: {e:.2e}")
            assert e <= GBM_BOUND, (n_steps, n_paths, sigma, e)


def test_bit_identities(eng):
    m = MULTI_SETS["eight"]
    gen = dict(seed=77, dt=DT, n_steps=10, n_paths=1301, path_begin=4097, **model_args(m))
    assets, _ = eng.gbm_multi(**gen)
    S = host(list(assets))
    for kind in KINDS:
        w = weights_of(m, kind)
        a2, fused = eng.gbm_multi(combine=kind, weights=w, **gen)
        two_step = eng.combine(a2, kind, w)
        f = host([fused])[0]
        assert bits(f) == bits(host([two_step])[0]), kind                    # fused == combine(assets)
        assert bits(host(a2)) == bits(S), kind                                # the assets do not notice the combination
        # three shards, an odd boundary and an empty one in the middle
        parts = []
        for begin, count in ((0, 513), (513, 0), (513, 788)):
            pa, pc = eng.gbm_multi(combine=kind, weights=w, **dict(gen, n_paths=count, path_begin=gen["path_begin"] + begin))
            assert (pc.n_paths, pc.n_steps) == (count, 10)
            parts.append((host(pa), host([pc])[0]))
        assert bits(np.concatenate([p[0] for p in parts], axis=2)) == bits(S), kind
        assert bits(np.concatenate([p[1] for p in parts], axis=1)) == bits(f), kind
        # again, and after other work on the ctx
        eng.gbm(5, 100.0, R, 0.3, DT, 7, 3000).free()
        _, again = eng.gbm_multi(combine=kind, weights=w, want_assets=False, **gen)
        eng.heston(5, 100.0, R, dt=DT, n_steps=5, n_paths=700, **PARAMS["feller"]).free()
        _, third = eng.gbm_multi(combine=kind, weights=w, want_assets=False, **gen)
        assert bits(host([again])[0]) == bits(f) and bits(host([third])[0]) == bits(f), kind
    # no weights: all ones
    _, c1 = eng.gbm_multi(combine=BASKET, want_assets=False, **gen)
    _, c2 = eng.gbm_multi(combine=BASKET, weights=[1.0] * 8, want_assets=False, **gen)
    assert bits(host([c1])[0]) == bits(host([c2])[0])


def test_combine_on_matrices_of_other_generators(eng):
    n_paths, n_steps = 1500, 9
    H = eng.heston(3, 100.0, R, dt=DT, n_steps=n_steps, n_paths=n_paths, **PARAMS["feller"])
    G = eng.gbm(4, 90.0, R, 0.25, DT, n_steps, n_paths)
    rng = np.random.default_rng(1)
    up = 100.0 * np.exp(0.1 * rng.standard_normal((n_paths, n_steps + 1)))
    U = eng.from_host(up)
    parts = np.stack([H.to_host_step_major(), G.to_host_step_major(), up.T])
    w = [0.5, 1.5, -0.25]
    T = n_steps * DT
    for kind in KINDS:
        wk = w if kind == BASKET else [1.0, 1.1, 0.9]
        M = eng.combine([H, G, U], kind, wk)
        got = M.to_host_step_major()
        if kind == BASKET:
            assert basket_error(got, parts, wk) <= 4 * EPS
        else:
            assert bits(got) == bits(combine_numpy(parts, kind, wk)), kind
        # an uploaded matrix among the inputs: S_T is not known to scale with e^{rT}
        assert math.isnan(eng.greeks_european(M, 100.0, R, T, True)["rho"])
        M.free()
        A = eng.combine([H, G], kind, wk[:2])
        g = eng.greeks_european(A, 100.0, R, T, True)
        assert math.isfinite(g["rho"]) and math.isfinite(g["delta"]), kind
        A.free()
    _, fused = eng.gbm_multi(5, [100.0, 90.0], R, [0.2, 0.3], np.eye(2), DT, n_steps, n_paths, combine=WORST_OF, want_assets=False)
    assert math.isfinite(eng.greeks_european(fused, 90.0, R, T, False)["rho"])
    fused.free()
    # refusals: another shape, another engine
    short = eng.gbm(4, 90.0, R, 0.25, DT, n_steps - 1, n_paths)
    fewer = eng.gbm(4, 90.0, R, 0.25, DT, n_steps, n_paths - 1)
    for other in (short, fewer):
        with pytest.raises(mc.McgError, match="paths x"):
            eng.combine([G, other], BASKET)
    with mc.PathEngine(0) as eng2:
        foreign = eng2.gbm(4, 90.0, R, 0.25, DT, n_steps, n_paths)
        with pytest.raises(mc.McgError, match="different ctx"):
            eng.combine([G, foreign], BASKET)
        foreign.free()
    eng.combine([G, H], BEST_OF).free()
    for M in (H, G, U, short, fewer):
        M.free()


def raw_multi(eng, n_assets, S0, sigma, corr, r=R, q=None, dt=DT, n_steps=8, n_paths=100, combine=N.C_BASKET, weights=None,
              want_assets=True, want_combined=True):
    """mcg_paths_gbm_multi as C sees it: (status, message, asset handles, combined handle); pointers may be None."""
    dp = C.POINTER(C.c_double)
    keep = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (S0, q, sigma, corr, weights)]
    S0p, qp, sp, cp, wp = (None if v is None else v.ctypes.data_as(dp) for v in keep)
    handles, h = (C.c_void_p * 8)(*([1] * 8)), C.c_void_p(1)
    rc = eng._L.mcg_paths_gbm_multi(eng._ctx, 7, n_assets, S0p, r, qp, sp, cp, dt, n_steps, 0, n_paths, combine, wp,
                                    handles if want_assets else None, C.byref(h) if want_combined else None)
    # (asset handles: those a valid n_assets names -- outside [1, 8] the library cannot know how many there are; an output
    # that was not passed counts as NULL)
    n = n_assets if want_assets and 1 <= n_assets <= 8 else 0
    return rc, eng._L.mcg_last_error().decode(), [handles[a] for a in range(n)], h.value if want_combined else None


def test_errors(eng):
    ok = dict(n_assets=2, S0=[100.0, 90.0], sigma=[0.2, 0.3], corr=[[1.0, 0.5], [0.5, 1.0]])
    nan, inf = float("nan"), float("inf")
    bad = [
        (dict(S0=None), "NULL"), (dict(sigma=None), "NULL"), (dict(corr=None), "NULL"),
        (dict(want_assets=False, want_combined=False), "both NULL"),
        (dict(n_assets=0), "[1, 8]"), (dict(n_assets=9, S0=[1.0] * 9, sigma=[0.1] * 9, corr=np.eye(9)), "[1, 8]"),
        (dict(S0=[100.0, nan]), "finite"), (dict(sigma=[inf, 0.3]), "finite"), (dict(q=[0.0, nan]), "finite"),
        (dict(r=nan), "finite"), (dict(dt=inf), "finite"), (dict(weights=[1.0, nan]), "finite"),
        (dict(corr=[[1.0, nan], [nan, 1.0]]), "finite"),
        (dict(S0=[100.0, 0.0]), "S0[1] must be > 0"), (dict(S0=[-1.0, 90.0]), "S0[0] must be > 0"),
        (dict(sigma=[0.2, -0.1]), "sigma[1] must be >= 0"),
        (dict(dt=0.0), "dt must be > 0"), (dict(dt=-DT), "dt must be > 0"),
        (dict(n_steps=0), "n_steps"), (dict(n_paths=-1), "n_paths"),
        (dict(corr=[[1.0, 0.5], [0.4, 1.0]]), "symmetric"), (dict(corr=[[1.0, 0.5], [0.5, 0.999]]), "diagonal"),
        (dict(corr=[[1.0, 1.0000001], [1.0000001, 1.0]]), "exceeds 1"), (dict(corr=[[1.0, 1.0], [1.0, 1.0]]), "not positive definite"),
        (dict(n_assets=3, S0=[1.0] * 3, sigma=[0.1] * 3, corr=[[1.0, 0.9, -0.9], [0.9, 1.0, 0.9], [-0.9, 0.9, 1.0]]), "not positive definite"),
        (dict(combine=3), "kind"), (dict(combine=-2), "kind"), (dict(combine=N.C_NONE), "MCG_C_NONE"),
        (dict(combine=N.C_BEST_OF, weights=[1.0, 0.0]), "> 0"), (dict(combine=N.C_WORST_OF, weights=[-1.0, 1.0]), "> 0"),
    ]
    for change, message in bad:
        rc, msg, handles, h = raw_multi(eng, **dict(ok, **change))
        assert rc == 1 and message in msg, (change, rc, msg)
        assert h is None and all(x is None for x in handles), (change, "handles")
        # ... and the ctx is as good as before
        rc, msg, handles, h = raw_multi(eng, **ok)
        assert rc == 0 and h is not None and len(handles) == 2 and all(handles), (change, msg)
        for x in handles + [h]:
            eng._L.mcg_paths_free(C.c_void_p(x))
    # valid edges: sigma = 0, MCG_C_NONE without a combined matrix, q and weights left out, negative basket weights
    rc, msg, handles, h = raw_multi(eng, **dict(ok, sigma=[0.0, 0.0], combine=N.C_NONE, want_combined=False))
    assert rc == 0 and all(handles), msg
    for x in handles:
        eng._L.mcg_paths_free(C.c_void_p(x))
    # mcg_paths_combine
    G = eng.gbm(4, 90.0, R, 0.25, DT, 8, 100)
    dp = C.POINTER(C.c_double)
    two = (C.c_void_p * 2)(G._h.value, G._h.value)
    wbad = np.array([1.0, float("nan")])
    wneg = np.array([1.0, -1.0])
    for args, message in (((None, 2, 0, None), "NULL"), ((two, 0, 0, None), "[1, 8]"), ((two, 9, 0, None), "[1, 8]"),
                          ((two, 2, 3, None), "kind"), ((two, 2, N.C_NONE, None), "kind"),
                          ((two, 2, 0, wbad.ctypes.data_as(dp)), "finite"), ((two, 2, 1, wneg.ctypes.data_as(dp)), "> 0"),
                          (((C.c_void_p * 2)(G._h.value, None), 2, 0, None), "NULL")):
        h = C.c_void_p(1)
        rc = eng._L.mcg_paths_combine(eng._ctx, *args, C.byref(h))
        assert rc == 1 and message in eng._L.mcg_last_error().decode() and h.value is None, (args[1:3], eng._L.mcg_last_error())
        eng.combine([G, G], BASKET, [1.0, -1.0]).free()
    assert eng._L.mcg_paths_combine(eng._ctx, two, 2, 0, None, None) == 1
    spread = eng.combine([G, G], BASKET, [1.0, -1.0])
    assert (spread.to_host_step_major() == 0.0).all()
    spread.free()
    G.free()
    with pytest.raises(mc.McgError, match="unknown combination"):
        eng.gbm_multi(1, [100.0], R, [0.2], [[1.0]], DT, 4, 10, combine="average")


def consumer_matrices(eng):
    """(name, matrix) of a worst-of performance matrix (weights 1 / S0: every row 0 is 1, strikes lie around 1) and a basket."""
    m = MULTI_SETS["three"]
    gen = dict(seed=20251031, dt=0.02, n_steps=50, n_paths=100_003, **model_args(dict(m, sigma=[0.2, 0.3, 0.4])))
    _, worst = eng.gbm_multi(combine=WORST_OF, weights=inv(m["S0"]), want_assets=False, **gen)
    _, basket = eng.gbm_multi(combine=BASKET, weights=[0.4, 0.6, 0.1], want_assets=False, **gen)
    return (("worst-of", worst), ("basket", basket))


def test_consumers(eng):
    T, dt = 1.0, 0.02
    for name, M in consumer_matrices(eng):
        S = M.to_host_step_major()
        level = float(S[0, 0])
        assert (S[0] == level).all() and (S > 0.0).all()
        D = math.exp(-R * T)
        for K, is_call in ((level, False), (0.9 * level, True), (1.1 * level, False)):
            x = np.maximum(S[-1] - K, 0.0) if is_call else np.maximum(K - S[-1], 0.0)
            got, se = eng.price_european(M, K, R, T, is_call)
            assert abs(got - D * x.mean()) <= 1e-12 * D * x.mean(), (name, K, is_call, got)
        st5 = stats_numpy(M.to_host(), 1)
        book = full_book(st5, (0.9 * level, level, 1.1 * level))
        price, se = eng.price_exotics(M, R, T, book)
        check_prices(price, se, book, st5, R, T, name)
        if name == "basket":
            eu, eu_se = eng.price_european(M, level, R, T, False)
            am, am_se = eng.price_lsm(M, R, level, T, dt, False, 2)
            print(f"basket put: European {eu:.4f} +- {eu_se:.4f}, LSM {am:.4f} +- {am_se:.4f}")
            assert am >= eu - 4.0 * math.hypot(eu_se, am_se)
            assert (am, am_se) == eng.price_lsm(M, R, level, T, dt, False, 2)
        M.free()


def test_american_max_call_through_lsm2(eng):
    """Two assets, S0 = K = 100, q = 0.10, sigma = 0.2, r = 0.05, rho = 0, T = 3, 9 exercise dates: the American max-call of
    Broadie and Glasserman (1997), 13.90 (Andersen and Broadie 2004: 13.902).  price_lsm2 regresses on the best-of with the
    worst-of as its second state; printed beside the benchmark and not asserted against it -- LSM's low bias is not derived here."""
    r, T, n_steps, K = 0.05, 3.0, 9, 100.0
    _, best = eng.gbm_multi(STAT_SEED, [100.0, 100.0], r, [0.2, 0.2], np.eye(2), T / n_steps, n_steps, 200_003, q=[0.1, 0.1],
                            combine=BEST_OF, want_assets=False)
    _, worst = eng.gbm_multi(STAT_SEED, [100.0, 100.0], r, [0.2, 0.2], np.eye(2), T / n_steps, n_steps, 200_003, q=[0.1, 0.1],
                             combine=WORST_OF, want_assets=False)
    B, W = best.to_host_step_major(), worst.to_host_step_major()
    assert (B >= W).all() and (B[1:] > W[1:]).any()
    for poly in (1, 2, 3):
        want, want_se, want_dropped, _ = lsm2_numpy(B, W, r, K, T, T / n_steps, True, poly)
        got, got_se, dropped = eng.price_lsm2(best, worst, r, K, T, T / n_steps, True, poly, return_dropped=True)
        e = abs(got - want) / want
        print(f"American max-call, order {poly}: {got:.4f} +- {got_se:.4f} (numpy {want:.4f}, rel {e:.2e}, dropped {dropped}); "
              "published benchmark 13.902")
        assert e <= LSM2_PRICE_BOUND and dropped == want_dropped, (poly, got, want, dropped, want_dropped)
    best.free()
    worst.free()


@pytest.mark.parametrize("name", sorted(STAT_SETS))
def test_statistics_against_the_closed_forms(eng, name):
    s = STAT_SETS[name]
    gen = dict(seed=STAT_SEED, dt=STAT_T / STAT_STEPS, n_steps=STAT_STEPS, n_paths=STAT_PATHS, **stat_model(s))
    assets, spread = eng.gbm_multi(combine=BASKET, weights=[1.0, -1.0], **gen)
    _, best = eng.gbm_multi(combine=BEST_OF, want_assets=False, **gen)
    _, worst = eng.gbm_multi(combine=WORST_OF, want_assets=False, **gen)
    ST = host(assets)[:, -1]
    check_statistics(s, ST, host([spread])[0][-1], host([best])[0][-1], host([worst])[0][-1], name)


def test_launch_accounting(eng):
    m = MULTI_SETS["two-high"]
    gen = dict(seed=1, dt=DT, n_steps=8, n_paths=5000, **model_args(m))
    eng.timing_enable(True)
    eng.timing_reset()
    _, c = eng.gbm_multi(combine=BEST_OF, want_assets=False, **gen)
    ms, launches = eng.timing_get(N.K_MULTI)
    assert launches == 1 and ms > 0.0 and eng.timing_get(N.K_GBM)[1] == 0
    c.free()
    eng.timing_reset()
    assets, _ = eng.gbm_multi(**gen)
    eng.combine(assets, BEST_OF).free()
    assert eng.timing_get(N.K_MULTI)[1] == 2 and eng.timing_get(N.K_GBM)[1] == 0
    eng.timing_enable(False)
    for a in assets:
        a.free()
