"""The multi-asset GBM generator and the combinations on the GPU (mcg_paths_gbm_multi, mcg_paths_combine;
PathEngine.gbm_multi, PathEngine.combine) against the numpy reference of tests/test_gbm_multi_reference.py on the same
(seed, path ids), against the one-asset GBM generator, for the bit identities of the contract, on matrices of other
generators, for its refusals, through the consumers of a path matrix and against closed forms.

Parity bounds: S is compared relatively.  The device draws the same normals with its own logarithm, sine / cosine and square
root, sums an exponent with fused multiply-adds and takes its own exponential (<= ~2 ulp each), so the difference from numpy
is rounding that accumulates over the steps.  S_BOUND is ten times the largest error observed on an MI355X over all cases of
this file (observed: 1.60e-14, on the 252-step shape of the "three" set; the dense sets of four to eight assets stay within
6.66e-15, on the 252-step shape of "dense-5"), far inside the 1e-9 it may not exceed; GBM_BOUND, for
the one-asset matrix against mcg_paths_gbm, is ten times the 4.11e-15 observed there (252 steps, sigma = 1.5), inside the
project's GBM bound of 1e-11.  A best-of / worst-of matrix equals combine_numpy of the downloaded asset matrices bit for bit
(one rounded product per asset, then max / min); a basket differs from it by the fused additions only: (D + 1) 2^-52 on the
scale sum |w_a| S^a (observed: 2.69e-16 from the fused kernels; 3.51e-16 from mcg_paths_combine of up to eight uploaded
matrices with entries of both signs).  Every k_gbm_multi<D, ., .>, D = 1 .. 8 in its three store forms, runs under an element-wise
assertion here: the parity test on sets of every asset count, the prefix identity that ties asset a of every D to the
eight-asset run, and every asset of every D out of the combined-only kernel alone; k_paths_combine runs at every n_assets and
on more rows than its grid's y holds.  The order-3 American max-call of test_american_max_call_through_lsm2 came out at
13.8977 +- 0.0156 beside the published 13.902."""
import ctypes as C
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from test_exotics_reference import stats_numpy
from test_gbm_multi_reference import (BASKET, BEST_OF, DT, KINDS, MULTI_SETS, R, STAT_SETS, STAT_STEPS, STAT_T, WORST_OF,
                                      check_covariances, check_statistics, combine_numpy, dense_model, model_args, reference,
                                      shapes_of, stat_model)
from test_gpu_exotics import check_prices, full_book
from test_gpu_lsm2 import PRICE_BOUND as LSM2_PRICE_BOUND
from test_heston_reference import PARAMS, SEED64, STAT_SEED
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


# The two shapes of the tests that tie the instantiations to each other: Philox tails 3 and 0, a last workgroup whose upper waves
# lie beyond the row with an odd path_begin above 2^33, and two workgroups.
TIE_SHAPES = ((7, 513, 2 ** 33 + 1, SEED64), (8, 1000, 0, 7))


def test_asset_prefixes_are_bit_identical(eng):
    """Asset a of the d-asset run has the bits of asset a of the eight-asset run, d = 1 .. 8: e_a sums the drivers b <= a only,
    in increasing b with explicit fused multiply-adds on constants of the leading block of the factor, and takes the same
    exponential, so the eight instantiations must agree -- no reference involved."""
    for n_steps, n_paths, begin, seed in TIE_SHAPES:
        gen = dict(seed=seed, dt=DT, n_steps=n_steps, n_paths=n_paths, path_begin=begin)
        eight = host(eng.gbm_multi(**gen, **model_args(dense_model(8)))[0])
        assert eight.shape == (8, n_steps + 1, n_paths) and (eight > 0.0).all() and len({bits(eight[a, 1:]) for a in range(8)}) == 8
        differing = []
        for d in range(1, 9):
            S = host(eng.gbm_multi(**gen, **model_args(dense_model(d)))[0])
            assert S.shape == (d, n_steps + 1, n_paths)
            differing += [(d, a, int((S[a] != eight[a]).sum())) for a in range(d) if bits(S[a]) != bits(eight[a])]
        print(f"{n_steps} x {n_paths}: 36 (d, asset) pairs against the eight-asset run, differing (d, asset, elements): {differing}")
        assert not differing, (n_steps, n_paths, differing)


def isolating_weights(kind, d, a):
    """Weights under which the combination of d positive prices is the price of asset a, exactly: a basket of 0 * S = +0 and
    fma(0, S, acc) = acc; a best-of whose other products, 1e-300 S, lie below every price; a worst-of whose others, 1e300 S, lie
    above."""
    other = {BASKET: 0.0, BEST_OF: 1e-300, WORST_OF: 1e300}[kind]
    return [1.0 if b == a else other for b in range(d)]


def test_every_asset_through_the_combined_only_kernel(eng):
    """k_gbm_multi<d, false, true> stores no asset, and the parity test sees its prices through a sum, a max or a min only:
    here each asset of each d comes out of it alone and must have the bits the assets-only kernel stored, rows 0 .. n_steps."""
    n_steps, n_paths, begin, seed = TIE_SHAPES[0]
    differing, compared = [], 0
    for d in range(1, 9):
        gen = dict(seed=seed, dt=DT, n_steps=n_steps, n_paths=n_paths, path_begin=begin, **model_args(dense_model(d)))
        S = host(eng.gbm_multi(**gen)[0])
        for a in range(d):
            for kind in KINDS:
                none, comb = eng.gbm_multi(combine=kind, weights=isolating_weights(kind, d, a), want_assets=False, **gen)
                c = host([comb])[0]
                compared += 1
                assert none is None and c.shape == S[a].shape
                if bits(c) != bits(S[a]):
                    differing.append((d, a, kind, int((c != S[a]).sum())))
    print(f"{compared} combined-only matrices against the stored assets, differing (d, asset, kind, elements): {differing}")
    assert compared == 108 and not differing, differing


def check_bit_identities(eng, m, gen):
    """Fused == combine(assets), three shards == one call, repeats == the first call, for every kind."""
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


def test_bit_identities(eng):
    m = MULTI_SETS["eight"]
    gen = dict(seed=77, dt=DT, n_steps=10, n_paths=1301, path_begin=4097, **model_args(m))
    check_bit_identities(eng, m, gen)
    # no weights: all ones
    _, c1 = eng.gbm_multi(combine=BASKET, want_assets=False, **gen)
    _, c2 = eng.gbm_multi(combine=BASKET, weights=[1.0] * 8, want_assets=False, **gen)
    assert bits(host([c1])[0]) == bits(host([c2])[0])


def test_bit_identities_of_five_assets(eng):
    """The same at an asset count other than eight, on the dense model: the three k_gbm_multi<5, ., .>, the instantiations with
    the tightest register allocation, and k_paths_combine of five matrices."""
    m = MULTI_SETS["dense-5"]
    gen = dict(seed=SEED64, dt=DT, n_steps=10, n_paths=1301, path_begin=2 ** 33 + 4097, **model_args(m))
    check_bit_identities(eng, m, gen)
    print("dense-5, 10 x 1301 from an odd path_begin above 2^33: fused == combine(assets), shards of 513 / 0 / 788 paths and two "
          "repeats after other work: bit-identical in every kind")


def test_combine_at_every_count(eng):
    """k_paths_combine takes n_assets at run time: n = 1 .. 8 uploaded matrices in every kind, two workgroups and an odd path
    count.  The basket takes entries and weights of both signs; best-of and worst-of positive ones, as the contract asks."""
    n_paths, n_cols = 701, 6
    rng = np.random.default_rng(8)
    signed = 100.0 * rng.standard_normal((8, n_paths, n_cols))
    assert (signed < 0.0).any() and (signed > 0.0).any()
    w_signed = [0.2, -0.1, 0.15, -0.3, 0.05, 0.2, -0.1, 0.25]
    w_positive = [1.0, 1.1, 0.9, 1.3, 0.7, 1.05, 0.95, 1.2]
    positive = np.abs(signed) + 1.0
    up_signed, up_positive = ([eng.from_host(x[a]) for a in range(8)] for x in (signed, positive))
    worst = 0.0
    for n in range(1, 9):
        for kind in KINDS:
            x, up, w = (signed, up_signed, w_signed[:n]) if kind == BASKET else (positive, up_positive, w_positive[:n])
            parts = x[:n].transpose(0, 2, 1)                # [n][n_cols][n_paths], as stored
            M = eng.combine(up[:n], kind, w)
            assert (M.n_paths, M.n_steps) == (n_paths, n_cols - 1)
            got = host([M])[0]
            if kind == BASKET:
                e = basket_error(got, parts, w)
                worst = max(worst, e)
                observed["combine basket"] = max(observed.get("combine basket", 0.0), e)
                assert e <= (n + 1) * EPS, (n, e)
            else:
                assert bits(got) == bits(combine_numpy(parts, kind, w)), (n, kind)
    print(f"combine of 1 .. 8 uploaded matrices: best-of and worst-of bit-identical to numpy, basket within {worst:.2e} of it "
          "on the scale sum |w_a S^a|")
    for M in up_signed + up_positive:
        M.free()


def test_combine_beyond_the_grid_clamp(eng):
    """k_paths_combine walks rows on blockIdx.y, which the launcher clamps to 65 535: on a matrix of 65 601 rows the rows from
    65 535 on are written by the second trip of its stride loop alone."""
    n_paths, n_rows, clamp = 3, 65_601, 65_535
    rng = np.random.default_rng(65_601)
    x = 100.0 * np.exp(0.2 * rng.standard_normal((2, n_paths, n_rows)))
    up = [eng.from_host(x[a]) for a in range(2)]
    assert all((U.n_paths, U.n_steps) == (n_paths, n_rows - 1) for U in up)
    parts = x.transpose(0, 2, 1)
    for kind, w in ((BASKET, [1.0, -0.75]), (BEST_OF, [1.0, 0.9]), (WORST_OF, [1.0, 0.9])):
        M = eng.combine(up, kind, w)
        got = M.to_host().T
        M.free()
        want = combine_numpy(parts, kind, w)
        assert got.shape == want.shape == (n_rows, n_paths)
        if kind == BASKET:
            e, e2 = basket_error(got, parts, w), basket_error(got[clamp:], parts[:, clamp:], w)
            print(f"{kind} of two 3 x 65 601 matrices: {e:.2e} of numpy on the scale sum |w_a S^a|, rows 65 535 .. 65 600 {e2:.2e}")
            observed["combine basket"] = max(observed.get("combine basket", 0.0), e)
            assert e2 <= 3 * EPS and e <= 3 * EPS, (e, e2)
        else:
            wrong, wrong2 = int((got != want).sum()), int((got[clamp:] != want[clamp:]).sum())
            print(f"{kind} of two 3 x 65 601 matrices: {wrong} elements differ from numpy, {wrong2} in rows 65 535 .. 65 600")
            assert bits(got[clamp:]) == bits(want[clamp:]) and bits(got) == bits(want), kind
    for U in up:
        U.free()


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


def test_covariance_law_of_eight_and_five_assets(eng):
    """All 36 + 15 covariances and 8 + 5 means of the terminal log-returns of the dense model against sigma_a sigma_b C_ab T and
    (r - q_a - sigma_a^2 / 2) T, within 4 closed-form standard errors: the check that shares neither the reference's reading
    of the packed triangle nor its stream numbers.  (numpy on the same 1M paths: 1.79 and 1.78 standard errors.)"""
    for d in (8, 5):
        m = dense_model(d)
        assets, _ = eng.gbm_multi(seed=STAT_SEED, dt=STAT_T / STAT_STEPS, n_steps=STAT_STEPS, n_paths=STAT_PATHS, **model_args(m))
        ST = np.stack([a.to_host_step_major()[-1] for a in assets])
        for a in assets:
            a.free()
        check_covariances(m, ST, f"MI355X, dense model, {d} assets")


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
