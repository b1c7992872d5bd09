"""numpy reference of the multi-asset GBM generator and of the combinations (mcg_paths_gbm_multi, mcg_paths_combine) -- the
yardstick of tests/test_gpu_gbm_multi.py: the contract of include/mcgpu.h line for line on the Philox normals of
tests/test_heston_reference.py; the Cholesky factor as a loop in Python floats, which mcg_cholesky_corr must reproduce bit for
bit; the reference's own rounding error on the parity cases (binary64 against 80-bit steps); the law of the scheme against
closed forms (forwards, correlations, Margrabe's exchange option from a spread, from a best-of and from a worst-of; every mean
and covariance of the log-returns of eight assets); that the first assets of a model, factor and scheme, do not depend on how
many follow; and what the library must answer without a GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from test_heston_reference import OWN_ERROR_BOUND, PARITY_SHAPES, SEED64, STAT_PATHS_CPU, STAT_SEED, STD_ERRORS, normal_quad

BASKET, BEST_OF, WORST_OF = "basket", "best_of", "worst_of"
KINDS = (BASKET, BEST_OF, WORST_OF)
R = 0.04
DT = 1.0 / 252.0


def stream_of(b):
    """Philox stream of driver b: the price driver, then 16..22."""
    return 0 if b == 0 else 15 + b


def cholesky_python(corr):
    """The loop of include/mcgpu.h in Python floats (binary64, no fused multiply-add): Cholesky-Banachiewicz, each sum from 0 in
    increasing k, then one subtraction.  Returns the lower factor as an n x n array; ValueError where a pivot is <= 1e-10."""
    c = [[float(x) for x in row] for row in corr]
    n = len(c)
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        s = 0.0
        for k in range(j):
            s = s + L[j][k] * L[j][k]
        d = c[j][j] - s
        if not d > 1e-10:
            raise ValueError("not positive definite")
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, n):
            s = 0.0
            for k in range(j):
                s = s + L[i][k] * L[j][k]
            L[i][j] = (c[i][j] - s) / L[j][j]
    return np.array(L, dtype=np.float64).reshape(n, n)


def gbm_multi_numpy(seed, S0, r, sigma, corr, dt, n_steps, n_paths, path_begin=0, q=None, terminal_only=False, dtype=np.float64):
    """The scheme of include/mcgpu.h: [n_assets][n_steps + 1][n_paths], row n of asset a = S^a_n; with terminal_only the last
    rows alone, [n_assets][n_paths].  dtype: the arithmetic of the constants and steps (Cholesky factor and draws are binary64)."""
    d = len(S0)
    L = cholesky_python(corr)
    q = [0.0] * d if q is None else q
    rr, dtt = dtype(r), dtype(dt)
    drift = [(rr - dtype(q[a]) - dtype(sigma[a]) * dtype(sigma[a]) / 2) * dtt for a in range(d)]
    A = [[dtype(sigma[a]) * np.sqrt(dtt) * dtype(L[a][b]) for b in range(a + 1)] for a in range(d)]
    path = np.uint64(path_begin) + np.arange(n_paths, dtype=np.uint64)
    S = [np.full(n_paths, S0[a], dtype=dtype) for a in range(d)]
    out = None if terminal_only else np.empty((d, n_steps + 1, n_paths), dtype=dtype)
    if out is not None:
        out[:, 0, :] = np.array(S)
    for n in range(n_steps):
        if n & 3 == 0:
            quads = [normal_quad(seed, path, n >> 2, stream_of(b)) for b in range(d)]
        z = [quads[b][n & 3].astype(dtype) for b in range(d)]
        for a in range(d):
            e = drift[a]
            for b in range(a + 1):
                e = e + A[a][b] * z[b]
            S[a] = S[a] * np.exp(e)
            if out is not None:
                out[a, n + 1] = S[a]
    return np.array(S) if terminal_only else out


def combine_numpy(assets, kind, weights=None):
    """The combined matrix of include/mcgpu.h from [n_assets][...] arrays: x_a = w_a S^a (one rounded product each); the basket
    adds them in asset order (the device fuses each further product into its addition), best-of / worst-of take max / min."""
    assets = np.asarray(assets)
    w = np.ones(len(assets)) if weights is None else np.asarray(weights, dtype=np.float64)
    x = [w[a] * assets[a] for a in range(len(assets))]
    acc = x[0]
    for a in range(1, len(assets)):
        acc = acc + x[a] if kind == BASKET else np.maximum(acc, x[a]) if kind == BEST_OF else np.minimum(acc, x[a])
    return acc


def banded(n, rho):
    return [[rho ** abs(i - j) for j in range(n)] for i in range(n)]


# ---- the element-wise cases (reused by tests/test_gpu_gbm_multi.py) -----------------------------------------------------------
# name -> model; every set runs over the shapes of test_heston_reference.PARITY_SHAPES (Philox tails 0..3, path counts that are
# no multiples of 512, an odd path_begin, ids above 2^33, both seeds), "three" and "dense-5" over one long shape too (the dense
# sets follow below: with them every asset count from one to eight has a set).  Basket weights hold a
# negative one (a spread) wherever there are two assets; best-of / worst-of take 1 / S0.
MULTI_SETS = {
    "one": dict(S0=[100.0], sigma=[0.2], corr=[[1.0]], q=None, weights=[0.7]),
    "two-high": dict(S0=[100.0, 80.0], sigma=[0.2, 0.35], corr=[[1.0, 0.95], [0.95, 1.0]], q=None, weights=[1.0, -1.25]),
    "two-low-div": dict(S0=[100.0, 120.0], sigma=[0.3, 0.15], corr=[[1.0, -0.95], [-0.95, 1.0]], q=[0.02, 0.05], weights=[0.5, 0.5]),
    "three": dict(S0=[100.0, 55.0, 210.0], sigma=[0.2, 0.0, 0.4], corr=[[1.0, 0.3, -0.5], [0.3, 1.0, 0.2], [-0.5, 0.2, 1.0]],
                  q=[0.0, 0.01, 0.03], weights=[1.0, 2.0, -0.5]),
    "eight": dict(S0=[100.0, 90.0, 110.0, 40.0, 250.0, 75.0, 130.0, 60.0], sigma=[0.2, 0.25, 0.15, 0.45, 0.1, 0.3, 0.22, 0.35],
                  corr=banded(8, 0.6), q=[0.0, 0.02, 0.0, 0.01, 0.03, 0.0, 0.015, 0.0],
                  weights=[0.2, 0.1, 0.15, -0.3, 0.05, 0.2, 0.1, 0.25]),
}
LONG_SHAPE = (252, 1300, 777, SEED64)

# A dense correlation matrix without Toeplitz structure, C_ij = s_i s_j exp(-|x_i - x_j|): the signed Ornstein-Uhlenbeck kernel
# on uneven points, exactly symmetric with an exact unit diagonal in Python floats (smallest squared pivot 0.095, smallest
# eigenvalue 0.047).  Below its first column the factor of banded(n, rho) depends on a - b alone, L_ab = rho^(a-b) sqrt(1 - rho^2),
# so a triangle index that is off by one row and one column reads the same number there; this factor has entries of both signs
# and no two alike.  Every sigma is positive (every driver moves every later asset) and the basket weights hold negative ones.
DENSE_X = [0.0, 0.3, 0.35, 1.1, 1.5, 2.6, 2.7, 4.0]
DENSE_SIGN = [1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0, -1.0]
DENSE_CORR = [[DENSE_SIGN[i] * DENSE_SIGN[j] * math.exp(-abs(DENSE_X[i] - DENSE_X[j])) for j in range(8)] for i in range(8)]
DENSE_WEIGHTS = [0.2, -0.1, 0.15, -0.3, 0.05, 0.2, -0.1, 0.25]


def dense_model(d):
    """The first d assets of the dense eight-asset model: the leading d x d block of its correlation matrix."""
    e = MULTI_SETS["eight"]
    return dict(S0=e["S0"][:d], sigma=e["sigma"][:d], corr=[row[:d] for row in DENSE_CORR[:d]], q=e["q"][:d], weights=DENSE_WEIGHTS[:d])


DENSE_NAMES = {4: "dense-4", 5: "dense-5", 6: "dense-6", 7: "dense-7", 8: "dense-eight"}
MULTI_SETS.update({name: dense_model(d) for d, name in DENSE_NAMES.items()})


def shapes_of(name):
    """"dense-5" takes the long shape as well: k_gbm_multi<5, ., .> is the instantiation with the tightest register allocation."""
    return PARITY_SHAPES + ((LONG_SHAPE,) if name in ("three", "dense-5") else ())


def model_args(m):
    return dict(S0=m["S0"], r=R, sigma=m["sigma"], corr=m["corr"], q=m["q"])


def reference(name, shape, cache={}):
    """One numpy run per (set, shape), shared by every test that needs it and never written to."""
    if (name, shape) not in cache:
        n_steps, n_paths, begin, seed = shape
        cache[(name, shape)] = gbm_multi_numpy(seed, dt=DT, n_steps=n_steps, n_paths=n_paths, path_begin=begin,
                                               **model_args(MULTI_SETS[name]))
    return cache[(name, shape)]


# ---- closed forms ---------------------------------------------------------------------------------------------------------
def norm_cdf(x):
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


def margrabe(S1, S2, q1, q2, s1, s2, rho, T):
    """e^{-rT} E (S^1_T - S^2_T)^+ (Margrabe 1978, with dividend yields)."""
    s = math.sqrt(s1 * s1 + s2 * s2 - 2.0 * rho * s1 * s2)
    d1 = (math.log(S1 / S2) + (q2 - q1 + 0.5 * s * s) * T) / (s * math.sqrt(T))
    return S1 * math.exp(-q1 * T) * norm_cdf(d1) - S2 * math.exp(-q2 * T) * norm_cdf(d1 - s * math.sqrt(T))


# The statistical cases (two assets, T = 1 in 4 steps: the scheme is exact in law at any step count).  The seed is
# test_heston_reference.STAT_SEED; the GPU file takes the first 1M paths of the same seed.
STAT_SETS = {"positive": dict(S0=[100.0, 95.0], sigma=[0.2, 0.3], rho=0.5, q=[0.01, 0.03]),
             "negative": dict(S0=[90.0, 100.0], sigma=[0.35, 0.15], rho=-0.4, q=[0.0, 0.02])}
STAT_T, STAT_STEPS = 1.0, 4


def stat_model(s):
    return dict(S0=s["S0"], r=R, sigma=s["sigma"], corr=[[1.0, s["rho"]], [s["rho"], 1.0]], q=s["q"])


def check_statistics(s, ST, spread, best, worst, where):
    """ST: [2][n] terminal prices; spread, best, worst: [n] terminal rows of the combinations with weights (1, -1), (1, 1), (1, 1).
    Every closed-form check of the issue, within STD_ERRORS of the sample's own standard error."""
    n = ST.shape[1]
    D = math.exp(-R * STAT_T)
    for a in range(2):
        want = s["S0"][a] * math.exp((R - s["q"][a]) * STAT_T)
        se = float(ST[a].std(ddof=1)) / math.sqrt(n)
        print(f"{where}: E S^{a}_T = {ST[a].mean():.4f} +- {se:.4f}, want {want:.4f}: {abs(ST[a].mean() - want) / se:.2f} std errors")
        assert abs(ST[a].mean() - want) <= STD_ERRORS * se, (where, a)
    lr = np.log(ST / np.array(s["S0"])[:, None])
    rho = float(np.corrcoef(lr)[0, 1])
    rho_se = (1.0 - s["rho"] ** 2) / math.sqrt(n)   # of the sample correlation of a bivariate normal
    print(f"{where}: correlation of the log-returns {rho:.5f} +- {rho_se:.5f}, want {s['rho']}: {abs(rho - s['rho']) / rho_se:.2f} std errors")
    assert abs(rho - s["rho"]) <= STD_ERRORS * rho_se, where
    want = margrabe(s["S0"][0], s["S0"][1], s["q"][0], s["q"][1], s["sigma"][0], s["sigma"][1], s["rho"], STAT_T)
    fwd1, fwd2 = s["S0"][0] * math.exp(-s["q"][0] * STAT_T), s["S0"][1] * math.exp(-s["q"][1] * STAT_T)
    x = D * np.maximum(spread, 0.0)
    estimates = {"spread": (float(x.mean()), float(x.std(ddof=1)) / math.sqrt(n)),
                 # max = S^2 + (S^1 - S^2)^+  and  min = S^1 - (S^1 - S^2)^+, the forwards taken in closed form
                 "best-of": (D * float(best.mean()) - fwd2, D * float(best.std(ddof=1)) / math.sqrt(n)),
                 "worst-of": (fwd1 - D * float(worst.mean()), D * float(worst.std(ddof=1)) / math.sqrt(n))}
    for k, (got, se) in estimates.items():
        print(f"{where}: Margrabe from the {k}: {got:.4f} +- {se:.4f}, closed form {want:.4f}: {abs(got - want) / se:.2f} std errors")
        assert abs(got - want) <= STD_ERRORS * se, (where, k, got, want, se)


def check_covariances(model, ST, where):
    """ST: [d][n] terminal prices of `model` (S0, sigma, corr, q) at STAT_T.  The log-returns are jointly normal with means
    (r - q_a - sigma_a^2 / 2) T and covariances sigma_a sigma_b C_ab T: every mean and every entry of the sample covariance
    matrix within STD_ERRORS closed-form standard errors, which are exact for a normal sample of size n -- sigma_a sqrt(T / n)
    for a mean, sqrt((var_a var_b + cov_ab^2) / (n - 1)) for a covariance.  Nothing here comes from the sample but the estimates.
    Returns the worst deviations (covariances, means) in standard errors."""
    d, n = ST.shape
    sigma, q, corr = model["sigma"], model["q"] or [0.0] * d, model["corr"]
    lr = np.log(ST / np.array(model["S0"])[:, None])
    mean, cov = lr.mean(axis=1), np.cov(lr, ddof=1).reshape(d, d)
    means, covs = [], []            # (deviation in standard errors, what, got, want, se)
    for a in range(d):
        want = (R - q[a] - sigma[a] * sigma[a] / 2.0) * STAT_T
        se = sigma[a] * math.sqrt(STAT_T / n)
        means.append((abs(float(mean[a]) - want) / se, (a,), float(mean[a]), want, se))
        for b in range(a + 1):
            want = sigma[a] * sigma[b] * corr[a][b] * STAT_T
            se = math.sqrt((sigma[a] ** 2 * sigma[b] ** 2 * STAT_T ** 2 + want * want) / (n - 1))
            covs.append((abs(float(cov[a, b]) - want) / se, (a, b), float(cov[a, b]), want, se))
    print(f"{where}: {d} assets, {n} paths: worst of {len(covs)} covariances {max(covs)[0]:.2f} std errors at {max(covs)[1]}, "
          f"worst of {d} means {max(means)[0]:.2f} at {max(means)[1]}")
    for dev, *rest in means + covs:
        assert dev <= STD_ERRORS, (where, dev, rest)
    return max(covs)[0], max(means)[0]


# ---- tests ----------------------------------------------------------------------------------------------------------------
CHOLESKY_CASES = {"n1": [[1.0]], "n2": [[1.0, -0.3], [-0.3, 1.0]], "n2-0.999": [[1.0, 0.999], [0.999, 1.0]],
                  "n3": MULTI_SETS["three"]["corr"], "n3-0.999": [[1.0, 0.999, 0.5], [0.999, 1.0, 0.52], [0.5, 0.52, 1.0]],
                  "n8": banded(8, 0.6), "n8-0.999": banded(8, 0.999), "n8-negative": banded(8, -0.7),
                  **{name: MULTI_SETS[name]["corr"] for name in DENSE_NAMES.values()}}


@pytest.mark.parametrize("name", sorted(CHOLESKY_CASES))
def test_cholesky_is_the_python_loop_bit_for_bit(name):
    c = np.array(CHOLESKY_CASES[name])
    got, want = mc.cholesky_corr(c), cholesky_python(c)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
    assert (np.triu(got, 1) == 0.0).all()
    e_np = float(np.abs(got - np.linalg.cholesky(c)).max())
    e_c = float(np.abs(got @ got.T - c).max())
    print(f"{name}: against numpy.linalg.cholesky {e_np:.2e}, L L^T against C {e_c:.2e}")
    assert e_np <= 1e-14 and e_c <= 1e-15


def test_cholesky_of_a_leading_block_is_the_leading_block_of_the_factor():
    """Row j of the Banachiewicz loop reads rows 0 .. j of C and of L only, so the factor of the leading d x d block is the
    leading block of the factor, bit for bit -- what makes asset a of mcg_paths_gbm_multi independent of n_assets."""
    c = np.array(DENSE_CORR)
    full, full_py = mc.cholesky_corr(c), cholesky_python(c)
    assert full.tobytes() == full_py.tobytes()
    assert len({abs(float(full[a, b])) for a in range(8) for b in range(a + 1)}) == 36       # no two entries alike ...
    assert (np.tril(full) < 0.0).any() and (np.tril(full, -1) > 0.0).any()                 # ... and both signs
    for d in range(1, 8):
        block = np.ascontiguousarray(c[:d, :d])
        want = np.ascontiguousarray(full[:d, :d])
        assert mc.cholesky_corr(block).tobytes() == want.tobytes(), d
        assert cholesky_python(block).tobytes() == want.tobytes(), d


def test_dense_model_is_what_it_says():
    c = np.array(DENSE_CORR)
    assert np.array_equal(c, c.T) and (np.diag(c) == 1.0).all()
    pivots = np.diag(cholesky_python(c)) ** 2
    eig = np.linalg.eigvalsh(c)
    print(f"dense model: smallest squared pivot {pivots.min():.3f}, smallest eigenvalue {eig.min():.3f}")
    assert pivots.min() > 0.09 and eig.min() > 0.04
    for d, name in DENSE_NAMES.items():
        m = MULTI_SETS[name]
        assert len(m["S0"]) == d and all(s > 0.0 for s in m["sigma"]) and min(m["weights"]) < 0.0
        assert m["corr"] == [row[:d] for row in DENSE_CORR[:d]]


def test_first_assets_of_the_scheme_do_not_depend_on_the_asset_count():
    """e_a sums the drivers b <= a only, with constants of the leading block of the factor: the first d assets of the
    eight-asset run are the d-asset run, bit for bit."""
    for shape in PARITY_SHAPES:
        n_steps, n_paths, begin, seed = shape
        eight = reference("dense-eight", shape)
        for d in range(1, 8):
            part = reference(DENSE_NAMES[d], shape) if d in DENSE_NAMES else gbm_multi_numpy(
                seed, dt=DT, n_steps=n_steps, n_paths=n_paths, path_begin=begin, **model_args(dense_model(d)))
            assert part.shape == (d, n_steps + 1, n_paths) and part.tobytes() == eight[:d].tobytes(), (shape, d)


def test_cholesky_may_work_in_place():
    c = np.array(CHOLESKY_CASES["n8"])
    want = mc.cholesky_corr(c)
    dp = C.POINTER(C.c_double)
    assert mc.load_library().mcg_cholesky_corr(c.ctypes.data_as(dp), 8, c.ctypes.data_as(dp)) == 0
    assert c.tobytes() == want.tobytes()


REJECTED = {"asymmetric": ([[1.0, 0.5], [0.4, 1.0]], "symmetric"),
            "diagonal": ([[1.0, 0.5], [0.5, 0.999]], "diagonal"),
            "above one": ([[1.0, 1.0000001], [1.0000001, 1.0]], "exceeds 1"),
            "perfectly correlated": ([[1.0, 1.0], [1.0, 1.0]], "not positive definite"),
            "indefinite": ([[1.0, 0.9, -0.9], [0.9, 1.0, 0.9], [-0.9, 0.9, 1.0]], "not positive definite"),
            "n = 0": (np.zeros((0, 0)), "[1, 8]"),
            "n = 9": (np.eye(9), "[1, 8]"),
            "nan": ([[1.0, float("nan")], [float("nan"), 1.0]], "finite")}


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_cholesky_rejects(name):
    c, message = REJECTED[name]
    c = np.ascontiguousarray(c, dtype=np.float64)
    L = mc.load_library()
    out = np.full(max(c.size, 1), 7.0)
    dp = C.POINTER(C.c_double)
    assert L.mcg_cholesky_corr(c.ctypes.data_as(dp), c.shape[0], out.ctypes.data_as(dp)) == 1    # MCG_ERR_INVALID
    assert message in L.mcg_last_error().decode(), L.mcg_last_error()
    assert (out == 7.0).all()                                                                    # nothing written
    with pytest.raises(mc.McgError, match=message.replace("[", r"\[").replace("]", r"\]")):
        mc.cholesky_corr(c)
    if name in ("perfectly correlated", "indefinite"):
        with pytest.raises(ValueError, match=message):
            cholesky_python(c)


def test_library_exports_and_rejects_without_a_gpu():
    L = mc.load_library()
    for name in ("mcg_cholesky_corr", "mcg_paths_gbm_multi", "mcg_paths_combine"):
        assert hasattr(L, name), name
    assert N.K_MULTI == 12 and N.KERNEL_NAMES[N.K_MULTI] == "multi"
    assert (N.C_NONE, N.C_BASKET, N.C_BEST_OF, N.C_WORST_OF) == (-1, 0, 1, 2)
    dp = C.POINTER(C.c_double)
    two = np.array([100.0, 90.0])
    corr = np.eye(2)
    handles, h = (C.c_void_p * 2)(1, 1), C.c_void_p(1)
    rc = L.mcg_paths_gbm_multi(None, 7, 2, two.ctypes.data_as(dp), 0.04, None, two.ctypes.data_as(dp), corr.ctypes.data_as(dp),
                               DT, 8, 0, 16, N.C_BASKET, None, handles, C.byref(h))
    assert rc == 1 and b"NULL" in L.mcg_last_error()
    assert h.value is None and handles[0] is None and handles[1] is None        # every output handle is NULL on error
    h = C.c_void_p(1)
    assert L.mcg_paths_combine(None, handles, 2, N.C_BASKET, None, C.byref(h)) == 1 and b"NULL" in L.mcg_last_error()
    assert h.value is None
    assert hasattr(mc.PathEngine, "gbm_multi") and hasattr(mc.PathEngine, "combine")


def test_scheme_shapes_shards_and_the_one_asset_law():
    m = MULTI_SETS["three"]
    S = gbm_multi_numpy(3, dt=DT, n_steps=11, n_paths=700, **model_args(m))
    assert S.shape == (3, 12, 700) and (S > 0.0).all() and all((S[a, 0] == m["S0"][a]).all() for a in range(3))
    S2 = gbm_multi_numpy(3, dt=DT, n_steps=11, n_paths=400, path_begin=300, **model_args(m))
    assert np.array_equal(S[:, :, 300:], S2)                                    # a path depends on (seed, id) only
    assert np.array_equal(gbm_multi_numpy(3, dt=DT, n_steps=11, n_paths=700, terminal_only=True, **model_args(m)), S[:, -1])
    # sigma = 0: the asset grows at r - q whatever the others do
    assert np.abs(S[1, -1] / (55.0 * math.exp((R - 0.01) * 11 * DT)) - 1.0).max() <= 1e-14
    # the first asset never sees the other drivers: it is the one-asset model, i.e. GBM on the price stream
    one = gbm_multi_numpy(3, [100.0], R, [0.2], [[1.0]], DT, 11, 700)
    assert np.array_equal(one[0], S[0])
    z = np.stack([normal_quad(3, np.arange(700, dtype=np.uint64), n >> 2, 0)[n & 3] for n in range(11)])
    gbm = 100.0 * np.exp(np.cumsum((R - 0.02) * DT + 0.2 * math.sqrt(DT) * z, axis=0))
    assert np.abs(one[0, 1:] / gbm - 1.0).max() <= 1e-13
    # combinations
    w = [1.0, 2.0, -0.5]
    assert np.allclose(combine_numpy(S, BASKET, w), S[0] + 2.0 * S[1] - 0.5 * S[2], rtol=1e-15)
    assert np.array_equal(combine_numpy(S, BEST_OF), S.max(axis=0)) and np.array_equal(combine_numpy(S, WORST_OF), S.min(axis=0))


@pytest.mark.skipif(np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps, reason="no wider float than binary64 here")
def test_parity_cases_are_well_conditioned():
    """The reference's own rounding error on every element-wise case of the GPU file: binary64 against 80-bit arithmetic on the
    same draws."""
    worst = 0.0
    for name, m in MULTI_SETS.items():
        shapes = shapes_of(name)
        assert {s[0] & 3 for s in shapes} == {0, 1, 2, 3} and all(s[1] % 512 for s in shapes)
        for shape in shapes:
            n_steps, n_paths, begin, seed = shape
            Sl = gbm_multi_numpy(seed, dt=DT, n_steps=n_steps, n_paths=n_paths, path_begin=begin, dtype=np.longdouble, **model_args(m))
            e = float(np.abs(reference(name, shape) / Sl - 1.0).max())
            worst = max(worst, e)
            assert e <= OWN_ERROR_BOUND, (name, shape, e)
    print(f"the reference against itself in 80-bit arithmetic: largest difference {worst:.2e}")


@pytest.mark.parametrize("name", sorted(STAT_SETS))
def test_scheme_against_the_closed_forms(name):
    s = STAT_SETS[name]
    ST = gbm_multi_numpy(STAT_SEED, dt=STAT_T / STAT_STEPS, n_steps=STAT_STEPS, n_paths=STAT_PATHS_CPU, terminal_only=True,
                         **stat_model(s))
    check_statistics(s, ST, combine_numpy(ST, BASKET, [1.0, -1.0]), combine_numpy(ST, BEST_OF), combine_numpy(ST, WORST_OF), name)


def test_scheme_against_the_covariance_law():
    """All 36 covariances and 8 means of the dense model's log-returns.  (The reference on this seed: 2.20 and 1.58 standard
    errors at 200 000 paths, 1.79 and 1.78 on the first 1M, the GPU file's sample.)"""
    m = dense_model(8)
    ST = gbm_multi_numpy(STAT_SEED, dt=STAT_T / STAT_STEPS, n_steps=STAT_STEPS, n_paths=STAT_PATHS_CPU, terminal_only=True,
                         **model_args(m))
    check_covariances(m, ST, "numpy, dense model")
    check_covariances(dense_model(5), ST[:5], "numpy, its first five assets")
