"""CPU side of the dual upper bound for LSM exercise policies (mcg_lsm_dual_upper; PathEngine.dual_upper_lsm): the numpy
restatement of the estimator of include/mcgpu.h that the GPU file (tests/test_gpu_lsm_dual.py) measures against, the cases both
files use, the identities of the restatement, and what needs no GPU -- the refusals and the host code under the sanitizers.

Yardstick
  dual_upper_numpy(policy, M, sigma, q, n_inner, seed, path_begin)   D per outer path, C [n_steps][n_outer], inner_steps and the
      number of undecided decisions: outer or inner decisions of EXERCISE_RULE rows with payoff > 1e-14 and
      |payoff - continuation| <= 1e-9 K (tests/test_lsm_policy_reference.py's notion): only there can a decision flip by
      rounding.  Philox and Box-Muller are tests/test_heston_reference.py's (checked there against the oracle); the inner
      draws are the extension of the RNG contract: key = seed, counter = (g_lo, g_hi, (j << 12) | b, 0x10000 + k), relative
      step s = l - j - 1 uses block s >> 2, element s & 3.  C_j adds its v in ascending k (the library adds slices of
      consecutive k in order: the same sum up to rounding).
Every case of DUAL_CASES, with each of its five policies, has no undecided decision: asserted here, so that on the GPU
inner_steps can be compared exactly and C and D differ by rounding only.
"""
import ctypes as C
import functools
import math
import os
import subprocess
import types

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from test_heston_reference import normal_quad
from test_lsm_policy_reference import (CONT, ITM_EPS, R, RULE, SIGMA, T, TERM, case, continuation_numpy, gbm_matrix, hand_made,
                                       lsm_fit_numpy, payoff)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER_STREAM0 = 0x10000


# ---- the restatement --------------------------------------------------------------------------------------------------------
def exercisable_dates(policy):
    """The dates D is a maximum over: every j < n with not (j dt > maturity), and n."""
    n = policy.n_steps
    return np.array([j for j in range(n) if not (float(j) * policy.dt > policy.maturity)] + [n], dtype=np.int64)


def outer_decisions(policy, M):
    """e [n + 1][n_outer] and the number of undecided ones: the rule at (j, S_j) whether or not the path is still alive."""
    n = policy.n_steps
    e = np.zeros(M.shape, dtype=bool)
    e[n] = True
    close = 0
    for j in range(n):
        if policy.kinds[j] != RULE:
            continue
        pay = payoff(M[j], policy.K, policy.is_call)
        cont = continuation_numpy(policy, j, M[j])
        itm = pay > ITM_EPS
        close += int((itm & (np.abs(pay - cont) <= 1e-9 * policy.K)).sum())
        e[j] = itm & ~(cont > pay)
    return e, close


def inner_values(policy, S_j, j, g, sigma, q, n_inner, seed):
    """v [n_outer][n_inner] of the inner paths from (j, S_j), the steps they took and the undecided decisions on the way."""
    n, K, call = policy.n_steps, policy.K, policy.is_call
    a, m = sigma * math.sqrt(policy.dt), (policy.r - q - 0.5 * sigma * sigma) * policy.dt
    disc = np.exp(-policy.r * policy.dt * np.arange(n + 1))
    shape = (len(S_j), n_inner)
    X, v, alive = np.zeros(shape), np.zeros(shape), np.ones(shape, dtype=bool)
    path = np.broadcast_to(g[:, None], shape)
    stream = np.broadcast_to((INNER_STREAM0 + np.arange(n_inner, dtype=np.uint64))[None, :], shape)
    steps = close = 0
    z = None
    for l in range(j + 1, n + 1):
        s = l - j - 1
        if s & 3 == 0:
            z = normal_quad(seed, path, (j << 12) | (s >> 2), stream)
        steps += int(alive.sum())
        X = X + (a * z[s & 3] + m)
        if l == n:
            stop = alive
            pay = payoff(S_j[:, None] * np.exp(X), K, call)
        elif policy.kinds[l] == RULE:
            S = S_j[:, None] * np.exp(X)
            pay = payoff(S, K, call)
            cont = continuation_numpy(policy, l, S)
            itm = alive & (pay > ITM_EPS)
            close += int((itm & (np.abs(pay - cont) <= 1e-9 * K)).sum())
            stop = itm & ~(cont > pay)
        else:
            continue
        v = np.where(stop, pay * disc[l], v)
        alive = alive & ~stop
        if not alive.any():
            break
    return v, steps, close


def dual_upper_numpy(policy, M, sigma, q, n_inner, seed, path_begin, return_v=False):
    """(D [n_outer], C [n_steps][n_outer], inner_steps, undecided) -- include/mcgpu.h's estimator on the step-major outer
    matrix M [n_steps + 1][n_outer]; with return_v also v [n_steps][n_outer][n_inner]."""
    n, n_outer = policy.n_steps, M.shape[1]
    g = np.uint64(path_begin) + np.arange(n_outer, dtype=np.uint64)
    disc = np.exp(-policy.r * policy.dt * np.arange(n + 1))
    h = payoff(M, policy.K, policy.is_call) * disc[:, None]
    e, close = outer_decisions(policy, M)
    Cm = np.zeros((n, n_outer))
    inner_steps = 0
    vs = []
    for j in range(n):
        v, steps, c = inner_values(policy, M[j], j, g, sigma, q, n_inner, seed)
        acc = np.zeros(n_outer)
        for k in range(n_inner):        # ascending k
            acc = acc + v[:, k]
        Cm[j] = acc / n_inner
        inner_steps += steps
        close += c
        if return_v:
            vs.append(v)
    exercisable = set(exercisable_dates(policy).tolist())
    Mt = np.zeros(n_outer)
    D = np.full(n_outer, -np.inf)
    for j in range(n + 1):
        if j > 0:
            L = h[n] if j == n else np.where(e[j], h[j], Cm[j])
            Mt = Mt + L - Cm[j - 1]
        if j in exercisable:
            D = np.maximum(D, h[j] - Mt)
    out = (D, Cm, inner_steps, close)
    return out + (np.array(vs),) if return_v else out


def mean_and_std_err_from_sums(D):
    n = len(D)
    s, s2 = math.fsum(D), math.fsum(D * D)
    m = s / n
    var = max(0.0, (s2 - n * m * m) / (n - 1)) if n > 1 else 0.0
    return m, math.sqrt(var / n)


# ---- the cases both files use -------------------------------------------------------------------------------------------------
POLICY_NAMES = ("all-continue", "exercise-in-the-money", "linear-boundary", "immediate", "fitted")


def dcase(n_paths, n_steps, n_inner, order, is_call, q=0.0, path_begin=0, names=POLICY_NAMES, **kw):
    c = case(n_paths, n_steps, order, is_call, **kw)
    c.update(n_inner=n_inner, q=q, path_begin=path_begin, inner_seed=900 + 13 * n_paths + n_inner, sigma=SIGMA, names=names)
    return c


# outer counts {1, 2, 3, 127, 129, 513}; dates {1, 2, 7, 50} and 300 once (j << 12 beyond 2^20, block numbers above 64); inner
# counts {1, 3, 64, 65, 130}; orders {0, 2, 3, 5, 15} -- with the hand-made policies' 0 and 1 every one of the three instances the
# inner kernel is compiled in (orders up to 3, up to 7, up to 15) runs; calls and puts; q of 0 and 0.03; one path_begin above 2^32; one case whose
# maturity cuts the last dates off.  Each is run with the four hand-made policies of hand_made() and a fit by lsm_fit_numpy
# (the 300-date case, whose restatement takes 45 000 numpy steps a policy, with the policy that walks every inner path to the
# last date and the fit).
DUAL_CASES = [
    dcase(1, 1, 1, 0, False, S0=95.0),
    dcase(2, 2, 3, 2, True),
    dcase(3, 7, 64, 3, False, q=0.03),
    dcase(127, 50, 3, 3, False),
    dcase(129, 7, 65, 15, True, q=0.03, path_begin=2 ** 32 + 12345, S0=104.0),
    dcase(513, 7, 130, 2, False),
    dcase(513, 50, 1, 3, False, maturity=0.71),
    dcase(5, 300, 2, 2, False, names=("all-continue", "fitted")),
    dcase(129, 50, 3, 5, True),
]
# The cases of the no-noise identity (sigma = 0 on a deterministic outer path): two puts that are in the money on the whole
# path, S0 = 92 (S stays above the linear boundary's 90: that rule holds to the end) and S0 = 85 (below it: that rule exercises
# at once), and a call with a dividend yield.  The GPU file runs the puts on 130 copies of the path.
NOISE_FREE_CASES = [
    dcase(130, 50, 3, 3, False, S0=92.0),
    dcase(130, 7, 2, 2, False, S0=85.0),
    dcase(130, 7, 2, 2, True, q=0.03, S0=108.0),
]


def dual_case_id(c):
    return (f"{c['n_paths']}x{c['n_steps']}x{c['n_inner']}-o{c['order']}-{'call' if c['is_call'] else 'put'}"
            + ("-q" if c["q"] else "") + ("-cut" if c["maturity"] < T else "") + ("-begin" if c["path_begin"] else ""))


def outer_rows(c):
    """The outer matrix of a case, [n_paths][n_steps + 1] (what from_host takes): GBM with the inner model's drift and sigma."""
    return gbm_matrix(c["seed"] + 500000, c["n_paths"], c["n_steps"], c["S0"], R - c["q"], c["sigma"], c["dt"])


@functools.lru_cache(maxsize=None)
def _policies(key):
    c = next(x for x in DUAL_CASES + NOISE_FREE_CASES if dual_case_id(x) == key)
    out = dict(hand_made(c))
    fit_on = gbm_matrix(c["seed"] + 700000, 4001, c["n_steps"], c["S0"], R - c["q"], c["sigma"], c["dt"])
    out["fitted"] = lsm_fit_numpy(np.ascontiguousarray(fit_on.T), R, c["K"], c["maturity"], c["dt"], c["is_call"], c["order"])
    return out


def policies(c):
    """name -> policy: hand_made(c) and an independent fit of the case's order on 4001 paths of its own."""
    return _policies(dual_case_id(c))


@functools.lru_cache(maxsize=None)
def _reference(key, name):
    c = next(x for x in DUAL_CASES if dual_case_id(x) == key)
    M = np.ascontiguousarray(outer_rows(c).T)
    return dual_upper_numpy(policies(c)[name], M, c["sigma"], c["q"], c["n_inner"], c["inner_seed"], c["path_begin"])


def reference(c, name):
    """dual_upper_numpy of (case, policy), computed once a process and shared: do not modify what it returns."""
    return _reference(dual_case_id(c), name)


@pytest.mark.parametrize("c", DUAL_CASES, ids=dual_case_id)
def test_no_undecided_decision_on_the_cases(c):
    for name in c["names"]:
        D, Cm, steps, close = reference(c, name)
        assert close == 0, (dual_case_id(c), name, close)
        assert np.isfinite(D).all() and np.isfinite(Cm).all() and steps >= c["n_paths"] * c["n_inner"] * c["n_steps"]
    n, ni, no = c["n_steps"], c["n_inner"], c["n_paths"]
    assert reference(c, "all-continue")[2] == no * ni * n * (n + 1) // 2      # every inner path walks to the last date


# ---- identities of the restatement ----------------------------------------------------------------------------------------------
def deterministic_matrix(c, n_outer=3):
    j = np.arange(c["n_steps"] + 1)[:, None]
    return np.ascontiguousarray(np.repeat(c["S0"] * np.exp((R - c["q"]) * c["dt"] * j), n_outer, axis=1))


def noise_free_reference(c, policy, n_outer=3):
    """(M, h, dual_upper_numpy(...)) of a policy at sigma = 0 on n_outer copies of the case's deterministic path."""
    M = deterministic_matrix(c, n_outer)
    h = payoff(M, policy.K, policy.is_call) * np.exp(-policy.r * policy.dt * np.arange(c["n_steps"] + 1))[:, None]
    return M, h, dual_upper_numpy(policy, M, 0.0, c["q"], c["n_inner"], 5, 0)


@pytest.mark.parametrize("c", NOISE_FREE_CASES, ids=dual_case_id)
def test_without_noise_the_bound_is_the_best_exercise_date(c):
    """sigma = 0 on an outer path that follows the inner drift: every inner path IS the outer path's future, so C_j is the
    policy's value from j on -- C_j = L_{j+1} --, the martingale vanishes and D = max over the exercisable dates of h_j,
    whatever the policy.  A put with r > 0 and q = 0: h_j = K e^{-r t_j} - S0 falls, D = K - S0, to 1e-13.  The puts are in
    the money on the whole path, so h, C and L are far from zero and the rules differ: all-CONTINUE and (S0 = 92) the linear
    boundary hold to the end, the others exercise at the first date reached or where the fit says."""
    n = c["n_steps"]
    values = set()
    for name, policy in policies(c).items():
        M, h, (D, Cm, steps, close) = noise_free_reference(c, policy)
        assert close == 0, (name, close)
        want = h[exercisable_dates(policy)].max(axis=0)
        assert want.min() > 0.01 * policy.K and Cm[0].min() > 0.01 * policy.K          # nothing here is a comparison of zeros
        assert np.max(np.abs(D - want)) <= 1e-12 * policy.K, (name, D, want)
        e, _ = outer_decisions(policy, M)
        for j in range(n):                                                              # the increments of the martingale
            L = h[n] if j + 1 == n else np.where(e[j + 1], h[j + 1], Cm[j + 1])
            assert np.max(np.abs(L - Cm[j])) <= 1e-12 * policy.K, (name, j)
        if not c["is_call"] and c["q"] == 0.0:
            assert np.max(np.abs(D - (policy.K - c["S0"]))) <= 1e-13, (name, D)
        values.add(round(float(Cm[0, 0]), 6))
    assert len(values) >= 2                                                             # the policies are worth different amounts


@pytest.mark.parametrize("c", [DUAL_CASES[2], DUAL_CASES[3], DUAL_CASES[6]], ids=dual_case_id)
def test_all_continue_telescopes(c):
    """Under an all-CONTINUE policy L_j = C_j, so Mt_j = C_j - C_0 (j < n), Mt_n = h_n - C_0 and
    D = C_0 + max(0, max over the exercisable j < n of (h_j - C_j))."""
    M = np.ascontiguousarray(outer_rows(c).T)
    policy = policies(c)["all-continue"]
    D, Cm, steps, close = reference(c, "all-continue")
    n = c["n_steps"]
    h = payoff(M, policy.K, policy.is_call) * np.exp(-policy.r * policy.dt * np.arange(n + 1))[:, None]
    ex = exercisable_dates(policy)[:-1]
    want = Cm[0] + np.maximum(0.0, (h[ex] - Cm[ex]).max(axis=0))
    assert np.max(np.abs(D - want)) <= 1e-12 * policy.K


def test_inner_sums_add_in_ascending_k():
    c = DUAL_CASES[2]
    M = np.ascontiguousarray(outer_rows(c).T)
    policy = policies(c)["fitted"]
    D, Cm, steps, close, v = dual_upper_numpy(policy, M, c["sigma"], c["q"], c["n_inner"], c["inner_seed"], c["path_begin"], return_v=True)
    assert v.shape == (c["n_steps"], c["n_paths"], c["n_inner"])
    for j in range(c["n_steps"]):
        for i in range(c["n_paths"]):
            acc = 0.0
            for k in range(c["n_inner"]):
                acc += float(v[j, i, k])
            assert Cm[j, i] == acc / c["n_inner"]
    # inner path k's draws are stream 0x10000 + k's, whatever n_inner is: the first inner path of a longer run is the only one of a short one
    v1 = dual_upper_numpy(policy, M, c["sigma"], c["q"], 1, c["inner_seed"], c["path_begin"], return_v=True)[4]
    assert np.max(np.abs(v1[:, :, 0] - v[:, :, 0])) <= 1e-13 * policy.K      # (numpy's vector loops may round a tail element otherwise)
    # ... and an outer path's depend on its global id alone
    Ds = dual_upper_numpy(policy, M[:, 1:], c["sigma"], c["q"], c["n_inner"], c["inner_seed"], c["path_begin"] + 1)[0]
    assert np.max(np.abs(Ds - D[1:])) <= 1e-13 * policy.K


# ---- refusals that need no GPU ---------------------------------------------------------------------------------------------------
def raw_dual(hdr, coef, model, ctx=None, paths=None, upper=True):
    L = mc.load_library()
    dp = C.POINTER(C.c_double)
    up = C.c_double()
    status = L.mcg_lsm_dual_upper(ctx, None if hdr is None else C.byref(hdr), None if coef is None else coef.ctypes.data_as(dp), paths,
                                  None if model is None else C.byref(model), C.byref(up) if upper else None, None, None, None, None, None)
    return status, L.mcg_last_error().decode()


def test_library_exports_and_rejects_without_a_gpu():
    L = mc.load_library()
    assert hasattr(L, "mcg_lsm_dual_upper") and hasattr(L, "mcg_debug_lsm_dual_executed")
    assert N.K_LSM_DUAL == 15 and C.sizeof(N.LsmDualModel) == 40
    good = mc.LsmPolicy.from_arrays(2, 1, False, 0.04, 100.0, 1.0, 0.5, coefficients=[[1.0, 2.0], [3.0, 4.0], [0.0, 0.0]])
    hdr = good._hdr()

    def model(**kw):
        m = N.LsmDualModel(7, 0.2, 0.0, 0, 16, 0)
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    def header(**kw):
        h = good._hdr()
        for k, v in kw.items():
            setattr(h, k, v)
        return h

    def rows(j, t, v):
        c = good.coef.copy()
        c[j, t] = v
        return c

    # a sound policy and model: what is left to refuse is the missing ctx
    status, msg = raw_dual(hdr, good.coef, model())
    assert status == 1 and "NULL" in msg
    bad = [(None, good.coef, model()), (hdr, None, model()), (hdr, good.coef, None),
           (hdr, good.coef, model(n_inner=0)), (hdr, good.coef, model(n_inner=-3)), (hdr, good.coef, model(n_inner=65537)),
           (hdr, good.coef, model(sigma=-0.1)), (hdr, good.coef, model(sigma=math.nan)), (hdr, good.coef, model(sigma=math.inf)),
           (hdr, good.coef, model(q=math.nan)), (hdr, good.coef, model(q=-math.inf)),
           (header(n_steps=16385), good.coef, model()),
           (header(poly_order=16), good.coef, model()), (header(K=0.0), good.coef, model()), (header(dt=-1.0), good.coef, model()),
           (header(r=math.nan), good.coef, model()), (header(n_steps=-1), good.coef, model()),
           (hdr, rows(0, 18, 3.0), model()), (hdr, rows(2, 18, float(CONT)), model()), (hdr, rows(0, 18, float(TERM)), model()),
           (hdr, rows(1, 1, math.nan), model()), (hdr, rows(0, 17, math.inf), model())]
    for h, c, m in bad:
        status, msg = raw_dual(h, c, m)
        assert status == 1 and msg and "ctx/paths/upper" not in msg, (status, msg)
    for m, word in ((model(n_inner=0), "n_inner"), (model(sigma=-0.1), "sigma"), (model(q=math.nan), "q"), (model(n_inner=65537), "65536")):
        assert word in raw_dual(hdr, good.coef, m)[1]
    assert "16384" in raw_dual(header(n_steps=16385), good.coef, model())[1]
    ex = C.c_int64()
    assert L.mcg_debug_lsm_dual_executed(None, C.byref(ex)) == 1 and b"NULL" in L.mcg_last_error()
    # the Python surface checks what a ctypes struct would silently truncate, before the library is called
    stub = types.SimpleNamespace(_alive=lambda: None, n_paths=1, n_steps=2, _h=None)
    for kw in (dict(n_inner=0), dict(n_inner=65537), dict(seed=-1), dict(seed=2 ** 64), dict(path_begin=-1)):
        args = dict(sigma=0.2, n_inner=4, seed=1)
        args.update(kw)
        with pytest.raises(mc.McgError) as e:
            mc.PathEngine.dual_upper_lsm(types.SimpleNamespace(), good, stub, **args)
        assert e.value.status == 1
    res = mc.DualResult(1.5, 0.25, np.array([3.0, 5.0, 2.0]), 12, d=np.zeros(2))
    assert len(res) == 5 and (res.upper, res.std_err, res.inner_steps) == (1.5, 0.25, 12) and res.cont is None and res[4] is res.d
    assert len(mc.DualResult(1.5, 0.25, np.zeros(3), 12)) == 4


# ---- the host code under the sanitizers -----------------------------------------------------------------------------------------
def test_host_dual_code_under_the_sanitizers(tmp_path):
    """tests/cpp/lsm_dual_host_main.cpp with host/lsm_dual.cpp and host/lsm_policy.cpp, compiled with
    -fsanitize=address,undefined into a stand-alone program (the sanitizers' runtimes linked into it) and run directly: the edge
    cases of what mcg_lsm_dual_upper rejects without a ctx and of the slicing of the inner paths; it must exit 0 with nothing
    reported."""
    exe = tmp_path / "lsm_dual_host_main"
    host = os.path.join(ROOT, "montecarlooptionspricer_amd", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "lsm_dual_host_main.cpp"),
           os.path.join(host, "lsm_dual.cpp"), os.path.join(host, "lsm_policy.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-3000:]
