"""numpy reference of the Bates / Merton generator (mcg_paths_bates) -- the yardstick of tests/test_gpu_bates.py: the jump
component of include/mcgpu.h line for line (Poisson thresholds, the count from the uniform of Philox stream 4, the size from
the normal of stream 5) on top of either variance scheme, on the draws of tests/test_heston_reference.py; two closed forms
that know nothing of each other (the Heston characteristic function times the jump factor, and Merton's Poisson-weighted
Black-Scholes series); the conditioning of the element-wise cases (a jump count is a discontinuity in uN: a case that sits
on a threshold cannot carry a bound); the scheme against the closed form; and what the library must answer without a GPU."""
import ctypes as C
import functools
import inspect
import math

import mpmath as mp
import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from test_heston_qe_reference import (DECISION_MARGIN, OWN_ERROR_BOUND, PSI_C, QE_LONG_SHAPE, qe_constants, uniform_of_words,
                                      uniforms)
from test_heston_reference import (FELLER_VIOLATING, LARGE_VOL, NODES, PARAMS, PARITY_SETS, PARITY_SHAPES, R, S0, STAT_PATHS_CPU,
                                   STAT_SEED, STD_ERRORS, STREAM_PRICE, STREAM_VOL, STRIKES, WEIGHTS, black_scholes,
                                   discounted_payoff, heston_cf, heston_closed_form, normal_quad, philox_words)

STREAM_JUMP_COUNT, STREAM_JUMP_SIZE = 4, 5
JUMP_CAP = 16


def jump_constants(lam, mu_j, sigma_j, dt):
    """(comp, c[16]) of include/mcgpu.h in binary64: the compensator of a step and the Poisson CDF, summed in the contract's
    order."""
    L = lam * dt
    kbar = math.exp(mu_j + sigma_j * sigma_j / 2.0) - 1.0
    t = math.exp(-L)
    c = [t]
    for j in range(1, JUMP_CAP):
        t = t * L / j
        c.append(c[-1] + t)
    return -lam * kbar * dt, np.array(c, dtype=np.float64)


def jump_thresholds(L):
    """The sixteen words T_k = floor(min(c_k, 1) 2^32 - 1/2) of lambda dt = L, as ints: uN > c_k <=> word > T_k."""
    _, c = jump_constants(L, 0.0, 0.0, 1.0)
    return [int(math.floor(min(float(ck), 1.0) * 2.0 ** 32 - 0.5)) for ck in c]


def bates_numpy(seed, S0, r, v0, kappa, theta, sigma_v, rho, lam, mu_j, sigma_j, dt, n_steps, n_paths, path_begin=0, scheme="euler",
                terminal_only=False, dtype=np.float64, trace=None):
    """The contract of mcg_paths_bates: (S, v), step-major [n_steps + 1][n_paths]; with terminal_only the last rows alone.
    dtype: the arithmetic of the steps (constants, draws and the jump count are binary64 either way).  trace: a dict that
    receives "jumps" ([n_steps][n_paths], the count of every step), "count_margin" (the smallest |uN - c_k| met) and, for
    the QE scheme, "psi_margin" and "u_margin" as heston_qe_numpy reports them, and "count_margins" ([n_steps][n_paths]: the
    smallest |uN - c_k| of every step)."""
    assert scheme in ("euler", "qe")
    path = np.uint64(path_begin) + np.arange(n_paths, dtype=np.uint64)
    S, v = np.full(n_paths, S0, dtype=dtype), np.full(n_paths, v0, dtype=dtype)
    comp, cdf = jump_constants(lam, mu_j, sigma_j, dt)
    comp, mu_j, sigma_j = dtype(comp), dtype(mu_j), dtype(sigma_j)
    if scheme == "qe":
        E, c1, c2, K0, K1, K2, K3 = (dtype(x) for x in qe_constants(kappa, theta, sigma_v, rho, dt))
        K4, psi_c = K3, dtype(PSI_C)
    r, kappa, theta, sigma_v, rho, dt = (dtype(x) for x in (r, kappa, theta, sigma_v, rho, dt))
    rho_c = np.sqrt(np.maximum(dtype(0.0), 1 - rho * rho))
    if not terminal_only:
        Sm, vm = np.empty((n_steps + 1, n_paths), dtype=dtype), np.empty((n_steps + 1, n_paths), dtype=dtype)
        Sm[0], vm[0] = S, v
    t = dict(jumps=np.zeros((n_steps, n_paths), dtype=np.int64), count_margin=math.inf, psi_margin=math.inf, u_margin=math.inf)
    if trace is not None:
        t["count_margins"] = np.empty((n_steps, n_paths))
    for n in range(n_steps):
        if n & 3 == 0:
            q1, q2 = normal_quad(seed, path, n >> 2, STREAM_PRICE), normal_quad(seed, path, n >> 2, STREAM_VOL)
            q3 = normal_quad(seed, path, n >> 2, STREAM_JUMP_SIZE)
            uq = uniforms(seed, path, n >> 2) if scheme == "qe" else None
            uNq = uniform_of_words(np.stack(philox_words(seed, path, n >> 2, STREAM_JUMP_COUNT)))
        z1, z2, z3, uN = q1[n & 3].astype(dtype), q2[n & 3].astype(dtype), q3[n & 3].astype(dtype), uNq[n & 3]
        # the base scheme's exponent of this step, and its variance
        if scheme == "euler":
            vp = np.maximum(v, 0)
            s = np.sqrt(vp * dt)
            e = (r - vp / 2) * dt + s * (rho * z2 + rho_c * z1)
            vn = v + kappa * (theta - vp) * dt + sigma_v * s * z2
        else:
            u = uq[n & 3].astype(dtype)
            m = theta + (v - theta) * E
            s2 = v * c1 + c2
            with np.errstate(all="ignore"):
                psi = s2 / (m * m)
                q = 2 / psi
                b2 = q - 1 + np.sqrt(q) * np.sqrt(q - 1)
                v_quad = m / (1 + b2) * (np.sqrt(b2) + z2) ** 2
                p = (psi - 1) / (psi + 1)
                beta = (1 - p) / m
                v_exp = np.where(u <= p, dtype(0), np.log((1 - p) / (1 - u)) / beta)
            exponential = (m != 0) & ~(psi <= psi_c)
            vn = np.where(m == 0, dtype(0), np.where(exponential, v_exp, v_quad)).astype(dtype)
            e = r * dt + K0 + K1 * v + K2 * vn + np.sqrt(K3 * v + K4 * vn) * z1
            if trace is not None:
                if (m != 0).any():
                    t["psi_margin"] = min(t["psi_margin"], float(np.abs(psi[m != 0] / psi_c - 1).min()))
                if exponential.any():
                    t["u_margin"] = min(t["u_margin"], float(np.abs(u - p)[exponential].min()))
        # the jump
        N = (uN[None, :] > cdf[:, None]).sum(axis=0)
        Nd = N.astype(dtype)
        J = comp + Nd * mu_j + np.where(N > 0, sigma_j * np.sqrt(Nd) * z3, dtype(0))
        S = S * np.exp(e + J)
        v = vn
        if not terminal_only:
            Sm[n + 1], vm[n + 1] = S, v
        if trace is not None:
            t["jumps"][n] = N
            t["count_margins"][n] = np.abs(uN[None, :] - cdf[:, None]).min(axis=0)
            t["count_margin"] = min(t["count_margin"], float(t["count_margins"][n].min()))
    if trace is not None:
        trace.update(t)
    return (S, v) if terminal_only else (Sm, vm)


# ---- closed forms ------------------------------------------------------------------------------------------------------------
def bates_closed_form(S0, K, r, T, v0, kappa, theta, sigma_v, rho, lam, mu_j, sigma_j, is_call):
    """heston_closed_form's two integrals with the characteristic function of X_T = ln(S_T / S0) - rT under Bates:
    heston_cf(u) exp(lambda T (exp(iu mu_J - sigma_J^2 u^2 / 2) - 1 - iu kbar))."""
    kbar = math.exp(mu_j + sigma_j * sigma_j / 2.0) - 1.0

    def cf(u):
        return heston_cf(u, T, v0, kappa, theta, sigma_v, rho) * np.exp(
            lam * T * (np.exp(1j * u * mu_j - sigma_j * sigma_j * u * u / 2.0) - 1.0 - 1j * u * kbar))

    k = math.log(K / S0) - r * T
    osc = np.exp(-1j * NODES * k) / (1j * NODES)
    P1 = 0.5 + float(np.sum(WEIGHTS * (osc * cf(NODES - 1j)).real)) / math.pi
    P2 = 0.5 + float(np.sum(WEIGHTS * (osc * cf(NODES)).real)) / math.pi
    D = math.exp(-r * T)
    return S0 * P1 - K * D * P2 if is_call else K * D * (1.0 - P2) - S0 * (1.0 - P1)


def merton_series(S0, K, r, T, sigma, lam, mu_j, sigma_j, is_call, terms=80):
    """Merton (1976): conditional on n jumps the price is Black-Scholes with r_n = r - lambda kbar + n ln(1 + kbar) / T and
    sigma_n^2 = sigma^2 + n sigma_J^2 / T, weighted by the Poisson law of intensity lambda (1 + kbar) T."""
    kbar = math.exp(mu_j + sigma_j * sigma_j / 2.0) - 1.0
    lt = lam * (1.0 + kbar) * T
    total, w = 0.0, math.exp(-lt)
    for n in range(terms):
        if n:
            w = w * lt / n
        r_n = r - lam * kbar + n * math.log1p(kbar) / T
        s_n = math.sqrt(sigma * sigma + n * sigma_j * sigma_j / T)
        total += w * black_scholes(S0, K, r_n, T, s_n, is_call)
    return total


# ---- the cases (reused by tests/test_gpu_bates.py) -------------------------------------------------------------------------
RARE_JUMPS = dict(lam=1.0, mu_j=-0.1, sigma_j=0.15)
# name -> (Heston parameters, jump parameters, dt, {scheme: shapes}); a shape is (n_steps, n_paths, path_begin, seed)
BATES_PARITY_SETS = {
    # lambda dt = 0.004: most waves (128 paths) have no jump in a Philox block
    "rare": (PARAMS["feller"], RARE_JUMPS, 1.0 / 252.0,
             {"euler": PARITY_SETS["feller"][2], "qe": PARITY_SHAPES + (QE_LONG_SHAPE,)}),
    # lambda dt = 0.5 on the 200 % volatility set: steps with two jumps and more, exponents far beyond 0.34
    "frequent": (LARGE_VOL, dict(lam=6.0, mu_j=0.05, sigma_j=0.2), 1.0 / 12.0,
                 {"euler": PARITY_SETS["large-vol"][2], "qe": PARITY_SHAPES + (QE_LONG_SHAPE,)}),
    # (the Euler form keeps the 40-step long shape of the Euler file: test_heston_reference.PARITY_SETS)
    "feller-violating": (FELLER_VIOLATING, dict(lam=4.0, mu_j=-0.05, sigma_j=0.1), 1.0 / 252.0,
                         {"euler": PARITY_SETS["feller-violating"][2], "qe": PARITY_SHAPES + (QE_LONG_SHAPE,)}),
}
PARITY_CASES = [(name, scheme) for name in BATES_PARITY_SETS for scheme in ("euler", "qe")]
# statistical rows: (id, scheme, Heston parameters, jump parameters, T, steps)
STAT_ROWS = (("euler-feller-T0.25-63", "euler", PARAMS["feller"], RARE_JUMPS, 0.25, 63),
             ("qe-feller-T1-32", "qe", PARAMS["feller"], RARE_JUMPS, 1.0, 32),
             ("qe-feller-violating-T1-8", "qe", FELLER_VIOLATING, dict(lam=4.0, mu_j=-0.05, sigma_j=0.1), 1.0, 8),
             ("qe-mild-T0.25-8", "qe", PARAMS["mild"], dict(lam=0.5, mu_j=0.1, sigma_j=0.25), 0.25, 8))
MERTON_ROW = dict(sigma=0.2, T=1.0, n_steps=32, **RARE_JUMPS)

# The count ladder: lambda dt = 1 exactly, where a few thousand paths hold some dozens of steps with 6, 7, 8 and 9 jumps, so that the
# thresholds of the device's second lazy load (T[6..15]) decide something.  The Euler form runs on Merton's parameters, QE
# (which needs sigma_v > 0) on the Feller set.  The seeds were picked with this file, among 1..40, for the conditions of
# test_parity_cases_are_well_conditioned (the margins, LADDER_MOST and LADDER_MANY): at lambda dt = 1 a step has 6 jumps or
# more with probability 5.9e-4, 46 of the 77825 steps of the two shapes on average, and 8 or more with probability 1.0e-5.
# Seed 11 gives the first shape 26 such steps and one of 8 jumps, seed 26 the second 35 and one of 9.
MERTON_BASE = dict(kappa=0.0, theta=0.04, sigma_v=0.0, rho=0.0, v0=0.04)
LADDER_BASE = {"euler": MERTON_BASE, "qe": PARAMS["feller"]}
LADDER_JUMPS, LADDER_DT = dict(lam=4.0, mu_j=-0.1, sigma_j=0.15), 0.25
LADDER_SHAPES = {s: ((7, 4097, 0, 11), (6, 8191, 3, 26)) for s in ("euler", "qe")}
LADDER_MOST, LADDER_MANY = 8, (6, 50)      # some step has >= 8 jumps; at least 50 steps have >= 6
LADDER_CASES = [("ladder", "euler"), ("ladder", "qe")]


def parity_set(name, scheme):
    """(Heston parameters, jump parameters, dt, shapes) of an element-wise case."""
    if name == "ladder":
        return LADDER_BASE[scheme], LADDER_JUMPS, LADDER_DT, LADDER_SHAPES[scheme]
    p, j, dt, shapes = BATES_PARITY_SETS[name]
    return p, j, dt, shapes[scheme]


# Words exactly on a threshold.  For k = 0..7 a path whose stream-4 word w of some step lies between T_k(1) and T_k(2^-40) =
# 2^32 - 1, and the two adjacent binary64 L with T_k(L_lo) = w (w > T_k fails: k jumps) and T_k(L_hi) = w - 1 (k + 1 jumps).
# dt = 1 makes lambda dt = L exactly.  The launch is 5 steps x 130 paths around the crafted path, which sits once in each of
# BOUNDARY_COLUMNS (the first column; an odd column of the wave's upper 32 lanes; the last column, an odd one in the second
# wave), and every other (path, step) of it keeps DECISION_MARGIN.
BOUNDARY_SEED, BOUNDARY_STEPS, BOUNDARY_PATHS, BOUNDARY_COLUMNS = 11, 5, 130, (0, 65, 129)
BOUNDARY_JUMPS = dict(mu_j=-0.5, sigma_j=0.1)
BOUNDARY_KS = {"euler": tuple(range(8)), "qe": (0, 2, 6)}      # QE: the first entry of each of the three threshold loads
BOUNDARY_DT = {"euler": 1.0, "qe": 1.0}


def threshold_pair(k, w):
    """The adjacent binary64 pair L_lo < L_hi with T_k(L_lo) = w and T_k(L_hi) = w - 1, by bisection (T_k falls as L grows,
    by at most one word per ulp of L: an ulp of L moves c_k 2^32 by about 1e-7)."""
    lo, hi = 2.0 ** -40, 1.0
    assert jump_thresholds(lo)[k] >= w > jump_thresholds(hi)[k]
    while True:
        mid = 0.5 * (lo + hi)
        if mid in (lo, hi):
            break
        if jump_thresholds(mid)[k] >= w:
            lo = mid
        else:
            hi = mid
    assert hi == math.nextafter(lo, 2.0) and jump_thresholds(lo)[k] == w and jump_thresholds(hi)[k] == w - 1, (k, w, lo, hi)
    return lo, hi


def boundary_runs(case, scheme):
    """The launches of one crafted case: (L, expected count at the crafted place, lambda, dt, path_begin, column)."""
    dt = BOUNDARY_DT[scheme]
    for L, count in ((case["L_lo"], case["k"]), (case["L_hi"], case["k"] + 1)):
        assert (L / dt) * dt == L
        for column in BOUNDARY_COLUMNS:
            yield L, count, L / dt, dt, case["path"] - column, column


def boundary_check(case, scheme):
    """None if every launch of the case is as the test needs it, or what is wrong; and the smallest margins met elsewhere."""
    worst = dict(count=math.inf, psi=math.inf, u=math.inf, own=0.0)
    wide = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    p = LADDER_BASE[scheme]
    for L, count, lam, dt, begin, column in boundary_runs(case, scheme):
        a = dict(S0=S0, r=R, dt=dt, n_steps=BOUNDARY_STEPS, n_paths=BOUNDARY_PATHS, path_begin=begin, scheme=scheme, lam=lam, **p,
                 **BOUNDARY_JUMPS)
        t = {}
        S, v = bates_numpy(BOUNDARY_SEED, trace=t, **a)
        if t["jumps"][case["step"], column] != count:
            return f"count {t['jumps'][case['step'], column]} at the crafted place, not {count}", worst
        others = t["count_margins"].copy()
        if not others[case["step"], column] < 2.0 ** -32:
            return "the crafted word is not next to its threshold", worst
        others[case["step"], column] = math.inf
        worst["count"] = min(worst["count"], float(others.min()))
        worst["psi"], worst["u"] = min(worst["psi"], t["psi_margin"]), min(worst["u"], t["u_margin"])
        if not (np.isfinite(S).all() and (S > 0.0).all()):
            return "S is not finite and positive", worst
        if wide:
            Sl, vl = bates_numpy(BOUNDARY_SEED, dtype=np.longdouble, **a)
            worst["own"] = max(worst["own"], float(np.abs(S / Sl - 1.0).max()), float(np.abs(v - vl).max()) / max(p["v0"], p["theta"]))
    if min(worst["count"], worst["psi"], worst["u"]) < DECISION_MARGIN:
        return "a decision elsewhere in the launch is closer than the margin", worst
    if worst["own"] > OWN_ERROR_BOUND:
        return "the reference's own rounding error exceeds its bound", worst
    return None, worst


@functools.lru_cache(maxsize=None)
def boundary_cases(scheme):
    """One crafted case per k of BOUNDARY_KS[scheme]: dict(k, path, step, word, L_lo, L_hi, margins), the first path id (from
    129 on, so that path_begin stays >= 0 in every column; up to 2^16, then up to 2^20) that boundary_check accepts."""
    found = {}
    lo_id = BOUNDARY_COLUMNS[-1]
    for hi_id in (2 ** 16, 2 ** 20):
        ids = np.arange(lo_id, hi_id + 1, dtype=np.uint64)
        words = np.stack(list(philox_words(BOUNDARY_SEED, ids, 0, STREAM_JUMP_COUNT)) +
                         [philox_words(BOUNDARY_SEED, ids, 1, STREAM_JUMP_COUNT)[0]])[:BOUNDARY_STEPS].astype(np.int64)
        T1 = jump_thresholds(1.0)
        for k in BOUNDARY_KS[scheme]:
            if k in found:
                continue
            at_id, at_step = np.nonzero(((words > T1[k]) & (words < 2 ** 32 - 1)).T)
            for i, step in zip(at_id, at_step):
                w = int(words[step, i])
                L_lo, L_hi = threshold_pair(k, w)
                case = dict(k=k, path=int(ids[i]), step=int(step), word=w, L_lo=L_lo, L_hi=L_hi)
                wrong, case["margins"] = boundary_check(case, scheme)
                if wrong is None:
                    found[k] = case
                    break
        if len(found) == len(BOUNDARY_KS[scheme]):
            break
    return [found[k] for k in BOUNDARY_KS[scheme] if k in found]


def stat_cases():
    for name, scheme, p, j, T, n_steps in STAT_ROWS:
        yield pytest.param(scheme, p, j, T, n_steps, id=name)


# ---- tests -------------------------------------------------------------------------------------------------------------------
def test_thresholds():
    for L in (0.0, 1.0 / 252.0, 0.1, 0.5, 1.0):
        _, c = jump_constants(L, -0.1, 0.15, 1.0)
        assert c.shape == (JUMP_CAP,) and (np.diff(c) >= 0.0).all() and c[0] == math.exp(-L)
        assert 1.0 - c[-1] < 2.0 ** -33                    # no uniform (at most 1 - 2^-33) lies above c_15
    _, c = jump_constants(0.0, -0.1, 0.15, 1.0)
    assert (c == 1.0).all()
    comp, _ = jump_constants(0.0, -0.1, 0.15, 1.0 / 252.0)
    assert comp == 0.0                                                   # a zero of either sign: exp(e + comp) = exp(e)
    print(f"1 - c_15 at L = 1: {1.0 - jump_constants(1.0, 0.0, 0.0, 1.0)[1][-1]:.2e}")
    # the device's integer form of the comparison is the same statement: uN > c_k  <=>  word > floor(c_k 2^32 - 1/2)
    rng = np.random.default_rng(11)
    for L in (1.0 / 252.0, 0.5, 1.0):
        _, c = jump_constants(L, 0.0, 0.0, 1.0)
        T = np.floor(c * 2.0 ** 32 - 0.5)
        assert (T >= 0.0).all() and (T <= 2.0 ** 32 - 1.0).all()
        near = (T[:, None] + np.arange(-3, 4)[None, :]).ravel()
        w = np.concatenate([rng.integers(0, 2 ** 32, 100_000).astype(np.float64), near[(near >= 0) & (near < 2.0 ** 32)]])
        assert np.array_equal(uniform_of_words(w.astype(np.uint64))[None, :] > c[:, None], w[None, :] > T[:, None])


THRESHOLD_LS = (0.0, 1e-300, 2.0 ** -40, 0.004, 0.5, 1.0 - 2.0 ** -53, 1.0)
CDF_OBSERVED = 4.47     # worst error of c_k against mpmath, in units of 2^-53 c_k (at L = 0.98498..., k = 11)


def threshold_ls():
    """THRESHOLD_LS and a few hundred random L, uniform and log-uniform in (0, 1)."""
    rng = np.random.default_rng(16)
    return THRESHOLD_LS + tuple(rng.uniform(0.0, 1.0, 200)) + tuple(10.0 ** rng.uniform(-12.0, 0.0, 200))


def test_word_thresholds_decide_as_the_uniform_does():
    """uN > c_k in binary64 <=> word > T_k, on the three words around every threshold: off by one word, or > against >=, at
    any k fails here.  T rises with k, and at L = 1 the last threshold is the last word: no word gives sixteen jumps."""
    top = 2 ** 32 - 1
    for L in threshold_ls():
        _, c = jump_constants(L, 0.0, 0.0, 1.0)
        T = jump_thresholds(L)
        assert len(T) == JUMP_CAP and all(0 <= t <= top for t in T) and all(a <= b for a, b in zip(T, T[1:])), (L, T)
        for k in range(JUMP_CAP):
            for w in (T[k] - 1, T[k], T[k] + 1):
                w = min(max(w, 0), top)
                assert ((w + 0.5) * 2.0 ** -32 > c[k]) == (w > T[k]), (L, k, w, T[k], c[k])
    assert jump_thresholds(1.0)[15] == top and jump_thresholds(0.0) == [top] * JUMP_CAP
    print("thresholds at L = 1:", jump_thresholds(1.0))


def test_cdf_against_mpmath():
    """c_k in binary64 (an exponential and at most fifteen products, quotients and sums of positive terms) against the Poisson
    CDF of the same binary64 L at 50 digits.  Observed: CDF_OBSERVED x 2^-53 relative; the bound is 1.5 times that."""
    mp.mp.dps = 50
    worst, at = 0.0, None
    for L in threshold_ls():
        _, c = jump_constants(L, 0.0, 0.0, 1.0)
        term = total = mp.exp(-mp.mpf(L))
        for k in range(JUMP_CAP):
            if k:
                term = term * mp.mpf(L) / k
                total += term
            err = float(abs(mp.mpf(float(c[k])) - total) / total * 2 ** 53)
            if err > worst:
                worst, at = err, (L, k)
    print(f"c_k against mpmath: worst {worst:.3f} x 2^-53 at (L, k) = {at}")
    assert worst <= 1.5 * CDF_OBSERVED, (worst, at)


def test_library_constants_are_the_references():
    """mcg_debug_bates_constants -- the function the launcher calls -- gives jump_thresholds(lambda dt) and the reference's comp
    exactly: the library's libm and Python's agree on every exponential a boundary case relies on."""
    from montecarlooptionspricer_amd.engine import bates_constants
    for L in threshold_ls():
        for mu_j, sigma_j in ((-0.1, 0.15), (-0.5, 0.1), (0.05, 0.2), (0.0, 0.0)):
            comp, T = bates_constants(L, mu_j, sigma_j, 1.0)
            assert T == jump_thresholds(L), (L, T)
            want = jump_constants(L, mu_j, sigma_j, 1.0)[0]
            assert np.float64(comp).tobytes() == np.float64(want).tobytes(), (L, mu_j, sigma_j, comp, want)       # (the zero's sign too)
    for lam, dt in ((4.0, 0.25), (6.0, 1.0 / 12.0), (1.0, 1.0 / 252.0), (252.0, 1.0 / 252.0)):
        comp, T = bates_constants(lam, -0.1, 0.15, dt)
        assert T == jump_thresholds(lam * dt) and comp == jump_constants(lam, -0.1, 0.15, dt)[0], (lam, dt)


def test_jump_streams_and_shards():
    path = np.array([0, 1, 2 ** 33 + 12345, 2 ** 64 - 1], dtype=np.uint64)
    for stream in (STREAM_JUMP_COUNT, STREAM_JUMP_SIZE):
        w = np.stack(philox_words(7, path, 5, stream))
        for other in (0, 1, 2, 3, 9 - stream):
            assert not np.array_equal(w, np.stack(philox_words(7, path, 5, other)))
    p, j, dt, _ = BATES_PARITY_SETS["frequent"]
    for scheme in ("euler", "qe"):
        a = dict(S0=100.0, r=0.04, dt=dt, n_steps=11, scheme=scheme, **p, **j)
        t = {}
        S, v = bates_numpy(3, n_paths=700, trace=t, **a)
        assert S.shape == v.shape == (12, 700) and (S[0] == 100.0).all() and (S > 0.0).all() and t["jumps"].max() >= 2
        S2, v2 = bates_numpy(3, n_paths=400, path_begin=300, **a)
        assert np.array_equal(S[:, 300:], S2) and np.array_equal(v[:, 300:], v2)       # a path depends on (seed, id) only
        ST, vT = bates_numpy(3, n_paths=700, terminal_only=True, **a)
        assert np.array_equal(ST, S[-1]) and np.array_equal(vT, v[-1])
        # jumps do not touch the variance, and without them the matrices are the base scheme's
        S0_, v0_ = bates_numpy(3, n_paths=700, **dict(a, lam=0.0))
        assert np.array_equal(v0_, v) and not np.array_equal(S0_, S)
    from test_heston_qe_reference import heston_qe_numpy
    from test_heston_reference import heston_numpy
    for scheme, base in (("euler", heston_numpy), ("qe", heston_qe_numpy)):
        a = dict(S0=100.0, r=0.04, dt=1.0 / 252.0, n_steps=11, n_paths=300, **FELLER_VIOLATING)
        Sb, vb = base(3, **a)
        S, v = bates_numpy(3, scheme=scheme, lam=0.0, mu_j=-0.1, sigma_j=0.15, **a)
        assert np.array_equal(v, vb) and np.array_equal(S, Sb)                         # (J = -0.0 + 0 mu_J = 0: e + J = e)
    # the law of the count: the mean number of jumps per step is lambda dt
    t = {}
    bates_numpy(5, 100.0, 0.04, lam=6.0, mu_j=0.0, sigma_j=0.1, dt=1.0 / 12.0, n_steps=12, n_paths=50_000, trace=t, **LARGE_VOL)
    mean = t["jumps"].mean()
    assert abs(mean - 0.5) <= 4.0 * math.sqrt(0.5 / t["jumps"].size), mean


def test_closed_form_without_jumps_is_hestons():
    for p in list(PARAMS.values()) + [FELLER_VIOLATING]:
        for K in STRIKES:
            for is_call in (True, False):
                for j in (dict(lam=0.0, mu_j=-0.1, sigma_j=0.15), dict(lam=0.0, mu_j=0.0, sigma_j=0.0)):
                    assert bates_closed_form(S0, K, R, 1.0, is_call=is_call, **p, **j) == heston_closed_form(S0, K, R, 1.0, is_call=is_call, **p)


def test_closed_form_against_the_merton_series():
    worst = 0.0
    for K in STRIKES:
        for is_call in (True, False):
            cf = bates_closed_form(S0, K, R, 1.0, 0.04, 0.0, 0.04, 1e-9, 0.0, is_call=is_call, **RARE_JUMPS)
            series = merton_series(S0, K, R, 1.0, 0.2, is_call=is_call, **RARE_JUMPS)
            worst = max(worst, abs(cf - series))
            assert abs(cf - series) <= 1e-7, (K, is_call, cf, series)
    print(f"characteristic function against the series: largest difference {worst:.2e}")
    # the series itself: no jumps is Black-Scholes, and put-call parity holds with jumps
    assert abs(merton_series(S0, 100.0, R, 1.0, 0.2, 0.0, -0.1, 0.15, True) - black_scholes(S0, 100.0, R, 1.0, 0.2, True)) <= 1e-12
    call, put = (merton_series(S0, 110.0, R, 1.0, 0.2, is_call=c, **RARE_JUMPS) for c in (True, False))
    assert abs(call - put - (S0 - 110.0 * math.exp(-R))) <= 1e-10


@pytest.mark.parametrize("name, scheme", PARITY_CASES + LADDER_CASES)
def test_parity_cases_are_well_conditioned(name, scheme):
    """Every element-wise case of the GPU file keeps every uN 1e-9 away from every threshold (and, under QE, the two margins of
    tests/test_heston_qe_reference.py), and the reference's own rounding error on it (binary64 against 80-bit arithmetic on the
    same draws, S relatively and v on the scale max(v0, theta)) stays below 1e-11.  The shapes of the ladder set hold a step
    with LADDER_MOST jumps or more and, together, LADDER_MANY[1] steps with LADDER_MANY[0] or more."""
    wide = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    p, j, dt, shapes = parity_set(name, scheme)
    if name == "ladder":
        assert j["lam"] * dt == 1.0 and all(s[1] % 512 for s in shapes)
    else:
        assert {s[0] & 3 for s in shapes} == {0, 1, 2, 3} and all(s[1] % 512 for s in shapes)
    worst, most, tally = 0.0, 0, np.zeros(JUMP_CAP + 1, dtype=np.int64)
    for n_steps, n_paths, begin, seed in shapes:
        a = dict(S0=S0, r=R, dt=dt, n_steps=n_steps, n_paths=n_paths, path_begin=begin, scheme=scheme, **p, **j)
        t = {}
        S, v = bates_numpy(seed, trace=t, **a)
        most = max(most, int(t["jumps"].max()))
        print(f"{name} {scheme} {n_steps} x {n_paths}: count margin {t['count_margin']:.2e}, psi margin {t['psi_margin']:.2e}, "
              f"u margin {t['u_margin']:.2e}, jumps {int(t['jumps'].sum())}, most in a step {int(t['jumps'].max())}")
        assert min(t["count_margin"], t["psi_margin"], t["u_margin"]) >= DECISION_MARGIN, (name, scheme, n_steps, t)
        assert np.isfinite(S).all() and (S > 0.0).all()
        if name == "frequent" and n_steps == 8:
            assert t["jumps"].max() >= 2, "steps with two jumps and more belong to this set's 8-step shape"
        tally += np.bincount(t["jumps"].ravel(), minlength=JUMP_CAP + 1)
        if wide:
            Sl, vl = bates_numpy(seed, dtype=np.longdouble, **a)
            es, ev = float(np.abs(S / Sl - 1.0).max()), float(np.abs(v - vl).max()) / max(p["v0"], p["theta"])
            worst = max(worst, es, ev)
            assert es <= OWN_ERROR_BOUND and ev <= OWN_ERROR_BOUND, (name, scheme, n_steps, es, ev)
    print(f"most jumps in a step {most}; the reference against itself in 80-bit arithmetic: {worst:.2e}")
    if name == "ladder":
        print(f"steps by count: {dict((n, int(c)) for n, c in enumerate(tally) if c)}")
        assert most >= LADDER_MOST and tally[LADDER_MANY[0]:].sum() >= LADDER_MANY[1], tally
    if not wide:
        pytest.skip("no wider float than binary64 here: the decision margins hold, the rounding comparison was not made")


@pytest.mark.parametrize("scheme", ["euler", "qe"])
def test_boundary_cases_are_well_conditioned(scheme):
    """The crafted launches of the GPU file (words exactly on a threshold): one per k, the count at the crafted place k at L_lo
    and k + 1 at L_hi in every column, every other (path, step) -- and QE's two decisions -- DECISION_MARGIN away, and the
    reference's own rounding error within its bound."""
    cases = boundary_cases(scheme)
    assert [c["k"] for c in cases] == list(BOUNDARY_KS[scheme]), [c["k"] for c in cases]
    for c in cases:
        m = c["margins"]
        print(f"{scheme} k = {c['k']}: path {c['path']}, step {c['step']}, word {c['word']}, L_lo = {c['L_lo']!r}; elsewhere: count "
              f"margin {m['count']:.2e}, psi margin {m['psi']:.2e}, u margin {m['u']:.2e}; own error {m['own']:.2e}")
        assert jump_thresholds(1.0)[c["k"]] < c["word"] < 2 ** 32 - 1 and c["path"] <= 2 ** 20
        assert jump_thresholds(c["L_lo"])[c["k"]] == c["word"] and jump_thresholds(c["L_hi"])[c["k"]] == c["word"] - 1
        assert c["L_hi"] == math.nextafter(c["L_lo"], 2.0)
        wrong, _ = boundary_check(c, scheme)
        assert wrong is None, (c, wrong)


@pytest.mark.parametrize("scheme, p, j, T, n_steps", stat_cases())
def test_scheme_against_the_closed_form(scheme, p, j, T, n_steps):
    ST, _ = bates_numpy(STAT_SEED, S0, R, dt=T / n_steps, n_steps=n_steps, n_paths=STAT_PATHS_CPU, scheme=scheme, terminal_only=True,
                        **p, **j)
    fwd, fwd_se = discounted_payoff(ST, 0.0, T, True)
    print(f"martingale: e^-rT mean(S_T) = {fwd:.5f} +- {fwd_se:.5f}, {(fwd - S0) / fwd_se:+.2f} std errors")
    assert abs(fwd - S0) <= STD_ERRORS * fwd_se
    for K in STRIKES:
        for is_call in (True, False):
            price, se = discounted_payoff(ST, K, T, is_call)
            want = bates_closed_form(S0, K, R, T, is_call=is_call, **p, **j)
            print(f"K={K:g} call={is_call}: {price:.5f} +- {se:.5f}, closed form {want:.5f}, {abs(price - want) / se:.2f} std errors")
            assert abs(price - want) <= STD_ERRORS * se, (K, is_call, price, want, se)


def test_library_exports_and_rejects_without_a_gpu():
    L = mc.load_library()
    assert hasattr(L, "mcg_paths_bates") and hasattr(L, "mcg_paths_bates_payoff")
    h = C.c_void_p()
    gen = (7, 100.0, 0.04, 0.04, 2.0, 0.04, 0.3, -0.7, 1.0, -0.1, 0.15, 1.0 / 252.0, 8, 0, 16)
    for scheme in (0, 1):
        assert L.mcg_paths_bates(None, *gen, scheme, C.byref(h), None) != 0
        assert b"NULL" in L.mcg_last_error()
        assert L.mcg_paths_bates_payoff(None, *gen, scheme, 100.0, 1, C.byref(h), None) != 0
        assert b"NULL" in L.mcg_last_error()
    assert hasattr(mc.PathEngine, "bates") and hasattr(mc.PathEngine, "merton")
    sig = inspect.signature(mc.PathEngine.bates)
    assert sig.parameters["scheme"].default == "euler" and "jump_intensity" in sig.parameters
    assert "scheme" not in inspect.signature(mc.PathEngine.merton).parameters
    # the value is checked before any library call: an engine that was never opened has neither a library nor a ctx
    eng = object.__new__(mc.PathEngine)
    with pytest.raises(ValueError):
        eng.bates(7, 100.0, 0.04, 0.04, 2.0, 0.04, 0.3, -0.7, 1.0, -0.1, 0.15, 1.0 / 252.0, 8, 16, scheme="nonsense")
