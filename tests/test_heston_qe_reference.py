"""numpy reference of the QE Heston generator (mcg_paths_heston_qe) -- the yardstick of tests/test_gpu_heston_qe.py: the
uniform of Philox stream 3, Andersen's quadratic-exponential scheme of include/mcgpu.h line for line on the draws of
tests/test_heston_reference.py, the conditioning of the element-wise cases (the two branch decisions of the scheme are
discontinuities: a case that sits on one cannot carry a bound), the scheme against the closed form at eight steps, and what
the library must answer without a GPU."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from test_heston_reference import (FELLER_VIOLATING, LARGE_VOL, PARAMS, PARITY_SETS, PARITY_SHAPES, R, S0, SEED64, STAT_SEED,
                                   STD_ERRORS, STREAM_PRICE, STREAM_VOL, STRIKES, discounted_payoff, heston_closed_form,
                                   normal_quad, philox_words)

STREAM_QE_UNIFORM = 3           # (2 belongs to the branching-process kernels)
PSI_C = 1.5


def uniform_of_words(w):
    """(word + 0.5) 2^-32: exact in binary64, strictly inside (0, 1)."""
    return (np.asarray(w, dtype=np.uint64).astype(np.float64) + 0.5) * 2.0 ** -32


def uniforms(seed, path, block):
    """[4][...]: the four uniforms of one Philox block of stream 3; element e belongs to step 4 block + e."""
    return uniform_of_words(np.stack(philox_words(seed, path, block, STREAM_QE_UNIFORM)))


def qe_constants(kappa, theta, sigma_v, rho, dt):
    """(E, c1, c2, K0, K1, K2, K3) of include/mcgpu.h in binary64 (K4 = K3)."""
    E = math.exp(-kappa * dt)
    if kappa > 0.0:
        c1 = sigma_v * sigma_v * E * (1.0 - E) / kappa
        c2 = theta * sigma_v * sigma_v * (1.0 - E) * (1.0 - E) / (2.0 * kappa)
    else:
        c1, c2 = sigma_v * sigma_v * dt, 0.0
    g = kappa * rho / sigma_v - 0.5
    return (E, c1, c2, -rho * kappa * theta * dt / sigma_v, dt * g / 2.0 - rho / sigma_v, dt * g / 2.0 + rho / sigma_v,
            dt * (1.0 - rho * rho) / 2.0)


def heston_qe_numpy(seed, S0, r, v0, kappa, theta, sigma_v, rho, dt, n_steps, n_paths, path_begin=0, terminal_only=False,
                    dtype=np.float64, trace=None):
    """The QE scheme of include/mcgpu.h: (S, v), step-major [n_steps + 1][n_paths], row n = S_n / v_n; with terminal_only the
    last rows alone.  dtype: the arithmetic of the steps (constants and draws are binary64 either way).  trace: a dict that
    receives the number of draws, of exponential-branch draws and of those that gave v' = 0, and the smallest distances
    |s2 / (psi_c m^2) - 1| and |u - p| from the two branch decisions."""
    path = np.uint64(path_begin) + np.arange(n_paths, dtype=np.uint64)
    S, v = np.full(n_paths, S0, dtype=dtype), np.full(n_paths, v0, dtype=dtype)
    E, c1, c2, K0, K1, K2, K3 = (dtype(x) for x in qe_constants(kappa, theta, sigma_v, rho, dt))
    K4 = K3
    r, theta, dt, psi_c = dtype(r), dtype(theta), dtype(dt), dtype(PSI_C)
    if not terminal_only:
        Sm, vm = np.empty((n_steps + 1, n_paths), dtype=dtype), np.empty((n_steps + 1, n_paths), dtype=dtype)
        Sm[0], vm[0] = S, v
    t = dict(draws=0, exponential=0, zeros=0, psi_margin=math.inf, u_margin=math.inf)
    for n in range(n_steps):
        if n & 3 == 0:
            q1, q2 = normal_quad(seed, path, n >> 2, STREAM_PRICE), normal_quad(seed, path, n >> 2, STREAM_VOL)
            uq = uniforms(seed, path, n >> 2)
        z1, z2, u = q1[n & 3].astype(dtype), q2[n & 3].astype(dtype), uq[n & 3].astype(dtype)
        m = theta + (v - theta) * E if kappa > 0.0 else v
        s2 = v * c1 + c2
        with np.errstate(all="ignore"):          # each branch is evaluated for every path and selected below
            psi = s2 / (m * m)
            q = 2 / psi
            b2 = q - 1 + np.sqrt(q) * np.sqrt(q - 1)
            v_quad = m / (1 + b2) * (np.sqrt(b2) + z2) ** 2
            p = (psi - 1) / (psi + 1)
            beta = (1 - p) / m
            v_exp = np.where(u <= p, dtype(0), np.log((1 - p) / (1 - u)) / beta)
        exponential = (m != 0) & ~(psi <= psi_c)
        vn = np.where(m == 0, dtype(0), np.where(exponential, v_exp, v_quad)).astype(dtype)
        S = S * np.exp(r * dt + K0 + K1 * v + K2 * vn + np.sqrt(K3 * v + K4 * vn) * z1)
        v = vn
        if not terminal_only:
            Sm[n + 1], vm[n + 1] = S, v
        if trace is not None:
            t["draws"] += n_paths
            t["exponential"] += int(exponential.sum())
            t["zeros"] += int((exponential & (u <= p)).sum())
            if (m != 0).any():
                t["psi_margin"] = min(t["psi_margin"], float(np.abs(psi[m != 0] / psi_c - 1).min()))
            if exponential.any():
                t["u_margin"] = min(t["u_margin"], float(np.abs(u - p)[exponential].min()))
    if trace is not None:
        trace.update(t)
    return (S, v) if terminal_only else (Sm, vm)


# ---- the cases (reused by tests/test_gpu_heston_qe.py) -------------------------------------------------------------------
# element-wise: the three parameter sets with their dt, the shapes of the Euler file and one long shape for every set (QE has
# no square root of a variance that passes closely above zero; the long Feller-violating shape needs no shortening)
QE_LONG_SHAPE = (252, 1300, 777, SEED64)
QE_PARITY_SETS = {name: (p, dt, PARITY_SHAPES + (QE_LONG_SHAPE,)) for name, (p, dt, _) in PARITY_SETS.items()}
DECISION_MARGIN = 1e-9
OWN_ERROR_BOUND = 1e-11
# statistical: (T, steps)
STAT_SETS = {"feller": PARAMS["feller"], "mild": PARAMS["mild"], "feller-violating": FELLER_VIOLATING}
STAT_ROWS = ((0.25, 8), (1.0, 32), (1.0, 8))
STAT_PATHS = 1_000_000


def stat_cases(rows):
    for name, p in STAT_SETS.items():
        for T, n_steps in rows:
            yield pytest.param(p, T, n_steps, id=f"{name}-T{T:g}-{n_steps}")


# ---- tests ------------------------------------------------------------------------------------------------------------------
def test_uniforms_are_stream_three_and_strictly_inside_the_unit_interval():
    lo, hi = float(uniform_of_words(0)), float(uniform_of_words(2 ** 32 - 1))
    assert 0.0 < lo == 2.0 ** -33 and hi == 1.0 - 2.0 ** -33 and hi < 1.0
    path = np.array([0, 1, 2 ** 33 + 12345, 2 ** 64 - 1], dtype=np.uint64)
    for seed, block in ((7, 0), (SEED64, 5), (2 ** 64 - 1, 2 ** 32 - 1)):
        u = uniforms(seed, path, block)
        w = np.stack(philox_words(seed, path, block, 3))
        assert u.shape == (4, 4) and np.array_equal(u, (w.astype(np.float64) + 0.5) / 2.0 ** 32)
        assert ((u > 0.0) & (u < 1.0)).all()
        for other in (STREAM_PRICE, STREAM_VOL, 2):
            assert not np.array_equal(w, np.stack(philox_words(seed, path, block, other)))


def test_scheme_shards_and_edges():
    a = dict(S0=100.0, r=0.04, dt=1.0 / 252.0, n_steps=11, **FELLER_VIOLATING)
    S, v = heston_qe_numpy(3, n_paths=700, **a)
    assert S.shape == v.shape == (12, 700) and (S[0] == 100.0).all() and (v[0] == 0.04).all() and (S > 0.0).all()
    S2, v2 = heston_qe_numpy(3, n_paths=400, path_begin=300, **a)
    assert np.array_equal(S[:, 300:], S2) and np.array_equal(v[:, 300:], v2)           # a path depends on (seed, id) only
    ST, vT = heston_qe_numpy(3, n_paths=700, terminal_only=True, **a)
    assert np.array_equal(ST, S[-1]) and np.array_equal(vT, v[-1])
    # the exponential branch is really taken on the violating set, with v' = 0 on some draws, and v is never negative
    t = {}
    Sl, vl = heston_qe_numpy(3, n_paths=4096, trace=t, **dict(a, n_steps=252))
    assert t["exponential"] > 0 and t["zeros"] > 0 and (vl == 0.0).any() and (vl >= 0.0).all() and np.isfinite(Sl).all()
    print(f"Feller-violating, dt = 1/252: exponential-branch share {t['exponential'] / t['draws']:.4f}, zeros {t['zeros']}")
    t = {}
    heston_qe_numpy(3, n_paths=4096, trace=t, **dict(a, dt=1.0 / 8.0, n_steps=8))
    assert 0.4 < t["exponential"] / t["draws"] < 0.65        # (0.517 at 1M paths)
    # ... and never on "feller" at daily steps
    t = {}
    Sf, vf = heston_qe_numpy(3, 100.0, 0.04, dt=1.0 / 252.0, n_steps=252, n_paths=4096, trace=t, **PARAMS["feller"])
    assert t["exponential"] == 0 and (vf > 0.0).all()
    # theta = 0 with v0 = 0: m = 0 on every draw, v stays 0 and S is deterministic
    Sz, vz = heston_qe_numpy(3, 100.0, 0.04, 0.0, 2.0, 0.0, 0.3, -0.7, 0.02, 9, 50)
    assert (vz == 0.0).all() and np.isfinite(Sz).all() and np.abs(Sz[-1] / (100.0 * math.exp(0.04 * 0.18)) - 1.0).max() <= 1e-14
    # kappa = 0 (E = 1, c1 = sigma_v^2 dt, c2 = 0), also from v0 = 0 (m = 0 although theta > 0), and |rho| = 1 (K3 = 0)
    for change in (dict(kappa=0.0), dict(kappa=0.0, v0=0.0), dict(rho=1.0), dict(rho=-1.0), dict(theta=0.0), dict(v0=0.0)):
        Sk, vk = heston_qe_numpy(3, n_paths=2000, **dict(a, **change))
        assert np.isfinite(Sk).all() and np.isfinite(vk).all() and (vk >= 0.0).all() and (Sk > 0.0).all(), change


def test_parity_cases_are_well_conditioned():
    """Every element-wise case of the GPU file keeps its distance from both branch decisions, and the reference's own
    rounding error on it (binary64 against 80-bit arithmetic on the same draws, S relatively and v on the scale max(v0, theta))
    stays below 1e-11."""
    wide = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    worst, psi_margin, u_margin = 0.0, math.inf, math.inf
    for name, (p, dt, shapes) in QE_PARITY_SETS.items():
        assert {s[0] & 3 for s in shapes} == {0, 1, 2, 3} and all(s[1] % 512 for s in shapes)
        for n_steps, n_paths, begin, seed in shapes:
            a = dict(S0=S0, r=R, dt=dt, n_steps=n_steps, n_paths=n_paths, path_begin=begin, **p)
            t = {}
            S, v = heston_qe_numpy(seed, trace=t, **a)
            print(f"{name} {n_steps} x {n_paths}: psi margin {t['psi_margin']:.2e}, u margin {t['u_margin']:.2e}, "
                  f"exponential draws {t['exponential']}, zeros {t['zeros']}")
            psi_margin, u_margin = min(psi_margin, t["psi_margin"]), min(u_margin, t["u_margin"])
            assert t["psi_margin"] >= DECISION_MARGIN and t["u_margin"] >= DECISION_MARGIN, (name, n_steps, t)
            assert (v >= 0.0).all()
            if wide:
                Sl, vl = heston_qe_numpy(seed, dtype=np.longdouble, **a)
                es, ev = float(np.abs(S / Sl - 1.0).max()), float(np.abs(v - vl).max()) / max(p["v0"], p["theta"])
                worst = max(worst, es, ev)
                assert es <= OWN_ERROR_BOUND and ev <= OWN_ERROR_BOUND, (name, n_steps, es, ev)
    print(f"smallest margins: psi {psi_margin:.2e}, u {u_margin:.2e}; the reference against itself in 80-bit arithmetic: "
          f"{worst:.2e}")
    if not wide:
        pytest.skip("no wider float than binary64 here: the decision margins hold, the rounding comparison was not made")


@pytest.mark.parametrize("p, T, n_steps", stat_cases(((0.25, 8), (1.0, 8))))
def test_scheme_against_the_closed_form(p, T, n_steps):
    ST, _ = heston_qe_numpy(STAT_SEED, S0, R, dt=T / n_steps, n_steps=n_steps, n_paths=STAT_PATHS, terminal_only=True, **p)
    fwd, fwd_se = discounted_payoff(ST, 0.0, T, True)
    print(f"martingale: e^-rT mean(S_T) = {fwd:.5f} +- {fwd_se:.5f}, {abs(fwd - S0) / fwd_se:.2f} std errors")
    assert abs(fwd - S0) <= STD_ERRORS * fwd_se
    for K in STRIKES:
        for is_call in (True, False):
            price, se = discounted_payoff(ST, K, T, is_call)
            want = heston_closed_form(S0, K, R, T, is_call=is_call, **p)
            print(f"K={K:g} call={is_call}: {price:.5f} +- {se:.5f}, closed form {want:.5f}, {abs(price - want) / se:.2f} std errors")
            assert abs(price - want) <= STD_ERRORS * se, (K, is_call, price, want, se)


def test_library_exports_and_rejects_without_a_gpu():
    L = mc.load_library()
    assert hasattr(L, "mcg_paths_heston_qe") and hasattr(L, "mcg_paths_heston_qe_payoff")
    h = C.c_void_p()
    gen = (7, 100.0, 0.04, 0.04, 2.0, 0.04, 0.3, -0.7, 1.0 / 252.0, 8, 0, 16)
    assert L.mcg_paths_heston_qe(None, *gen, C.byref(h), None) != 0
    assert b"NULL" in L.mcg_last_error()
    assert L.mcg_paths_heston_qe_payoff(None, *gen, 100.0, 1, C.byref(h), None) != 0
    assert b"NULL" in L.mcg_last_error()
    sig = inspect.signature(mc.PathEngine.heston)
    assert sig.parameters["scheme"].default == "euler"
    # the value is checked before any library call: an engine that was never opened has neither a library nor a ctx
    eng = object.__new__(mc.PathEngine)
    with pytest.raises(ValueError):
        eng.heston(7, 100.0, 0.04, 0.04, 2.0, 0.04, 0.3, -0.7, 1.0 / 252.0, 8, 16, scheme="nonsense")


# ---- one QE step in high precision (the yardstick of test_gpu_heston_qe.py::test_one_step_*) --------------------------------
# The step of include/mcgpu.h evaluated by mpmath at 50 digits from binary64 constants and inputs, on cases built to reach every
# corner of it.  The scheme has two discontinuities (psi against psi_c, u against p): a case within STEP_MARGIN of one, in the
# reference's own arithmetic, carries no bound, and at most STEP_LEFT_OUT of the cases may be such.
STEP_MARGIN = 1e-12
STEP_LEFT_OUT = 1e-3
STEP_SEED, STEP_BLOCK, STEP_ELEM = SEED64, 5, 2
STEP_POOL = 1 << 18             # path ids whose stream-3 uniform the cases choose from
STEP_SETS = {                   # name -> (model parameters, dt)
    "feller": (PARAMS["feller"], 1.0 / 252.0),
    "violating-daily": (FELLER_VIOLATING, 1.0 / 252.0),
    "violating-eighth": (FELLER_VIOLATING, 1.0 / 8.0),
    "large-vol": (LARGE_VOL, 1.0 / 12.0),
    "theta-zero": (dict(FELLER_VIOLATING, theta=0.0), 1.0 / 52.0),
    "kappa-zero": (dict(FELLER_VIOLATING, kappa=0.0), 1.0 / 52.0),
    "rho-plus-one": (dict(FELLER_VIOLATING, rho=1.0), 1.0 / 8.0),
    "rho-minus-one": (dict(PARAMS["mild"], rho=-1.0), 1.0 / 252.0),
}


def step_constants(p, dt, r=R):
    """The eight HestonQe::Consts {theta, E, c1, c2, drift, K1, K2, K3} in binary64 (theta: 0 where kappa = 0, so that m = v)."""
    E, c1, c2, K0, K1, K2, K3 = qe_constants(p["kappa"], p["theta"], p["sigma_v"], p["rho"], dt)
    return (p["theta"] if p["kappa"] > 0.0 else 0.0, E, c1, c2, r * dt + K0, K1, K2, K3)


def qe_step_mp(consts, v, z1, z2, S, u):
    """One step in mpmath.  Returns (v', S', exponential?, m, margin, scale of v', size of the exponent): margin = the smaller
    relative distance from the decisions the case meets, |s2 - 1.5 m^2| and (exponential branch) |u d - (s2 - m^2)|."""
    import mpmath as mp
    theta, E, c1, c2, drift, K1, K2, K3 = (mp.mpf(x) for x in consts)
    v, z1, z2, S, u = (mp.mpf(x) for x in (v, z1, z2, S, u))
    with mp.workdps(400):           # (exactly: at v = 1e-300 the sum cancels 300 digits)
        m = theta + (v - theta) * E
    m = +m
    s2, m2 = v * c1 + c2, m * m
    exponential = m != 0 and s2 > PSI_C * m2
    margin = abs(s2 - PSI_C * m2) / max(s2, PSI_C * m2) if m != 0 else mp.inf
    if m == 0:
        vn = mp.mpf(0)
    elif exponential:
        d = s2 + m2
        margin = min(margin, abs(u * d - (s2 - m2)) / max(u * d, abs(s2 - m2)))
        vn = mp.mpf(0) if u * d <= s2 - m2 else mp.log(2 * m2 / (d * (1 - u))) * d / (2 * m)     # ln((1 - p) / (1 - u)) / beta
    else:
        q = 2 * m2 / s2
        b2 = q - 1 + mp.sqrt(q * (q - 1))
        vn = m / (1 + b2) * (mp.sqrt(b2) + z2) ** 2
    root = mp.sqrt(K3 * (v + vn)) * z1
    Sn = S * mp.exp(drift + K1 * v + K2 * vn + root)
    # the scales errors are measured on.  v': the branch's own scale -- m, or 1 / beta = m (psi + 1) / 2, the mean of the
    # exponential part (its inversion turns a rounding of y next to 1 into that much times the rounding) -- plus v' itself (the
    # last product rounds at its size: ln(1 / y) reaches 15 where u is next to 1), times the roundings m itself carries: it is
    # formed as theta + (v - theta) E from terms of size theta, an ulp of theta is theta / m ulps of m, and v' follows m with
    # a condition number of order one (through m and through psi = s2 / m^2).
    # S': the terms of the exponent, each rounded at its own size, and 1 for the exponential.
    v_scale = 0 if m == 0 else (s2 + m2) / (2 * m) if exponential else m
    m_roundings = 1 if m == 0 else max(1, theta / m)
    e_size = 1 + abs(drift) + abs(K1 * v) + abs(K2 * vn) + abs(root)
    return vn, Sn, bool(exponential), m, margin, (v_scale + vn) * m_roundings, e_size


_step_pool = {}


def step_pool():
    """(ids sorted by their uniform, the uniforms): stream-3 uniform of element STEP_ELEM of block STEP_BLOCK, seed STEP_SEED."""
    if not _step_pool:
        ids = np.arange(STEP_POOL, dtype=np.uint64)
        u = uniform_of_words(philox_words(STEP_SEED, ids, STEP_BLOCK, STREAM_QE_UNIFORM)[STEP_ELEM])
        order = np.argsort(u)
        _step_pool["v"] = (ids[order], u[order])
    return _step_pool["v"]


def path_with_uniform_near(target):
    ids, u = step_pool()
    k = min(int(np.searchsorted(u, target)), len(u) - 1)
    return int(ids[k]), float(u[k])


def step_cases(name):
    """[n][6] (v, z1, z2, S, path id, u) for one parameter set: the listed variances and random ones against random uniforms and
    against uniforms far below p, near 1 and next to p; for the sets whose psi is monotone in v (theta = 0, kappa = 0: c2 = 0),
    variances tuned to put p at relative distances 1e-6 .. 1e-16 on either side of u and psi next to psi_c."""
    p, dt = STEP_SETS[name]
    theta, E, c1, c2 = step_constants(p, dt)[:4]
    rs = np.random.RandomState(sum(name.encode()))
    ids, us = step_pool()
    rows = []

    def add(v, target_u=None):
        k = rs.randint(len(ids)) if target_u is None else min(int(np.searchsorted(us, target_u)), len(us) - 1)
        rows.append((v, rs.normal(), rs.normal(), 100.0 * math.exp(rs.normal(0, 0.3)), float(ids[k]), us[k]))

    listed = [0.0, 1e-300, 1e-200, 1e-12]
    random_v = np.concatenate([rs.uniform(0, 1, 320), 10.0 ** rs.uniform(-8, 0, 320), max(theta, 0.04) * np.exp(rs.normal(0, 1, 320))])
    for v in listed * 8 + list(random_v):
        add(v)
    for v in listed + list(random_v[::5]):
        m = theta + (v - theta) * E
        s2 = v * c1 + c2
        if m > 0 and s2 > PSI_C * m * m:                    # exponential: uniforms placed relative to p
            pr = (s2 - m * m) / (s2 + m * m)
            for t in (1e-9, 0.001 * pr, pr * (1 - 1e-4), pr + (1 - pr) * 1e-4, pr + (1 - pr) * 0.5, 1 - 1e-9):
                add(v, t)
    if c2 == 0.0 and name in ("theta-zero", "kappa-zero"):
        # psi = c1 / (v E'^2) with m = E' v (E' = E for theta = 0, 1 for kappa = 0): p = (psi - 1) / (psi + 1)
        Em = E if p["theta"] == 0.0 else 1.0
        for _ in range(12):
            k = rs.randint(len(ids) // 4, len(ids))        # u in (1/4, 1): p there means psi in (5/3, inf): exponential
            u = us[k]
            for delta in (1e-6, -1e-6, 1e-9, -1e-9, 1e-11, -1e-11):
                pt = u * (1 + delta)
                if pt < 1:
                    rows.append((c1 / (Em * Em * (1 + pt) / (1 - pt)), rs.normal(), rs.normal(), 100.0, float(ids[k]), u))
        k = len(ids) // 2
        v_at = c1 / (Em * Em * (1 + us[k]) / (1 - us[k]))   # p = u up to rounding: y within an ulp or two of 1
        for v in (v_at, np.nextafter(v_at, 0), np.nextafter(v_at, 1)):
            rows.append((v, rs.normal(), rs.normal(), 100.0, float(ids[k]), us[k]))
        for delta in (1e-6, -1e-6, 1e-9, -1e-9, 1e-11, -1e-11):
            rows.append((c1 / (Em * Em * PSI_C) * (1 + delta), rs.normal(), rs.normal(), 100.0, float(ids[0]), us[0]))
        rows.append((c1 / (Em * Em * PSI_C), rs.normal(), rs.normal(), 100.0, float(ids[0]), us[0]))
    return np.array(rows)


_step_reference = {}


def step_reference(name):
    """(cases, mpmath results) of one parameter set, computed once and never written to."""
    if name not in _step_reference:
        p, dt = STEP_SETS[name]
        cases = step_cases(name)
        consts = step_constants(p, dt)
        _step_reference[name] = (cases, [qe_step_mp(consts, *row[:4], row[5]) for row in cases])
    return _step_reference[name]


def test_step_cases_reach_every_corner_and_keep_their_margins():
    total = left_out = 0
    seen = dict(quadratic=0, exponential=0, zero=0, m_zero=0, K3_zero=0)
    for name, (p, dt) in STEP_SETS.items():
        cases, ref = step_reference(name)
        ids = cases[:, 4].astype(np.uint64)
        assert np.array_equal(cases[:, 5], uniform_of_words(philox_words(STEP_SEED, ids, STEP_BLOCK, STREAM_QE_UNIFORM)[STEP_ELEM]))
        for row, (vn, Sn, exponential, m, margin, _, _) in zip(cases, ref):
            total += 1
            left_out += margin < STEP_MARGIN
            assert vn >= 0 and Sn > 0
            seen["exponential" if exponential else "quadratic"] += 1
            seen["zero"] += exponential and vn == 0
            seen["m_zero"] += m == 0
        seen["K3_zero"] += len(cases) * (step_constants(p, dt)[7] == 0.0)
    print(f"{total} cases, {left_out} within {STEP_MARGIN:g} of a decision; {seen}")
    assert all(seen.values()), seen
    assert 0 < left_out <= STEP_LEFT_OUT * total, (left_out, total)
