"""The dual upper bound for LSM exercise policies on the GPU (mcg_lsm_dual_upper; PathEngine.dual_upper_lsm) against the numpy
restatement and the cases of tests/test_lsm_dual_reference.py, the exact identities (repeats, shards, batches of outer paths,
no noise, one inner path, the one-launch switch), the bracket of the Longstaff-Schwartz put, the European limit, refusals and timing.

Every (case, policy) pair has no undecided decision, outer or inner (asserted in the CPU file), so numpy takes the decisions the
device takes: inner_steps is compared exactly, which proves every inner stopping decision, and C and D differ by rounding only.

Bounds: ten times the largest differences observed on an MI355X over all cases and policies, as the Bates and local-vol tests
set theirs.  Observed: C 5.92e-16 K, D 1.42e-15 K, upper 9.91e-16 relative, std_err 2.26e-14 by the se_error rule of
tests/test_gpu_lsm2.py -- the device exponential and the Box-Muller tables against numpy's, a few ulps of values of the size
of K.  A difference above 1e-10 K would be a bug, not a tolerance.  Without noise (sigma = 0, puts in the money) D equalled
K - S0 exactly in all ten runs, where the test allows 1e-13, and C the restatement's to 7.1e-17 K.

The Longstaff-Schwartz put (S0 = 36, K = 40, sigma = 0.2, r = 0.06, T = 1, 50 dates, B = 4.478015), as observed on an MI355X:
fit_lsm at order 3 on 200 003 paths; on 2 000 independent outer paths the lower bound is 4.3782 +- 0.0691 and the dual
upper bound with 2 048 inner paths 4.4980 +- 0.0018: upper - B = 0.0200, duality gap upper - lower = 0.1198 (the two share
the outer paths, and the lower bound's std error is most of it); 2.99e9 inner steps, 0.572 of the executed lane-steps live;
with 64 inner paths 4.8095 +- 0.0103, with the all-CONTINUE policy 4.7576 +- 0.0108.
"""
import ctypes as C
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from test_gpu_lsm2 import rel, se_error
from test_heston_reference import black_scholes
from test_lsm_dual_reference import (DUAL_CASES, NOISE_FREE_CASES, deterministic_matrix, dual_case_id, mean_and_std_err_from_sums,
                                     noise_free_reference, outer_rows, policies, reference)
from test_lsm_policy_reference import CONT, LS, R, TERM, ls_put_reference

pytestmark = pytest.mark.gpu

C_BOUND = 5.92e-15        # |C - numpy| / K: ten times the largest observed (module docstring)
D_BOUND = 1.42e-14        # |D - numpy| / K
UPPER_BOUND = 9.91e-15    # upper against mean(D of numpy), relative
SE_DUAL_BOUND = 2.26e-13  # std_err, where the spread of D resolves it (se_error)
observed = {"C / K": 0.0, "D / K": 0.0, "upper": 0.0, "std_err": 0.0}


@pytest.fixture(scope="module")
def eng():
    with mc.PathEngine(0) as e:
        yield e


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest differences in this run: " + ", ".join(f"{k} {v:.2e}" for k, v in observed.items()))


@pytest.fixture(scope="module")
def uploaded(eng):
    """Per case: the outer matrix on the host (rows as from_host takes them) and on the device, made once."""
    made = {}

    def get(c):
        key = dual_case_id(c)
        if key not in made:
            rows = outer_rows(c)
            made[key] = (rows, eng.from_host(rows))
        return made[key]

    yield get
    for _, P in made.values():
        P.free()


def dual(eng, c, policy, P, **kw):
    args = dict(sigma=c["sigma"], n_inner=c["n_inner"], seed=c["inner_seed"], q=c["q"], path_begin=c["path_begin"])
    args.update(kw)
    return eng.dual_upper_lsm(policy, P, **args)


def same_bits(a, b):
    return (np.asarray(a, dtype=np.float64).view(np.int64) == np.asarray(b, dtype=np.float64).view(np.int64)).all()


# ---- 1. against numpy --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", DUAL_CASES, ids=dual_case_id)
def test_against_numpy(eng, uploaded, c):
    rows, P = uploaded(c)
    for name in c["names"]:
        policy = policies(c)[name]
        D, Cm, steps, close = reference(c, name)
        assert close == 0
        res = dual(eng, c, policy, P, return_cont=True, return_d=True)
        assert res.inner_steps == steps, (name, res.inner_steps, steps)
        assert res.cont.shape == Cm.shape and res.d.shape == D.shape and res.sums3[2] == c["n_paths"]
        eC, eD = float(np.max(np.abs(res.cont - Cm))) / policy.K, float(np.max(np.abs(res.d - D))) / policy.K
        want, want_se = mean_and_std_err_from_sums(D)
        eU = rel(res.upper, want)
        eS = se_error(res.upper, res.std_err, want_se, c["n_paths"], (dual_case_id(c), name))
        print(f"{dual_case_id(c)} {name}: C {eC:.2e} K, D {eD:.2e} K, upper {res.upper:.6f} ({eU:.2e}), std_err {res.std_err:.6f} ({eS:.2e}), "
              f"{steps} inner steps, live share {steps / max(eng.debug_lsm_dual_executed(), 1):.3f}")
        for k, v in (("C / K", eC), ("D / K", eD), ("upper", eU), ("std_err", eS)):
            observed[k] = max(observed[k], v)
        assert eC <= C_BOUND and eD <= D_BOUND, (name, eC, eD)
        assert eU <= UPPER_BOUND and eS <= SE_DUAL_BOUND, (name, eU, eS)
        assert abs(res.sums3[0] / c["n_paths"] - res.upper) <= 1e-15 * abs(res.upper)
        assert steps <= eng.debug_lsm_dual_executed() <= c["n_paths"] * c["n_inner"] * c["n_steps"] * (c["n_steps"] + 1) // 2
        if name == "all-continue":
            assert eng.debug_lsm_dual_executed() == steps        # nobody stops early: every executed lane-step is live


# ---- 2. exact identities -----------------------------------------------------------------------------------------------------
def test_repeated_calls_are_bit_identical(eng, uploaded):
    c = next(c for c in DUAL_CASES if c["n_paths"] == 513 and c["n_inner"] == 130)
    rows, P = uploaded(c)
    policy = policies(c)["fitted"]
    first = dual(eng, c, policy, P, return_cont=True, return_d=True)
    eng.price_lsm(P, R, c["K"], c["maturity"], c["dt"], c["is_call"], 2)      # other users of the ctx's workspaces
    eng.apply_lsm(policy, P)
    again = dual(eng, c, policy, P, return_cont=True, return_d=True)
    assert same_bits(first[:2], again[:2]) and same_bits(first.sums3, again.sums3) and first.inner_steps == again.inner_steps
    assert same_bits(first.cont, again.cont) and same_bits(first.d, again.d)
    plain = dual(eng, c, policy, P)                                           # the optional outputs change nothing
    assert len(plain) == 4 and same_bits(plain[:2], first[:2]) and plain.inner_steps == first.inner_steps


@pytest.mark.parametrize("name", ["fitted", "linear-boundary"])
def test_shards_give_the_same_bits(eng, uploaded, name):
    """513 outer paths as shards of 1, 255 and 257 with their path_begin (an empty shard beside them is refused with
    MCG_ERR_EMPTY_PATHS and adds nothing): d_out and cont_out equal the whole's column by column, bit for bit; inner_steps adds
    exactly, sums3 to the rounding of three partial sums."""
    c = next(c for c in DUAL_CASES if c["n_paths"] == 513 and c["n_inner"] == 130)
    rows, P = uploaded(c)
    policy = policies(c)[name]
    whole = dual(eng, c, policy, P, return_cont=True, return_d=True)
    sums, steps, lo = np.zeros(3), 0, 0
    E = eng.gbm(3, 100.0, R, 0.2, c["dt"], c["n_steps"], 0)
    with pytest.raises(mc.McgError) as e:
        dual(eng, c, policy, E, path_begin=c["path_begin"] + 1)
    assert e.value.status == 6
    E.free()
    for size in (1, 255, 257):
        S = eng.from_host(rows[lo:lo + size])
        part = dual(eng, c, policy, S, path_begin=c["path_begin"] + lo, return_cont=True, return_d=True)
        S.free()
        assert same_bits(part.d, whole.d[lo:lo + size]) and same_bits(part.cont, whole.cont[:, lo:lo + size]), (name, lo, size)
        sums += part.sums3
        steps += part.inner_steps
        lo += size
    assert lo == 513 and steps == whole.inner_steps and sums[2] == whole.sums3[2] == 513
    assert abs(sums[0] - whole.sums3[0]) <= 1e-13 * abs(whole.sums3[0]) and abs(sums[1] - whole.sums3[1]) <= 1e-13 * whole.sums3[1]


@pytest.mark.parametrize("c", [c for c in NOISE_FREE_CASES if not c["is_call"]], ids=dual_case_id)
def test_without_noise_the_bound_is_K_minus_S0(eng, c):
    """sigma = 0 on an outer path with the inner drift, a put in the money on the whole path (S0 = 92 and 85 under K = 100;
    the `immediate` policy has K = 1.2 S0): every inner path is the outer path's future, C_j is the policy's value from j on --
    several to some tens of the currency, and different from policy to policy --, the martingale vanishes and D = max_j h_j =
    K - S0 to 1e-13 (absolute), whatever the rule; C against the restatement at sigma = 0."""
    P = eng.from_host(np.ascontiguousarray(deterministic_matrix(c, 130).T))
    values = set()
    for name, policy in policies(c).items():
        M, h, (D, Cm, steps, close) = noise_free_reference(c, policy, 130)
        assert close == 0
        res = dual(eng, c, policy, P, sigma=0.0, q=0.0, seed=5, path_begin=0, return_cont=True, return_d=True)
        want = policy.K - c["S0"]
        eD, eC = float(np.max(np.abs(res.d - want))), float(np.max(np.abs(res.cont - Cm))) / policy.K
        print(f"{dual_case_id(c)} {name}: K - S0 = {want:.4f}, |D - (K - S0)| {eD:.2e}, C_0 = {res.cont[0, 0]:.6f}, C {eC:.2e} K")
        assert want > 5.0 and res.cont[0].min() > 1.0
        assert eD <= 1e-13 and abs(res.upper - want) <= 1e-13 and res.std_err <= 1e-13, (name, res.upper, want)
        assert res.inner_steps == steps and eC <= C_BOUND, (name, eC)
        values.add(round(float(res.cont[0, 0]), 6))
    assert len(values) >= 2
    P.free()


# ---- 2b. batches of outer paths ------------------------------------------------------------------------------------------------
def test_forced_batches_change_no_bit(eng, uploaded):
    """The outer set is worked through in batches that bound the workspace.  With the bound set so low that a batch is the
    smallest there is, 512 outer paths, the 513-path case takes two batches (512 + 1): every output, sums3 included, equals
    the one-batch run's bit for bit, and inner_steps equals numpy's."""
    c = next(c for c in DUAL_CASES if c["n_paths"] == 513 and c["n_inner"] == 130)
    rows, P = uploaded(c)
    for name in ("fitted", "exercise-in-the-money"):
        policy = policies(c)[name]
        one = dual(eng, c, policy, P, return_cont=True, return_d=True)
        eng.debug_lsm_dual_workspace(1)
        try:
            two = dual(eng, c, policy, P, return_cont=True, return_d=True)
        finally:
            eng.debug_lsm_dual_workspace(0)
        assert same_bits(one[:2], two[:2]) and same_bits(one.sums3, two.sums3) and one.inner_steps == two.inner_steps == reference(c, name)[2]
        assert same_bits(one.d, two.d) and same_bits(one.cont, two.cont)


def test_two_batches_at_the_default_bound(eng):
    """8192 outer paths x 50 dates x 41 inner paths: 41 slices, so the default bound of 2^24 doubles holds 7680 outer paths and
    the call takes two batches (7680 + 512).  Shards of 5000 and 3192 paths, one batch each, give d_out and cont_out bit for
    bit, inner_steps exactly and sums3 to the rounding of two partial sums; sixteen forced batches of 512 give every bit,
    sums3 included."""
    n, n_outer, n_inner = LS["n_steps"], 8192, 41
    dt = LS["T"] / n
    F = eng.gbm(LS["fit_seed"], LS["S0"], LS["r"], LS["sigma"], dt, n, 20011)
    _, _, policy = eng.fit_lsm(F, LS["r"], LS["K"], LS["T"], dt, False, 5)       # (order 5: the instance for orders 4..7)
    F.free()
    P = eng.gbm(LS["apply_seed"], LS["S0"], LS["r"], LS["sigma"], dt, n, n_outer)
    rows = np.ascontiguousarray(P.to_host_step_major().T)
    args = dict(sigma=LS["sigma"], n_inner=n_inner, seed=78, return_cont=True, return_d=True)
    whole = eng.dual_upper_lsm(policy, P, **args)
    P.free()
    sums, steps, lo = np.zeros(3), 0, 0
    for size in (5000, 3192):
        S = eng.from_host(rows[lo:lo + size])
        part = eng.dual_upper_lsm(policy, S, path_begin=lo, **args)
        S.free()
        assert same_bits(part.d, whole.d[lo:lo + size]) and same_bits(part.cont, whole.cont[:, lo:lo + size]), (lo, size)
        sums += part.sums3
        steps += part.inner_steps
        lo += size
    assert lo == n_outer and steps == whole.inner_steps and sums[2] == whole.sums3[2] == n_outer
    assert abs(sums[0] - whole.sums3[0]) <= 1e-13 * whole.sums3[0] and abs(sums[1] - whole.sums3[1]) <= 1e-13 * whole.sums3[1]
    S = eng.from_host(rows)
    eng.debug_lsm_dual_workspace(1)
    try:
        many = eng.dual_upper_lsm(policy, S, **args)
    finally:
        eng.debug_lsm_dual_workspace(0)
    S.free()
    assert same_bits(many[:2], whole[:2]) and same_bits(many.sums3, whole.sums3) and many.inner_steps == whole.inner_steps
    assert same_bits(many.d, whole.d) and same_bits(many.cont, whole.cont)
    assert whole.upper > 4.4 and 0 < whole.inner_steps < n_outer * n_inner * n * (n + 1) // 2


def test_one_inner_path_runs(eng, uploaded):
    c = DUAL_CASES[3]
    rows, P = uploaded(c)
    policy = policies(c)["fitted"]
    one = dual(eng, c, policy, P, n_inner=1, return_cont=True)
    three = dual(eng, c, policy, P, return_cont=True)
    assert math.isfinite(one.upper) and c["n_paths"] * c["n_steps"] <= one.inner_steps < three.inner_steps
    assert one.upper > three.upper - 4.0 * math.hypot(one.std_err, three.std_err)      # fewer inner paths: more upward bias


def test_the_one_launch_switch_changes_nothing():
    """The bound neither reads nor changes mcg_lsm_one_launch_enabled: the same bits with the one-launch LSM sweep allowed and
    after its hand-shake has been made to give up (the existing hook: spin limit 0)."""
    c = DUAL_CASES[3]
    policy = policies(c)["fitted"]
    with mc.PathEngine(0) as e:
        P = e.from_host(outer_rows(c))
        Q = e.gbm(11, 100.0, 0.04, 0.2, 0.02, 20, 300_000)
        assert e.lsm_one_launch_enabled()
        on = dual(e, c, policy, P, return_d=True)
        assert e.lsm_one_launch_enabled()
        e.debug_lsm_hooks(spin_limit=0)
        e.price_lsm(Q, 0.04, 100.0, 0.4, 0.02, False, 2)
        e.debug_lsm_hooks()
        assert not e.lsm_one_launch_enabled()
        off = dual(e, c, policy, P, return_d=True)
        assert not e.lsm_one_launch_enabled()
        e.lsm_one_launch_reset()
        assert same_bits(on[:2], off[:2]) and same_bits(on.d, off.d) and on.inner_steps == off.inner_steps
        Q.free()
        P.free()


# ---- 3. the Longstaff-Schwartz put ---------------------------------------------------------------------------------------------
def test_bracket_of_the_longstaff_schwartz_put(eng):
    B = ls_put_reference()["B"]
    dt = LS["T"] / LS["n_steps"]
    F = eng.gbm(LS["fit_seed"], LS["S0"], LS["r"], LS["sigma"], dt, LS["n_steps"], LS["n_paths"])
    _, _, policy = eng.fit_lsm(F, LS["r"], LS["K"], LS["T"], dt, False, LS["order"])
    F.free()
    P = eng.gbm(LS["apply_seed"], LS["S0"], LS["r"], LS["sigma"], dt, LS["n_steps"], 2000)
    lower, lower_se = eng.apply_lsm(policy, P)
    up = eng.dual_upper_lsm(policy, P, LS["sigma"], 2048, seed=77)
    live = up.inner_steps / eng.debug_lsm_dual_executed()
    few = eng.dual_upper_lsm(policy, P, LS["sigma"], 64, seed=77)
    nothing = mc.LsmPolicy.from_arrays(LS["n_steps"], LS["order"], False, LS["r"], LS["K"], LS["T"], dt,
                                       kinds=[CONT] * LS["n_steps"] + [TERM])
    crude = eng.dual_upper_lsm(nothing, P, LS["sigma"], 2048, seed=77)
    P.free()
    print(f"B = {B:.6f}; lower {lower:.4f} +- {lower_se:.4f}; upper (2048 inner) {up.upper:.4f} +- {up.std_err:.4f}: upper - B = "
          f"{up.upper - B:.4f}, duality gap {up.upper - lower:.4f}; {up.inner_steps} inner steps, live share {live:.3f}; "
          f"64 inner {few.upper:.4f} +- {few.std_err:.4f}; all-CONTINUE {crude.upper:.4f} +- {crude.std_err:.4f}")
    assert up.upper + 4.0 * up.std_err >= B                                              # (a)
    assert lower - 4.0 * lower_se <= B                                                   # (b)
    assert crude.upper - up.upper > 4.0 * math.hypot(crude.std_err, up.std_err)          # (c) a good rule gives a tighter bound
    assert few.upper >= up.upper - 4.0 * math.hypot(few.std_err, up.std_err)             # (d) the inner noise biases upwards
    assert crude.inner_steps == 2000 * 2048 * 50 * 51 // 2 and up.inner_steps < crude.inner_steps


# ---- 4. the European limit -----------------------------------------------------------------------------------------------------
def test_european_limit(eng):
    """A call without dividends is never exercised early, and under the all-CONTINUE policy D = C_0 + max(0, max (h_j - C_j)) with
    h_j below the European value C_j up to the inner noise: the bound is Black-Scholes within 4 of its own std errors plus 4 std
    errors of an inner mean."""
    S0, K, r, sigma, T_, n, n_outer, n_inner = 100.0, 100.0, 0.04, 0.2, 1.0, 12, 1000, 1024
    dt = T_ / n
    policy = mc.LsmPolicy.from_arrays(n, 2, True, r, K, T_, dt, kinds=[CONT] * n + [TERM])
    P = eng.gbm(31, S0, r, sigma, dt, n, n_outer)
    res = eng.dual_upper_lsm(policy, P, sigma, n_inner, seed=32, return_cont=True, return_d=True)
    # the std error of one inner mean, from the spread of the discounted terminal payoff
    ST = P.to_host_step_major()[n]
    P.free()
    pay = np.maximum(ST - K, 0.0) * math.exp(-r * T_)
    inner_se = float(pay.std(ddof=1)) / math.sqrt(n_inner)
    bs = black_scholes(S0, K, r, T_, sigma, True)
    print(f"European limit: upper {res.upper:.4f} +- {res.std_err:.4f}, Black-Scholes {bs:.4f}, inner std error {inner_se:.4f}, "
          f"mean(D - C_0) = {float(np.mean(res.d - res.cont[0])):.4f}")
    assert abs(res.upper - bs) <= 4.0 * res.std_err + 4.0 * inner_se
    assert res.inner_steps == n_outer * n_inner * n * (n + 1) // 2 == eng.debug_lsm_dual_executed()
    assert (res.d >= res.cont[0] - 1e-12 * K).all()


# ---- 5. refusals that need a ctx -----------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(eng, uploaded):
    c = DUAL_CASES[3]
    rows, P = uploaded(c)
    policy = policies(c)["fitted"]
    L, dp = eng._L, C.POINTER(C.c_double)
    up, hdr = C.c_double(), policy._hdr()
    model = N.LsmDualModel(5, 0.2, 0.0, 0, 2, 0)
    coef = policy.coef.ctypes.data_as(dp)

    def call(ctx=eng._ctx, h=C.byref(hdr), k=coef, paths=P._h, m=C.byref(model), upper=C.byref(up)):
        return L.mcg_lsm_dual_upper(ctx, h, k, paths, m, upper, None, None, None, None, None), L.mcg_last_error().decode()

    assert call()[0] == 0                                         # (every optional output NULL is fine)
    short = eng.gbm(5, 100.0, R, 0.2, c["dt"], c["n_steps"] - 1, 64)
    empty = eng.gbm(5, 100.0, R, 0.2, c["dt"], c["n_steps"], 0)
    bad_model = N.LsmDualModel(5, -0.2, 0.0, 0, 2, 0)
    with mc.PathEngine(0) as other:
        Q = other.from_host(rows)
        for kw in (dict(ctx=None), dict(h=None), dict(k=None), dict(paths=None), dict(m=None), dict(upper=None), dict(paths=Q._h),
                   dict(paths=short._h), dict(m=C.byref(bad_model))):
            status, msg = call(**kw)
            assert status == 1 and msg, (kw, status, msg)
        other.set_allreduce(lambda ptr, count, stream: None)
        status, msg = call(ctx=other._ctx, paths=Q._h)
        assert status == 1 and "collective" in msg, (status, msg)
    status, msg = call(paths=empty._h)
    assert status == 6 and msg
    short.free()
    empty.free()
    with pytest.raises(mc.McgError) as e:
        eng.dual_upper_lsm(policy, P, -0.1, 4, seed=1)
    assert e.value.status == 1 and "sigma" in str(e.value)


# ---- 6. timing ------------------------------------------------------------------------------------------------------------------------
def test_device_time_is_booked_under_lsm_dual(eng, uploaded):
    c = DUAL_CASES[3]
    rows, P = uploaded(c)
    policy = policies(c)["fitted"]
    eng.timing_enable(True)
    eng.timing_reset()
    try:
        for k in range(1, 4):
            dual(eng, c, policy, P)
            ms, launches = eng.timing_get(N.K_LSM_DUAL)
            assert ms > 0.0 and launches == 2 * k            # the nested simulation and the recursion
        assert eng.timing_get(N.K_LSM_APPLY)[1] == 0
    finally:
        eng.timing_enable(False)
