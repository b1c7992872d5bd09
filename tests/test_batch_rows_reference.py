"""The batched row kernels (csrc/kernels_batch.hip): the case lists of tests/test_gpu_batch_rows.py, and the checks that
make those lists trustworthy -- all on the CPU.

* spectrum_numpy restates k_batch_weights (lambda, the direct DFT on the Mphi grid, the symmetrised amplitudes, the
  compensator) and is compared with Oracle.rbergomi_spectrum, which goes through the host FFT: measured, amplitudes within
  2.9e-15 of the row's largest amplitude and compensators within 4.4e-16 (relatively) at every size; ten times that is asserted.
* Every pricer case of the GPU file is well conditioned: the oracle's price on the case's matrix and on a copy whose entries
  after column 0 are multiplied by 1 + 1e-13 N(0, 1) differ, on the scale of the strike, by at most RESPONSE_SHARE of the
  column's bound (BOUNDS, below), so that a kernel that misses a bound is wrong and not unlucky.  Errors are measured on the
  scale of the strike because MartingaleOptimization's price is ~1e-16 where nothing is ever in the money.

BOUNDS[column] = ten times the largest |got - oracle| / K observed on an MI355X over all cases of test_gpu_batch_rows.py
(the observed values stand in its docstring), never above what the project already states for the same quantity (CAPS).

The perturbation itself moves a price: a payoff is Lipschitz in the path, so a mean of discounted payoffs over n paths answers
1 + 1e-13 N(0, 1) with up to ~1e-13 S / K however well the case is conditioned (measured over the cases below: up to
2.4e-13).  The exact columns (AsymptoticAnalysis, BranchingProcesses: the device differs from the oracle only in the last bit
of exp; bounds 1.3e-15 and 6.4e-15) have bounds BELOW that, so for them a tenth of the bound cannot be the yardstick of any
case, whatever its seed or strike; first_order (the perturbation's own size, 6 sigma of it on the largest entry of the matrix
over K) is allowed on top.  What the check excludes is amplification: an exercise decision, a regression or a maximum that
turns 1e-13 into more than that.  The committed seeds were searched (C_RESEED, D_RESEED, ...) until every case answered with
less than 0.9 first_order, so the check holds whatever the bounds are.  The constant matrices are the one family it cannot
speak about (degenerate_cases says why)."""
import math

import numpy as np
import pytest

from oracle.binding import Oracle

DT = 1.0 / 252.0
R = 0.04
S0 = 100.0
SEED64 = 0x5DEECE66D00000C3          # a non-zero high word: both Philox key words matter
STRIKES = (90.0, 100.0, 110.0)
SPECTRUM_STEPS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1020)
H_ETA = ((0.05, 1.9), (0.1, 1.9), (0.3, 1.0), (0.6, 0.03), (0.0, 1.0))
AMP_AGAINST_ORACLE = 2.9e-14         # ten times the measured 2.9e-15 (of the row's largest amplitude)
COMP_AGAINST_ORACLE = 4.4e-15        # ten times the measured 4.4e-16 (relative)
BRANCHES = (0, 1, 3, 4, 5, 8, 9, 12, 13, 40)   # quads of four Philox words: 0, part of one, one, one and a part, two, ...
ITERATIONS = (1, 2, 5)
COLUMNS = ("asym", "branching", "lsm", "lsm3", "lsm4", "mart", "mart4")

# what the project already states for the same quantities (test_gpu_parity.py, test_martingale_matches_oracle, ...)
CAPS = {"paths": 1e-9, "asym": 1e-12, "branching": 1e-12, "lsm": 1e-8, "lsm3": 1e-8, "lsm4": 2e-6, "mart": 1e-8, "mart4": 2e-6}
# ten times the largest error observed on an MI355X (test_gpu_batch_rows.py's docstring gives the observed values)
BOUNDS = {"amp": 3e-14, "comp": 2.3e-15, "paths": 1e-13, "asym": 1.3e-15, "branching": 6.4e-15, "lsm": 6e-12, "lsm3": 1.6e-9,
          "lsm4": 1.6e-10, "mart": 8.8e-12, "mart4": 2.5e-12}
assert all(BOUNDS[k] <= cap for k, cap in CAPS.items())
RESPONSE_SHARE = 0.1
PERTURBATION = 1e-13


def column_of(kind, poly_order=0):
    """The bound's name of a price: the regressions have one for orders <= 2, one for order 3 and one for order 4."""
    if kind == "lsm":
        return "lsm" if poly_order <= 2 else "lsm%d" % poly_order
    if kind == "mart":
        return "mart4" if poly_order == 4 else "mart"
    return kind


def next_pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def lds_class(M):
    return 0 if M <= 128 else 1 if M == 256 else 2 if M == 512 else 3


# ---- k_batch_weights, restated ---------------------------------------------------------------------------------------
def spectrum_numpy(H, eta, dt, steps):
    """(amp[M], comp[steps]) as k_batch_weights forms them: phi_k = sum_n lam_n e^{2 pi i k n / Mphi} by the direct sum on
    the grid Mphi = next_pow2(steps + 1) (2M when steps is a power of two), P_k = |phi_k|^2 for k < steps and 0 up to M,
    a_k = eta sqrt(2H) / M sqrt((P_k + P_{(M - k) mod M}) / 2), comp_n = -eta^2 / 2 (n dt)^{2H}."""
    M, Mphi = next_pow2(steps), next_pow2(steps + 1)
    n = np.arange(steps + 1)
    lam = 0.5 * np.power(n * dt, 2.0 * H)
    q = (np.arange(steps)[:, None] * n[None, :]) & (Mphi - 1)
    ang = 2.0 * np.pi * q / Mphi
    re, im = (lam * np.cos(ang)).sum(axis=1), (lam * np.sin(ang)).sum(axis=1)
    P = np.zeros(M)
    P[:steps] = re * re + im * im
    k = np.arange(M)
    amp = eta * math.sqrt(2.0 * H) / M * np.sqrt(0.5 * (P + P[(M - k) & (M - 1)]))
    comp = -0.5 * eta * eta * np.power(np.arange(steps) * dt, 2.0 * H)
    return amp, comp


def spectrum_errors(got_amp, got_comp, want_amp, want_comp):
    """(amplitude error on the scale of the row's largest amplitude, relative compensator error); a row whose amplitudes
    are all zero (H = 0) must be met exactly."""
    top = float(np.abs(want_amp).max())
    ea = float(np.abs(got_amp - want_amp).max()) / top if top > 0.0 else (0.0 if not np.any(got_amp) else math.inf)
    nz = want_comp != 0.0
    ec = float(np.abs(got_comp[nz] / want_comp[nz] - 1.0).max()) if nz.any() else 0.0
    if np.any(got_comp[~nz]):
        ec = math.inf
    return ea, ec


# ---- rows ------------------------------------------------------------------------------------------------------------
def row(steps, H, eta, strike=S0, maturity=None, is_call=0, s0=S0, xi=0.09):
    return dict(S0=s0, xi=xi, H=H, eta=eta, rho=-0.7, strike=strike, maturity=steps * DT if maturity is None else maturity,
                sigma=0.3, dividend=0.02, n_steps=steps, is_call=int(is_call))


def weight_rows():
    """(a): every (steps, (H, eta)) of the two lists in ONE call.  Rows of the four LDS classes are interleaved, every class
    holds several lengths, and the longest row of a class is neither the first nor the last row of its class."""
    rs = np.random.RandomState(1)
    per_class = [[], [], [], []]
    for steps in SPECTRUM_STEPS:
        for H, eta in H_ETA:
            per_class[lds_class(next_pow2(steps))].append(row(steps, H, eta))
    ordered = []
    for rows in per_class:
        longest = max(d["n_steps"] for d in rows)
        short = [d for d in rows if d["n_steps"] != longest]
        inner = short[1:-1] + [d for d in rows if d["n_steps"] == longest]
        inner = [inner[i] for i in rs.permutation(len(inner))]
        ordered.append([short[0]] + inner + [short[-1]])
    out = []
    while any(ordered):
        for rows in ordered:
            if rows:
                out.append(rows.pop(0))
    return out


# (b): (n_paths, steps of the call's rows).  The 250-path call has one row per transform size M = 1 .. 1024; the others meet
# the generator's workgroup map with one share (M <= 32), two (M = 64 from 129 paths) and many; 1020 steps at <= 64 paths.
PATH_CALLS = [(250, (1, 2, 3, 7, 16, 31, 64, 100, 200, 500, 1020))]
PATH_CALLS += [(n, (5, 40, 64, 100, 130, 1020)) for n in (1, 2, 3, 63, 64)]
PATH_CALLS += [(n, (5, 40, 64, 100, 130, 300, 600)) for n in (65, 127, 128, 129, 255, 256)]


def path_rows(steps_list):
    return [row(s, *H_ETA[i % len(H_ETA)], s0=80.0 + 7.0 * i, xi=0.04 + 0.01 * i) for i, s in enumerate(steps_list)]


def maturities(steps):
    """The five maturity rules of a row: 0, one date exactly (j dt as the kernels compute it), between two dates before the
    horizon, the horizon, beyond the horizon."""
    j = max(1, steps // 2)
    return (0.0, j * DT, 0.69 * steps * DT, steps * DT, 1.5 * steps * DT)


# (c): fifteen calls = every (order, iterations) pair; the branch counts twice over; path counts at which the last pair is
# odd, a wave is partly filled and 2 n_paths crosses order + 1.  A call's thirty rows are calls and puts x three strikes x
# five maturities, of different lengths inside class 0 (k_batch_asym's max_steps offset); some calls add rows of the longer
# classes, several lengths to a class.
_C_PATHS = (250, 64, 65, 3, 2, 129, 256, 128, 1, 3, 250, 63, 4, 2, 1)
_C_STEPS = (1, 2, 3, 5, 16, 17, 33, 64, 65, 100, 128)
_C_LONG = {0: (129, 256, 200), 5: (257, 512, 300), 1: (513, 1020, 700), 11: (130, 1020, 256, 600), 8: (129, 1020)}
# "A case that fails the conditioning check is given another seed": the calls, shapes and small path counts whose first seed
# gave a row that amplifies the perturbation (a regression on a handful of samples often does), and how often they moved on
C_RESEED = {3: 211, 9: 13, 12: 8, 13: 11}
D_RESEED = {5: 2, 6: 37, 11: 13, 15: 3, 17: 1}
SMALL_RESEED = {2: 1, 3: 2}
DUP_RESEED = {(2, 3): 3}


def pricer_calls():
    calls = []
    for c in range(15):
        rows = []
        k = c
        for is_call in (0, 1):
            for strike in STRIKES:
                for m in range(5):
                    steps = _C_STEPS[k % len(_C_STEPS)]
                    k += 1
                    H, eta = H_ETA[k % len(H_ETA)]
                    rows.append(row(steps, H, eta, strike, maturities(steps)[m], is_call))
        for i, steps in enumerate(_C_LONG.get(c, ())):
            H, eta = H_ETA[(c + i) % 4]
            rows.append(row(steps, H, eta, STRIKES[(c + i) % 3], maturities(steps)[(2 + 3 * i + c) % 5], (c + i) % 2))
        calls.append(dict(n_paths=_C_PATHS[c], poly_order=c % 5, num_branches=BRANCHES[c % len(BRANCHES)],
                          max_iterations=ITERATIONS[c % 3], seed=SEED64 + c + (C_RESEED.get(c, 0) << 16), rows=rows))
    return calls


def oracle_four(orc, block, d, call, i, step_major=True):
    """The oracle's four columns of row i of a (c) call on the matrix `block`."""
    ex = np.arange(d["n_steps"], dtype=np.int32)
    cp = bool(d["is_call"])
    K, T = d["strike"], d["maturity"]
    return [orc.asymptotic_price(block, R, K, T, DT, cp, d["sigma"], d["dividend"], step_major=step_major),
            orc.branching_price(block, R, K, T, DT, cp, call["num_branches"], ex, call["seed"], mode="philox",
                                path_begin=i << 32, step_major=step_major)[0],
            orc.lsm_price(block, R, K, T, DT, cp, call["poly_order"], step_major=step_major),
            orc.martingale_price(block, R, K, T, DT, cp, call["poly_order"], call["max_iterations"], step_major=step_major)[0]]


def four_columns(poly_order):
    return ("asym", "branching", column_of("lsm", poly_order), column_of("mart", poly_order))


# ---- (d): matrices uploaded through the class API (path-major, [n_paths][steps + 1]) -----------------------------------
D_SHAPES = [(1, 1), (1, 17), (2, 2), (2, 33), (3, 3), (3, 16), (4, 15), (5, 16), (5, 1020), (63, 17), (64, 1020), (65, 33), (128, 1),
            (129, 15), (192, 2), (193, 17), (250, 33), (256, 16), (256, 3)]
D_BRANCHES = BRANCHES + (1024,)
D_SEED = 0x00C0FFEE0000BEEF


def gbm_matrix(n_paths, steps, seed, dt=DT, sigma=0.3):
    z = np.random.RandomState(seed).standard_normal((n_paths, steps))
    m = np.empty((n_paths, steps + 1))
    m[:, 0] = S0
    m[:, 1:] = S0 * np.exp(np.cumsum((R - 0.5 * sigma * sigma) * dt + sigma * math.sqrt(dt) * z, axis=1))
    return m


def d_maturities(steps, dt=DT):
    """0, negative, exactly on a date, between two dates, beyond the horizon."""
    j = max(1, steps // 2)
    return (0.0, -0.5 * steps * dt, j * dt, (j - 0.5) * dt, 1.5 * steps * dt)


def case(kind, matrix, is_call, K, T, dt=DT, **kw):
    d = dict(kind=kind, matrix=matrix, is_call=bool(is_call), K=K, T=T, dt=dt, poly_order=0, max_iterations=5, num_branches=10,
             sigma=0.3, dividend=0.02)
    d.update(kw)
    return d


def crafted_matrices():
    """name -> (matrix, is_call, K).  Every path out of the money at every date; exactly one path in the money at one date; a
    constant matrix in the money (rank-1 regressions at every order; with r > 0 its first date is the maximum); a constant
    matrix AT the money (every payoff 0: ties in BranchingProcesses' strict > and MartingaleOptimization's first maximum); in
    the money only at the last column."""
    rs = np.random.RandomState(12)
    n, steps = 65, 17
    otm = 100.0 + 30.0 * rs.uniform(0.05, 1.0, (n, steps + 1))           # puts at K = 100: S > K everywhere
    one = otm.copy()
    one[37, 9] = 93.0
    const_in = np.full((n, steps + 1), 95.0)
    const_at = np.full((n, steps + 1), 100.0)
    last = otm.copy()
    last[:, -1] = 100.0 - 20.0 * rs.uniform(0.05, 1.0, n)
    calls_otm = 100.0 - 30.0 * rs.uniform(0.05, 1.0, (n, steps + 1))     # calls at K = 100: S < K everywhere
    return {"out of the money": (otm, False, 100.0), "one path once": (one, False, 100.0), "constant, in": (const_in, False, 100.0),
            "constant, at": (const_at, False, 100.0), "last column only": (last, False, 100.0),
            "calls out of the money": (calls_otm, True, 100.0), "constant call, in": (np.full((n, steps + 1), 104.0), True, 100.0)}


def class_api_cases(kind):
    """The cases of one pricer: the shapes x the five maturities with calls / puts, strikes, orders, iteration and branch counts
    cycling through them; 1 .. 3 paths at orders 3 and 4 with 1 and 5 iterations; the crafted matrices."""
    cases, k = [], 0
    for s, (n_paths, steps) in enumerate(D_SHAPES):
        m = gbm_matrix(n_paths, steps, 100 + s + 1000 * D_RESEED.get(s, 0))
        for t, T in enumerate(d_maturities(steps)):
            cases.append(case(kind, m, k % 2, STRIKES[k % 3], T, poly_order=(k // 5 + k) % 5, max_iterations=(1, 5)[(k // 2) % 2],
                              num_branches=D_BRANCHES[k % len(D_BRANCHES)]))
            k += 1
    if kind in ("lsm", "mart"):
        for n_paths in (1, 2, 3):
            m = gbm_matrix(n_paths, 16, 200 + n_paths + 1000 * SMALL_RESEED.get(n_paths, 0))
            for order in (3, 4):
                for it in (1, 5):
                    cases.append(case(kind, m, (n_paths + order + it) % 2, STRIKES[(n_paths + order) % 3], 16 * DT, poly_order=order,
                                      max_iterations=it))
    if kind == "mart":   # deep in the money at date 0: every path stops there, its sample S0 is in the regression once per path, and
        for n_paths, order in ((2, 3), (2, 4), (3, 4), (4, 4), (5, 3)):   # fewer DISTINCT prices than coefficients are left
            m = gbm_matrix(n_paths, 5, 400 + n_paths + order + 1000 * DUP_RESEED.get((n_paths, order), 0))
            for it in (2, 5):
                cases.append(case(kind, m, False, 110.0, 0.69 * 5 * DT, poly_order=order, max_iterations=it))
    for name, (m, is_call, K) in crafted_matrices().items():
        if name.startswith("constant"):
            continue            # (degenerate_cases)
        steps = m.shape[1] - 1
        for order in (range(5) if kind in ("lsm", "mart") else (0,)):
            for T in (steps * DT, 0.69 * steps * DT):
                cases.append(case(kind, m, is_call, K, T, poly_order=order, max_iterations=(1, 5)[order % 2], num_branches=(10, 4)[order % 2]))
    if kind == "asym":
        cases += asym_special_cases()
    for d in cases:
        d.setdefault("r", R)
    return cases


def degenerate_cases(kind):
    """The constant matrices: rank-1 regressions at every order and, at r = 0, where every date's discounted payoff is the
    SAME number, ties in BranchingProcesses' strict > between exercise and continuation and in MartingaleOptimization's first
    maximum.  Both sides see identical numbers (exp(-0 t) = 1 exactly), so the comparison with the oracle is as sharp as
    anywhere.  But a tie and an exactly rank-deficient regression are discontinuities BY CONSTRUCTION: 1 + 1e-13 N(0, 1) on the
    entries breaks the tie and lifts the rank, after which the reference's own rank rule fits the noise (measured: the oracle's
    MartingaleOptimization price of a perturbed constant matrix moves by 8e-4 K at order 1).  No seed or strike changes that, so
    the conditioning check cannot speak about these cases and they stand in a list of their own, outside it."""
    cases = []
    for name in ("constant, in", "constant call, in", "constant, at"):
        m, is_call, K = crafted_matrices()[name]
        for order in (range(5) if kind in ("lsm", "mart") else (0,)):
            for r in (R, 0.0):
                for T in (17 * DT, 0.69 * 17 * DT):
                    cases.append(case(kind, m, is_call, K, T, r=r, poly_order=order, num_branches=(9, 4)[order % 2], max_iterations=(5, 1)[order % 2]))
    return cases


def asym_special_cases():
    out = []
    # dt = 0.25, 8 steps, T = 2: T - t >= 1 at t <= 1, where log(1 / eps) <= 0 and the boundary's square root is NaN (> 1) or 0 (= 1)
    m = gbm_matrix(129, 8, 300, dt=0.25)
    for is_call in (False, True):
        out.append(case("asym", m, is_call, 100.0, 2.0, dt=0.25))
        out.append(case("asym", m, is_call, 100.0, 1.0, dt=0.25))      # (T - t = 1 at the first date)
    # dates with T - t < 0.01 (the boundary's drift term) and T - t < 1e-10 (the boundary is the strike)
    m = gbm_matrix(65, 33, 301)
    for is_call in (False, True):
        for T in (20 * DT + 0.003, 20 * DT + 5e-11, 33 * DT + 0.009, 5e-11):
            out.append(case("asym", m, is_call, 100.0, T, sigma=0.45, dividend=0.07))
    # a NaN and an Inf at the first, a middle and the last date of a path of the second, third and fourth 64-lane group
    base = gbm_matrix(250, 17, 302)
    for bad in (math.nan, math.inf, -math.inf):
        for date, path in ((0, 64 + 5), (8, 128 + 7), (17, 192 + 9)):
            m = base.copy()
            m[path, date] = bad
            out.append(case("asym", m, date % 2 == 0, 100.0, 17 * DT))
    m = base.copy()
    m[64 + 5, 0], m[128 + 7, 8], m[192 + 9, 17], m[249, 3] = math.nan, math.inf, math.nan, -math.inf
    out.append(case("asym", m, False, 105.0, 17 * DT))
    return out


def oracle_price(orc, d, matrix=None):
    """The oracle's price of a (d) case (on `matrix` in place of the case's own, for the conditioning check)."""
    m = d["matrix"] if matrix is None else matrix
    a = (m, d["r"], d["K"], d["T"], d["dt"], d["is_call"])
    if d["kind"] == "asym":
        return orc.asymptotic_price(*a, d["sigma"], d["dividend"], step_major=False)
    if d["kind"] == "branching":
        return orc.branching_price(*a, d["num_branches"], np.arange(m.shape[1] - 1, dtype=np.int32), D_SEED, mode="philox",
                                   step_major=False)[0]
    if d["kind"] == "lsm":
        return orc.lsm_price(*a, d["poly_order"], step_major=False)
    return orc.martingale_price(*a, d["poly_order"], d["max_iterations"], step_major=False)[0]


def perturbed(matrix, seed, date_axis):
    """A copy whose entries after the first date are multiplied by 1 + 1e-13 N(0, 1)."""
    z = np.random.RandomState(seed).standard_normal(matrix.shape)
    f = 1.0 + PERTURBATION * z
    if date_axis == 0:
        f[0, :] = 1.0
    else:
        f[:, 0] = 1.0
    return matrix * f


def first_order(matrix, K):
    """What 1 + 1e-13 N(0, 1) on the entries can move a mean of discounted payoffs by, over K (the module's docstring)."""
    top = float(np.nanmax(np.where(np.isfinite(matrix), np.abs(matrix), 0.0)))
    return 6.0 * PERTURBATION * top / K


# ---- the checks -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.mark.parametrize("H,eta", H_ETA)
def test_spectrum_restatement_against_the_oracle(orc, H, eta):
    worst = [0.0, 0.0]
    for steps in SPECTRUM_STEPS:
        amp, comp = spectrum_numpy(H, eta, DT, steps)
        wamp, wcomp = orc.rbergomi_spectrum(H, eta, DT, steps)
        assert amp.shape == wamp.shape == (next_pow2(steps),) and comp.shape == wcomp.shape == (steps,)
        ea, ec = spectrum_errors(amp, comp, wamp, wcomp)
        worst = [max(worst[0], ea), max(worst[1], ec)]
        assert ea <= AMP_AGAINST_ORACLE and ec <= COMP_AGAINST_ORACLE, (steps, H, eta, ea, ec)
    print(f"\nspectrum restatement against the oracle, H {H} eta {eta}: amplitudes {worst[0]:.2e}, compensator {worst[1]:.2e}")


def test_weight_rows_order():
    rows = weight_rows()
    assert sorted((d["n_steps"], d["H"], d["eta"]) for d in rows) == sorted((s, H, e) for s in SPECTRUM_STEPS for H, e in H_ETA)
    for c in range(4):
        mine = [d["n_steps"] for d in rows if lds_class(next_pow2(d["n_steps"])) == c]
        assert len(set(mine)) >= 2 and mine[0] != max(mine) and mine[-1] != max(mine), (c, mine)
    classes = [lds_class(next_pow2(d["n_steps"])) for d in rows[:8]]
    assert len(set(classes)) == 4                       # interleaved: a chunk's rows are not consecutive rows of the call


def test_path_calls_cover_what_they_name():
    assert sorted(n for n, _ in PATH_CALLS) == [1, 2, 3, 63, 64, 65, 127, 128, 129, 250, 255, 256]
    assert {next_pow2(s) for s in PATH_CALLS[0][1]} == {1 << k for k in range(11)}
    for n, steps in PATH_CALLS:
        assert len(steps) >= 4                          # row indices 0, 1 and one >= 3
        assert n <= 64 or n == 250 or max(steps) < 1020


def test_pricer_calls_cover_the_sweep():
    calls = pricer_calls()
    assert {(c["poly_order"], c["max_iterations"]) for c in calls} == {(o, i) for o in range(5) for i in ITERATIONS}
    assert {c["num_branches"] for c in calls} == set(BRANCHES)
    for c in calls:
        seen = {(d["is_call"], d["strike"]) for d in c["rows"]}
        assert seen == {(cp, K) for cp in (0, 1) for K in STRIKES}
        assert len({d["n_steps"] for d in c["rows"] if d["n_steps"] <= 128}) >= 5
        assert all(d["n_steps"] < 1020 or c["n_paths"] <= 64 for d in c["rows"])
        for d in c["rows"][:30]:
            assert d["maturity"] in maturities(d["n_steps"])
    # 2 n_paths on both sides of order + 1 at orders 3 and 4
    assert {(c["n_paths"], c["poly_order"]) for c in calls} >= {(1, 3), (2, 4), (3, 3), (3, 4)}
    assert {lds_class(next_pow2(d["n_steps"])) for c in calls for d in c["rows"]} == {0, 1, 2, 3}


@pytest.mark.parametrize("kind", ["asym", "branching", "lsm", "mart"])
def test_class_api_cases_cover_the_sweep(kind):
    cases = class_api_cases(kind)
    assert {d["matrix"].shape[0] for d in cases} >= {1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 192, 193, 250, 256}
    assert {d["matrix"].shape[1] - 1 for d in cases} >= {1, 2, 3, 15, 16, 17, 33, 1020}
    assert {(d["is_call"], d["K"]) for d in cases} >= {(cp, K) for cp in (False, True) for K in STRIKES}
    assert any(d["T"] < 0.0 for d in cases) and any(d["T"] == 0.0 for d in cases)
    if kind in ("lsm", "mart"):
        assert {(d["poly_order"], d["max_iterations"]) for d in cases} >= {(o, i) for o in range(5) for i in (1, 5)}
        assert {(d["matrix"].shape[0], d["poly_order"], d["max_iterations"]) for d in cases} >= {(n, o, i) for n in (1, 2, 3) for o in (3, 4) for i in (1, 5)}
    if kind == "branching":
        assert {d["num_branches"] for d in cases} >= set(D_BRANCHES)


def assert_conditioned(responses):
    bad = [x for x in responses if x[1] > x[2]]
    assert not bad, bad[:5]


@pytest.mark.parametrize("c", range(15))
def test_batch_cases_are_well_conditioned(orc, c):
    """(c): the matrix of row i is the oracle's own rBergomi block (the device's differs from it by ~1e-13, the size of the
    perturbation)."""
    call = pricer_calls()[c]
    cols = four_columns(call["poly_order"])
    out = []
    for i, d in enumerate(call["rows"]):
        block = orc.paths_rbergomi(call["seed"], d["S0"], R, d["xi"], d["H"], d["eta"], d["rho"], DT, d["n_steps"], i << 32, call["n_paths"])
        a = oracle_four(orc, block, d, call, i)
        b = oracle_four(orc, perturbed(block, 1000 * c + i, 0), d, call, i)
        allow = first_order(block, d["strike"])
        for col, x, y in zip(cols, a, b):
            out.append(((c, i, col, x, y), abs(x - y) / d["strike"], RESPONSE_SHARE * BOUNDS[col] + allow))
    assert_conditioned(out)


@pytest.mark.parametrize("kind", ["asym", "branching", "lsm", "mart"])
def test_class_api_cases_are_well_conditioned(orc, kind):
    out = []
    for k, d in enumerate(class_api_cases(kind)):
        x, y = oracle_price(orc, d), oracle_price(orc, d, perturbed(d["matrix"], 5000 + k, 1))
        col = column_of(kind, d["poly_order"])
        out.append(((kind, k, d["matrix"].shape, d["poly_order"], d["T"], x, y), abs(x - y) / d["K"],
                    RESPONSE_SHARE * BOUNDS[col] + first_order(d["matrix"], d["K"])))
    assert_conditioned(out)
