"""The Bates / Merton generator on the GPU (mcg_paths_bates, mcg_paths_bates_payoff; PathEngine.bates, PathEngine.merton)
against the numpy reference of tests/test_bates_reference.py on the same (seed, path ids), against the Heston generators at
lambda = 0 bit for bit, against two closed forms, and through the consumers of a path matrix.

Parity bounds: S is compared relatively, v on the scale max(v0, theta).  The device evaluates the same scheme with its own
logarithm, sine / cosine, square root, reciprocal and exponential (<= ~2 ulp each) and with fused multiply-adds, so the
difference from numpy is rounding that accumulates over the steps; the jump adds one more normal, a square root of a small
integer and two fused multiply-adds to the exponent of a step.  S_BOUND and V_BOUND are ten times the largest error
observed on an MI355X over all cases of this file, per base scheme (observed: Euler S 1.87e-14, v 6.94e-15, on the 252-step
shapes; QE S 8.15e-14, v 5.74e-13, both on the 252-step Feller-violating shape), far inside the 1e-9 they may not exceed.
The cases are test_bates_reference.BATES_PARITY_SETS, where every uniform keeps a distance of 1e-9 from every threshold of
the jump count (and from QE's two branch decisions) and the reference's own rounding error is held to 1e-11.
The fused payoff, the consumers and the exotics keep the bounds of the Heston files (test_gpu_heston.py, test_gpu_heston_qe.py).

The jump count N = #{k : uN > c_k}, which the device decides as word > floor(c_k 2^32 - 1/2) on a ladder of thresholds that a
wave climbs only as far as one of its lanes passes, is tested at every threshold and every count it can reach:
  - the "ladder" set (lambda dt = 1; 7 x 4097 and 6 x 8191 paths with steps of 6, 7, 8 and 9 jumps) and launches in which one
    word lies exactly on threshold k (k = 0..7; QE: 0, 2, 6) at two adjacent lambda dt, on the product path in all its
    compiled forms.  These carry exponents the older sets never had, so their error is measured apart ("ladder ..." in the
    report).  Observed on an MI355X: Euler S 1.11e-15, v 0 (Merton's parameters: the variance never moves); QE S 1.11e-15,
    v 4.86e-15 -- a few steps only, below the bounds above, which therefore hold for them as they stand;
  - the counts no seed reaches (10..12 at lambda dt = 1 need a word within 1e-9 of 2^32) and the wave-level behaviour of the
    ladder through mcg_debug_eval_v fn 9, which runs WithJumps::count and WithJumps::jump -- the product's code -- on chosen
    words: counts as exact integers against the contract's comparison in binary64, J against mpmath (observed: 6.66 ulp of
    |J| where N mu_J and sigma_J sqrt(N) z3 cancel to a third of their size, inside the four roundings the code makes).
Mutation check (each in a scratch build, one run of this file on an MI355X; every test that existed before stayed green):
  (a) `>` becomes `>=` in the count's comparison: caught on the product path (test_words_exactly_on_a_threshold, both schemes:
      the path on the threshold is off by 36 % at L_lo) and by the hook (test_count_of_every_word_next_to_a_threshold at every
      L, test_quiet_wave_beside_a_jumping_wave); the ladder set does not see it, as no word of it lies on a threshold;
  (b) the second lazy load reads T[j + 1] for T[j]: caught on the product path (test_count_ladder_parity_with_numpy, both
      schemes, by its steps of 7 jumps and more: 15 % in S; test_words_exactly_on_a_threshold at k = 6) and by the hook (three
      tests).  The second load filling T[6..11] only: caught by the hook alone (counts of 13..16 at the last four words, in
      test_count_of_every_word_next_to_a_threshold[1.0], test_one_lane_drives_the_ladder and test_jump_size_against_mpmath)
      -- no seed brings a word within 1e-9 of 2^32, which is why the hook exists;
  (c) the host takes floor(c_k 2^32) without the half: caught on the product path (test_words_exactly_on_a_threshold, both
      schemes, at L_hi, where the word must pass the threshold and does not: 56 %), by every hook test through the constants
      they first compare with the reference's, and without a GPU by test_bates_reference.py::test_library_constants_are_the_references."""
import math

import mpmath as mp
import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from montecarlooptionspricer_amd.engine import bates_constants
from test_bates_reference import (BATES_PARITY_SETS, BOUNDARY_JUMPS, BOUNDARY_KS, BOUNDARY_PATHS, BOUNDARY_SEED, BOUNDARY_STEPS,
                                  JUMP_CAP, LADDER_BASE, LADDER_CASES, MERTON_ROW, PARITY_CASES, RARE_JUMPS, bates_closed_form,
                                  bates_numpy, boundary_cases, boundary_runs, jump_constants, jump_thresholds, merton_series,
                                  parity_set, stat_cases)
from test_heston_qe_reference import uniform_of_words
from test_exotics_reference import stats_numpy
from test_gpu_exotics import check_prices, full_book
from test_heston_reference import PARAMS, R, S0, SEED64, STAT_SEED, STD_ERRORS, STRIKES

pytestmark = pytest.mark.gpu

S_BOUND = {"euler": 1.9e-13, "qe": 8.2e-13}
V_BOUND = {"euler": 7.0e-14, "qe": 5.8e-12}
DT = 1.0 / 252.0
STAT_PATHS = 1_000_000
observed = {"euler S": 0.0, "euler v": 0.0, "qe S": 0.0, "qe v": 0.0}
# the same over the cases of lambda dt up to 1 (the ladder set and the words on a threshold), which carry exponents the older
# sets never had: measured apart, held to the same bounds
observed.update({"ladder " + k: 0.0 for k in list(observed)})


@pytest.fixture(scope="module")
def eng():
    with mc.PathEngine(0) as e:
        yield e


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest errors against numpy in this run: " + ", ".join(f"{k} {v:.2e}" for k, v in observed.items()))


def bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


def jumps(j):
    """The jump parameters of the reference file under the names of PathEngine.bates."""
    return dict(jump_intensity=j["lam"], jump_mean=j["mu_j"], jump_std=j["sigma_j"])


def gen(p, j, dt, n_steps, scheme):
    return dict(S0=S0, r=R, dt=dt, n_steps=n_steps, scheme=scheme, **p, **jumps(j))


def reference(seed, p, j, dt, n_steps, n_paths, path_begin, scheme, cache={}):
    """One numpy run per case, shared by its four forms (never written to): (S, v, jumps per (step, path))."""
    key = (seed, tuple(sorted(p.items())), tuple(sorted(j.items())), dt, n_steps, n_paths, path_begin, scheme)
    if key not in cache:
        t = {}
        S, v = bates_numpy(seed, S0, R, dt=dt, n_steps=n_steps, n_paths=n_paths, path_begin=path_begin, scheme=scheme, trace=t, **p, **j)
        cache[key] = (S, v, t["jumps"])
    return cache[key]


def check_parity(eng, seed, p, j, dt, n_steps, n_paths, path_begin, scheme, want_variance, payoff, where, tag=""):
    S, v, _ = reference(seed, p, j, dt, n_steps, n_paths, path_begin, scheme)
    got = eng.bates(seed, n_paths=n_paths, path_begin=path_begin, payoff=payoff, want_variance=want_variance,
                    **gen(p, j, dt, n_steps, scheme))
    P, V = got if want_variance else (got, None)
    assert (P.n_paths, P.n_steps) == (n_paths, n_steps)
    gs = P.to_host_step_major()
    es = float(np.abs(gs / S - 1.0).max())
    observed[tag + scheme + " S"] = max(observed[tag + scheme + " S"], es)
    print(f"{where}: S {es:.2e}", end="")
    assert es <= S_BOUND[scheme], (where, "S", es)
    if V is not None:
        assert (V.n_paths, V.n_steps) == (n_paths, n_steps)
        gv = V.to_host_step_major()
        ev = float(np.abs(gv - v).max()) / max(p["v0"], p["theta"])
        observed[tag + scheme + " v"] = max(observed[tag + scheme + " v"], ev)
        print(f", v {ev:.2e}", end="")
        assert ev <= V_BOUND[scheme], (where, "v", ev)
        if scheme == "qe":
            assert (gv >= 0.0).all() and np.array_equal(gv == 0.0, v == 0.0), (where, "the zeros of v")
        V.free()
    print()
    if payoff is not None:
        K, is_call = payoff
        T = n_steps * dt
        x = np.maximum(gs[-1] - K, 0.0) if is_call else np.maximum(K - gs[-1], 0.0)
        m, se = eng.price_european(P, K, R, T, is_call)
        D = math.exp(-R * T)
        assert abs(m - D * x.mean()) <= 1e-12 * max(D * x.mean(), 1e-300), (where, "fused price")
        if n_paths > 1 and x.std() > 0.0:
            # the library forms the std error from {sum, sum^2}: the relative error of the sums times (1/2 + mean^2 / variance)
            want_se = D * x.std(ddof=1) / math.sqrt(n_paths)
            cond = max(1.0, 0.5 + (x.mean() / x.std()) ** 2)
            assert abs(se - want_se) <= 1e-9 * cond * want_se, (where, "fused std error", se, want_se, cond)
    P.free()


@pytest.mark.parametrize("name, scheme", PARITY_CASES)
def test_parity_with_numpy(eng, name, scheme):
    p, j, dt, shapes = BATES_PARITY_SETS[name]
    for k, (n_steps, n_paths, begin, seed) in enumerate(shapes[scheme]):
        for want_variance in (False, True):
            for payoff in (None, (100.0, (k + want_variance) % 2 == 0)):
                check_parity(eng, seed, p, j, dt, n_steps, n_paths, begin, scheme, want_variance, payoff,
                             (name, scheme, n_steps, n_paths, begin, want_variance, payoff))


@pytest.mark.parametrize("name, scheme", LADDER_CASES)
def test_count_ladder_parity_with_numpy(eng, name, scheme):
    """lambda dt = 1: steps with 6, 7, 8 and 9 jumps, so that the thresholds of the second lazy load decide (the older sets reach
    6 once).  Every compiled form of the kernel."""
    p, j, dt, shapes = parity_set(name, scheme)
    for k, (n_steps, n_paths, begin, seed) in enumerate(shapes):
        assert reference(seed, p, j, dt, n_steps, n_paths, begin, scheme)[2].max() >= 8
        for want_variance in (False, True):
            for payoff in (None, (100.0, (k + want_variance) % 2 == 0)):
                check_parity(eng, seed, p, j, dt, n_steps, n_paths, begin, scheme, want_variance, payoff,
                             (name, scheme, n_steps, n_paths, begin, want_variance, payoff), tag="ladder ")


@pytest.mark.parametrize("scheme", ["euler", "qe"])
def test_words_exactly_on_a_threshold(eng, scheme):
    """A stream-4 word w of one path and the two adjacent binary64 lambda dt with T_k = w (w > T_k fails: k jumps) and T_k = w - 1
    (k + 1 jumps), for every k of BOUNDARY_KS: > against >=, a threshold off by one word or the half left out of the floor
    moves that path's ln S by mu_J + sigma_J z3 = -0.5 +- 0.1 z3.  The crafted path sits in the first column, in an odd column
    of the wave's upper lanes and in the last column (an odd one in the second wave); the four forms of the kernel take turns."""
    p = LADDER_BASE[scheme]
    cases = boundary_cases(scheme)
    assert [c["k"] for c in cases] == list(BOUNDARY_KS[scheme])
    form = 0
    for c in cases:
        for L, count, lam, dt, begin, column in boundary_runs(c, scheme):
            j = dict(lam=lam, **BOUNDARY_JUMPS)
            counts = reference(BOUNDARY_SEED, p, j, dt, BOUNDARY_STEPS, BOUNDARY_PATHS, begin, scheme)[2]
            assert counts[c["step"], column] == count, (c, L, column)
            want_variance, payoff = form & 1 == 1, ((100.0, form & 4 == 0) if form & 2 else None)
            form += 1
            check_parity(eng, BOUNDARY_SEED, p, j, dt, BOUNDARY_STEPS, BOUNDARY_PATHS, begin, scheme, want_variance, payoff,
                         ("threshold", scheme, c["k"], L, column, want_variance, payoff), tag="ladder ")


def test_lambda_dt_of_one_is_the_edge(eng):
    ok = dict(seed=1, S0=100.0, r=0.04, v0=0.04, kappa=2.0, theta=0.04, sigma_v=0.3, rho=-0.7, jump_mean=-0.1, jump_std=0.15, n_steps=5,
              n_paths=100)
    for scheme in ("euler", "qe"):
        for lam, dt in ((1.0, 1.0), (4.0, 0.25), (0.5, 2.0)):
            assert lam * dt == 1.0
            M = eng.bates(**ok, jump_intensity=lam, dt=dt, scheme=scheme)
            assert np.isfinite(M.to_host_step_major()).all()
            M.free()
        with pytest.raises(mc.McgError) as e:
            eng.bates(**ok, jump_intensity=math.nextafter(1.0, 2.0), dt=1.0, scheme=scheme)
        assert e.value.status == 1 and "lambda * dt <= 1" in str(e.value) and "more steps" in str(e.value), str(e.value)


# ---- the count and the jump size on chosen words (mcg_debug_eval_v fn 9: WithJumps::count and WithJumps::jump) ----------------
V_BATES_COUNT = 9
TOP = 2 ** 32 - 1
J_OBSERVED = 6.66      # worst error of J against mpmath, in ulp of |J|: at mu_J = -0.5, sigma_J = 0.1, N = 2, z3 = 5


def hook(eng, L, words, z3=None, elem=0, mu_j=-0.1, sigma_j=0.15):
    """words: [n][4] stream-4 words -> (counts [n][4], J [n] of element elem, comp), and the constants the library derives."""
    words = np.asarray(words, dtype=np.int64)
    comp, T = bates_constants(L, mu_j, sigma_j, 1.0)
    assert T == jump_thresholds(L) and comp == jump_constants(L, mu_j, sigma_j, 1.0)[0]
    z3 = np.zeros(len(words)) if z3 is None else np.asarray(z3, dtype=np.float64)
    y = eng.debug_eval_v(V_BATES_COUNT, np.column_stack([words.astype(np.float64), z3]), [L, mu_j, sigma_j, comp] + T + [elem])
    cnt = y[:, 0].astype(np.int64)
    assert (cnt == y[:, 0]).all() and (y[:, 2:] == 0.0).all()
    return np.stack([(cnt >> (8 * e)) & 0xFF for e in range(4)], axis=1), y[:, 1], comp


def counts_of(L, words):
    """The contract's count of every word: #{k : uN > c_k}, uN = (word + 1/2) 2^-32, in binary64."""
    c = jump_constants(L, 0.0, 0.0, 1.0)[1]
    return (uniform_of_words(np.asarray(words, dtype=np.uint64))[..., None] > c).sum(axis=-1)


@pytest.mark.parametrize("L", [0.004, 0.5, 1.0])
def test_count_of_every_word_next_to_a_threshold(eng, L):
    """The words 0, 1, T_k - 1, T_k, T_k + 1 (k = 0..15), 2^32 - 2 and 2^32 - 1 in each of the four element positions, alone
    in their path and beside three others.  At L = 1 the largest count is 12 (T_12 = ... = T_15 = 2^32 - 1): never 16."""
    T = jump_thresholds(L)
    W = sorted({min(max(w, 0), TOP) for w in [0, 1, TOP - 1, TOP] + [t + d for t in T for d in (-1, 0, 1)]})
    m = len(W)
    alone = [[w if e == pos else 0 for e in range(4)] for pos in range(4) for w in W]
    mixed = [[W[i], W[(i + 7) % m], W[(i + 19) % m], W[(i + 31) % m]] for i in range(m)]
    words = np.array(alone + mixed + mixed[::-1], dtype=np.int64)
    assert all(set(words[:, e]) >= set(W) for e in range(4))
    got, _, _ = hook(eng, L, words)
    want = counts_of(L, words)
    assert np.array_equal(want, (words[..., None] > np.array(T)).sum(axis=-1))
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    print(f"L = {L}: {len(words)} paths, {m} words, largest count {got.max()}")
    assert got.max() == (12 if L == 1.0 else want.max()) and got.max() < JUMP_CAP


def test_one_lane_drives_the_ladder(eng):
    """A wave (128 paths) in which one path has c jumps in one step and the other 127 none, c = 1..12 at lambda dt = 1: the
    thresholds above T_0 are looked at because of that one lane.  The lane is 0, 31, 32 or 63 and the path its first or second."""
    L = 1.0
    T = jump_thresholds(L)
    spots = [(c, lane, which) for c in range(1, 13) for lane in (0, 31, 32, 63) for which in (0, 1)]
    words = np.zeros((128 * len(spots), 4), dtype=np.int64)
    for g, (c, lane, which) in enumerate(spots):
        words[128 * g + 2 * lane + which, (c + lane + which) % 4] = T[c - 1] + 1
    want = counts_of(L, words)
    per_wave = want.reshape(len(spots), -1)
    assert ((per_wave != 0).sum(axis=1) == 1).all() and list(per_wave.max(axis=1)) == [c for c, _, _ in spots]
    got, _, _ = hook(eng, L, words)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_quiet_wave_beside_a_jumping_wave(eng):
    """Inside one workgroup (512 paths, four waves): waves in which no path jumps, next to waves in which most do.  The quiet
    waves' counts are zero and their J is comp bit for bit, whatever z3 holds; so it is for the paths of a jumping wave that do
    not jump."""
    L, elem = 0.5, 2
    T = jump_thresholds(L)
    rng = np.random.default_rng(5)
    quiet = np.array([0, 1, 0, 1, 1, 0, 1, 1], dtype=bool)                 # two workgroups
    words = np.where(np.repeat(quiet, 128)[:, None], rng.integers(0, T[0] + 1, (1024, 4)), rng.integers(0, 2 ** 32, (1024, 4)))
    words[128:256:9, 1] = T[0]                                             # on the threshold is not above it
    z3 = rng.standard_normal(1024)
    z3[::5] = np.nan
    z3[1::7] = np.inf
    want = counts_of(L, words)
    assert (want.reshape(8, -1).sum(axis=1) == 0).tolist() == quiet.tolist() and want.max() >= 3
    got, J, comp = hook(eng, L, words, z3, elem)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    still = want[:, elem] == 0
    assert still[~np.repeat(quiet, 128)].any() and bits(J[still]) == bits(np.full(still.sum(), comp))
    fine = ~still & np.isfinite(z3)
    ref = comp + want[:, elem] * -0.1 + 0.15 * np.sqrt(want[:, elem]) * np.where(fine, z3, 0.0)
    assert np.abs(J[fine] - ref[fine]).max() <= 1e-14


@pytest.fixture(scope="module")
def jump_sizes():
    """(mu_j, sigma_j) -> [(N, z3, J at 50 digits, its inner sum and its normal term)], N = 0..12 and seven z3."""
    mp.mp.dps = 50
    out = {}
    for mu_j, sigma_j in ((-0.1, 0.15), (-0.5, 0.1), (0.05, 0.2)):
        comp = jump_constants(1.0, mu_j, sigma_j, 1.0)[0]
        out[mu_j, sigma_j] = [(n, z, mp.mpf(comp) + n * mp.mpf(mu_j) + mp.mpf(sigma_j) * mp.sqrt(n) * mp.mpf(z),
                               mp.mpf(comp) + n * mp.mpf(mu_j), mp.mpf(sigma_j) * mp.sqrt(n) * mp.mpf(z))
                              for n in range(13) for z in (0.0, 1e-3, -1e-3, 1.0, -1.0, 5.0, -5.0)]
    return out


def test_jump_size_against_mpmath(eng, jump_sizes):
    """J = comp + N mu_J + sigma_J sqrt(N) z3 for N = 0..12 at lambda dt = 1, in every element position, against 50 digits.
    The device rounds four times: fm::sqrt_pos (<= 1 ulp, test_gpu_math.py), its product with sigma_J, the fused comp + N mu_J
    and the fused sum -- at most 2^-53 (4 |sigma_J sqrt(N) z3| + |comp + N mu_J| + |J|), asserted as it stands.  In ulp of
    |J| that is a few, more where the two terms cancel; observed on an MI355X: J_OBSERVED = 6.66 (-1 + comp against 0.707),
    held to 1.5 times that.
    N = 0: J is comp bit for bit."""
    L = 1.0
    T = jump_thresholds(L)
    worst, at = 0.0, None
    for (mu_j, sigma_j), rows in jump_sizes.items():
        for elem in range(4):
            words = np.zeros((len(rows), 4), dtype=np.int64)
            words[:, elem] = [T[n - 1] + 1 if n else 0 for n, _, _, _, _ in rows]
            got, J, comp = hook(eng, L, words, [z for _, z, _, _, _ in rows], elem, mu_j, sigma_j)
            assert list(got[:, elem]) == [n for n, _, _, _, _ in rows] and not got[:, [e for e in range(4) if e != elem]].any()
            for (n, z, exact, inner, normal), j in zip(rows, J):
                if n == 0:
                    assert bits(j) == bits(comp), (n, z, j, comp)
                    continue
                err = abs(mp.mpf(float(j)) - exact)
                assert err <= mp.mpf(2) ** -53 * (4 * abs(normal) + abs(inner) + abs(exact)), (mu_j, sigma_j, n, z, float(j), float(err))
                ulps = float(err / mp.mpf(float(np.spacing(abs(float(exact))))))
                if ulps > worst:
                    worst, at = ulps, (mu_j, sigma_j, n, z)
    print(f"J against mpmath: worst {worst:.3f} ulp of |J| at (mu_j, sigma_j, N, z3) = {at}")
    assert worst <= 1.5 * J_OBSERVED, (worst, at)


def test_hook_refuses_what_is_no_word(eng):
    comp, T = bates_constants(1.0, -0.1, 0.15, 1.0)
    good = [1.0, -0.1, 0.15, comp] + T + [0]
    x = np.zeros((3, 5))
    eng.debug_eval_v(V_BATES_COUNT, x, good)
    for change in ({0: 1.5}, {0: -0.1}, {4: 0.5}, {19: 2.0 ** 32}, {20: 4}, {20: 0.5}):
        with pytest.raises(mc.McgError):
            eng.debug_eval_v(V_BATES_COUNT, x, [change.get(i, v) for i, v in enumerate(good)])
    for w in (-1.0, 2.0 ** 32, 0.5, float("nan")):
        bad = x.copy()
        bad[1, 2] = w
        with pytest.raises(mc.McgError):
            eng.debug_eval_v(V_BATES_COUNT, bad, good)
    with pytest.raises(mc.McgError):
        eng.debug_eval_v(V_BATES_COUNT, x, good[:-1])


@pytest.mark.parametrize("scheme", ["euler", "qe"])
def test_no_jumps_is_heston_bit_for_bit(eng, scheme):
    p = PARAMS["feller"]
    for n_steps, n_paths, begin in ((11, 5000, 0), (3, 513, 2 ** 33 + 1)):
        a = dict(S0=S0, r=R, dt=DT, n_steps=n_steps, n_paths=n_paths, path_begin=begin, scheme=scheme, **p)
        for mu_j, sigma_j in ((-0.1, 0.15), (0.1, 0.25), (0.0, 0.0)):       # (kbar < 0, > 0, = 0: comp = +0, -0, -0)
            j = dict(jump_intensity=0.0, jump_mean=mu_j, jump_std=sigma_j)
            H, HV = eng.heston(SEED64, want_variance=True, **a)
            B, BV = eng.bates(SEED64, want_variance=True, **a, **j)
            assert bits(B.to_host_step_major()) == bits(H.to_host_step_major())
            assert bits(BV.to_host_step_major()) == bits(HV.to_host_step_major())
            HF = eng.heston(SEED64, payoff=(100.0, False), **a)
            BF = eng.bates(SEED64, payoff=(100.0, False), **a, **j)
            T = n_steps * DT
            assert bits(eng.price_european(BF, 100.0, R, T, False)) == bits(eng.price_european(HF, 100.0, R, T, False))
            assert bits(BF.to_host_step_major()) == bits(H.to_host_step_major())
            for M in (H, HV, B, BV, HF, BF):
                M.free()


@pytest.mark.parametrize("scheme", ["euler", "qe"])
def test_sharding_and_determinism(eng, scheme):
    n, n_steps = 5000, 11
    for name in ("rare", "frequent"):
        p, j, dt, _ = BATES_PARITY_SETS[name]
        a = gen(p, j, dt, n_steps, scheme)
        P, V = eng.bates(SEED64, n_paths=n, want_variance=True, **a)
        whole_s, whole_v = P.to_host_step_major(), V.to_host_step_major()
        Q, W = eng.bates(SEED64, n_paths=n, want_variance=True, **a)
        assert bits(Q.to_host_step_major()) == bits(whole_s) and bits(W.to_host_step_major()) == bits(whole_v)
        only_s = eng.bates(SEED64, n_paths=n, **a)
        assert bits(only_s.to_host_step_major()) == bits(whole_s)          # the variance matrix changes nothing in S
        f1 = eng.bates(SEED64, n_paths=n, payoff=(100.0, False), **a)
        f2 = eng.bates(SEED64, n_paths=n, payoff=(100.0, False), **a)
        assert bits(eng.price_european(f1, 100.0, R, n_steps * dt, False)) == bits(eng.price_european(f2, 100.0, R, n_steps * dt, False))
        assert bits(f1.to_host_step_major()) == bits(whole_s)
        for M in (Q, W, only_s, f1, f2):
            M.free()
        # a shard boundary regroups the paths into other waves: a block skipped for a wave that needed it would show here
        for cut in (1537, 64, 4999):
            A, VA = eng.bates(SEED64, n_paths=cut, want_variance=True, **a)
            B, VB = eng.bates(SEED64, n_paths=n - cut, path_begin=cut, want_variance=True, **a)
            assert bits(np.hstack([A.to_host_step_major(), B.to_host_step_major()])) == bits(whole_s), (name, cut)
            assert bits(np.hstack([VA.to_host_step_major(), VB.to_host_step_major()])) == bits(whole_v), (name, cut)
            for M in (A, VA, B, VB):
                M.free()
        if name == "rare":
            # ... and the skip is exercised: some wave (128 adjacent paths) has no jump in some Philox block, some wave has
            # jumps in some of its lanes only; and the whole matrix is the reference's
            S, _, count = reference(SEED64, p, j, dt, n_steps, n, 0, scheme)
            per_block = np.stack([count[4 * b:4 * b + 4, :4992].sum(axis=0) for b in range((n_steps + 3) // 4)]).reshape(-1, 39, 128)
            assert (per_block.sum(axis=2) == 0).any()
            jumped = per_block > 0
            assert (jumped.any(axis=2) & ~jumped.all(axis=2)).any()
            assert float(np.abs(whole_s / S - 1.0).max()) <= S_BOUND[scheme]
        P.free()
        V.free()


def test_merton(eng):
    # without jumps: the GBM generator, to the bound of test_gpu_heston.py::test_reduction_to_gbm
    n_steps, n_paths, dt = 50, 3000, 0.02
    M0 = eng.merton(7, S0, R, 0.2, 0.0, -0.1, 0.15, dt, n_steps, n_paths, path_begin=5)
    G = eng.gbm(7, S0, R, 0.2, dt, n_steps, n_paths, path_begin=5)
    m, g = M0.to_host_step_major(), G.to_host_step_major()
    err = float(np.abs(m / g - 1.0).max())
    print(f"Merton without jumps against the GBM generator {err:.2e}")
    assert err <= 2e-11 and (m[0] == S0).all()
    M0.free()
    G.free()
    # with jumps: Merton's series
    c = MERTON_ROW
    T, n_steps = c["T"], c["n_steps"]
    j = dict(jump_intensity=c["lam"], jump_mean=c["mu_j"], jump_std=c["sigma_j"])
    P = eng.merton(STAT_SEED, S0, R, c["sigma"], dt=T / n_steps, n_steps=n_steps, n_paths=STAT_PATHS, **j)
    fwd, fwd_se = eng.price_european(P, 0.0, R, T, True)
    print(f"martingale: e^-rT mean(S_T) = {fwd:.5f} +- {fwd_se:.5f}, {(fwd - S0) / fwd_se:+.2f} std errors")
    assert fwd_se > 0.0 and abs(fwd - S0) <= STD_ERRORS * fwd_se
    for K in STRIKES:
        for is_call in (True, False):
            want = merton_series(S0, K, R, T, c["sigma"], c["lam"], c["mu_j"], c["sigma_j"], is_call)
            price, se = eng.price_european(P, K, R, T, is_call)
            print(f"K={K:g} call={is_call}: {price:.5f} +- {se:.5f}, series {want:.5f}, {abs(price - want) / se:.2f} std errors")
            assert se > 0.0 and abs(price - want) <= STD_ERRORS * se, (K, is_call, price, want, se)
    F = eng.merton(STAT_SEED, S0, R, c["sigma"], dt=T / n_steps, n_steps=n_steps, n_paths=STAT_PATHS, payoff=(100.0, False), **j)
    assert bits(F.to_host_step_major()[-1]) == bits(P.to_host_step_major()[-1])
    F.free()
    P.free()


@pytest.mark.parametrize("scheme, p, j, T, n_steps", stat_cases())
def test_closed_form_and_martingale(eng, scheme, p, j, T, n_steps):
    a = gen(p, j, T / n_steps, n_steps, scheme)
    P = eng.bates(STAT_SEED, n_paths=STAT_PATHS, **a)
    fwd, fwd_se = eng.price_european(P, 0.0, R, T, True)
    print(f"martingale: e^-rT mean(S_T) = {fwd:.5f} +- {fwd_se:.5f}, {(fwd - S0) / fwd_se:+.2f} std errors")
    assert fwd_se > 0.0 and abs(fwd - S0) <= STD_ERRORS * fwd_se
    for K in STRIKES:
        for is_call in (True, False):
            want = bates_closed_form(S0, K, R, T, is_call=is_call, **p, **j)
            price, se = eng.price_european(P, K, R, T, is_call)
            print(f"K={K:g} call={is_call}: {price:.5f} +- {se:.5f}, closed form {want:.5f}, {abs(price - want) / se:.2f} std errors")
            assert se > 0.0 and abs(price - want) <= STD_ERRORS * se, (K, is_call, price, want, se)
            F = eng.bates(STAT_SEED, n_paths=STAT_PATHS, payoff=(K, is_call), **a)
            fused, fused_se = eng.price_european(F, K, R, T, is_call)
            F.free()
            assert abs(fused - price) <= 1e-12 * price and abs(fused_se - se) <= 1e-9 * se
            assert abs(fused - want) <= STD_ERRORS * fused_se
            g = eng.greeks_european(P, K, R, T, is_call, sigma=0.0)
            assert abs(g["price"] - want) <= STD_ERRORS * g["price_se"] and abs(g["price"] - price) <= 1e-12 * price
            assert all(math.isfinite(g[k]) for k in ("delta", "rho", "dual_delta")) and math.isnan(g["gamma"]) and math.isnan(g["vega"])
    P.free()


def test_consumers_accept_the_matrix(eng):
    p, n_steps, dt, n = PARAMS["feller"], 50, 0.02, 100_000
    T = n_steps * dt
    P, V = eng.bates(STAT_SEED, n_paths=n, want_variance=True, **gen(p, RARE_JUMPS, dt, n_steps, "qe"))
    put, put_se = eng.price_european(P, 100.0, R, T, False)
    lsm, lsm_se = eng.price_lsm(P, R, 100.0, T, dt, False, 2)
    lsm2, lsm2_se = eng.price_lsm2(P, V, R, 100.0, T, dt, False, 2)
    print(f"European put {put:.4f} +- {put_se:.4f}, LSM put {lsm:.4f} +- {lsm_se:.4f}, on (S, v) {lsm2:.4f} +- {lsm2_se:.4f}")
    assert math.isfinite(lsm) and math.isfinite(lsm2) and lsm >= put - 3.0 * put_se and lsm2 >= put - 3.0 * put_se
    X = P.to_host()
    for first_row in (0, 1):
        st5 = stats_numpy(X, first_row)
        book = full_book(st5, (90.0, 100.0, 110.0))
        price, se = eng.price_exotics(P, R, T, book, first_row=first_row)
        check_prices(price, se, book, st5, R, T, ("bates-qe", first_row))
    # jumps reach the barrier: the down-and-out put at 80 is worth less than without them
    knock = [mc.exotic("barrier_down_out", False, 100.0, 80.0, 0.0)]
    H = eng.bates(STAT_SEED, n_paths=n, **gen(p, dict(RARE_JUMPS, lam=0.0), dt, n_steps, "qe"))
    (with_j,), (with_se,) = eng.price_exotics(P, R, T, knock)
    (without,), (without_se,) = eng.price_exotics(H, R, T, knock)
    print(f"down-and-out put at 80: {with_j:.4f} +- {with_se:.4f} with jumps, {without:.4f} +- {without_se:.4f} without")
    assert abs(with_j - without) > 5.0 * math.hypot(with_se, without_se)
    for M in (P, V, H):
        M.free()


def test_invalid_arguments_and_edges(eng):
    L = mc.load_library()
    ok = dict(seed=1, S0=100.0, r=0.04, v0=0.04, kappa=2.0, theta=0.04, sigma_v=0.3, rho=-0.7, jump_intensity=1.0, jump_mean=-0.1,
              jump_std=0.15, dt=DT, n_steps=8, n_paths=100)
    nan, inf = float("nan"), float("inf")
    base_bad = [dict(S0=0.0), dict(S0=-1.0), dict(dt=0.0), dict(dt=-DT), dict(v0=-0.01), dict(kappa=-1.0), dict(theta=-0.04),
                dict(sigma_v=-0.3), dict(rho=1.0001), dict(rho=-1.5), dict(n_steps=0), dict(n_paths=-1)]
    base_bad += [{k: x} for k in ("S0", "r", "v0", "kappa", "theta", "sigma_v", "rho", "dt") for x in (nan, inf, -inf)]
    jump_bad = [dict(jump_intensity=-0.5), dict(jump_std=-0.1), dict(jump_intensity=253.0), dict(jump_intensity=1.0001 / DT),
                dict(jump_mean=1.0001), dict(jump_mean=-1.5), dict(jump_std=1.0001)]
    jump_bad += [{k: x} for k in ("jump_intensity", "jump_mean", "jump_std") for x in (nan, inf, -inf)]
    for scheme in ("euler", "qe"):
        eng.bates(**ok, scheme=scheme).free()
        for change in base_bad + jump_bad + ([dict(sigma_v=0.0)] if scheme == "qe" else []):
            for extra in (dict(), dict(payoff=(100.0, True)), dict(want_variance=True)):
                with pytest.raises(mc.McgError) as e:
                    eng.bates(**dict(ok, **change), scheme=scheme, **extra)
                assert e.value.status == 1 and str(e.value) and L.mcg_last_error(), change
                if change.get("jump_intensity", 0.0) > 1.0 / DT and math.isfinite(change["jump_intensity"]):
                    assert "lambda * dt <= 1" in str(e.value) and "more steps" in str(e.value), str(e.value)
        with pytest.raises(mc.McgError) as e:
            eng.bates(**ok, scheme=scheme, payoff=(nan, True))
        assert e.value.status == 1
    with pytest.raises(ValueError):
        eng.bates(**ok, scheme="nonsense")
    # a scheme number that is neither value, in both C forms
    import ctypes as C
    h = C.c_void_p()
    model = (eng._ctx, 1, 100.0, 0.04, 0.04, 2.0, 0.04, 0.3, -0.7, 1.0, -0.1, 0.15, DT, 8, 0, 100)
    for scheme in (2, -1):
        assert L.mcg_paths_bates(*model, scheme, C.byref(h), None) == 1 and b"scheme" in L.mcg_last_error()
        assert L.mcg_paths_bates_payoff(*model, scheme, 100.0, 1, C.byref(h), None) == 1 and b"scheme" in L.mcg_last_error()
    # the edges of the valid set
    edges = (dict(jump_intensity=0.0), dict(jump_std=0.0), dict(jump_mean=0.0), dict(jump_intensity=4.0, dt=0.25), dict(n_paths=0),
             dict(rho=1.0), dict(rho=-1.0), dict(v0=0.0), dict(jump_mean=1.0, jump_std=1.0), dict(jump_mean=-1.0, jump_std=1.0))
    for scheme in ("euler", "qe"):
        for change in edges:
            a = dict(ok, **change)
            M, V = eng.bates(**a, scheme=scheme, want_variance=True)
            if M.n_paths:
                s, v = M.to_host_step_major(), V.to_host_step_major()
                assert np.isfinite(s).all() and np.isfinite(v).all() and (s > 0.0).all(), (scheme, change)
            M.free()
            V.free()
    # sigma_v = 0 stays valid under the Euler scheme (PathEngine.merton is that case)
    eng.bates(**dict(ok, sigma_v=0.0), scheme="euler").free()


def test_launch_accounting(eng):
    eng.timing_enable(True)
    eng.timing_reset()
    a = gen(PARAMS["feller"], RARE_JUMPS, DT, 8, "qe")
    P = eng.bates(1, n_paths=10_000, **a)
    ms, launches = eng.timing_get(N.K_HESTON)
    assert launches == 1 and ms > 0.0 and eng.timing_get(N.K_GBM)[1] == 0 and eng.timing_get(N.K_PAYOFF)[1] == 0
    Q, V = eng.bates(1, n_paths=10_000, payoff=(100.0, True), want_variance=True, **dict(a, scheme="euler"))
    assert eng.timing_get(N.K_HESTON)[1] == 2 and eng.timing_get(N.K_GBM)[1] == 0
    M = eng.merton(1, S0, R, 0.2, 1.0, -0.1, 0.15, DT, 8, 10_000)
    assert eng.timing_get(N.K_HESTON)[1] == 3 and eng.timing_get(N.K_GBM)[1] == 0
    eng.timing_enable(False)
    for X in (P, Q, V, M):
        X.free()


def test_launch_frame(eng):
    """One launch under the Heston kernel id with the variance matrix stored, the fused sums and their reuse
    (test_gpu_parity.check_launch_frame)."""
    from test_gpu_parity import FRAME_PATHS, FRAME_STEPS, check_launch_frame
    check_launch_frame(eng, N.K_HESTON, lambda payoff: eng.bates(1, 100.0, R, dt=DT, n_steps=FRAME_STEPS, n_paths=FRAME_PATHS, payoff=payoff,
                                                                 want_variance=True, **PARAMS["feller"], **jumps(RARE_JUMPS)))
