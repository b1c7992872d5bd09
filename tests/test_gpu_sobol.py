"""The Sobol' generators on the GPU (mcg_paths_gbm_sobol*, mcg_paths_localvol_sobol*; PathEngine.gbm_sobol, local_vol_sobol)
against the numpy restatement of tests/sobol_ref.py: Phi^-1 and the matrices element-wise (at every bit of the path id, every
edge of the launch's n_bits and every shape of bridge program), the bit-identities of the contract, the rejections, the
consumers, and the statistics of randomised quasi-Monte Carlo.

Bounds: ten times the worst relative difference measured on an MI355X (the project's rule for its generators); the measured
values stand beside them.  They come from rounding alone: numpy has no fused multiply-add and its log and exp are not the
device's, and a 1024-step path multiplies 1024 rounded exponentials.
"""
import ctypes as C
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
import sobol_ref as ref
from test_exotics_reference import price_numpy, stats_numpy
from test_localvol_reference import CEV, DT, NARROW, Q, R, S0, Surface, cev_half_closed_form, nodes
from test_sobol_reference import BRIDGE_PROGRAM_STEPS, BRIDGE_STEPS, normal_test_points

pytestmark = pytest.mark.gpu

SEED = 20261020
# on an MI355X: Phi^-1 9.99e-16 over normal_test_points(); gbm_sobol 1.55e-14 (513 x 1024 steps; 5.8e-15 at 252 steps, below 9e-16 up
# to 17); local_vol_sobol 4.88e-15 (the one-slice surface at 63 x 252; 1.3e-15 at 17 steps); the flat surface against gbm_sobol
# 7.55e-15 (sigma = 1.5 over 1024 steps; the same bits at sigma = 0.2 and 0)
# The cases at every index bit, n_bits edge and bridge length, on an MI355X: gbm_sobol 1.55e-14 again (601 x 1024 around
# 0xAAAAAAAA; every other window at 2^k 1.51e-14 or less, the 56 bridge lengths of three paths 1.27e-14, the n_bits edges 1.11e-15),
# except 6.79e-14 in the unscrambled first window (64 x 1024 from id 0, time order), where it is the restatement's: point 0 is
# x = 0 in every dimension, so path 0 takes the same step z = Phi^-1(2^-33) = -6.34 1024 times and numpy repeats one rounding
# error 1024 times; against the same product in 50 digits (mpmath) the restatement's last row of that path is off by 8.0e-14.
# local_vol_sobol at the two high windows 4.88e-15 (64 x 252 at 2^31) and 1.55e-15 (300 x 33 across 2^24).  No constant moved.
NORMAL_OBSERVED, GBM_OBSERVED, LV_OBSERVED, FLAT_OBSERVED = 9.99e-16, 1.55e-14, 4.88e-15, 7.55e-15
observed = {"normal": 0.0, "gbm": 0.0, "local vol": 0.0, "flat against gbm_sobol": 0.0}
SCRAMBLES = {0: "plain", 1: "shift", 2: "lms"}
END = "end"  # path_begin = 2^32 - n_paths: the last points of the sequence


def bound(seen):
    return 10.0 * seen


@pytest.fixture(scope="module")
def eng():
    with mc.PathEngine(0) as e:
        yield e


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest relative differences in this run: " + ", ".join(f"{k} {v:.2e}" for k, v in observed.items()))


def bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


def host(M):
    """The step-major matrix of M, which it frees."""
    out = M.to_host_step_major()
    M.free()
    return out


def begin_of(begin, n_paths):
    return 2 ** 32 - n_paths if begin == END else begin


def sobol_of(scramble, bridge, replicate=0, seed=SEED):
    return mc.Sobol(seed, replicate, SCRAMBLES[scramble], bridge)


# ---- Phi^-1 ---------------------------------------------------------------------------------------------------------------------
def test_normal_against_the_restatement(eng):
    x = normal_test_points()
    got = eng.debug_eval(16, x.astype(np.float64))[:, 0]
    want = ref.normal(x)
    e = float(np.abs(got / want - 1.0).max())
    observed["normal"] = e
    print(f"Phi^-1 against the restatement: {e:.2e} relative over {len(x)} points")
    assert np.isfinite(got).all() and (np.sign(got) == np.sign(want)).all()
    assert e <= bound(NORMAL_OBSERVED)


# ---- gbm_sobol element-wise -------------------------------------------------------------------------------------------------------
# (n_paths, n_steps, path_begin, scramble, bridge): every value of every axis occurs, the smallest together and the largest
# together; n_steps covers the tail steps, tree depths 0 to 10 and trees that are not powers of two
GBM_CASES = (
    (1, 1, 0, 0, False), (1, 1, END, 2, True), (2, 2, 1, 1, True), (63, 3, 777, 2, True), (511, 4, 0, 0, True),
    (513, 5, 1, 1, False), (1000, 7, 777, 2, False), (63, 8, END, 0, True), (511, 9, 777, 1, True), (513, 17, 0, 2, True),
    (1000, 252, 1, 2, True), (2, 1024, 0, 1, False), (513, 1024, 777, 0, True), (1000, 1024, END, 2, True),
)
GBM = dict(S0=100.0, r=0.05, sigma=0.2, dt=1.0 / 64.0)


def test_gbm_cases_cover_the_axes():
    for axis, values in ((0, (1, 2, 63, 511, 513, 1000)), (1, (1, 2, 3, 4, 5, 7, 8, 9, 17, 252, 1024)), (2, (0, 1, 777, END)),
                         (3, (0, 1, 2)), (4, (False, True))):
        assert {c[axis] for c in GBM_CASES} == set(values), axis


@pytest.mark.parametrize("case", GBM_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_gbm_sobol_against_the_restatement(eng, case):
    n_paths, n_steps, begin, scramble, bridge = case
    begin = begin_of(begin, n_paths)
    want = ref.gbm_sobol_numpy(SEED, 0, scramble, bridge, GBM["S0"], GBM["r"], GBM["sigma"], GBM["dt"], n_steps, n_paths, begin)
    P = eng.gbm_sobol(sobol_of(scramble, bridge), GBM["S0"], GBM["r"], GBM["sigma"], GBM["dt"], n_steps, n_paths, path_begin=begin)
    assert (P.n_paths, P.n_steps) == (n_paths, n_steps)
    got = host(P)
    e = float(np.abs(got / want - 1.0).max())
    observed["gbm"] = max(observed["gbm"], e)
    print(f"gbm_sobol {case}: {e:.2e}")
    assert (got[0] == GBM["S0"]).all()
    assert e <= bound(GBM_OBSERVED), (case, e)


# ---- gbm_sobol at every index bit, n_bits edge and bridge length -------------------------------------------------------------------
# The cases above sit in two corners of the sequence: Gray bits 0 .. 12 and bit 31.  These walk the rest of it, in the format
# of GBM_CASES.
# 64 paths either side of 2^k for k = 6 .. 31, and the first 64: the window at 2^k tells its ids apart by Gray bits 0 .. 4 and k
# (bit k - 1 is set in all of them), the first by bits 0 .. 5; 1024 steps, so every dimension is drawn; scramble and bridge
# alternate through their six combinations
INDEX_KS = (0,) + tuple(range(6, 32))
INDEX_WINDOWS = tuple((64, 1024, 2 ** k - 32 if k else 0, j % 3, j % 2 == 1) for j, k in enumerate(INDEX_KS))
# 601 paths around the id whose Gray code has every bit set, twice: from 0xAAAAAAAA - 300, which is even, and from the odd id
# before it, which puts the pair (0xAAAAAAA9, 0xAAAAAAAA) into one lane
EVERY_BIT_SET = 0xAAAAAAAA
EVERY_BIT_WINDOWS = ((601, 1024, EVERY_BIT_SET - 300, 2, True), (601, 1024, EVERY_BIT_SET - 301, 1, False))
# launch_sobol's n_bits: the last id of a launch decides how many groups of eight direction numbers sobol_pair reads
N_BITS_EDGES = (2 ** 8, 2 ** 16, 2 ** 24)
SMALL_LAUNCHES = ((0, 256), (0, 257), (0, 1), (2 ** 32 - 1, 1))    # (path_begin, n_paths): n_bits 8, 9, 0 and 32
BRIDGE_BEGIN = 2 ** 20 - 1
PAYOFF_COUNTS, PAYOFF_BEGIN = (1, 2, 255, 256, 257, 513), 2 ** 16 - 129


def edge_case(E, reach_E, bridge):
    """17 steps of the ids from the odd E - 301 (from 1 where that is negative) to E - 1, or to E: one lane holds the pair (E - 1, E)."""
    begin = max(E - 301, 1)
    return (E - begin + (1 if reach_E else 0), 17, begin, 2, bridge)


def bridge_case(n_steps):
    return (3, n_steps, BRIDGE_BEGIN, 2, True)


def assert_the_new_axes():
    """Every Gray bit 0 .. 31 set and clear, every n_bits class and edge, the listed bridge lengths."""
    assert [w[2] for w in INDEX_WINDOWS] == [0] + [2 ** k - 32 for k in range(6, 32)] and {w[:2] for w in INDEX_WINDOWS} == {(64, 1024)}
    for k, w in zip(INDEX_KS, INDEX_WINDOWS):
        assert ref.gray_bits(w[2], w[0]) == ({0, 1, 2, 3, 4, k} if k else {0, 1, 2, 3, 4, 5}), k
        assert ref.n_bits(w[2], w[0]) == (k + 1 if k else 6), k
    assert set().union(*(ref.gray_bits(w[2], w[0]) for w in INDEX_WINDOWS)) == set(range(32))
    for scramble in (0, 1, 2):
        assert sum(w[3] == scramble for w in INDEX_WINDOWS) >= 8, scramble
    for bridge in (False, True):
        assert sum(w[4] == bridge for w in INDEX_WINDOWS) >= 8, bridge
    assert {(w[3], w[4]) for w in INDEX_WINDOWS} == {(s, b) for s in (0, 1, 2) for b in (False, True)}
    # n_bits 1 .. 8, 9 .. 16, 17 .. 24 and 25 .. 32: one, two, three and four groups
    assert {(ref.n_bits(w[2], w[0]) + 7) // 8 for w in INDEX_WINDOWS} == {1, 2, 3, 4}
    for n_paths, n_steps, begin, scramble, bridge in EVERY_BIT_WINDOWS:
        codes = ref.gray_codes(begin, n_paths)
        assert 2 ** 32 - 1 in codes and ref.n_bits(begin, n_paths) == 32 and len(ref.gray_bits(begin, n_paths)) >= 10
    assert EVERY_BIT_WINDOWS[0][2] == EVERY_BIT_SET - 300 and EVERY_BIT_WINDOWS[1][2] % 2 == 1
    assert (EVERY_BIT_SET - 1 - EVERY_BIT_WINDOWS[1][2]) % 2 == 0      # (the lane that starts at ...A9 holds ...AA)
    for E in N_BITS_EDGES:
        k = E.bit_length() - 1
        for bridge in (False, True):
            below, reach = edge_case(E, False, bridge), edge_case(E, True, bridge)
            assert below[2] == reach[2] and below[2] % 2 == 1 and (E - 1 - below[2]) % 2 == 0 and below[1] == reach[1] == 17
            assert below[2] + below[0] - 1 == E - 1 and reach[2] + reach[0] - 1 == E
            assert (ref.n_bits(below[2], below[0]), ref.n_bits(reach[2], reach[0])) == (k, k + 1) and k % 8 == 0
    assert [ref.n_bits(b, n) for b, n in SMALL_LAUNCHES] == [8, 9, 0, 32]
    assert set(BRIDGE_PROGRAM_STEPS) == set(range(1, 41)) | {63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 511, 512, 513, 683, 1000, 1023}
    assert set(BRIDGE_PROGRAM_STEPS) <= set(BRIDGE_STEPS) and bridge_case(5) == (3, 5, 2 ** 20 - 1, 2, True)
    assert PAYOFF_COUNTS == (1, 2, 255, 256, 257, 513) and PAYOFF_BEGIN % 2 == 1
    assert ref.n_bits(PAYOFF_BEGIN, 129) == 16 and ref.n_bits(PAYOFF_BEGIN, 255) == 17
    assert {s[2:] for s in LV_SHAPES} >= {(2 ** 24 - 150, 2, True), (2 ** 31 - 32, 1, False)}


def test_new_cases_cover_their_axes():
    assert_the_new_axes()


def compare_gbm(eng, case):
    """The step-major matrix of a case, held to bound(GBM_OBSERVED) against the restatement; a miss names its worst element."""
    n_paths, n_steps, begin, scramble, bridge = case
    want = ref.gbm_sobol_numpy(SEED, 0, scramble, bridge, GBM["S0"], GBM["r"], GBM["sigma"], GBM["dt"], n_steps, n_paths, begin)
    got = host(eng.gbm_sobol(sobol_of(scramble, bridge), GBM["S0"], GBM["r"], GBM["sigma"], GBM["dt"], n_steps, n_paths, path_begin=begin))
    assert got.shape == want.shape == (n_steps + 1, n_paths)
    rel = np.abs(got / want - 1.0)
    t, j = np.unravel_index(int(np.argmax(rel)), rel.shape)
    e = float(rel[t, j])
    observed["gbm"] = max(observed["gbm"], e)
    print(f"gbm_sobol {case}: {e:.2e}")
    assert (got[0] == GBM["S0"]).all()
    code = ref.gray_codes(begin + int(j), 1)[0]
    assert e <= bound(GBM_OBSERVED), (f"{case}: {e:.2e} at row {t} of path id {begin + int(j)}, Gray code {code:#034b}, "
                                      f"{'bridge: every dimension up to the row' if bridge else f'dimension {t - 1}'}")
    return got


@pytest.mark.parametrize("case", INDEX_WINDOWS + EVERY_BIT_WINDOWS, ids=lambda c: "-".join(str(v) for v in c))
def test_gbm_sobol_at_every_index_bit(eng, case):
    compare_gbm(eng, case)


@pytest.mark.parametrize("bridge", [True, False])
@pytest.mark.parametrize("E", N_BITS_EDGES)
def test_n_bits_edges(eng, E, bridge):
    """A launch that ends at E - 1 reads one group of direction numbers fewer than one that ends at E: both are the
    restatement's, and the columns they share are the same bytes."""
    below, reach = compare_gbm(eng, edge_case(E, False, bridge)), compare_gbm(eng, edge_case(E, True, bridge))
    assert reach.shape[1] == below.shape[1] + 1 and bits(reach[:, :-1]) == bits(below), (E, bridge)


@pytest.mark.parametrize("bridge", [True, False])
def test_smallest_and_largest_n_bits(eng, bridge):
    mats = {(begin, n_paths): compare_gbm(eng, (n_paths, 17, begin, 2, bridge)) for begin, n_paths in SMALL_LAUNCHES}
    assert bits(mats[0, 257][:, :256]) == bits(mats[0, 256]) and bits(mats[0, 256][:, :1]) == bits(mats[0, 1])


@pytest.mark.parametrize("n_steps", BRIDGE_PROGRAM_STEPS)
def test_every_shape_of_bridge_program(eng, n_steps):
    compare_gbm(eng, bridge_case(n_steps))


# ---- local_vol_sobol element-wise -----------------------------------------------------------------------------------------------
# one slice of 64 nodes; 12 knots x 64 nodes (knots off the step grid, a skew that turns with time); a grid that a step
# leaves at once, so that most path-steps sit on either clamp
KNOTS_12 = Surface([0.4 * DT + 2.3 * DT * i for i in range(12)], -0.8, 0.8,
                   [[0.2 + 0.05 * math.sin(0.7 * i) - (0.15 - 0.02 * i) * x + 0.1 * x * x for x in nodes(-0.8, 0.8, 64)] for i in range(12)])
LV_SURFACES = {"cev": CEV, "knots-12": KNOTS_12, "narrow": NARROW}
# (n_paths, n_steps, path_begin, scramble, bridge)
# the last two at high indices: ids that straddle 2^24 (n_bits 24 and 25 in one workgroup's launch) and 2^31
LV_SHAPES = ((513, 9, 777, 2, True), (1000, 17, 1, 1, True), (63, 252, END, 2, False), (300, 33, 2 ** 24 - 150, 2, True),
             (64, 252, 2 ** 31 - 32, 1, False))


def test_local_vol_surfaces_are_what_they_are_meant_to_be():
    assert (CEV.n_t, CEV.n_x) == (1, 64) and (KNOTS_12.n_t, KNOTS_12.n_x) == (12, 64) and (KNOTS_12.sigma > 0.0).all()
    X = np.log(ref.localvol_sobol_numpy(SEED, 0, 2, True, S0, R, NARROW, DT, 17, 1000, q=Q)[1:] / S0)
    assert (X < NARROW.x_min).any() and (X > NARROW.x_max).any()


@pytest.mark.parametrize("name", sorted(LV_SURFACES))
def test_local_vol_sobol_against_the_restatement(eng, name):
    surface = LV_SURFACES[name]
    for n_paths, n_steps, begin, scramble, bridge in LV_SHAPES:
        begin = begin_of(begin, n_paths)
        want = ref.localvol_sobol_numpy(SEED, 3, scramble, bridge, S0, R, surface, DT, n_steps, n_paths, begin, q=Q)
        got = host(eng.local_vol_sobol(sobol_of(scramble, bridge, 3), S0, R, surface, DT, n_steps, n_paths, path_begin=begin, q=Q))
        e = float(np.abs(got / want - 1.0).max())
        observed["local vol"] = max(observed["local vol"], e)
        print(f"local_vol_sobol {name} {n_paths} x {n_steps}: {e:.2e}")
        assert (got[0] == S0).all()
        assert e <= bound(LV_OBSERVED), (name, n_paths, n_steps, e)


# ---- bit-identities -----------------------------------------------------------------------------------------------------------
def generators(eng):
    """(name, gen(sobol, n_paths, path_begin, payoff)) of 17 steps: GBM, one slice, and a surface with a time axis."""
    yield "gbm", lambda s, n, b, payoff=None: eng.gbm_sobol(s, 100.0, 0.05, 0.2, DT, 17, n, path_begin=b, payoff=payoff)
    for name in ("cev", "knots-12"):
        yield name, (lambda s, n, b, payoff=None, surface=LV_SURFACES[name]:
                     eng.local_vol_sobol(s, S0, R, surface, DT, 17, n, path_begin=b, q=Q, payoff=payoff))


@pytest.mark.parametrize("bridge", [True, False])
def test_bit_identities(eng, bridge):
    T = 17 * DT
    for name, gen in generators(eng):
        sobol = sobol_of(2, bridge, 1)
        for begin in (0, 4097):     # (an odd first column: no lane's pair of paths starts at an even point)
            whole = host(gen(sobol, 1000, begin))
            assert bits(host(gen(sobol, 1000, begin))) == bits(whole), (name, "two calls")
            cuts = (0, 1, 256, 511, 999, 1000)
            parts = [host(gen(sobol, hi - lo, begin + lo)) for lo, hi in zip(cuts[:-1], cuts[1:])]
            assert bits(np.concatenate(parts, axis=1)) == bits(whole), (name, begin, "shards")
        # the _payoff form: the same matrix, and sums that are price_european's on the plain one
        for K, is_call in ((100.0, True), (95.0, False)):
            plain = gen(sobol, 1000, 4097)
            want, want_se = eng.price_european(plain, K, R, T, is_call)
            fused = gen(sobol, 1000, 4097, (K, is_call))
            got, got_se = eng.price_european(fused, K, R, T, is_call)
            assert want > 0.0 and abs(got - want) <= 1e-12 * want and abs(got_se - want_se) <= 1e-9 * want_se, (name, K, got, want)
            assert bits(host(fused)) == bits(whole), (name, "payoff form")
            plain.free()
        # another replicate is another matrix
        assert bits(host(gen(sobol_of(2, bridge, 2), 1000, 4097))) != bits(whole)


@pytest.mark.parametrize("bridge", [True, False])
@pytest.mark.parametrize("E", (2 ** 16, 2 ** 24))
def test_shards_across_an_n_bits_edge(eng, E, bridge):
    """[E - 500, E) reads one group of direction numbers fewer than [E, E + 500) and than the whole: the same bytes all the same."""
    assert ref.n_bits(E - 500, 500) + 1 == ref.n_bits(E, 500) == ref.n_bits(E - 500, 1000) and ref.n_bits(E - 500, 500) % 8 == 0
    for name, gen in generators(eng):
        sobol = sobol_of(2, bridge, 1)
        whole = host(gen(sobol, 1000, E - 500))
        parts = [host(gen(sobol, 500, E - 500)), host(gen(sobol, 500, E))]
        assert bits(np.concatenate(parts, axis=1)) == bits(whole), (name, E, "shards")


@pytest.mark.parametrize("n_paths", PAYOFF_COUNTS)
def test_payoff_form_at_small_and_ragged_counts(eng, n_paths):
    """Up to 256 paths the workgroup's upper two waves lie beyond the padded row; 257 and 513 end a row one column into a wave."""
    T, disc = 17 * DT, math.exp(-R * 17 * DT)
    for name, gen in generators(eng):
        sobol = sobol_of(2, True, 1)
        for K, is_call in ((100.0, True), (100.0, False)):
            plain = gen(sobol, n_paths, PAYOFF_BEGIN)
            want, want_se = eng.price_european(plain, K, R, T, is_call)
            fused = gen(sobol, n_paths, PAYOFF_BEGIN, (K, is_call))
            got, got_se = eng.price_european(fused, K, R, T, is_call)
            X = host(plain)
            assert X.shape == (18, n_paths) and bits(host(fused)) == bits(X), (name, n_paths, "payoff form")
            assert abs(got - want) <= 1e-12 * want and abs(got_se - want_se) <= 1e-9 * want_se, (name, n_paths, K, is_call, got, want)
            pay = disc * (np.maximum(X[-1] - K, 0.0) if is_call else np.maximum(K - X[-1], 0.0))
            m, se = float(pay.mean()), float(pay.std(ddof=1)) / math.sqrt(n_paths) if n_paths > 1 else 0.0
            # the std error comes from sum and sum of squares: its bound scales as in test_path_counts of test_gpu_exotics.py
            tol_se = 1e-9 * se * (max(1.0, 0.5 + (m / se) ** 2 / n_paths) if se > 0.0 else 1.0)
            print(f"{name} {n_paths} paths, K {K}, call {is_call}: price {got!r} (numpy {m!r}), std error {got_se!r} (numpy {se!r})")
            assert abs(got - m) <= 1e-12 * m and abs(got_se - se) <= tol_se, (name, n_paths, K, is_call, got, m, got_se, se)
            if n_paths == 1:
                assert got_se == 0.0 and want_se == 0.0
        # a call or a put at the money pays on at least one path
        assert float(np.abs(X[-1] - 100.0).max()) > 0.0


# ---- the flat surface and the rejections ---------------------------------------------------------------------------------------
def test_flat_surface_against_gbm_sobol(eng):
    for n_paths, n_steps, begin, scramble, bridge in ((513, 9, 777, 2, True), (1000, 17, 1, 1, False), (63, 252, END, 2, True),
                                                      (511, 1024, 0, 2, True)):
        begin = begin_of(begin, n_paths)
        for sigma in (0.2, 0.0, 1.5):
            s = sobol_of(scramble, bridge)
            L = host(eng.local_vol_sobol(s, S0, R, Surface.flat(sigma), DT, n_steps, n_paths, path_begin=begin))
            G = host(eng.gbm_sobol(s, S0, R, sigma, DT, n_steps, n_paths, path_begin=begin))
            e = float(np.abs(L / G - 1.0).max())
            observed["flat against gbm_sobol"] = max(observed["flat against gbm_sobol"], e)
            print(f"flat surface {n_paths} x {n_steps}, sigma {sigma}: {e:.2e}")
            assert e <= bound(FLAT_OBSERVED), (n_paths, n_steps, sigma, e)


def test_rejections_leave_the_handle_alone(eng):
    L = eng._L
    dp = C.POINTER(C.c_double)
    times, sigma = np.array([0.0]), np.array([0.2, 0.2])
    good = dict(scramble=2, bridge=1, n_steps=8, begin=0, n_paths=16)
    for change in (dict(n_steps=1025), dict(begin=2 ** 32 - 15, n_paths=16), dict(begin=1, n_paths=2 ** 32), dict(scramble=3),
                   dict(n_steps=0), dict(bridge=2), dict(scramble=-1)):
        a = dict(good, **change)
        spec = N.SobolSpec(SEED, 0, a["scramble"], a["bridge"])
        for payoff in (False, True):
            tail = (100.0, 1) if payoff else ()
            h = C.c_void_p()
            fn = L.mcg_paths_gbm_sobol_payoff if payoff else L.mcg_paths_gbm_sobol
            rc = fn(eng._ctx, C.byref(spec), 100.0, 0.05, 0.2, DT, a["n_steps"], a["begin"], a["n_paths"], *tail, C.byref(h))
            assert rc == 1 and h.value is None and L.mcg_last_error(), (change, "gbm", rc)
            h = C.c_void_p()
            fn = L.mcg_paths_localvol_sobol_payoff if payoff else L.mcg_paths_localvol_sobol
            rc = fn(eng._ctx, C.byref(spec), 100.0, 0.05, 0.0, times.ctypes.data_as(dp), 1, -1.0, 1.0, 2, sigma.ctypes.data_as(dp), DT,
                    a["n_steps"], a["begin"], a["n_paths"], *tail, C.byref(h))
            assert rc == 1 and h.value is None and L.mcg_last_error(), (change, "local vol", rc)
        with pytest.raises(mc.McgError) as err:
            eng.gbm_sobol(mc.Sobol(SEED, 0, a["scramble"], bool(a["bridge"]) if a["bridge"] < 2 else 2), 100.0, 0.05, 0.2, DT,
                          a["n_steps"], a["n_paths"], path_begin=a["begin"])
        assert err.value.status == 1
    # the last points of the sequence and an empty matrix are valid
    E = eng.gbm_sobol(sobol_of(2, True), 100.0, 0.05, 0.2, DT, 8, 0, path_begin=2 ** 32)
    assert (E.n_paths, E.n_steps) == (0, 8) and E.to_host_step_major().shape == (9, 0)
    E.free()


# ---- consumers ------------------------------------------------------------------------------------------------------------------
def test_consumers_and_launch_accounting(eng):
    n_steps, n_paths, r, T = 17, 5003, 0.05, 17 * DT
    eng.timing_enable(True)
    eng.timing_reset()
    P = eng.gbm_sobol(sobol_of(2, True), 100.0, r, 0.3, DT, n_steps, n_paths, path_begin=777)
    ms, launches = eng.timing_get(N.K_SOBOL)
    assert launches == 1 and ms > 0.0 and eng.timing_get(N.K_GBM)[1] == 0 and eng.timing_get(N.K_LOCALVOL)[1] == 0
    eng.local_vol_sobol(sobol_of(2, True), S0, R, CEV, DT, n_steps, n_paths, payoff=(100.0, False)).free()
    assert eng.timing_get(N.K_SOBOL)[1] == 2 and eng.timing_get(N.K_LOCALVOL)[1] == 0 and eng.timing_get(N.K_GBM)[1] == 0
    eng.timing_enable(False)
    X = P.to_host()
    for K, is_call in ((100.0, True), (102.0, False)):
        m, se = eng.price_european(P, K, r, T, is_call)
        x = math.exp(-r * T) * (np.maximum(X[:, -1] - K, 0.0) if is_call else np.maximum(K - X[:, -1], 0.0))
        assert abs(m - x.mean()) <= 1e-12 * x.mean() and abs(se - x.std(ddof=1) / math.sqrt(n_paths)) <= 1e-9 * se, (K, is_call)
    st5 = stats_numpy(X, 1)
    got = eng.path_stats(P)
    for q in (0, 3, 4):
        assert np.array_equal(got[q], st5[q]), q
    assert np.abs(got[1] / st5[1] - 1.0).max() <= 1e-14 and np.abs(got[2] / st5[2] - 1.0).max() <= 2e-14
    book = [mc.exotic("asian_arith_fixed", True, 100.0), mc.exotic("asian_arith_fixed", False, 101.0)]
    price, se = eng.price_exotics(P, r, T, book)
    for i, c in enumerate(book):
        want, want_se = price_numpy(st5, c, r, T)
        assert abs(price[i] - want) <= 1e-12 * want and abs(se[i] - want_se) <= 1e-12 * want_se, (c, price[i], want)
    P.free()


# ---- statistics -----------------------------------------------------------------------------------------------------------------
def test_rqmc_statistics_of_the_gbm_case(eng):
    """The README's case by 16 replicates of the matrix scramble + shift + bridge.  tests/test_sobol_reference.py passes the
    same checks on the restatement, whose matrices these equal element-wise: the GPU run cannot decide differently."""
    c = ref.RQMC
    n, N_, T, r, K = c["n_steps"], c["n_paths"], c["T"], c["r"], c["K"]
    asian = [mc.exotic("asian_arith_fixed", True, K)]
    prices = []
    for k in range(c["replicates"]):
        P = eng.gbm_sobol(mc.Sobol(c["seed"], k, "lms", True), c["S0"], r, c["sigma"], T / n, n, N_)
        prices.append((eng.price_european(P, K, r, T, True)[0], eng.price_exotics(P, r, T, asian)[0][0]))
        P.free()
    prices = np.array(prices)
    mean, se = mc.rqmc_combine(prices[:, 0])
    bs = ref.black_scholes_call(c["S0"], K, r, c["sigma"], T)
    print(f"European call {mean:.5f} +- {se:.5f} by rqmc_combine (Black-Scholes {bs:.5f})")
    assert abs(mean - bs) <= 4.0 * se
    # the iid standard errors of the Philox generator at the same N
    G = eng.gbm(c["seed"], c["S0"], r, c["sigma"], T / n, n, N_)
    iid = eng.price_european(G, K, r, T, True)[1], eng.price_exotics(G, r, T, asian)[1][0]
    G.free()
    sd = prices.std(axis=0, ddof=1)
    for i, name in enumerate(("european", "asian")):
        ratio = (iid[i] / sd[i]) ** 2
        restated = (ref.IID_STD_ERR[name] / ref.RQMC_LMS_BRIDGE_STD[name]) ** 2
        print(f"{name}: std dev across replicates {sd[i]:.3g}, iid std error {iid[i]:.3g}, variance ratio {ratio:.3g} (restatement {restated:.3g})")
        assert ratio >= 0.25 * restated, (name, ratio, restated)


def test_rqmc_statistics_of_the_cev_case(eng):
    """ref.CEV_STAT (which says why this horizon and this grid): the CEV call within 4 replicate standard errors of the closed form."""
    c = ref.CEV_STAT
    surface = Surface.cev(c["sigma0"], c["beta"], -c["x_max"], c["x_max"], c["n_x"])
    n, T = c["n_steps"], c["T"]
    prices = []
    for k in range(c["replicates"]):
        P = eng.local_vol_sobol(mc.Sobol(c["seed"], k, "lms", True), c["S0"], c["r"], surface, T / n, n, c["n_paths"], q=c["q"])
        prices.append(eng.price_european(P, c["K"], c["r"], T, True)[0])
        P.free()
    mean, se = mc.rqmc_combine(prices)
    want = cev_half_closed_form(c["S0"], c["K"], c["r"], c["q"], T, c["sigma0"], True)
    print(f"CEV call {mean:.6f} +- {se:.6f} by rqmc_combine (closed form {want:.6f}: {(mean - want) / se:+.2f} standard errors)")
    assert abs(mean - want) <= 4.0 * se


def test_launch_frame(eng):
    """GBM through the bridge: one launch under the generator's kernel id, the fused sums and their reuse
    (test_gpu_parity.check_launch_frame)."""
    from test_gpu_parity import FRAME_PATHS, FRAME_STEPS, check_launch_frame
    check_launch_frame(eng, N.K_SOBOL,
                       lambda payoff: eng.gbm_sobol(mc.Sobol(5, 0, "lms", True), 100.0, R, 0.2, DT, FRAME_STEPS, FRAME_PATHS, payoff=payoff))
