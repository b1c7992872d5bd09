"""CPU side of the Sobol' generators (mcg_sobol_table, mcg_sobol_bridge, mcg_rqmc_combine; PathEngine.gbm_sobol and
local_vol_sobol): the library's host functions against the numpy restatement (tests/sobol_ref.py) and against scipy, the
identities of the restatement that tests/test_gpu_sobol.py relies on, the host code under the sanitizers, and what randomised
quasi-Monte Carlo buys on the README's case.  No GPU.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
import sobol_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261020


# ---- the point set ---------------------------------------------------------------------------------------------------------------
def test_plain_table_is_scipys_unscrambled_sequence():
    """1024 points in all 1024 dimensions, exactly: scipy's Sobol(d, scramble=False, bits=32) point i times 2^32."""
    from scipy.stats import qmc
    V, shift = mc.sobol_table(mc.Sobol(SEED, 0, "plain"), N.SOBOL_MAX_DIMS)
    assert V.shape == (1024, 32) and V.dtype == np.uint32 and not shift.any()
    assert (V == ref.direction_numbers(1024)).all()
    want = qmc.Sobol(1024, scramble=False, bits=32).random(1024) * 2.0 ** 32
    assert (want == np.floor(want)).all()
    assert (ref.points(V, shift, 0, 1024).T == want.astype(np.uint64)).all()
    # a later stretch of the sequence, through path_begin
    eng = qmc.Sobol(64, scramble=False, bits=32)
    eng.fast_forward(777)
    assert (ref.points(V[:64], shift[:64], 777, 300).T == (eng.random(300) * 2.0 ** 32).astype(np.uint64)).all()


def test_plain_table_is_scipys_in_all_32_columns():
    """Points 0 .. 1076 above use Gray bits 0 .. 10 only; this is every direction number, and points near 2^14, 2^20 and 2^26."""
    from scipy.stats import qmc
    V, shift = mc.sobol_table(mc.Sobol(SEED, 0, "plain"), N.SOBOL_MAX_DIMS)
    # scipy's own matrix where it shows it (a private attribute: without it the public check below stands alone)
    sv = getattr(qmc.Sobol(N.SOBOL_MAX_DIMS, scramble=False, bits=32), "_sv", None)
    if sv is not None:
        assert sv.shape == (1024, 32) and sv.dtype == np.uint32
        assert (V == sv).all() and (ref.direction_numbers(1024) == sv).all()
    # the public interface: 64 points either side of 2^k in the first four dimensions (forwarding costs time per dimension)
    for k in (14, 20, 26):
        eng = qmc.Sobol(4, scramble=False, bits=32)
        eng.fast_forward(2 ** k - 32)
        want = eng.random(64) * 2.0 ** 32
        assert (want == np.floor(want)).all()
        assert k in ref.gray_bits(2 ** k - 32, 64)
        assert (ref.points(V[:4], shift[:4], 2 ** k - 32, 64).T == want.astype(np.uint64)).all(), k


def test_gray_bits_and_n_bits():
    """The helpers that the coverage assertions stand on, against the ids written out."""
    assert ref.gray_codes(0, 4) == [0, 1, 3, 2] and ref.gray_codes(0xAAAAAAAA, 1) == [0xFFFFFFFF]
    assert ref.gray_bits(0, 1) == set() and ref.gray_bits(0, 2) == {0} and ref.gray_bits(1, 2) == {1} and ref.gray_bits(0, 1000) == set(range(10))
    assert ref.gray_bits(777, 1000) == set(range(11)) and ref.gray_bits(4097, 1000) == set(range(10))     # (bits 11 and 12 are set in all)
    assert ref.gray_bits(2 ** 32 - 1000, 1000) == set(range(10))                                                   # (and so is bit 31)
    assert ref.gray_bits(2 ** 20 - 32, 64) == {0, 1, 2, 3, 4, 20} and ref.gray_bits(2 ** 31, 2) == {0}
    for begin, n in ((0, 1000), (777, 1000), (2 ** 20 - 32, 64), (2 ** 32 - 5, 5)):
        i = np.arange(begin, begin + n, dtype=np.uint64)
        on = (((i ^ (i >> np.uint64(1)))[:, None] >> np.arange(32, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
        assert ref.gray_bits(begin, n) == {b for b in range(32) if on[:, b].any() and not on[:, b].all()}, (begin, n)
    assert [ref.n_bits(b, n) for b, n in ((0, 1), (1, 1), (0, 256), (0, 257), (2 ** 16 - 3, 3), (2 ** 16 - 3, 4), (2 ** 31 - 1, 1),
                                          (2 ** 31, 1), (2 ** 32 - 1, 1))] == [0, 1, 8, 9, 16, 17, 31, 32, 32]


def test_gpu_cases_cover_every_gray_bit_and_n_bits_class():
    """What tests/test_gpu_sobol.py asserts of its own cases before it runs them, here without a GPU."""
    import test_gpu_sobol as G
    G.assert_the_new_axes()


def moved_by(case, d, b):
    """The largest relative move of the restatement's matrix of a case of tests/test_gpu_sobol.py (n_paths, n_steps, path_begin,
    scramble, bridge) when the lowest bit of V'[d][b], as the device would receive it, is flipped."""
    import test_gpu_sobol as G
    n_paths, n_steps, begin, scramble, bridge = case
    gbm = lambda: ref.gbm_sobol_numpy(G.SEED, 0, scramble, bridge, G.GBM["S0"], G.GBM["r"], G.GBM["sigma"], G.GBM["dt"], n_steps, n_paths, begin)  # noqa: E731
    right, table = gbm(), ref.table

    def wrong_table(*args):
        V, shift = table(*args)
        V = V.copy()
        V[d, b] ^= np.uint32(1)
        return V, shift
    ref.table = wrong_table
    try:
        wrong = gbm()
    finally:
        ref.table = table
    return float(np.abs(wrong / right - 1.0).max())


def test_a_wrong_direction_number_moves_the_new_cases():
    """The new GPU cases can fail: one wrong last bit in one direction number of a bit that tells a window's ids apart moves the
    matrix by at least 100 times the bound the device is held to, and a bit that no id of the window has set moves nothing.

    A last bit is the smallest possible error, 2^-32 in u, so at least 2^-32 sqrt(2 pi) = 5.8e-10 in z (more away from z = 0) and
    sigma sqrt(dt) sd times that in ln S, where sd >= sqrt(1/2) is the weight of the node that takes the dimension (1 in time
    order): at least 1.03e-11, 66 bounds, and that only where the one path that has the bit set draws z = 0 at a leaf.  In an
    index window 32 ids or more have the bit set, and the largest move among them is asserted to be 100 bounds, as measured:
    the smallest is 1.9e-11 = 125 bounds (the window at 2^12, dimension 1023, bit 0).  In the n_bits edges and the three-path
    bridge cases one or two ids have it (bit k of an edge is the id E's alone): those are held to the floor above, which the
    edge at 2^8 meets in dimension 8 (1.03e-11 = 67 bounds)."""
    import test_gpu_sobol as G
    limit = G.bound(G.GBM_OBSERVED)
    one_path_floor = 0.99 * 2.0 ** -32 * math.sqrt(2.0 * math.pi) * G.GBM["sigma"] * math.sqrt(G.GBM["dt"]) * math.sqrt(0.5)
    assert 100.0 * limit > one_path_floor >= 60.0 * limit
    sample = [w for w in G.INDEX_WINDOWS if w[2] in tuple(2 ** k - 32 for k in (6, 7, 12, 13, 20, 21, 28, 29, 31))]
    # at least one window per group of eight bits, with and without the bridge: all of them held to 100 bounds
    groups = {((ref.n_bits(c[2], c[0]) + 7) // 8, c[4]) for c in sample}
    assert groups == {(k, bridge) for k in (1, 2, 3, 4) for bridge in (True, False)}
    sample += [G.edge_case(E, True, bridge) for E in G.N_BITS_EDGES for bridge in (True, False)]
    sample += [G.bridge_case(n) for n in (1, 2, 37, 683)]
    smallest = math.inf
    for case in sample:
        n_paths, n_steps, begin = case[:3]
        varying = ref.gray_bits(begin, n_paths)
        codes = ref.gray_codes(begin, n_paths)
        unused = [b for b in range(32) if not any((g >> b) & 1 for g in codes)]
        assert varying and not varying & set(unused), case
        for d in sorted({0, min(1, n_steps - 1), n_steps // 2, n_steps - 1}):
            for b in (min(varying), max(varying)):
                several = case in G.INDEX_WINDOWS
                assert not several or sum((g >> b) & 1 for g in codes) >= 32
                e = moved_by(case, d, b)
                smallest = min(smallest, e)
                print(f"{case}: V[{d}][{b}] moves the matrix by {e:.2e} = {e / limit:.0f} bounds")
                assert e >= (100.0 * limit if several else one_path_floor), (case, d, b, e)
            for b in unused[:1] + unused[-1:]:
                assert moved_by(case, d, b) == 0.0, (case, d, b)
    print(f"smallest move {smallest:.2e} against the bound {limit:.2e}")


@pytest.mark.parametrize("scramble", ["shift", "lms"])
def test_scrambled_tables_equal_the_restatement(scramble):
    code = N.SOBOL_SCRAMBLES[scramble]
    for seed, replicate, n_dims in ((SEED, 0, 1024), (0, 0, 1), (2 ** 64 - 1, 2 ** 32 - 1, 65), (SEED, 7, 252)):
        V, shift = mc.sobol_table(mc.Sobol(seed, replicate, scramble), n_dims)
        Vr, sr = ref.table(seed, replicate, code, n_dims)
        assert (V == Vr).all() and (shift == sr).all(), (seed, replicate, n_dims)
    # both scrambles of a (seed, replicate) share their shifts, and a shift leaves the direction numbers alone
    Vs, ss = mc.sobol_table(mc.Sobol(SEED, 7, "shift"), 252)
    Vl, sl = mc.sobol_table(mc.Sobol(SEED, 7, "lms"), 252)
    assert (ss == sl).all() and (Vs == ref.direction_numbers(252)).all() and (Vl != Vs).any()


def test_the_matrix_scramble_keeps_the_net():
    """The first 2^k points of every dimension fall one per interval of width 2^-k."""
    V, shift = mc.sobol_table(mc.Sobol(SEED, 1, "lms"), N.SOBOL_MAX_DIMS)
    for k in (4, 10, 14):
        x = ref.points(V, shift, 0, 1 << k)
        cells = np.sort(x >> np.uint32(32 - k), axis=1)
        assert (cells == np.arange(1 << k, dtype=np.uint32)[None, :]).all(), k


def test_seed_and_replicate_select_the_table():
    base = mc.sobol_table(mc.Sobol(SEED, 0, "lms"), 32)
    again = mc.sobol_table(mc.Sobol(SEED, 0, "lms"), 32)
    assert (base[0] == again[0]).all() and (base[1] == again[1]).all()
    for seed, replicate in ((SEED, 1), (SEED + 1, 0), (SEED, 2 ** 32 - 1), (SEED ^ (1 << 63), 0)):
        other = mc.sobol_table(mc.Sobol(seed, replicate, "lms"), 32)
        assert (other[0] != base[0]).any() and (other[1] != base[1]).all(), (seed, replicate)
        assert (mc.sobol_table(mc.Sobol(seed, replicate, "shift"), 32)[1] == other[1]).all()


# ---- the bridge -------------------------------------------------------------------------------------------------------------------
# The lengths whose bridge program tests/test_gpu_sobol.py walks on the device with three paths: every n to 40 (all shapes of
# the first five tree levels), powers of two and their neighbours (a full tree, one node short, one node over), and lengths
# in between; schedule, orthogonality and program are judged at the same n.
BRIDGE_PROGRAM_STEPS = tuple(range(1, 41)) + (63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 511, 512, 513, 683, 1000, 1023)
BRIDGE_STEPS = tuple(sorted(set((1, 2, 3, 4, 5, 7, 8, 9, 13, 17, 252, 1024) + BRIDGE_PROGRAM_STEPS)))
# max |QQ^T - I| (element-wise) of the restatement over BRIDGE_STEPS: 4.4e-16, at 252 and 1024 steps
ORTHOGONALITY_OBSERVED = 4.4e-16


@pytest.mark.parametrize("n", BRIDGE_STEPS)
def test_bridge_schedule(n):
    got = mc.sobol_bridge(n, True)
    assert [tuple(e) for e in got.tolist()] == ref.bridge_schedule(n, True)       # exactly, weights included
    assert sorted(got["t"].tolist()) == list(range(1, n + 1))                    # every t once
    assert got[0]["t"] == n and got[0]["sd"] == math.sqrt(n)
    ident = mc.sobol_bridge(n, False)
    assert [tuple(e) for e in ident.tolist()] == ref.bridge_schedule(n, False) == [(d + 1, d, d, 1.0, 0.0, 1.0) for d in range(n)]
    # the map from the normals to the increments is orthogonal: the law of the paths is that of the Philox generators
    Q = ref.bridge_matrix(n)
    e = float(np.abs(Q @ Q.T - np.eye(n)).max())
    print(f"n = {n}: max |QQ^T - I| = {e:.2e}")
    assert e <= 10.0 * ORTHOGONALITY_OBSERVED
    assert (ref.bridge_matrix(n, False) == np.eye(n)).all()


# ---- the normal -------------------------------------------------------------------------------------------------------------------
def normal_test_points():
    """The 2^16 smallest and largest x, both sides of the branch point |u - 1/2| = 0.425, and 10^6 random x."""
    edge = int(math.floor((0.5 + ref.SPLIT) * 2.0 ** 32))
    near = np.arange(-2048, 2048, dtype=np.int64)
    rng = np.random.default_rng(SEED)
    x = np.concatenate([np.arange(1 << 16), 2 ** 32 - 1 - np.arange(1 << 16), edge + near, 2 ** 32 - 1 - edge + near,
                        np.array([2 ** 31 - 1, 2 ** 31]), rng.integers(0, 2 ** 32, 10 ** 6)])
    return x.astype(np.uint32)


# worst relative difference between the restatement and scipy.special.ndtri over normal_test_points(): 1.11e-15
NDTRI_OBSERVED = 1.11e-15


def test_normal_against_scipy():
    """The only place where AS241 is judged against an outside authority."""
    from scipy.special import ndtri
    x = normal_test_points()
    u = (x.astype(np.float64) + 0.5) * 2.0 ** -32
    assert u.min() == 2.0 ** -33 and u.max() == 1.0 - 2.0 ** -33
    z, want = ref.normal(x), ndtri(u)
    e = float(np.abs(z / want - 1.0).max())
    print(f"restatement against ndtri: {e:.2e} relative")
    assert e <= 10.0 * NDTRI_OBSERVED
    # both branches were taken, the tail stays below r = 5, and the map is odd and increasing
    q = np.abs(u - 0.5)
    assert (q <= ref.SPLIT).any() and (q > ref.SPLIT).any() and math.sqrt(-math.log(2.0 ** -33)) < 5.0
    assert (ref.normal(~x) == -z).all()
    order = np.argsort(x, kind="stable")
    assert (np.diff(z[order]) >= 0.0).all()


# ---- the host code under the sanitizers -----------------------------------------------------------------------------------------
def test_host_sobol_code_under_the_sanitizers(tmp_path):
    """tests/cpp/sobol_host_main.cpp with host/sobol.cpp, compiled with -fsanitize=address,undefined into a stand-alone program
    (the sanitizers' runtimes linked into it) and run directly: every n_dims and n_steps from 1 to 1024, all scrambles, the
    invalid arguments and mcg_rqmc_combine; it must exit 0 with nothing reported."""
    exe = tmp_path / "sobol_host_main"
    host = os.path.join(ROOT, "montecarlooptionspricer_amd", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sobol_host_main.cpp"),
           os.path.join(host, "sobol.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-3000:]


# ---- the Python layer without a GPU -----------------------------------------------------------------------------------------------
def test_python_mirrors_and_rejections():
    assert N.K_SOBOL == 16 and len(N.KERNEL_NAMES) == 14
    s = mc.Sobol(5)
    assert (s.seed, s.replicate, s.scramble, s.bridge) == (5, 0, N.SOBOL_LMS_SHIFT, True)
    assert mc.Sobol(5, 2, "PLAIN", False)._spec().scramble == N.SOBOL_PLAIN and mc.Sobol(5, 2, 1)._spec().replicate == 2
    for bad in (lambda: mc.Sobol(5, scramble="owen"), lambda: mc.Sobol(-1)._spec(), lambda: mc.Sobol(1, 2 ** 32)._spec(),
                lambda: mc.sobol_table(mc.Sobol(1, 0, 3), 4), lambda: mc.sobol_table(mc.Sobol(1), 0),
                lambda: mc.sobol_table(mc.Sobol(1), 1025), lambda: mc.sobol_bridge(0), lambda: mc.sobol_bridge(1025),
                lambda: mc.rqmc_combine([1.0])):
        with pytest.raises(mc.McgError) as e:
            bad()
        assert e.value.status == 1
    est = [10.4, 10.5, 10.45, 10.47]
    mean, se = mc.rqmc_combine(est)
    assert abs(mean - np.mean(est)) <= 1e-15 * mean and abs(se - np.std(est, ddof=1) / 2.0) <= 1e-15 * se
    # the generators check their point set before they look at the ctx: MCG_ERR_INVALID without a GPU, the handle untouched
    import ctypes as C
    L = mc.load_library()
    for spec, n_steps, begin, n_paths in ((N.SobolSpec(1, 0, 3, 1), 8, 0, 16), (N.SobolSpec(1, 0, 2, 2), 8, 0, 16),
                                          (N.SobolSpec(1, 0, 2, 1), 1025, 0, 16), (N.SobolSpec(1, 0, 2, 1), 8, 2 ** 32 - 15, 16)):
        h = C.c_void_p(12345)
        rc = L.mcg_paths_gbm_sobol(None, C.byref(spec), 100.0, 0.05, 0.2, 0.01, n_steps, begin, n_paths, C.byref(h))
        assert rc == 1 and b"sobol" in L.mcg_last_error() and h.value == 12345, (spec.scramble, n_steps, begin)
    h = C.c_void_p(12345)
    assert L.mcg_paths_gbm_sobol(None, None, 100.0, 0.05, 0.2, 0.01, 8, 0, 16, C.byref(h)) == 1 and h.value == 12345


# ---- what it buys -----------------------------------------------------------------------------------------------------------------
# Standard deviation across the 16 replicates of the README's case (GBM, S0 = K = 100, r = 0.05, sigma = 0.2, T = 1, 64 steps,
# 2^14 points; seed 20261020), European call / arithmetic Asian call, and the variance ratio against the iid standard errors
# 0.115 / 0.0621 of a sample of the same size, as this test prints them:
#   shift, dimensions in time order        0.0133   / 0.00958    ratio     75 /    42
#   shift + bridge                         0.00224  / 0.00169    ratio  2 600 / 1 350
#   matrix scramble + shift + bridge       0.000464 / 0.00104    ratio 61 500 / 3 540
RQMC_SETTINGS = (("shift, time order", ref.SHIFT, False), ("shift + bridge", ref.SHIFT, True), ("lms + shift + bridge", ref.LMS_SHIFT, True))


def rqmc_table(cache={}):
    if not cache:
        for name, scramble, bridge in RQMC_SETTINGS:
            cache[name] = np.array([ref.rqmc_prices(scramble, bridge, k) for k in range(ref.RQMC["replicates"])])
    return cache


def test_rqmc_effect_on_the_restatement():
    c = ref.RQMC
    bs = ref.black_scholes_call(c["S0"], c["K"], c["r"], c["sigma"], c["T"])
    sd = {}
    for name, prices in rqmc_table().items():
        sd[name] = prices.std(axis=0, ddof=1)
        ratio = (ref.IID_STD_ERR["european"] / sd[name][0]) ** 2, (ref.IID_STD_ERR["asian"] / sd[name][1]) ** 2
        mean, se = mc.rqmc_combine(prices[:, 0])
        print(f"{name}: std dev across replicates {sd[name][0]:.3g} / {sd[name][1]:.3g}, variance ratio {ratio[0]:.3g} / {ratio[1]:.3g}, "
              f"European call {mean:.5f} +- {se:.5f} (Black-Scholes {bs:.5f})")
        assert abs(mean - bs) <= 4.0 * se, name
    # only the ordering is asserted: the bridge beats time order for the Asian call
    assert sd["shift + bridge"][1] < sd["shift, time order"][1]
    # ... and that the figures tests/test_gpu_sobol.py builds its variance ratios from are still this restatement's
    for i, name in enumerate(("european", "asian")):
        assert abs(sd["lms + shift + bridge"][i] / ref.RQMC_LMS_BRIDGE_STD[name] - 1.0) <= 0.01, name
