"""The wide GBM generator (kernels_gbm.hip k_gbm_paths_wide: one 16-wave workgroup per CU, sin/cos from two 4096-entry LDS
tables, waves that draw 128-column tiles from a ticket counter), forced through mcg_debug_gbm_route at shapes a test can afford,
against the oracle's Philox restatement at the bar of the narrow kernel's tests (1e-11, every row, padded columns included), and
the properties that must not depend on which wave ran which tile.  Run with -m gpu on an MI355X.

Shapes: 1 000 paths (ld 1 024 = 8 tiles: fewer than one workgroup has waves); 6 221 paths (50 tiles: four workgroups, the last
with two waves at work); 1 573 164 paths (ld 1 573 376 = 12 292 tiles: more than three per wave of a 256-CU device, so every
wave goes back to the counter).  Reference: src/models/RoughVolatility.cpp:354-364 with v = sigma^2."""
import math

import mpmath as mp
import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd.engine import _DevView
from oracle.binding import Oracle

pytestmark = pytest.mark.gpu
mp.mp.dps = 50

SEED, DT = 20251031, 1.0 / 252.0
NARROW, WIDE = 1, 2
BIG_N, BIG_STEPS, K = 1_573_164, 5, 100.0
GBM = dict(S0=100.0, r=0.04, sigma=0.2)


@pytest.fixture(scope="module")
def eng():
    e = mc.PathEngine(0)
    e.debug_gbm_route(WIDE)
    yield e
    e.close()


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _gbm(eng, steps, n, path_begin=0, payoff=None, sigma=GBM["sigma"], dt=DT, seed=SEED):
    return eng.gbm(seed, GBM["S0"], GBM["r"], sigma, dt, steps, n, path_begin=path_begin, payoff=payoff)


def _device_matrix(P):
    """[n_steps + 1][ld] where it lies (a zero-copy torch view over mcg_paths_info's pointer)."""
    import torch
    t = torch.as_tensor(_DevView(P.device_ptr, (P.n_steps + 1) * P.ld), device=torch.device("cuda", 0))
    return t.view(P.n_steps + 1, P.ld)


def _columns(P, eng, begin, count):
    eng.synchronize()
    return _device_matrix(P)[:, begin:begin + count].cpu().numpy()


def _max_rel(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


@pytest.fixture(scope="module")
def big(eng):
    """The 1 573 164 x 5 payoff launch by the wide kernel, left on the device for the tests that compare with it."""
    P = _gbm(eng, BIG_STEPS, BIG_N, payoff=(K, True))
    assert eng.debug_gbm_route() == WIDE and P.ld == 1_573_376
    yield P
    P.free()


def test_sincos_two_level_on_the_device(eng):
    """mcg_debug_eval fn 10 (tables read from device memory) on the words of test_gpu_math.py::test_sincos_table and on the
    corners of both tables' index ranges: <= 3.5e-16 absolute against mpmath, and the point stays on the unit circle."""
    rs = np.random.RandomState(3)
    words = rs.randint(0, 2 ** 32, size=6000, dtype=np.uint64)
    edge = np.array([0, 2 ** 32 - 1, 1 << 29, (1 << 29) - 1, 3 << 29, (5 << 29) + 255, 7 << 29, 1 << 8, 255,
                     1 << 30, (1 << 30) - 1, 1 << 31, (1 << 31) - 1, 3 << 30, (3 << 30) - 1, 1 << 23, (1 << 23) - 1], dtype=np.uint64)
    corners = np.array([(i << 20) | (j << 8) | low for i in (0, 1023, 1024, 2047, 2048, 4095) for j in (0, 4095) for low in (0, 255)],
                       dtype=np.uint64)
    words = np.concatenate([words, edge, corners])
    y = eng.debug_eval(10, words.astype(np.float64))
    worst = 0.0
    for w, (c, s, _, _) in zip(words, y):
        ec, es = mp.cos_sin(2 * mp.pi * (mp.mpf(int(w) >> 8) + mp.mpf(1) / 2) / mp.mpf(2) ** 24)
        worst = max(worst, float(abs(mp.mpf(c) - ec)), float(abs(mp.mpf(s) - es)))
    print("sincos_two_level: worst absolute error", worst)
    assert worst <= 3.5e-16, worst
    assert np.max(np.abs(y[:, 0] ** 2 + y[:, 1] ** 2 - 1.0)) < 1e-15


def _check_all_columns(eng, orc, P, steps, n, path_begin, sigma, dt, tag):
    assert eng.debug_gbm_route() == WIDE, tag
    got = _columns(P, eng, 0, P.ld)
    want = orc.paths_gbm(SEED, GBM["S0"], GBM["r"], sigma, dt, steps, path_begin, P.ld)
    assert got.shape == want.shape == (steps + 1, P.ld)
    assert np.all(got[0] == GBM["S0"]), tag
    err = _max_rel(got, want)
    print(tag, "max rel", err)
    assert err < 1e-11, (tag, err)


def test_fewer_tiles_than_waves(eng, orc):
    P = _gbm(eng, 7, 1000)                      # 8 tiles; 7 = one Philox block + a remainder of 3
    assert P.ld == 1024
    _check_all_columns(eng, orc, P, 7, 1000, 0, GBM["sigma"], DT, "1000x7")
    P.free()


@pytest.mark.parametrize("steps", [1, 2, 4, 5, 6])
def test_step_remainders_far_into_the_stream(eng, orc, steps):
    begin = 2 ** 33 + 6
    P = _gbm(eng, steps, 6221, path_begin=begin)
    assert P.ld == 6400
    _check_all_columns(eng, orc, P, steps, 6221, begin, GBM["sigma"], DT, "6221x%d" % steps)
    P.free()


@pytest.mark.parametrize("mode,sigma,dt", [(3, 0.2, DT), (2, 0.015 * math.sqrt(252.0), DT), (1, 0.0, DT), (0, 1.0, 1.0 / 12.0)])
def test_the_four_modes(eng, orc, mode, sigma, dt):
    """launch_gbm's mode from (drift, vol): 3 and 2 the small-exponent steps with vol folded into the logarithm (bounds 0.1
    and 0.125), 1 the same without the fold (vol = 0), 0 the general exponential."""
    drift, vol = (GBM["r"] - 0.5 * sigma * sigma) * dt, sigma * math.sqrt(dt)
    reach = abs(drift) + vol * 7.55
    assert mode == (0 if reach > 0.125 else 1 if vol == 0.0 else 3 if reach <= 0.1 else 2)
    P = _gbm(eng, 6, 6221, sigma=sigma, dt=dt)
    _check_all_columns(eng, orc, P, 6, 6221, 0, sigma, dt, "mode %d" % mode)
    P.free()


def test_every_wave_loops_slices_match_oracle(eng, orc, big):
    n = BIG_N
    mid = ((n // 128) // 2) * 128 - 500
    for begin, count in ((0, 1024), (mid, 1024), (n - 513, 513 + (big.ld - n))):
        got = _columns(big, eng, begin, count)
        want = orc.paths_gbm(SEED, GBM["S0"], GBM["r"], GBM["sigma"], DT, BIG_STEPS, begin, count)
        assert got.shape == want.shape and np.all(got[0] == GBM["S0"])
        err = _max_rel(got, want)
        print("1573164x5 slice", begin, count, "max rel", err)
        assert err < 1e-11, (begin, count, err)


def test_payoff_and_plain_launches_write_the_same_bits(eng, big):
    import torch
    Q = _gbm(eng, BIG_STEPS, BIG_N)
    assert eng.debug_gbm_route() == WIDE
    eng.synchronize()
    assert torch.equal(_device_matrix(big), _device_matrix(Q))
    Q.free()


def test_repeated_launches_give_the_same_matrix_and_sums(eng, big):
    import torch
    T = BIG_STEPS * DT
    first = eng.price_european(big, K, GBM["r"], T, True)
    for _ in range(2):
        Q = _gbm(eng, BIG_STEPS, BIG_N, payoff=(K, True))
        eng.synchronize()
        assert torch.equal(_device_matrix(big), _device_matrix(Q))
        assert eng.price_european(Q, K, GBM["r"], T, True) == first     # the same sums, to the last bit
        Q.free()


def test_a_split_at_an_odd_column_reproduces_the_single_launch(eng, big):
    import torch
    cut = 786_431                                   # odd: every lane of the second launch carries another pair of paths
    A = _gbm(eng, BIG_STEPS, cut)
    B = _gbm(eng, BIG_STEPS, BIG_N - cut, path_begin=cut)
    assert eng.debug_gbm_route() == WIDE
    eng.synchronize()
    whole = _device_matrix(big)
    assert torch.equal(_device_matrix(A)[:, :cut], whole[:, :cut])
    assert torch.equal(_device_matrix(B)[:, :BIG_N - cut], whole[:, cut:BIG_N])
    A.free()
    B.free()


def test_fused_sums_agree_with_exactly_rounded_host_sums(eng, big):
    T = BIG_STEPS * DT
    gm, gse = eng.price_european(big, K, GBM["r"], T, True)
    eng.synchronize()
    last = _device_matrix(big)[BIG_STEPS, :BIG_N].cpu().numpy()
    pay = np.maximum(last - K, 0.0)
    m = math.fsum(pay) / BIG_N
    se = math.sqrt(max(0.0, (math.fsum(pay * pay) - BIG_N * m * m) / (BIG_N - 1)) / BIG_N)
    disc = math.exp(-GBM["r"] * T)
    assert abs(gm - disc * m) <= 1e-12 * disc * m, (gm, disc * m)
    assert abs(gse - disc * se) <= 1e-9 * disc * se, (gse, disc * se)


def test_wide_against_narrow(eng):
    W = _gbm(eng, 6, 6221)
    assert eng.debug_gbm_route(NARROW) == WIDE
    try:
        Nw = _gbm(eng, 6, 6221)
        assert eng.debug_gbm_route() == NARROW
    finally:
        eng.debug_gbm_route(WIDE)
    a, b = _columns(W, eng, 0, W.ld), _columns(Nw, eng, 0, Nw.ld)
    err = _max_rel(a, b)
    print("wide against narrow, 6221x6: max rel", err)
    assert err < 1e-11, err
    W.free()
    Nw.free()


def test_dispatch_by_size(eng):
    eng.debug_gbm_route(0)
    try:
        P = _gbm(eng, 252, 10_000_000)
        assert eng.debug_gbm_route() == WIDE
        P.free()
        Q = _gbm(eng, 252, 100_000)
        assert eng.debug_gbm_route() == NARROW
        Q.free()
    finally:
        eng.debug_gbm_route(WIDE)
