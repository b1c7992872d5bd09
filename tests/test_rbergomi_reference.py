"""High-precision reference of the rBergomi generator (mcg_paths_rbergomi) -- the yardstick of tests/test_gpu_rbergomi.py.

One path pair, as k_rb_generic_spectrum / k_rb_generic_x / k_rb_generic_step (csrc/kernels_rbergomi.hip) state it and under the
RNG contract of csrc/philox.hpp, with amp[Mz] and comp[n_steps] of mcg_rbergomi_spectrum taken as exact binary64 inputs (they are
the device's inputs too; the spectrum has its own tests):
    Y_{2b} = amp[2b] (z0 + i z1),  Y_{2b+1} = amp[2b+1] (z2 + i z3)      z: block b of stream 1 of the PAIR id path_id >> 1
    x_n = sum_k Y_k e^{2 pi i k n / Mz}     summed directly, the angle reduced exactly by k n mod Mz;  X(even path) = Re, X(odd) = Im
    e = exp((X_n + comp_n) / 2)
    inc = sqrt(xi dt) e z_n - xi dt e^2 / 2 + r dt                       z_n: stream 0 of the path id, block n >> 2, element n & 3
    S_{n+1} = S_n exp(inc)
Everything after the 32-bit Philox words -- the radius logarithm, sine and cosine, the sum, both exponentials, the product -- is
evaluated in numpy.longdouble where that has 63 mantissa bits or more (asserted: LD_OK), otherwise pair by pair in mpmath.

Wave-tiles.  A wave of the FFT kernels (32 <= Mz <= 2048) holds 128 / G consecutive paths of a launch, G = Mz / 16 lanes per
pair (Mz / 32 at 2048); a tile is 4 G consecutive steps; the wave takes expm1_small6_2, expm1_small9_2 or exp_full2 - 1 for a
tile by the largest |inc| that any of its lanes holds (bounds 0.1 and 0.34, rb_fft_block).  wave_tile_max() returns that
maximum over the LIVE path-steps of every wave-tile.  Dead steps: the device's ballot also sees the steps beyond the grid in a
last tile and the columns beyond n_paths in a last wave, which are computed like any other and never stored.  They are not part
of the classes here.  That may move a wave UP a branch on the device and never changes a class assertion of this file: each
asserts that a live path-step is large enough to force the branch it names (or, for `small`, is a statement about live steps only).
Every branch is accurate on the range of the branches below it, so the parity bounds hold whichever of them a wave took.

The class assertions are made on float64 evaluations of the same code (the whole launch, every column; a matrix product per
shape), never closer than CLASS_MARGIN to a threshold, so that the arithmetic of the evaluation cannot change a class.

No path-step is left out of any comparison: the reference and the oracle stay finite on every set and shape (asserted), and S is
compared relatively with no cap and no exclusion."""
import math

import numpy as np
import pytest

from montecarlooptionspricer_amd.engine import rbergomi_spectrum
from test_heston_reference import STREAM_PRICE, STREAM_VOL, philox_words

LD = np.longdouble
LD_OK = np.finfo(LD).nmant >= 63
S0, R = 100.0, 0.04
SEED64 = 0x9E3779B97F4A7C15
SMALL_BOUND, MIDDLE_BOUND = 0.1, 0.34          # fm::SMALL6_EXP_BOUND and the 0.34 of rb_fft_block
CLASS_MARGIN = 1e-6
# The reference against mpmath at 50 digits, relative in S: 1/100 of the smallest bound of tests/test_gpu_rbergomi.py (asserted below)
OWN_ERROR_BOUND = 2e-16
# The oracle (binary64, libm, the same direct sum) against the reference: the yardstick of every 1e-9 comparison of
# tests/test_gpu_parity.py.  Its bound is rounding alone: per step an exponential, a product and the exponent's own rounding,
# 4 ulp of 2^-53 at most, over the 2500 steps of the longest shape.  What it is, per set, on the cases of this file:
ORACLE_BOUND = 2500 * 4 * 2.0 ** -53            # 1.1e-12
ORACLE_OBSERVED = {"small": 8.9e-15, "middle": 9.7e-15, "full": 1.9e-14, "mixed": 9.5e-15, "large-x": 8.1e-15, "smooth": 6.8e-15,
                   "eta-zero": 5.7e-15}

# name -> generator parameters.  What each name promises is asserted in test_sets_reach_the_branches_they_name.
PARITY_SETS = {
    "small": dict(xi=0.04, H=0.1, eta=1.9, dt=1.0 / 252.0),       # the parameters of every earlier rBergomi test
    "middle": dict(xi=0.9, H=0.1, eta=0.1, dt=1.0 / 252.0),       # sqrt(xi dt) = 0.06: 0.1 is 1.7 sigma, 0.34 is 5.7 sigma
    "full": dict(xi=0.5, H=0.1, eta=0.5, dt=1.0 / 12.0),          # 70 % volatility on monthly steps: sqrt(xi dt) = 0.2
    # rough and strongly lognormal: quiet and violent wave-tiles side by side at every horizon.  (A smooth driver -- H = 0.49,
    # eta = 1 on weekly steps -- mixes as well at 252 steps, but its X has variance t^0.98: at 1000 steps and more X + comp reaches
    # 19, a step's variance 1e8, and S underflows to zero.)
    "mixed": dict(xi=2.0, H=0.05, eta=3.0, dt=1.0 / 52.0),
    "large-x": dict(xi=0.09, H=0.05, eta=4.0, dt=1.0 / 12.0),     # |X + comp| beyond 5: exp2_pair leaves the first octaves
    "smooth": dict(xi=0.04, H=0.57, eta=0.03, dt=1.0 / 252.0),
    "eta-zero": dict(xi=0.04, H=0.3, eta=0.0, dt=1.0 / 252.0),    # constant variance: GBM with sigma^2 = xi
}
# k_rbergomi_small (Mz <= 16) | LG 1-4, two staging buffers | LG 5, 6, one buffer | k_rbergomi_fft<6,3> | the generic route
STEPS = (1, 7, 16, 17, 40, 100, 252, 300, 1000, 2048, 2500)
FFT_STEPS = tuple(s for s in STEPS if 16 < s <= 2048)


def transform_size(n_steps):
    M = 1
    while M < n_steps:
        M *= 2
    return M


def lanes_per_pair(M):
    assert 32 <= M <= 2048
    return 64 if M == 2048 else M // 16


def pairs_per_block(M):
    """rb_pairs_per_block (csrc/rbergomi_device.hpp); 128 on the generic route (launch_rbergomi)."""
    return 256 if M < 32 else 128 if M > 2048 else 4 * (64 // lanes_per_pair(M))


def path_begin_of(n_steps):
    """Even, different from shape to shape, beyond 2^32 at 7 and at 252 steps."""
    return (1 << 33) + 2 * n_steps + 10 if n_steps in (7, 252) else 998 + 2 * n_steps


def seed_of(n_steps):
    return SEED64 if n_steps % 2 else 20251031


def pair_budget(M):
    """Pairs the reference is evaluated on per launch: 64 columns while a pair costs little."""
    return 32 if M <= 256 else 16 if M <= 1024 else 8 if M == 2048 else 3


def pick_pairs(n_paths, M, must, budget=None):
    """Sorted pair indices of a launch of n_paths columns: `must`, then pairs drawn at random up to the budget."""
    n_pairs = (n_paths + 1) // 2
    budget = min(budget or pair_budget(M), n_pairs)
    chosen = sorted({p for p in must if 0 <= p < n_pairs})
    rng = np.random.default_rng(n_paths + M)
    while len(chosen) < budget:
        p = int(rng.integers(0, n_pairs))
        if p not in chosen:
            chosen = sorted(chosen + [p])
    return chosen


def ragged_launch(n_steps):
    """(n_paths, path_begin, seed, pairs): two shares, the second ragged and ending on a lone A path; the pairs are the first and
    the last of the first share, the two of the ragged share, and random ones."""
    M = transform_size(n_steps)
    ppb = pairs_per_block(M)
    n_paths = 2 * ppb + 3
    return n_paths, path_begin_of(n_steps), seed_of(n_steps), pick_pairs(n_paths, M, (0, ppb - 1, ppb, ppb + 1))


# ---- the reference -------------------------------------------------------------------------------------------------------
def normals(seed, path, block, stream, dtype):
    """[4][...]: the four standard normals of Philox block(s) `block` of (path, stream), evaluated in dtype."""
    w = philox_words(seed, path, block, stream)
    two_pi = 8.0 * np.arctan(dtype(1.0))
    z = []
    for wa, wb in ((w[0], w[1]), (w[2], w[3])):
        u = ((((wb & np.uint64(0xFF)) << np.uint64(32)) + wa).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -40)
        rad = np.sqrt(dtype(-2.0) * np.log(u))
        ang = two_pi * (((wb >> np.uint64(8)).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -24))
        z += [rad * np.cos(ang), rad * np.sin(ang)]
    return np.stack(z)


def draws(seed, ids, n_draws, stream, dtype):
    """[n_draws][len(ids)]: draw n is element n & 3 of block n >> 2."""
    nb = max((n_draws + 3) // 4, 1)
    z = normals(seed, np.asarray(ids, dtype=np.uint64)[None, :], np.arange(nb, dtype=np.uint64)[:, None], stream, dtype)
    return np.transpose(z, (1, 0, 2)).reshape(4 * nb, -1)[:n_draws]


def rbergomi_reference(seed, S0, r, xi, H, eta, dt, n_steps, pair_ids, dtype=None):
    """S [n_steps + 1][2 len(pair_ids)], inc [n_steps][...], X + comp [n_steps][...]: columns 2j and 2j + 1 are the paths
    2 pair_ids[j] and 2 pair_ids[j] + 1.  dtype None: longdouble where it is wide enough, else mpmath pair by pair (returned
    as longdouble)."""
    if dtype is None and not LD_OK:
        out = [reference_pair_mp(seed, S0, r, xi, H, eta, dt, n_steps, int(q)) for q in pair_ids]
        return tuple(np.concatenate([np.array(o[i], dtype=LD) for o in out], axis=1) for i in range(3))
    dtype = dtype or LD
    amp, comp = rbergomi_spectrum(H, eta, dt, n_steps)
    M = len(amp)
    pair_ids = np.asarray(pair_ids, dtype=np.uint64)
    z = draws(seed, pair_ids, 2 * M, STREAM_VOL, dtype)                    # (g_k, h_k) = draws 2k, 2k + 1 of the pair's stream 1
    a = amp.astype(dtype)[:, None]
    yr, yi = a * z[0::2], a * z[1::2]                                      # [M][pairs]
    xr, xi_ = np.zeros((n_steps, len(pair_ids)), dtype=dtype), np.zeros((n_steps, len(pair_ids)), dtype=dtype)
    if amp.any():
        ang = 8.0 * np.arctan(dtype(1.0)) * (np.arange(M).astype(dtype) / dtype(M))
        ct, st = np.cos(ang), np.sin(ang)
        k = np.arange(M, dtype=np.int64)[None, :]
        rows = max(1, (1 << 19) // M)
        for n0 in range(0, n_steps, rows):
            q = (np.arange(n0, min(n0 + rows, n_steps), dtype=np.int64)[:, None] * k) & (M - 1)
            c, s = ct[q], st[q]
            xr[n0:n0 + rows] = c @ yr - s @ yi
            xi_[n0:n0 + rows] = s @ yr + c @ yi
    X = np.empty((n_steps, 2 * len(pair_ids)), dtype=dtype)
    X[:, 0::2], X[:, 1::2] = xr, xi_
    ids = np.repeat(pair_ids * np.uint64(2), 2) + np.tile(np.array([0, 1], dtype=np.uint64), len(pair_ids))
    zp = draws(seed, ids, n_steps, STREAM_PRICE, dtype)
    xc = X + comp.astype(dtype)[:, None]
    e = np.exp(xc / dtype(2.0))
    xi_dt = dtype(xi) * dtype(dt)
    inc = np.sqrt(xi_dt) * e * zp - xi_dt * e * e / dtype(2.0) + dtype(r) * dtype(dt)
    S = np.empty((n_steps + 1, inc.shape[1]), dtype=dtype)
    S[0] = dtype(S0)
    S[1:] = dtype(S0) * np.cumprod(np.exp(inc), axis=0)
    return S, inc, xc


def reference_pair_mp(seed, S0, r, xi, H, eta, dt, n_steps, pair_id, digits=50):
    """The same pair in mpmath at `digits` digits: lists [n_steps + 1][2], [n_steps][2], [n_steps][2] of mpf.  The direct sum
    runs in exact integer arithmetic on the mpmath terms scaled by 2^220 (a 4096-term sum in mpf takes minutes)."""
    import mpmath
    with mpmath.workprec(int(digits * 3.33) + 8):
        mp = mpmath.mp
        amp, comp = rbergomi_spectrum(H, eta, dt, n_steps)
        M = len(amp)

        def mp_normals(path, n_draws, stream):
            out = []
            for b in range(max((n_draws + 3) // 4, 1)):
                w = [int(x) for x in philox_words(seed, np.uint64(path), b, stream)]
                for wa, wb in ((w[0], w[1]), (w[2], w[3])):
                    u = (mp.mpf(((wb & 0xFF) << 32) + wa) + 0.5) * mp.mpf(2) ** -40
                    rad = mp.sqrt(-2 * mp.log(u))
                    ang = 2 * mp.pi * (mp.mpf(wb >> 8) + 0.5) * mp.mpf(2) ** -24
                    out += [rad * mp.cos(ang), rad * mp.sin(ang)]
            return out[:n_draws]

        z = mp_normals(pair_id, 2 * M, STREAM_VOL)
        scale = mp.mpf(2) ** 220
        fix = lambda x: int(mp.nint(x * scale))  # noqa: E731
        yr = np.array([fix(mp.mpf(float(amp[k])) * z[2 * k]) for k in range(M)], dtype=object)
        yi = np.array([fix(mp.mpf(float(amp[k])) * z[2 * k + 1]) for k in range(M)], dtype=object)
        ct = np.array([fix(mp.cos(2 * mp.pi * q / M)) for q in range(M)], dtype=object)
        st = np.array([fix(mp.sin(2 * mp.pi * q / M)) for q in range(M)], dtype=object)
        k = np.arange(M, dtype=np.int64)
        zp = [mp_normals(2 * pair_id + h, n_steps, STREAM_PRICE) for h in (0, 1)]
        xi_dt = mp.mpf(xi) * mp.mpf(dt)
        S, inc, xc = [[mp.mpf(S0)] * 2], [], []
        for n in range(n_steps):
            q = (k * n) & (M - 1)
            c, s = ct[q], st[q]
            x = (mp.mpf(int(np.dot(c, yr) - np.dot(s, yi))) / scale / scale, mp.mpf(int(np.dot(s, yr) + np.dot(c, yi))) / scale / scale)
            xc.append([x[h] + mp.mpf(float(comp[n])) for h in (0, 1)])
            e = [mp.exp(v / 2) for v in xc[-1]]
            inc.append([mp.sqrt(xi_dt) * e[h] * zp[h][n] - xi_dt * e[h] * e[h] / 2 + mp.mpf(r) * mp.mpf(dt) for h in (0, 1)])
            S.append([S[-1][h] * mp.exp(inc[-1][h]) for h in (0, 1)])
        return S, inc, xc


_cache = {}


def reference_columns(name, n_steps, seed, path_begin, pairs):
    """(S, inc, X + comp) of the reference on the pairs `pairs` (indices within the launch) of a launch that begins at
    path_begin: computed once per (set, shape, seed, pairs) and shared; callers leave it unchanged."""
    key = (name, n_steps, seed, path_begin, tuple(pairs))
    if key not in _cache:
        ids = np.uint64(path_begin >> 1) + np.asarray(pairs, dtype=np.uint64)
        out = rbergomi_reference(seed, S0, R, n_steps=n_steps, pair_ids=ids, **PARITY_SETS[name])
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def columns_of(pairs, n_paths):
    """(columns of the launch, columns of the reference's matrices) of the live paths of `pairs`."""
    cols = np.array([2 * p + h for p in pairs for h in (0, 1)])
    live = cols < n_paths
    return cols[live], np.nonzero(live)[0]


def wave_tile_max(inc, M):
    """[waves][tiles]: the largest |inc| over the live path-steps of every wave-tile; inc holds EVERY column of a launch from
    its first (waves are counted from column 0 of the launch: a share is four whole waves)."""
    G = lanes_per_pair(M)
    wave, tile = 128 // G, 4 * G
    a = np.abs(np.asarray(inc, dtype=np.float64))
    n_steps, n_paths = a.shape
    return np.array([[a[t:t + tile, w:w + wave].max() for t in range(0, n_steps, tile)] for w in range(0, n_paths, wave)])


def launch_classes(name, n_steps, n_paths, path_begin, seed):
    """wave_tile_max of a whole launch and its |inc| and X + comp, from a float64 evaluation."""
    ids = np.uint64(path_begin >> 1) + np.arange((n_paths + 1) // 2, dtype=np.uint64)
    _, inc, xc = rbergomi_reference(seed, S0, R, n_steps=n_steps, pair_ids=ids, dtype=np.float64, **PARITY_SETS[name])
    inc, xc = inc[:, :n_paths], xc[:, :n_paths]
    return wave_tile_max(inc, transform_size(n_steps)), np.abs(inc), xc


def class_of(m):
    """0 small, 1 middle, 2 full; never within CLASS_MARGIN of a threshold."""
    m = np.asarray(m)
    assert (np.abs(m - SMALL_BOUND) > CLASS_MARGIN).all() and (np.abs(m - MIDDLE_BOUND) > CLASS_MARGIN).all()
    return (m > SMALL_BOUND).astype(int) + (m > MIDDLE_BOUND).astype(int)


# The launch on which `mixed` shows all three classes within one workgroup: 252 steps, four shares and a ragged one.
MIXED_STEPS, MIXED_PATHS = 252, 2 * 4 * pairs_per_block(256) + 3


def complete(n_steps, n_paths, M):
    """[waves][tiles] bool: wave-tiles whose 512 path-steps are all live."""
    G = lanes_per_pair(M)
    wave, tile = 128 // G, 4 * G
    return np.array([[t + tile <= n_steps and w + wave <= n_paths for t in range(0, n_steps, tile)] for w in range(0, n_paths, wave)])


# ---- tests -------------------------------------------------------------------------------------------------------------
def test_longdouble_is_wide_enough_or_mpmath_stands_in():
    if LD_OK:
        assert np.finfo(LD).nmant >= 63 and LD(1.0) + LD(2.0) ** -63 != LD(1.0)
    else:
        import mpmath  # noqa: F401
    S, inc, xc = rbergomi_reference(3, S0, R, n_steps=5, pair_ids=[4], **PARITY_SETS["small"])
    assert S.shape == (6, 2) and inc.shape == xc.shape == (5, 2) and (S[0] == S0).all()


def test_reference_shapes_shards_and_eta_zero():
    p = PARITY_SETS["mixed"]
    S, inc, _ = rbergomi_reference(7, S0, R, n_steps=40, pair_ids=np.arange(10, 20), dtype=np.float64, **p)
    S2, _, _ = rbergomi_reference(7, S0, R, n_steps=40, pair_ids=[13, 17], dtype=np.float64, **p)
    assert np.abs(S[:, [6, 7, 14, 15]] / S2 - 1.0).max() <= 1e-13               # a pair depends on (seed, pair id) only
    assert np.abs(np.log(S[1:] / S[:-1]) - inc).max() <= 1e-14
    # eta = 0: X = 0 and S is GBM with sigma^2 = xi on the price stream
    q = PARITY_SETS["eta-zero"]
    S, inc, xc = rbergomi_reference(7, S0, R, n_steps=9, pair_ids=[0, 1, 2], **q)
    assert (xc == 0.0).all()
    z = draws(7, np.arange(6, dtype=np.uint64), 9, STREAM_PRICE, np.float64)
    gbm = S0 * np.exp(np.cumsum((R - 0.5 * q["xi"]) * q["dt"] + math.sqrt(q["xi"] * q["dt"]) * z, axis=0))
    assert np.abs(S[1:].astype(np.float64) / gbm - 1.0).max() <= 1e-14


def test_wave_tile_bookkeeping():
    inc = np.zeros((100, 40))                      # Mz = 128: G = 8, waves of 16 paths, tiles of 32 steps
    inc[31, 15], inc[32, 16], inc[99, 39] = 0.2, -0.5, 0.05
    m = wave_tile_max(inc, 128)
    assert m.shape == (3, 4) and m[0, 0] == 0.2 and m[1, 1] == 0.5 and m[2, 3] == 0.05 and np.count_nonzero(m) == 3
    assert complete(100, 40, 128).sum() == 2 * 3
    assert [pairs_per_block(M) for M in (1, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096)] == [256, 256, 128, 64, 32, 16, 8, 4, 4, 128]
    assert [lanes_per_pair(M) for M in (32, 256, 1024, 2048)] == [2, 16, 64, 64]
    for n_steps in STEPS:
        n_paths, begin, _, pairs = ragged_launch(n_steps)
        ppb = pairs_per_block(transform_size(n_steps))
        assert begin % 2 == 0 and n_paths == 2 * ppb + 3 and {0, ppb - 1, ppb, ppb + 1} <= set(pairs) and len(pairs) <= 32
    assert sum(path_begin_of(s) > 2 ** 32 for s in STEPS) == 2


def test_sets_reach_the_branches_they_name():
    """On the reference's increments (float64 evaluation of every column of every FFT-sized ragged launch, and of the
    MIXED_STEPS x MIXED_PATHS launch of the split tests):
      small     every wave-tile's maximum is at most 0.1
      middle    no path-step exceeds 0.34, and every complete wave-tile (512 live path-steps) exceeds 0.1.  A ragged wave of three
                paths, or a last tile of one step, cannot promise a draw beyond 1.7 sigma; on the device those waves hold the
                dead lanes and steps too (module docstring)
      full      at least half of the wave-tiles exceed 0.34
      mixed     within one launch, and within ONE workgroup (the first share) of the 252-step launch, wave-tiles of all three
                classes
      large-x   X + comp below -5 on some steps and above 2 ln 2 on others: the variance factor e^{(X + comp)/2} leaves the first
                octave of exp2_pair downwards by several octaves and upwards (much further up the paths no longer stay finite)
      smooth, eta-zero   small, like today's parameters"""
    stats = {}
    for name in PARITY_SETS:
        cls, comp_cls, big_x = [], [], [0.0, 0.0]
        for n_steps in FFT_STEPS:
            n_paths, begin, seed, _ = ragged_launch(n_steps)
            m, a, xc = launch_classes(name, n_steps, n_paths, begin, seed)
            assert np.isfinite(a).all() and np.isfinite(xc).all()
            c = class_of(m)
            cls.append(c.ravel())
            comp_cls.append(c[complete(n_steps, n_paths, transform_size(n_steps))])
            big_x = [max(big_x[0], float(xc.max())), max(big_x[1], float(-xc.min()))]
        m, a, xc = launch_classes(name, MIXED_STEPS, MIXED_PATHS, path_begin_of(MIXED_STEPS), seed_of(MIXED_STEPS))
        c = class_of(m)
        cls.append(c.ravel())
        comp_cls.append(c[complete(MIXED_STEPS, MIXED_PATHS, 256)])
        first_workgroup = set(c[:4].ravel())
        cls, comp_cls = np.concatenate(cls), np.concatenate(comp_cls)
        stats[name] = (np.bincount(cls, minlength=3), np.bincount(comp_cls, minlength=3), first_workgroup, big_x)
        print(f"{name}: wave-tiles small/middle/full {stats[name][0]}, complete ones {stats[name][1]}, first workgroup of the "
              f"252-step launch {sorted(first_workgroup)}, X + comp within [-{big_x[1]:.2f}, {big_x[0]:.2f}]")
    for name in ("small", "smooth", "eta-zero"):
        assert stats[name][0][1] == stats[name][0][2] == 0, name
    assert stats["middle"][0][2] == 0 and stats["middle"][1][0] == 0 and stats["middle"][1][1] >= 50
    assert 2 * stats["full"][0][2] >= stats["full"][0].sum()
    assert stats["mixed"][2] == {0, 1, 2} and (stats["mixed"][0] > 0).all()
    assert stats["large-x"][3][0] > 2.0 * math.log(2.0) and stats["large-x"][3][1] > 5.0


def parity_cases(name):
    for n_steps in STEPS:
        n_paths, begin, seed, pairs = ragged_launch(n_steps)
        yield n_steps, n_paths, begin, seed, pairs


def test_reference_against_mpmath():
    """The reference's own error: a few pairs per set re-evaluated in mpmath at 50 digits -- the first pair and the lone last
    A path of the ragged launches at 7, 40 and 252 steps on every set, and at 2048 and 2500 steps (the longest sums and products)
    on the two sets with the largest exponents."""
    import mpmath

    import test_gpu_rbergomi as g

    def to_mpf(x):                                   # a longdouble as the exact sum of two doubles
        hi = float(x)
        return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))

    assert OWN_ERROR_BOUND <= min(g.S_BOUND.values()) / 100.0
    worst = {}
    for name in PARITY_SETS:
        for n_steps in (7, 40, 252) + ((2048, 2500) if name in ("mixed", "large-x") else ()):
            n_paths, begin, seed, pairs = ragged_launch(n_steps)
            S, _, _ = reference_columns(name, n_steps, seed, begin, pairs)
            for j in ((0, len(pairs) - 1) if n_steps <= 252 else (len(pairs) - 1,)):
                Sm, _, _ = reference_pair_mp(seed, S0, R, n_steps=n_steps, pair_id=(begin >> 1) + pairs[j], **PARITY_SETS[name])
                with mpmath.workprec(180):
                    err = max(abs(to_mpf(S[n, 2 * j + h]) / Sm[n][h] - 1) for n in range(n_steps + 1) for h in (0, 1))
                worst[name] = max(worst.get(name, 0.0), float(err))
                assert err <= OWN_ERROR_BOUND, (name, n_steps, j, float(err))
    print("the reference against mpmath at 50 digits, largest relative error in S: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("name", list(PARITY_SETS))
def test_oracle_against_the_reference(name):
    """Oracle.paths_rbergomi on the cases of the GPU file: finite everywhere, and within ORACLE_BOUND of the reference with no
    path-step left out.  The largest error per set is printed and kept in ORACLE_OBSERVED."""
    from oracle.binding import Oracle
    orc = Oracle()
    p = PARITY_SETS[name]
    worst = 0.0
    for n_steps, n_paths, begin, seed, pairs in parity_cases(name):
        S, inc, _ = reference_columns(name, n_steps, seed, begin, pairs)
        assert np.isfinite(S.astype(np.float64)).all() and (S > 0).all()
        cols, ref_cols = columns_of(pairs, n_paths)
        got = np.empty((n_steps + 1, 2 * len(pairs)))
        for j, q in enumerate(pairs):
            got[:, 2 * j:2 * j + 2] = orc.paths_rbergomi(seed, S0, R, p["xi"], p["H"], p["eta"], -0.9, p["dt"], n_steps, begin + 2 * q, 2)
        assert np.isfinite(got).all()
        err = float(np.abs(got[:, ref_cols].astype(LD) / S[:, ref_cols] - 1).max())
        worst = max(worst, err)
        assert err <= ORACLE_BOUND, (name, n_steps, err)
    print(f"oracle against the reference on {name}: largest relative error in S {worst:.2e} (recorded: {ORACLE_OBSERVED[name]:.2e})")
    assert worst <= 10.0 * ORACLE_OBSERVED[name]                 # the record stays true (another libm may round otherwise)
