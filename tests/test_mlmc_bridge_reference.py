"""numpy restatement of mcg_mlmc_localvol_level_ex (include/mcgpu.h): mlmc_level_numpy of tests/test_mlmc_reference.py with the
Milstein correction and the Brownian-bridge survival probabilities of a book's barrier levels along both grids -- the yardstick
of tests/test_gpu_mlmc_bridge.py.  Checked here: the restatement against mlmc_level_numpy and against itself on a flat surface,
the flat surface against Reiner-Rubinstein, telescoping and the decay of the level variances on the CEV surface, the telescoping
sum against a plain continuous-barrier estimate, the host entry points and their rejections, the conditioning of the GPU file's
parity cases, and a sanitizer build of the host code."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
from test_barrier_bridge_reference import barrier_out_closed_form, sample_numpy
from test_exotics_reference import payoff_numpy
from test_heston_reference import SEED64, normal_quad
from test_localvol_reference import BAD_MODELS, BAD_SURFACES, CEV, DT, SURFACES, Q, R, S0, table_python
from test_mlmc_reference import (BAD_LEVELS, EURO, SQRT_HALF, case_T, mlmc_combine_python, mlmc_level_numpy)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARRIER_KINDS = (N.X_BARRIER_UP_OUT, N.X_BARRIER_UP_IN, N.X_BARRIER_DOWN_OUT, N.X_BARRIER_DOWN_IN)
UP_KINDS = (N.X_BARRIER_UP_OUT, N.X_BARRIER_UP_IN)
SLOT_NONE, SLOT_UNTOUCHED = -2, -1


def bridge_plan_python(book):
    """(levels [(B, up)], slot per contract) of include/mcgpu.h: first appearance, duplicates compared bitwise share a level, a
    down barrier at zero takes none."""
    levels, slots = [], []
    for kind, _, _, B, _ in book:
        if kind not in BARRIER_KINDS:
            slots.append(SLOT_NONE)
            continue
        up = kind in UP_KINDS
        if not up and B == 0.0:
            slots.append(SLOT_UNTOUCHED)
            continue
        assert B > 0.0, B
        key = (np.float64(B).tobytes(), up)
        keys = [(np.float64(b).tobytes(), u) for b, u in levels]
        if key not in keys:
            assert len(levels) < N.MLMC_BRIDGE_L_MAX, book
            levels.append((float(B), up))
            keys.append(key)
        slots.append(keys.index(key))
    return levels, slots


def mlmc_bridge_numpy(seed, S0, r, surface, T, n_fine, n_paths, has_coarse=True, stride_fine=1, stride_coarse=1, first_obs=1,
                      path_begin=0, q=0.0, scheme=0, levels=(), full=False):
    """(stats10, surv) of include/mcgpu.h: stats10 as mlmc_level_numpy gives it, surv[(1 or 2) len(levels)][n_paths] the survival
    probabilities of `levels` = [(B, up)] on the fine grid, then on the coarse one.  full: also the smallest |X - h| over every
    row and coarse midpoint of every path and level (inf without levels)."""
    n_x = surface.n_x
    inv_dx = float(n_x - 1) / (float(surface.x_max) - float(surface.x_min))
    u0 = -float(surface.x_min) * inv_dx
    path = np.uint64(path_begin) + np.arange(n_paths, dtype=np.uint64)
    h = [math.log(float(B) / float(S0)) for B, _ in levels]
    closest = [math.inf]

    class Grid:
        def __init__(self, dt, n_steps, stride):
            self.tab = table_python(surface.times, n_x, surface.sigma, dt, n_steps)
            self.m = (float(r) - float(q)) * dt
            self.stride, self.row = stride, 0
            self.S, self.X = np.full(n_paths, float(S0)), np.zeros(n_paths)
            on = first_obs == 0
            self.sumS, self.sumX = np.full(n_paths, float(S0) if on else 0.0), np.zeros(n_paths)
            self.mn, self.mx = np.full(n_paths, float(S0) if on else np.inf), np.full(n_paths, float(S0) if on else -np.inf)
            self.nd = float(n_steps // stride + 1 - first_obs)
            # survival: d at the last row, the running product, the extremes of X over the rows (row 0: X = 0)
            self.dprev = [np.full(n_paths, 0.0 - hl) for hl in h]
            self.prod = [np.ones(n_paths) for _ in h]
            self.lo, self.hi = np.zeros(n_paths), np.zeros(n_paths)
            for hl in h:
                closest[0] = min(closest[0], abs(hl))

        def step(self, z):
            """one step; returns the step volatility"""
            uu = self.X * inv_dx + u0
            u = np.minimum(np.maximum(uu, 0), n_x - 1)
            j = np.minimum(u.astype(np.int64), n_x - 2)
            f = u - j
            sl = self.tab[self.row if len(self.tab) > 1 else 0]
            a = f * sl[j, 1] + sl[j, 0]
            e = a * z + (-0.5 * a * a + self.m)
            if scheme:
                g = np.where((uu > 0) & (uu < n_x - 1), sl[j, 1] * inv_dx, 0.0)
                e = (0.5 * a) * g * (z * z - 1.0) + e
            self.X = self.X + e
            self.S = self.S * np.exp(e)
            self.row += 1
            if self.row % self.stride == 0:
                self.sumS = self.sumS + self.S
                self.sumX = self.sumX + self.X
                self.mn, self.mx = np.minimum(self.mn, self.S), np.maximum(self.mx, self.S)
            return a

        def interval(self, x, w):
            """the sub-interval that ends in the row x, of variance w"""
            self.lo, self.hi = np.minimum(self.lo, x), np.maximum(self.hi, x)
            with np.errstate(divide="ignore", invalid="ignore"):
                c = -2.0 / w
                for l, hl in enumerate(h):
                    d = x - hl
                    closest[0] = min(closest[0], float(np.abs(d).min()))
                    m = np.maximum(self.dprev[l] * d, 0.0)
                    t = np.where(w > 0.0, m * c, -np.inf)
                    self.prod[l] = self.prod[l] * (1.0 - np.exp(t))
                    self.dprev[l] = d

        def stats(self):
            return [self.S, self.sumS / self.nd, float(S0) * np.exp(self.sumX / self.nd), self.mn, self.mx]

        def surv(self):
            return [np.where((self.hi < hl) if up else (self.lo > hl), self.prod[l], 0.0) for l, ((_, up), hl) in enumerate(zip(levels, h))]

    dt_f = T / float(n_fine)
    F = Grid(dt_f, n_fine, stride_fine)
    Cg = Grid(2.0 * dt_f, n_fine // 2, stride_coarse) if has_coarse else None
    for n in range(n_fine):
        if n & 3 == 0:
            quad = normal_quad(seed, path, n >> 2, 0)
        s = F.step(quad[n & 3])
        F.interval(F.X, s * s)
        if has_coarse and n & 1:
            za, zb = quad[(n & 3) - 1], quad[n & 3]
            x0 = Cg.X
            s = Cg.step((za + zb) * SQRT_HALF)
            xm = (0.5 * s) * ((za - zb) * SQRT_HALF) + 0.5 * (x0 + Cg.X)
            w = 0.5 * (s * s)
            Cg.interval(xm, w)
            Cg.interval(Cg.X, w)
    stats = np.stack(F.stats() + (Cg.stats() if has_coarse else []))
    surv = np.array(F.surv() + (Cg.surv() if has_coarse else [])).reshape((2 if has_coarse else 1) * len(levels), n_paths)
    return (stats, surv, closest[0]) if full else (stats, surv)


def samples_numpy(stats, surv, book, bridge):
    """(P_f, P_c) per contract, [n_contracts][n_paths] each: with bridge a barrier contract is sample_numpy on its level's
    survival probability (1 for a down barrier at zero), everything else payoff_numpy on the five statistics."""
    coarse = len(stats) == 10
    levels, slots = bridge_plan_python(book) if bridge else ([], [SLOT_NONE] * len(book))
    pf, pc = [], []
    for c, sl in zip(book, slots):
        if sl == SLOT_NONE:
            pf.append(payoff_numpy(stats[:5], c))
            pc.append(payoff_numpy(stats[5:], c) if coarse else np.zeros(stats.shape[1]))
        else:
            one = np.ones(stats.shape[1])
            pf.append(sample_numpy(stats[0], one if sl < 0 else surv[sl], c))
            pc.append(sample_numpy(stats[5], one if sl < 0 else surv[len(levels) + sl], c) if coarse else np.zeros(stats.shape[1]))
    return np.array(pf), np.array(pc)


def book_sums_bridge_numpy(stats, surv, book, bridge):
    """sums[6 n_contracts + 1] of include/mcgpu.h (numpy's own summation order)."""
    pf, pc = samples_numpy(stats, surv, book, bridge)
    out = []
    for f, c in zip(pf, pc):
        y = f - c
        out += [y.sum(), (y * y).sum(), f.sum(), (f * f).sum(), c.sum(), (c * c).sum()]
    return np.array(out + [float(stats.shape[1])])


# ---- the element-wise cases (reused by tests/test_gpu_mlmc_bridge.py) ----------------------------------------------------------
# Barriers off the round numbers, within a few daily steps of S0 = 100 so that P is neither 0 nor 1 on most paths.
DOP = (N.X_BARRIER_DOWN_OUT, False, 100.21, 98.77, 1.5)
UIC = (N.X_BARRIER_UP_IN, True, 99.71, 101.47, 0.25)
UOP = (N.X_BARRIER_UP_OUT, False, 102.3, 102.57, 0.0)
DOC_ABOVE = (N.X_BARRIER_DOWN_OUT, True, 100.0, 101.47, 0.0)      # a down barrier above S0: P = 0 everywhere
LOOK = (N.X_LOOKBACK_FLOAT, True, 0.0, 0.0, 0.0)
BOOKS = {
    "one-level": [EURO(100.37), DOP, LOOK],
    "two-levels": [UIC, DOP, (N.X_BARRIER_UP_OUT, True, 100.0, 101.47, 0.5), EURO(99.0, False)],            # one level duplicated
    "four-levels": [DOP, UIC, LOOK, UOP, (N.X_BARRIER_DOWN_IN, False, 101.0, 98.77, 2.0), EURO(100.37), DOC_ABOVE],
}
BRIDGE_SURFACES = ("cev", "skew-term", "narrow", "two-nodes", "wide-128")
COUNTS, BEGINS = (1, 257, 513, 1000), (0, 12345, 2 ** 33 + 1)


def _cases():
    """name -> list of (n_fine, has_coarse, n_paths, path_begin, seed, scheme, book name): with a coarse path n_fine in {2 .. 14}
    and 252 x 1300, without one n_fine in {1, 2, 3, 4, 5, 7}; the path counts, the offsets, the seeds, the schemes and the books
    rotate through the list.  The strides stay 1: the survival probabilities do not read them."""
    out, k = {}, 0
    names = list(BOOKS)
    for name in BRIDGE_SURFACES:
        rows = []
        for n_fine, coarse in [(n, True) for n in (2, 4, 6, 8, 10, 12, 14)] + [(n, False) for n in (1, 2, 3, 4, 5, 7)]:
            rows.append((n_fine, coarse, COUNTS[k % 4], BEGINS[k % 3], SEED64 if k % 5 == 0 else 7, (k // 2) % 2, names[k % 3]))
            k += 1
        rows.append((252, True, 1300, 777, SEED64, k % 2, "four-levels"))
        k += 1
        out[name] = rows
    return out


CASES = _cases()


def reference(name, case, cache={}):
    """One numpy run per case, shared by every test that needs it and never written to: (stats10, surv, closest)."""
    if (name, case) not in cache:
        n_fine, coarse, n_paths, begin, seed, scheme, book = case
        levels, _ = bridge_plan_python(BOOKS[book])
        got = mlmc_bridge_numpy(seed, S0, R, SURFACES[name], case_T(n_fine), n_fine, n_paths, coarse, 1, 1, 1, begin, Q, scheme, levels, full=True)
        got[0].setflags(write=False)
        got[1].setflags(write=False)
        cache[(name, case)] = got
    return cache[(name, case)]


# ---- the statistical run (CEV, T = 1, n0 = 4, levels 0 .. 5, 100 000 paths a level, seed 20261021 + l) ---------------------------
STAT_T, N0, STAT_LEVELS, STAT_PATHS = 1.0, 4, 6, 100_000
MLMC_SEED = 20261021       # the first one tried (the seed may be picked, never the bound)
STAT_BOOK = [(N.X_BARRIER_DOWN_OUT, False, 100.0, 85.0, 0.0), (N.X_BARRIER_UP_OUT, True, 100.0, 120.0, 0.0), EURO(100.0),
             (N.X_BARRIER_DOWN_IN, False, 100.0, 85.0, 0.0)]
STAT_NAMES = ("down-and-out put", "up-and-out call", "European call", "down-and-in put")
STAT_LEVELS_OF_BOOK = bridge_plan_python(STAT_BOOK)[0]


def stat_run(scheme, cache={}):
    """per level: (P_f, P_c) of STAT_BOOK with the bridge, [n_contracts][n_paths] each, and the stats10 of the level"""
    if scheme not in cache:
        rows = []
        for l in range(STAT_LEVELS):
            st, sv = mlmc_bridge_numpy(MLMC_SEED + l, S0, R, CEV, STAT_T, N0 << l, STAT_PATHS, has_coarse=l > 0, q=Q, scheme=scheme,
                                       levels=STAT_LEVELS_OF_BOOK)
            rows.append(samples_numpy(st, sv, STAT_BOOK, True) + (st,))
        cache[scheme] = rows
    return cache[scheme]


def level_variances(rows, c):
    return [float((pf[c] - pc[c]).var(ddof=1)) for pf, pc, _ in rows]


# ---- tests ----------------------------------------------------------------------------------------------------------------
def test_restatement_identities():
    # scheme 0 without levels: mlmc_level_numpy bit for bit
    for name, n_fine, n_paths, coarse, sf, sc, first_obs, begin in (("cev", 12, 300, True, 2, 1, 0, 5), ("skew-term", 7, 257, False, 7, 1, 1, 2 ** 33 + 1),
                                                                   ("two-nodes", 10, 100, True, 1, 1, 1, 0)):
        want = mlmc_level_numpy(7, S0, R, SURFACES[name], case_T(n_fine), n_fine, n_paths, coarse, sf, sc, first_obs, begin, Q)
        got, sv = mlmc_bridge_numpy(7, S0, R, SURFACES[name], case_T(n_fine), n_fine, n_paths, coarse, sf, sc, first_obs, begin, Q)
        assert got.tobytes() == want.tobytes() and sv.shape == (0, n_paths)
        # the levels change no statistic, and a path depends on (seed, id) only
        lv = [(98.77, False), (101.47, True)]
        st2, sv2 = mlmc_bridge_numpy(7, S0, R, SURFACES[name], case_T(n_fine), n_fine, n_paths, coarse, sf, sc, first_obs, begin, Q, 0, lv)
        assert st2.tobytes() == want.tobytes() and sv2.shape == ((4 if coarse else 2), n_paths)
        st3, sv3 = mlmc_bridge_numpy(7, S0, R, SURFACES[name], case_T(n_fine), n_fine, n_paths - 40, coarse, sf, sc, first_obs, begin + 40, Q, 0, lv[1:])
        assert st3.tobytes() == want[:, 40:].tobytes() and sv3.tobytes() == sv2[1::2, 40:].tobytes()
        assert ((sv2 >= 0.0) & (sv2 <= 1.0)).all()
    # a flat surface: Milstein is log-Euler bit for bit, and P_f and P_c of a level agree to rounding
    flat, worst = SURFACES["flat"], 0.0
    lv = [(85.0, False), (120.0, True)]
    for n_fine in (2, 8, 32):
        e = mlmc_bridge_numpy(3, S0, R, flat, 1.0, n_fine, 2000, q=Q, scheme=0, levels=lv)
        m = mlmc_bridge_numpy(3, S0, R, flat, 1.0, n_fine, 2000, q=Q, scheme=1, levels=lv)
        assert e[0].tobytes() == m[0].tobytes() and e[1].tobytes() == m[1].tobytes()
    # ... the coarse midpoint rebuilds the fine path: X_2k+1 = xm exactly in real arithmetic when sigma is constant
    st, sv = mlmc_bridge_numpy(3, S0, R, flat, 1.0, 32, 20_000, q=Q, scheme=1, levels=lv)
    worst = float(np.abs(sv[:2] - sv[2:]).max())
    print(f"flat surface, 32 steps: largest |P_f - P_c| {worst:.2e}")
    assert worst <= 9.0e-14           # ten times the 8.99e-15 measured here
    assert np.abs(st[0] / st[5] - 1.0).max() <= 1e-13


@pytest.mark.parametrize("n_fine", (2, 8, 32))
def test_flat_surface_against_the_closed_form(n_fine):
    sigma, n = 0.2, 200_000
    book = [(N.X_BARRIER_DOWN_OUT, False, 100.0, 85.0, 0.0), (N.X_BARRIER_UP_OUT, True, 100.0, 120.0, 0.0)]
    levels, _ = bridge_plan_python(book)
    st, sv = mlmc_bridge_numpy(MLMC_SEED + n_fine, S0, R, SURFACES["flat"], 1.0, n_fine, n, q=0.0, scheme=1, levels=levels)
    pf, pc = samples_numpy(st, sv, book, True)
    disc = math.exp(-R * 1.0)
    for c, x in enumerate(book):
        want = barrier_out_closed_form(S0, x[2], x[3], R, sigma, 1.0, x[1], x[0] == N.X_BARRIER_UP_OUT)
        for grid, y in (("fine", pf[c]), ("coarse", pc[c])):
            price, se = disc * float(y.mean()), disc * float(y.std(ddof=1)) / math.sqrt(n)
            print(f"{n_fine} steps, contract {c}, {grid}: {price:.4f} +- {se:.4f}, closed form {want:.4f}: {abs(price - want) / se:.2f} std errors")
            assert abs(price - want) <= 4.0 * se, (n_fine, c, grid, price, se, want)


def test_statistical_run_telescoping_and_variance_decay():
    mil, eul = stat_run(1), stat_run(0)
    for label, rows in (("Milstein + bridge", mil), ("log-Euler + bridge", eul)):
        for c, name in enumerate(STAT_NAMES):
            V = level_variances(rows, c)
            print(f"{label}, {name}: V_l = {', '.join(f'{v:.4g}' for v in V)}")
            for l in range(1, STAT_LEVELS):
                pc, pf = rows[l][1][c], rows[l - 1][0][c]
                z = abs(float(pc.mean()) - float(pf.mean())) / math.sqrt(float(pc.var(ddof=1)) / len(pc) + float(pf.var(ddof=1)) / len(pf))
                assert z <= 4.0, (label, name, l, z)
    for c in (0, 1):
        V = level_variances(mil, c)
        print(f"{STAT_NAMES[c]}: V_1 / V_5 = {V[1] / V[5]:.1f} (rate 1: 16, rate 1/2: 4)")
        assert V[5] <= V[1] / 16.0, (c, V)
    V = level_variances(mil, 2)
    print(f"European call: V_1 / V_5 = {V[1] / V[5]:.1f} with Milstein (rate 2: 256), {level_variances(eul, 2)[1] / level_variances(eul, 2)[5]:.1f} with log-Euler")
    assert V[5] <= V[1] / 64.0, V
    # log-Euler + bridge against the coupling of mcg_mlmc_localvol_level on the same paths (the discretely monitored payoff)
    st = eul[1][2]
    plain_v1 = float((payoff_numpy(st[:5], STAT_BOOK[0]) - payoff_numpy(st[5:], STAT_BOOK[0])).var(ddof=1))
    bridge_v1 = level_variances(eul, 0)[1]
    print(f"down-and-out put, V_1: {plain_v1:.4g} without the bridge, {bridge_v1:.4g} with it: ratio {plain_v1 / bridge_v1:.1f}")
    assert bridge_v1 < plain_v1 / 10.0


def test_telescoping_sum_against_a_plain_estimate():
    rows = stat_run(1)[:5]
    st, sv = mlmc_bridge_numpy(MLMC_SEED + 1000, S0, R, CEV, STAT_T, N0 << 4, 2 * STAT_PATHS, has_coarse=False, q=Q, scheme=1, levels=STAT_LEVELS_OF_BOOK)
    plain, _ = samples_numpy(st, sv, STAT_BOOK, True)
    disc = math.exp(-R * STAT_T)
    for c, name in enumerate(STAT_NAMES):
        y = [pf[c] - pc[c] for pf, pc, _ in rows]
        price, se = mlmc_combine_python([v.sum() for v in y], [(v * v).sum() for v in y], [len(v) for v in y], R, STAT_T)
        pm, pse = disc * float(plain[c].mean()), disc * float(plain[c].std(ddof=1)) / math.sqrt(plain.shape[1])
        z = abs(price - pm) / math.hypot(se, pse)
        print(f"{name}: multilevel {price:.4f} +- {se:.4f}, plain 64 steps {pm:.4f} +- {pse:.4f}: {z:.2f} combined std errors")
        assert z <= 4.0, (name, price, se, pm, pse)


def raw_level_ex(scheme=0, bridge=0, ctx=None, S0=100.0, r=R, q=Q, times=(0.0, 0.1), n_t=2, x_min=-1.0, x_max=1.0, n_x=3,
                 sigma=((0.2, 0.25, 0.3), (0.1, 0.2, 0.3)), T=8 * DT, n_fine=8, has_coarse=1, stride_fine=2, stride_coarse=1, first_obs=1,
                 path_begin=0, n_paths=100, book=(EURO(100.0),), n_contracts=None, with_lv=True, with_book=True, with_sums=True,
                 dt=None, n_steps=None, payoff=None):
    """mcg_mlmc_localvol_level_ex as C sees it: (status, message); raw_level of tests/test_mlmc_reference.py with the two switches."""
    L = mc.load_library()
    dp = C.POINTER(C.c_double)
    if n_steps is not None:
        n_fine, has_coarse, stride_fine = n_steps, 0, 1
    if dt is not None:
        T = dt * n_fine
    t = None if times is None else np.ascontiguousarray(times, dtype=np.float64)
    s = None if sigma is None else np.ascontiguousarray(sigma, dtype=np.float64)
    lv = N.MlmcLevel(7, n_fine, has_coarse, stride_fine, stride_coarse, first_obs, path_begin, n_paths)
    arr = mc.engine.make_book(list(book))
    sums = np.full(6 * len(arr) + 1, 7.0)
    rc = L.mcg_mlmc_localvol_level_ex(ctx, S0, r, q, None if t is None else t.ctypes.data_as(dp), n_t, x_min, x_max, n_x,
                                      None if s is None else s.ctypes.data_as(dp), T, C.byref(lv) if with_lv else None, scheme, bridge,
                                      arr if with_book else None, len(arr) if n_contracts is None else n_contracts,
                                      sums.ctypes.data_as(dp) if with_sums else None, None, None)
    assert (sums == 7.0).all() or rc == 0
    return rc, L.mcg_last_error().decode()


def out_put(B, up=False):
    return (N.X_BARRIER_UP_OUT if up else N.X_BARRIER_DOWN_OUT, False, 100.0, B, 0.0)


FIVE_LEVELS = [out_put(80.0), out_put(85.0), out_put(120.0, True), out_put(85.0, True), out_put(80.0), out_put(90.0)]
# what mcg_mlmc_localvol_level_ex rejects of its own, as changes to one valid call, with a word of the message
BAD_BRIDGES = [
    (dict(bridge=1, book=FIVE_LEVELS), "more than 4 distinct bridge levels"), (dict(bridge=1, book=(EURO(100.0), out_put(-1.0))), "contract 1: a bridge level"),
    (dict(bridge=1, book=(out_put(0.0, True),)), "contract 0: a bridge level"), (dict(bridge=1, book=(out_put(-0.5, True),)), "contract 0: a bridge level"),
    (dict(scheme=2), "scheme must be"), (dict(scheme=-1), "scheme must be"), (dict(bridge=2), "bridge must be 0 or 1"),
    (dict(bridge=-1), "bridge must be 0 or 1"),
]


def test_library_exports_and_rejects_without_a_gpu():
    L = mc.load_library()
    for name in ("mcg_mlmc_localvol_level_ex", "mcg_mlmc_bridge_levels"):
        assert hasattr(L, name), name
    assert hasattr(mc, "mlmc_bridge_levels") and "mlmc_bridge_levels" in mc.__all__
    assert len(N.KERNEL_NAMES) == 14 and C.sizeof(N.MlmcLevel) == 48                    # neither the timing enum nor the level grows
    header = open(os.path.join(ROOT, "include", "mcgpu.h")).read()
    assert f"#define MCG_MLMC_BRIDGE_L_MAX {N.MLMC_BRIDGE_L_MAX}\n" in header
    assert "enum mcg_mlmc_scheme { MCG_MLMC_LOG_EULER = 0, MCG_MLMC_MILSTEIN = 1 };" in header and N.MLMC_SCHEMES == {"euler": 0, "milstein": 1}
    # a valid call fails on the NULL ctx only, in every combination of the switches
    for scheme in (0, 1):
        for bridge in (0, 1):
            for book in ((EURO(100.0),), FIVE_LEVELS[:5], (out_put(-1.0),) if not bridge else (out_put(0.0),)):
                rc, msg = raw_level_ex(scheme, bridge, book=book)
                assert rc == 1 and "ctx is NULL" in msg, (scheme, bridge, book, msg)
    for change, message in BAD_BRIDGES:
        rc, msg = raw_level_ex(**change)
        assert rc == 1 and message in msg, (change, rc, msg)
    # everything the old entry point rejects, with the switches on
    for change, message, status in BAD_LEVELS:
        rc, msg = raw_level_ex(1, 1, **change)
        assert rc == status and message in msg, (change, rc, msg)
    for change, message in BAD_SURFACES + BAD_MODELS:
        if "payoff" in change or "n_paths" in change:
            continue
        rc, msg = raw_level_ex(1, 1, **change)
        if "dt" in change:
            message = message.replace("dt must", "T must")
        if "n_steps" in change:
            message = "n_fine must be >= 1"
        assert rc == 1 and message in msg, (change, rc, msg)


def test_bridge_levels_of_a_book():
    for name, book in list(BOOKS.items()) + [("stat", STAT_BOOK), ("five-of-four", FIVE_LEVELS[:5]), ("none", [EURO(100.0), LOOK])]:
        want, _ = bridge_plan_python(book)
        assert mc.mlmc_bridge_levels(book) == want, name
    assert [len(bridge_plan_python(b)[0]) for b in BOOKS.values()] == [1, 2, 4]
    assert mc.mlmc_bridge_levels([out_put(85.0), out_put(85.0, True), out_put(85.0)]) == [(85.0, False), (85.0, True)]
    assert mc.mlmc_bridge_levels([out_put(0.0), out_put(-0.0)]) == []                # the EURO idiom, either zero
    for bad, word in ((FIVE_LEVELS, "more than 4"), ([out_put(-1.0)], "bridge level"), ([out_put(0.0, True)], "bridge level"),
                      ([out_put(float("nan"))], "barrier must be finite"), ([(10, True, 1.0, 1.0, 0.0)], "kind must be in [0, 9]"), ([], "n_contracts")):
        with pytest.raises(mc.McgError, match=word.replace("[", r"\[").replace("]", r"\]")) as e:
            mc.mlmc_bridge_levels(bad)
        assert e.value.status == 1
    L = mc.load_library()
    arr, b, up, n = mc.engine.make_book([out_put(85.0)]), np.zeros(4), (C.c_int * 4)(), C.c_int(-1)
    dp = C.POINTER(C.c_double)
    assert L.mcg_mlmc_bridge_levels(None, 1, b.ctypes.data_as(dp), up, C.byref(n)) == 1 and b"NULL" in L.mcg_last_error()
    assert L.mcg_mlmc_bridge_levels(arr, 1, None, up, C.byref(n)) == 1 and L.mcg_mlmc_bridge_levels(arr, 1, b.ctypes.data_as(dp), up, None) == 1
    assert L.mcg_mlmc_bridge_levels(arr, 1, b.ctypes.data_as(dp), up, C.byref(n)) == 0 and n.value == 1 and b[0] == 85.0 and up[0] == 0


def test_parity_cases_are_well_conditioned():
    """In no restated parity case of tests/test_gpu_mlmc_bridge.py does a row's X, or a coarse midpoint, lie within 1e-9 of an h:
    a last-bit difference on the GPU cannot flip a safe decision.  The cases cover what the GPU file's docstring lists."""
    closest, n_cases = math.inf, 0
    seen = {k: set() for k in ("n_fine_coarse", "n_fine_plain", "counts", "begins", "schemes", "books")}
    inner = 0
    for name, rows in CASES.items():
        for case in rows:
            st, sv, near = reference(name, case)
            assert np.isfinite(st).all() and (st > 0.0).all() and ((sv >= 0.0) & (sv <= 1.0)).all()
            closest = min(closest, near)
            inner += int(((sv > 0.0) & (sv < 1.0)).sum())
            n_cases += 1
            n_fine, coarse, n_paths, begin, seed, scheme, book = case
            seen["n_fine_coarse" if coarse else "n_fine_plain"].add(n_fine)
            seen["counts"].add(n_paths), seen["begins"].add(begin), seen["schemes"].add(scheme), seen["books"].add(book)
    print(f"{n_cases} parity cases: the row closest to a level lies {closest:.2e} from it; {inner} probabilities strictly inside (0, 1)")
    assert closest > 1e-9 and inner > 10_000
    assert seen["n_fine_coarse"] == {2, 4, 6, 8, 10, 12, 14, 252} and seen["n_fine_plain"] == {1, 2, 3, 4, 5, 7}
    assert seen["counts"] == {1, 257, 513, 1000, 1300} and seen["begins"] == {0, 12345, 2 ** 33 + 1, 777}
    assert seen["schemes"] == {0, 1} and seen["books"] == set(BOOKS)


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/mlmc_bridge_host_main.cpp with host/mlmc.cpp, compiled with -fsanitize=address,undefined into a stand-alone
    program (the sanitizers' runtimes linked into it) and run directly; it must exit 0 with nothing reported."""
    exe = tmp_path / "mlmc_bridge_host_main"
    host = os.path.join(ROOT, "montecarlooptionspricer_amd", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "cpp", "mlmc_bridge_host_main.cpp"),
           os.path.join(host, "mlmc.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-3000:]
