"""The numpy restatement of the Sobol' generators, written from the words of include/mcgpu.h (the section on randomised
quasi-Monte Carlo) and calling no function of the library: the direction numbers from Joe and Kuo's polynomials, the SplitMix64
stream, the linear matrix scramble and the shift, the points, Phi^-1 (AS241), the bridge schedule, the walk, and the GBM and
local-volatility steps.  tests/test_sobol_reference.py checks the library's host functions and this file against each other and
against scipy; tests/test_gpu_sobol.py measures the kernels against it.

Arithmetic: binary64 with no fused multiply-add (numpy has none); the kernels use fma in the Horner sums, the bridge and the
exponents, which is where the last-bit differences that the GPU tests bound come from.
"""
import functools
import math
import os

import numpy as np

MAX_DIMS = 1024
PLAIN, SHIFT, LMS_SHIFT = 0, 1, 2
MASK64 = (1 << 64) - 1


# ---- direction numbers ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def joe_kuo():
    """(poly, vinit) of new-joe-kuo-6 as scipy ships them: poly with its leading and trailing coefficients, vinit = m_1 .. m_s."""
    import scipy.stats
    z = np.load(os.path.join(os.path.dirname(scipy.stats.__file__), "_sobol_direction_numbers.npz"))
    return z["poly"][:MAX_DIMS].astype(np.int64), z["vinit"][:MAX_DIMS].astype(np.int64)


@functools.lru_cache(maxsize=None)
def direction_numbers(n_dims):
    """V [n_dims][32] uint32, leading digit in bit 31: m_j = 2 a_1 m_{j-1} ^ 4 a_2 m_{j-2} ^ ... ^ 2^s m_{j-s} ^ m_{j-s}."""
    poly, vinit = joe_kuo()
    V = np.zeros((n_dims, 32), dtype=np.uint32)
    for d in range(n_dims):
        p = int(poly[d])
        s = p.bit_length() - 1
        if s == 0:
            m = [1] * 32
        else:
            m = [int(x) for x in vinit[d, :s]]
            for j in range(s, 32):
                x = m[j - s] ^ (m[j - s] << s)
                for k in range(1, s):
                    if (p >> (s - k)) & 1:
                        x ^= m[j - k] << k
                m.append(x)
        V[d] = [m[j] << (31 - j) for j in range(32)]
    V.setflags(write=False)
    return V


# ---- the scramble -------------------------------------------------------------------------------------------------------------
class SplitMix64:
    def __init__(self, state):
        self.s = state & MASK64

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & MASK64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
        return z ^ (z >> 31)

    def word(self):
        return self.next() >> 32


def splitmix_hash(x):
    return SplitMix64(x).next()


def parity32(x):
    x = x ^ (x >> np.uint32(16))
    x = x ^ (x >> np.uint32(8))
    x = x ^ (x >> np.uint32(4))
    x = x ^ (x >> np.uint32(2))
    x = x ^ (x >> np.uint32(1))
    return x & np.uint32(1)


@functools.lru_cache(maxsize=64)
def table(seed, replicate, scramble, n_dims):
    """(V', shift): [n_dims][32] and [n_dims] uint32."""
    V = direction_numbers(n_dims).copy()
    shift = np.zeros(n_dims, dtype=np.uint32)
    if scramble != PLAIN:
        rng = SplitMix64(splitmix_hash(splitmix_hash(seed) ^ replicate))
        bit = np.uint32(31) - np.arange(32, dtype=np.uint32)      # the bit that M_j decides
        for d in range(n_dims):
            shift[d] = rng.word()
            w = np.array([rng.word() for _ in range(32)], dtype=np.uint32)
            if scramble == LMS_SHIFT:
                M = ((w >> bit) | np.uint32(1)) << bit
                V[d] = (parity32(M[None, :] & V[d][:, None]) << bit[None, :]).sum(axis=1, dtype=np.uint32)   # (distinct bits: sum = or)
    V.setflags(write=False)
    shift.setflags(write=False)
    return V, shift


def points(V, shift, path_begin, n_paths):
    """x [n_dims][n_paths] uint32: coordinate d of the points path_begin .. path_begin + n_paths - 1."""
    i = (np.uint64(path_begin) + np.arange(n_paths, dtype=np.uint64)).astype(np.uint32)     # (ids are below 2^32)
    g = i ^ (i >> np.uint32(1))
    x = np.repeat(shift[:, None], n_paths, axis=1)
    for b in range(32):
        on = ((g >> np.uint32(b)) & np.uint32(1)).astype(bool)
        if on.any():
            x[:, on] ^= V[:, b][:, None]
    return x


def gray_codes(path_begin, n_paths):
    """The Gray codes g = id ^ (id >> 1) of the ids path_begin .. path_begin + n_paths - 1, as Python ints."""
    return [i ^ (i >> 1) for i in range(path_begin, path_begin + n_paths)]


def gray_bits(path_begin, n_paths):
    """The bits that are set in the Gray code of some id of the window and clear in another's: the direction numbers V[d][b]
    that tell the window's points apart."""
    g = gray_codes(path_begin, n_paths)
    some, every = functools.reduce(int.__or__, g, 0), functools.reduce(int.__and__, g, (1 << 32) - 1)
    return {b for b in range(32) if ((some & ~every) >> b) & 1}


def n_bits(path_begin, n_paths):
    """The smallest k with every id of the window below 2^k: 0 for the single id 0, 32 from 2^31 on."""
    return (path_begin + n_paths - 1).bit_length()


# ---- the normal: AS241 (PPND16) -----------------------------------------------------------------------------------------------
A = (3.3871328727963666080e+0, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
     4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3)
B = (1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3, 2.1213794301586595867e+4,
     3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3)
C = (1.42343711074968357734e+0, 4.63033784615654529590e+0, 5.76949722146069140550e+0, 3.64784832476320460504e+0,
     1.27045825245236838258e+0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4)
D = (1.0, 2.05319162663775882187e+0, 1.67638483018380384940e+0, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
     1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9)
SPLIT = 0.425


def horner(c, r):
    y = np.full_like(r, c[-1])
    for k in c[-2::-1]:
        y = y * r + k
    return y


def normal(x):
    """z = Phi^-1((x + 1/2) 2^-32) of uint32 coordinates x."""
    u = (np.asarray(x, dtype=np.uint32).astype(np.float64) + 0.5) * 2.0 ** -32
    q = u - 0.5
    z = np.empty_like(u)
    mid = np.abs(q) <= SPLIT
    r = 0.180625 - q[mid] * q[mid]
    z[mid] = q[mid] * horner(A, r) / horner(B, r)
    qt, ut = q[~mid], u[~mid]
    r = np.sqrt(-np.log(np.where(qt < 0.0, ut, 1.0 - ut))) - 1.6
    t = horner(C, r) / horner(D, r)
    z[~mid] = np.where(qt < 0.0, -t, t)
    return z


# ---- the bridge ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bridge_schedule(n, bridge=True):
    """The schedule in dimension order: a list of (t, l, r, wl, wr, sd)."""
    if not bridge:
        return [(d + 1, d, d, 1.0, 0.0, 1.0) for d in range(n)]
    out = [(n, 0, 0, 0.0, 0.0, math.sqrt(float(n)))]
    level = [(0, n)]
    while level:
        nxt = []
        for l, r in level:
            if r - l < 2:
                continue
            m = (l + r) // 2
            w = float(r - l)
            out.append((m, l, r, float(r - m) / w, float(m - l) / w, math.sqrt(float(m - l) * float(r - m) / w)))
            nxt += [(l, m), (m, r)]
        level = nxt
    return out


def increments(z, bridge=True):
    """dz [n][n_paths], the increments of the steps in units of sqrt(dt), from the normals z [n][n_paths] of the dimensions.
    The values B(t) do not depend on the order in which the nodes are visited, so dimension order serves."""
    n = z.shape[0]
    if not bridge:
        return z
    Bt = np.zeros((n + 1,) + z.shape[1:])
    for d, (t, l, r, wl, wr, sd) in enumerate(bridge_schedule(n, True)):
        Bt[t] = wl * Bt[l] + (wr * Bt[r] + sd * z[d])
    return Bt[1:] - Bt[:-1]


def bridge_matrix(n, bridge=True):
    """Q [n][n]: increments = Q z."""
    return increments(np.eye(n), bridge)


# ---- the generators -------------------------------------------------------------------------------------------------------------
def sobol_increments(seed, replicate, scramble, bridge, n_steps, n_paths, path_begin=0):
    V, shift = table(seed, replicate, scramble, n_steps)
    return increments(normal(points(V, shift, path_begin, n_paths)), bridge)


def gbm_sobol_numpy(seed, replicate, scramble, bridge, S0, r, sigma, dt, n_steps, n_paths, path_begin=0):
    """Step-major [n_steps + 1][n_paths]: S_{t+1} = S_t exp(m + s z_t)."""
    dz = sobol_increments(seed, replicate, scramble, bridge, n_steps, n_paths, path_begin)
    m, s = (r - 0.5 * sigma * sigma) * dt, sigma * math.sqrt(dt)
    out = np.empty((n_steps + 1, n_paths))
    out[0] = S0
    for t in range(n_steps):
        out[t + 1] = out[t] * np.exp(s * dz[t] + m)
    return out


def localvol_table(times, n_x, sigma, dt, n_steps):
    """The table of include/mcgpu.h (mcg_localvol_table), [n_slices][n_x - 1][2] = {a_j, a_{j+1} - a_j}."""
    times = [float(t) for t in times]
    n_slices = 1 if len(times) == 1 else n_steps
    sq = math.sqrt(dt)
    out = np.empty((n_slices, n_x - 1, 2))
    for n in range(n_slices):
        t = float(n) * dt
        if t <= times[0]:
            row = [float(s) for s in sigma[0]]
        elif t >= times[-1]:
            row = [float(s) for s in sigma[-1]]
        else:
            i = 0
            while not t < times[i + 1]:
                i += 1
            g = (t - times[i]) / (times[i + 1] - times[i])
            row = [float(sigma[i][j]) + g * (float(sigma[i + 1][j]) - float(sigma[i][j])) for j in range(n_x)]
        a = [row[j] * sq for j in range(n_x)]
        for j in range(n_x - 1):
            out[n, j] = (a[j], a[j + 1] - a[j])
    return out


def localvol_sobol_numpy(seed, replicate, scramble, bridge, S0, r, surface, dt, n_steps, n_paths, path_begin=0, q=0.0):
    """Step-major [n_steps + 1][n_paths]: the step of mcg_paths_localvol with z = z_t."""
    dz = sobol_increments(seed, replicate, scramble, bridge, n_steps, n_paths, path_begin)
    n_x = surface.n_x
    tab = localvol_table(surface.times, n_x, surface.sigma, dt, n_steps)
    inv_dx = float(n_x - 1) / (surface.x_max - surface.x_min)
    u0 = -surface.x_min * inv_dx
    m = (r - q) * dt
    S, X = np.full(n_paths, float(S0)), np.zeros(n_paths)
    out = np.empty((n_steps + 1, n_paths))
    out[0] = S
    for t in range(n_steps):
        u = np.minimum(np.maximum(X * inv_dx + u0, 0.0), float(n_x - 1))
        j = np.minimum(u.astype(np.int64), n_x - 2)
        f = u - j
        sl = tab[t if len(tab) > 1 else 0]
        a = f * sl[j, 1] + sl[j, 0]
        e = a * dz[t] + (-0.5 * a * a + m)
        X = X + e
        S = S * np.exp(e)
        out[t + 1] = S
    return out


# ---- the randomised quasi-Monte Carlo case of the README (GBM, S0 = K = 100, r = 0.05, sigma = 0.2, T = 1) ------------------------
RQMC = dict(S0=100.0, K=100.0, r=0.05, sigma=0.2, T=1.0, n_steps=64, n_paths=1 << 14, replicates=16, seed=20261020)
IID_STD_ERR = {"european": 0.115, "asian": 0.0621}    # of a numpy normal sample of the same N (the issue's baseline)


def rqmc_prices(scramble, bridge, replicate, case=RQMC):
    """(European call, arithmetic Asian call over rows 1 .. n) of one replicate of the README's case."""
    n = case["n_steps"]
    M = gbm_sobol_numpy(case["seed"], replicate, scramble, bridge, case["S0"], case["r"], case["sigma"], case["T"] / n, n, case["n_paths"])
    disc = math.exp(-case["r"] * case["T"])
    return (disc * np.maximum(M[-1] - case["K"], 0.0).mean(), disc * np.maximum(M[1:].mean(axis=0) - case["K"], 0.0).mean())


def black_scholes_call(S0, K, r, sigma, T):
    Nc = lambda x: 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))  # noqa: E731
    d1 = (math.log(S0 / K) + (r + 0.5 * sigma * sigma) * T) / (sigma * math.sqrt(T))
    return S0 * Nc(d1) - K * math.exp(-r * T) * Nc(d1 - sigma * math.sqrt(T))


# What tests/test_sobol_reference.py measured on this restatement for the matrix scramble + shift + bridge (it asserts that these
# still hold): the standard deviation across the 16 replicates of the European and of the Asian call.  tests/test_gpu_sobol.py
# forms the variance ratios it compares the GPU's with from these.
RQMC_LMS_BRIDGE_STD = {"european": 0.000464, "asian": 0.00104}

# The local-volatility statistic: a CEV call (beta = 1/2, sigma0 = 0.2) at K = 100 by 16 replicates of 2^14 x 64 against the
# noncentral chi-square closed form, within 4 replicate standard errors (about 3e-5 here).  At that resolution the scheme's own
# biases show, so the case keeps them below the error bar: the closed form prices the exact CEV model, the generator its
# bilinear interpolant on the surface's nodes (volatility too high by dx^2 / 32 relative) in log-Euler steps.  With 64 nodes on
# [-1.5, 1.5] and T = 1 the restatement is off by 8.9e-4 = 11 standard errors, with 128 nodes on [-1, 1] still by 5.7e-4 = 7 (the
# steps); with T = 1/4 (steps of about a trading day) and 128 nodes on [-0.5, 0.5] (five standard deviations of ln S_T) by
# 5.8e-5 = 2.0.
CEV_STAT = dict(S0=100.0, K=100.0, r=0.04, q=0.01, T=0.25, sigma0=0.2, beta=0.5, x_max=0.5, n_x=128, n_steps=64, n_paths=1 << 14,
                replicates=16, seed=20261020)
