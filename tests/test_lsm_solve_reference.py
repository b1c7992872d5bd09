"""Cases and high-precision references for the regression solves of the LSM sweeps (csrc/lsm_device.hpp): lsm_solve_nb (the
first pass: equilibrated LDL^T on the Hankel moment matrix, and the trust decision that asks for a re-fit), lsm_solve_centered
(the re-fit: Eigen's truncated SVD on raw monomials by two Jacobi iterations), lsm_rcp / lsm_rsqrt and lsm_continuation.  Runs
on the CPU; tests/test_gpu_lsm_solve.py imports the cases and the references and runs the device code on them.

A case starts from samples (S_i, b_i) and a strike K.  x = S/K - 1 (about its mean mu for the centred solve); the moments are
formed in 60-digit arithmetic and rounded ONCE to binary64: those binary64 moments are the input of the device, of the numpy
restatement and of the reference alike, so what is measured is the solve and not the summation.

References.
  fast path   the exact solution (60 digits) of the Hankel system of the binary64 moments, with kappa = lambda_max / lambda_min
              of the equilibrated matrix and the exact pivots of its LDL^T.  Error of a coefficient vector: p(x) = sum coef[t] x^t
              on up to 50 of the samples against the exact solution's values there, largest absolute difference over largest
              absolute exact value.
  centred     Eigen's rule in exact arithmetic (_exact_eigen_rule_fit, which tests/test_oracle_models.py imports from here): the
              fitted values at the samples; error = largest absolute difference over largest absolute exact fitted value.

Decisions.  Every case is moved (its seed advanced, and for the fast path its spread narrowed by 1.5% a move: the pivots of
5000 samples hardly depend on the seed) until no decision it takes depends on rounding, all in 60 digits: every exact
pivot the factorisation reads is a factor 2 away from 1e-10 and from 1e-6 (after the first pivot <= 1e-10 the device computes on
a stand-in and reads no further pivot, so none is asked of those), est is a factor 2 away from 1e4 nb eps, and every singular
value of a centred case's raw design is a factor 10 away from min(rows, cols) eps sigma_max.  Where the variance behind est is
pure cancellation (spreads <= 1e-6) est itself is rounding noise in binary64; there a pivot below 1e-6 must decide, and the test
asks for that.

Trusted sizes.  The wide spreads (0.5) are there to find trusted cases at nb = 8, 9.  None does: with prices of order 1 (so that
est does not refuse) and samples crowding at the strike the smallest pivot reaches 2e-6 at nb = 7 and stays below 2e-7 at nb = 8,
3e-9 at nb = 9.  So nb 1..7 have trusted cases and nb = 8, 9 are tested for their decisions (and their provisional
coefficients) only; test_trusted_sizes prints the count per nb and asserts this.

The threshold mutation (min(count, nb) -> nb in lsm_solve_centered) cannot flip a decision on a case that keeps every singular
value a factor 10 from the threshold: nb <= 16 and a second singular value needs count >= 2, so the two thresholds differ by a
factor 8 at most.  It is caught by probe_threshold(), two prices a few ulp apart at nb = 16 whose second singular value lies
between 2 eps sigma_max and 16 eps sigma_max, a factor >= 2 from both (not the factor 10 of the regular cases, which is why it
is a labelled extra case); tests/test_gpu_lsm_solve.py sends it to the device as well."""
import functools
import math

import mpmath as mp
import numpy as np
import pytest

EPS = 2.0 ** -52
DPS = 60
MAX_NB, C_COUNT, C_CENTER, C_REFINE, C_HINT, COEF_STRIDE = 16, 16, 17, 18, 19, 24       # lsm_device.hpp: LSM_C_*
FN_NB, FN_NB_TAN, FN_ONE, FN_CENTRED, FN_CENTRED_TAN, FN_RCP_RSQRT, FN_CONTINUATION = range(7)    # mcg_debug_lsm_solve
FAST_NB = range(1, 10)
CENTRED_NB = range(1, 17)
N_EVAL = 50               # samples the fast path's error is evaluated on
SKIP_ABOVE = 1e-3         # 8 eps kappa above this: provisional coefficients of an untrusted date, accuracy not asked


# ---- Eigen's rule in exact arithmetic (moved here from tests/test_oracle_models.py) -----------------------------------------
def _exact_eigen_rule(S, bs, p):
    """Eigen's bdcSvd().solve(b) on raw monomials of S (LSMPricer.cpp:61-76) in 60-digit arithmetic: minimum-norm least
    squares with singular values <= min(rows, cols) eps sigma_max dropped.  bs: right-hand sides.  Returns the fitted values at
    the data per right-hand side, and sigma / sigma_max of the design."""
    mp.mp.dps = 60
    n = len(S)
    A = mp.matrix(n, p + 1)
    for i in range(n):
        for k in range(p + 1):
            A[i, k] = mp.mpf(float(S[i])) ** k
    U, sv, V = mp.svd_r(A, full_matrices=False, compute_uv=True)
    thr = min(n, p + 1) * mp.mpf(np.finfo(float).eps) * sv[0]
    fits = []
    for b in bs:
        coef = mp.matrix(p + 1, 1)
        for j in range(len(sv)):
            if sv[j] > thr:
                proj = sum(U[i, j] * mp.mpf(float(b[i])) for i in range(n)) / sv[j]
                for t in range(p + 1):
                    coef[t] += proj * V[j, t]
        fit = A * coef
        fits.append(np.array([float(fit[i]) for i in range(n)]))
    return fits, [float(sv[j] / sv[0]) for j in range(len(sv))]


def _exact_eigen_rule_fit(S, b, p):
    """The fitted values at the data of Eigen's rule in 60-digit arithmetic (see _exact_eigen_rule)."""
    return _exact_eigen_rule(S, [b], p)[0][0]


# ---- samples and moments -------------------------------------------------------------------------------------------------------
def samples(seed, n, base, spread, K, distinct=None, power=1.0):
    """n prices about `base` with relative spread `spread` (all on one side of K), `distinct` of them different when given;
    power > 1 makes them denser towards the upper end (in-the-money puts of a diffusion crowd at the strike).  Right-hand
    sides b (a discounted option value: the payoff bent and noisy) and b2 (a tangent: mixed signs)."""
    rs = np.random.RandomState(seed)
    m = n if distinct is None else distinct
    pool = base * (1.0 + spread * (1.0 - 2.0 * rs.uniform(0.0, 1.0, m) ** power))
    S = pool if distinct is None else pool[np.concatenate([np.arange(m), rs.randint(0, m, n - m)])]
    assert (S < K).all() or (S > K).all()
    b = np.abs(K - S) * (1.0 + 0.1 * rs.uniform(-1.0, 1.0, n)) + 0.02 * K * rs.uniform(0.0, 1.0, n)
    b2 = rs.uniform(-1.0, 1.0, n)
    return S, b, b2


def mp_x(S, K, mu=0.0):
    return [mp.mpf(float(s)) / mp.mpf(float(K)) - 1 - mp.mpf(float(mu)) for s in S]


def mp_moments(x, b, b2, nb):
    """The 4 nb - 1 moments of lsm_sums (power sums, cross sums with b, cross sums with b2), each rounded once to binary64."""
    n_p = 2 * nb - 1
    m = [mp.mpf(0)] * (4 * nb - 1)
    for xi, bi, ci in zip(x, b, b2):
        pw, bi, ci = mp.mpf(1), mp.mpf(float(bi)), mp.mpf(float(ci))
        for t in range(n_p):
            m[t] += pw
            if t < nb:
                m[n_p + t] += pw * bi
                m[n_p + nb + t] += pw * ci
            pw *= xi
    return np.array([float(v) for v in m])


def as_tangent_rhs(m4, nb):
    """The 3 nb - 1 moments whose right-hand side is the tangent's cross sums."""
    return np.concatenate([m4[:2 * nb - 1], m4[3 * nb - 1:4 * nb - 1]])


# ---- the fast path's exact reference -------------------------------------------------------------------------------------------
def est_threshold(nb):
    return 1e4 * nb * 2.220446049250313e-16


def analyse_fast(m, nb, min_count, K):
    """What lsm_solve_nb<nb> must decide on the binary64 moments m (60 digits), and the exact solutions where it factorises."""
    count = float(m[0])
    a = dict(zero=not (count >= min_count and count > 0.0), refine=False, hint=0.0, ok=False, trusted=False, pivots=[], est=None,
             kappa=math.inf, exact=None, exact2=None, distance_ok=True, noise_decided=True, pivots_trusted=False)
    if a["zero"]:
        return a
    M = [mp.mpf(float(v)) for v in m]
    d = [1 / mp.sqrt(M[2 * i]) if M[2 * i] > 0 else mp.mpf(0) for i in range(nb)]
    G = mp.matrix(nb, nb)
    for i in range(nb):
        for j in range(nb):
            G[i, j] = M[i + j] * d[i] * d[j]
    L, piv, ok = mp.eye(nb), [], True
    for j in range(nb):
        dj = G[j, j] - sum(L[j, k] ** 2 * piv[k] for k in range(j))
        piv.append(dj)
        if not dj > mp.mpf("1e-10"):
            ok = False
            break                  # the device goes on with a stand-in pivot and reads no later one
        for i in range(j + 1, nb):
            L[i, j] = (G[i, j] - sum(L[i, k] * L[j, k] * piv[k] for k in range(j))) / dj
    a["ok"], a["pivots"] = ok, [float(p) for p in piv]
    for p in piv:
        for bar in ("1e-10", "1e-6"):
            if mp.mpf(bar) / 2 <= p <= mp.mpf(bar) * 2:
                a["distance_ok"] = False
    piv_ok = ok and min(piv) > mp.mpf("1e-6")
    a["pivots_trusted"] = piv_ok
    trusted = ok
    if nb > 1 and K > 0.0:
        mean_x = M[1] / M[0]
        second = M[2] / M[0]
        var_x = max(second - mean_x ** 2, mp.mpf(0))
        scale = max(abs(mp.mpf(float(K)) * (1 + mean_x)), mp.mpf(1))
        est = (mp.mpf(float(K)) * mp.sqrt(var_x) / scale ** 2) ** (nb - 1)
        thr = mp.mpf(est_threshold(nb))
        a["est"] = float(est)
        if var_x < mp.mpf("1e-10") * second:        # binary64 keeps < 6 digits of it: est must not be what decides
            a["noise_decided"] = not piv_ok
        elif thr / 2 <= est <= thr * 2:
            a["distance_ok"] = False
        trusted = piv_ok and est > thr
        a["refine"] = not trusted
        a["hint"] = float(mean_x) if a["refine"] else 0.0
    a["trusted"] = trusted and piv_ok
    if ok:
        ev = mp.eigsy(G, eigvals_only=True)
        lo, hi = min(ev), max(ev)
        a["kappa"] = float(hi / lo) if lo > 0 else math.inf
        n_p = 2 * nb - 1
        for key, off in (("exact", n_p), ("exact2", n_p + nb)):
            if len(M) >= off + nb:
                rhs = mp.matrix([M[off + i] * d[i] for i in range(nb)])
                s = mp.lu_solve(G, rhs)
                a[key] = [s[i] * d[i] for i in range(nb)]
    return a


def mp_poly(c, x):
    v = mp.mpf(0)
    for t in range(len(c) - 1, -1, -1):
        v = v * x + (c[t] if isinstance(c[t], mp.mpf) else mp.mpf(float(c[t])))
    return v


def poly_error(coef, exact, xs):
    """Largest |p_coef(x) - p_exact(x)| over the points over the largest |p_exact(x)| (60 digits)."""
    with mp.workdps(DPS):
        want = [mp_poly(exact, x) for x in xs]
        diff = max(abs(mp_poly(list(coef), x) - w) for x, w in zip(xs, want))
        top = max(abs(w) for w in want)
        return float(diff / top) if top > 0 else float(diff)


def fitted_error(coef, mu, c):
    """Centred solve: fitted values sum coef[t] y^t at the case's samples against Eigen's rule in exact arithmetic."""
    with mp.workdps(DPS):
        ys = mp_x(c["S"], c["K"], mu)
        nb = c["nb"]
        out = []
        for block, want in ((coef[:nb], c["fit"]),):
            diff = max(abs(mp_poly(list(block), y) - mp.mpf(float(w))) for y, w in zip(ys, want))
            out.append(float(diff / max(abs(w) for w in want)))
        return out[0]


# ---- the cases -----------------------------------------------------------------------------------------------------------------
K0 = 100.0
MAX_MOVES = 60


def _fast_specs(nb):
    """(name, count, base, spread, distinct, min_count, K given to the solve[, K of the samples, power of their density])"""
    put, call = 60.0, 150.0
    specs = [
        # prices of order 1: est is not what refuses the fast path there, so these are the sets that can be trusted at nb >= 6
        ("put-0.5-unit", 40, 0.66, 0.5, None, 1, 1.0, 1.0, 1.0), ("put-0.5-unit-near", 40, 0.66, 0.5, None, 1, 1.0, 1.0, 2.0),
        ("put-0.5-unit-near-5000", 5000, 0.665, 0.5, None, 1, 1.0, 1.0, 3.0), ("call-0.5-unit", 40, 2.1, 0.5, None, 1, 1.0, 1.0, 1.0),
        ("K-negative-wide", 40, 0.66, 0.5, None, 1, -1.0, 1.0, 2.0),
        ("put-0.5-unit-nearer", 40, 0.665, 0.5, None, 1, 1.0, 1.0, 3.0), ("put-0.5-unit-nearer-400", 400, 0.665, 0.5, None, nb, 1.0, 1.0, 3.0),
        ("put-0.5-unit-nearer-2000", 2000, 0.665, 0.5, None, 1, 1.0, 1.0, 3.5), ("put-0.5-unit-near-1000", 1000, 0.665, 0.5, None, 1, 1.0, 1.0, 2.5),
        ("put-0.5", 40, put, 0.5, None, 1, K0), ("put-0.3", 40, 70.0, 0.3, None, 1, K0), ("put-0.1", 40, 85.0, 0.1, None, 1, K0),
        ("call-0.3", 40, call, 0.3, None, 1, K0), ("call-0.5", 40, 210.0, 0.5, None, 1, K0),
        ("put-0.3-5000", 5000, 70.0, 0.3, None, 1, K0), ("put-0.5-5000", 5000, put, 0.5, None, nb, K0),
        ("put-1e-2", 40, 90.0, 1e-2, None, 1, K0), ("call-1e-4", 40, 110.0, 1e-4, None, 1, K0), ("put-1e-6", 40, 90.0, 1e-6, None, 1, K0),
        ("put-1e-8", 40, 90.0, 1e-8, None, nb, K0),
        ("atm-put-1e-2", 40, 99.0, 1e-2, None, 1, K0),        # x in (-0.02, 0): well-conditioned pivots at a small est
        ("atm-put-1e-4", 40, 99.98, 1e-4, None, 1, K0),       # ... at nb >= 3 est alone refuses the fast path
        ("put-1e-3", 40, 90.0, 1e-3, None, 1, K0),            # a pivot between 1e-10 and 1e-6 at nb = 3: provisional coefficients
        ("count-nb", nb, 70.0, 0.3, None, nb, K0), ("count-nb+1", nb + 1, 70.0, 0.3, None, 1, K0),
        ("single", 1, 90.0, 0.0, None, 1, K0),
        ("count-0", 0, 90.0, 0.0, None, 1, K0),               # count < min_count = 1
        ("K-zero", 40, 70.0, 0.3, None, 1, 0.0), ("K-negative", 40, 85.0, 0.1, None, 1, -K0),
        ("K-zero-dup", 40, 70.0, 0.3, max(nb - 1, 1), 1, 0.0),
    ]
    if nb >= 2:
        specs += [("count-nb-1", nb - 1, 70.0, 0.3, None, 1, K0), ("too-few", nb - 1, 70.0, 0.3, None, nb, K0),
                  ("duplicates", 40, 70.0, 0.3, nb - 1, nb, K0), ("call-duplicates", 12, call, 0.1, max(nb // 2, 1), 1, K0)]
    return specs


def _prescreen(S, K, nb):
    """False where a cheap extended-precision look at a large sample set already shows a decision too close to its bar: spares
    the 60-digit moments of a move that would be rejected anyway (what is accepted is still decided in 60 digits)."""
    x = np.asarray(S, dtype=np.longdouble) / np.longdouble(K) - np.longdouble(1.0)
    m = [np.sum(x ** t) for t in range(2 * nb - 1)]
    d = [1.0 / np.sqrt(m[2 * a]) for a in range(nb)]
    G = [[m[a + b] * d[a] * d[b] for b in range(nb)] for a in range(nb)]
    L, piv = [[0.0] * nb for _ in range(nb)], []
    for j in range(nb):
        dj = G[j][j] - sum(L[j][k] ** 2 * piv[k] for k in range(j))
        piv.append(dj)
        if any(bar / 2.5 <= dj <= bar * 2.5 for bar in (1e-10, 1e-6)):
            return False
        if not dj > 1e-10:
            break
        for i in range(j + 1, nb):
            L[i][j] = (G[i][j] - sum(L[i][k] * L[j][k] * piv[k] for k in range(j))) / dj
    return True


@functools.lru_cache(maxsize=None)
def fast_cases(nb):
    """The fast path's cases at one basis size, each moved until its decisions are a factor 2 from every bar."""
    out = []
    with mp.workdps(DPS):
        for i, spec in enumerate(_fast_specs(nb)):
            name, n, base, spread, distinct, min_count, Kp = spec[:7]
            K, power = spec[7:] if len(spec) > 7 else (K0, 1.0)
            for move in range(MAX_MOVES):
                seed = 1000 * nb + 10 * i + 100000 * move
                if n == 0:
                    S, b, b2 = np.zeros(0), np.zeros(0), np.zeros(0)
                else:
                    S, b, b2 = samples(seed, n, base, spread * 0.985 ** move, K, distinct, power)
                if n >= 1000 and move < MAX_MOVES - 1 and not _prescreen(S, K, nb):
                    continue
                x = mp_x(S, K)
                m = mp_moments(x, b, b2, nb)
                a = analyse_fast(m, nb, float(min_count), Kp)
                if (a["distance_ok"] and a["noise_decided"]) or n <= 1:
                    break
            c = dict(id=f"nb{nb}-{name}", nb=nb, name=name, S=S, b=b, b2=b2, K=K, K_param=Kp, min_count=float(min_count),
                     spread=spread, moments=m, x=x[:N_EVAL], moves=move, **a)
            out.append(c)
    return out


def _centred_specs(nb):
    """(name, count, base, spread, distinct)"""
    many = 40 if nb <= 9 else nb + 1
    specs = [("put-0.3", nb + 1, 70.0, 0.3, None), ("put-1e-2", many, 90.0, 1e-2, None), ("call-1e-4", nb, 110.0, 1e-4, None),
             ("put-1e-6", nb + 1, 90.0, 1e-6, None), ("put-1e-8", many, 90.0, 1e-8, None), ("single", 1, 90.0, 0.0, None),
             ("duplicates-1e-2", nb + 2, 90.0, 1e-2, max(nb // 2, 1)), ("duplicates-1e-6", nb + 2, 90.0, 1e-6, max(nb - 1, 1))]
    if nb >= 2:
        specs += [("count-nb-1-1e-4", nb - 1, 90.0, 1e-4, None), ("count-nb-1-0.3", nb - 1, 70.0, 0.3, None)]
    # The error of ANY binary64 solve on a near-degenerate date varies by more than a factor 10 with the sample set (it is
    # rounding noise amplified by the conditioning), so a group's recorded error -- which the device's bound is taken from --
    # is the largest over several sets per group, not that of one or two.
    specs += [(f"{name}-{rep}", n, base, spread, distinct) for rep in ("b", "c") for name, n, base, spread, distinct in list(specs)
              if 0.0 < spread <= 1e-2]
    return specs


def spread_decade(spread):
    return 0 if spread <= 0.0 else int(math.floor(math.log10(spread) + 1e-9))


@functools.lru_cache(maxsize=None)
def centred_cases(nb):
    """The centred solve's cases at one basis size, each moved until every singular value of its raw design is a factor 10
    from Eigen's threshold."""
    out = []
    for i, (name, n, base, spread, distinct) in enumerate(_centred_specs(nb)):
        for move in range(MAX_MOVES):
            S, b, b2 = samples(2000 * nb + 10 * i + 100000 * move + 7, n, base, spread * 0.93 ** move, K0, distinct)
            (fit, fit2), sv = _exact_eigen_rule(S, [b, b2], nb - 1)
            thr = min(n, nb) * EPS
            if all(s > 10.0 * thr or s < thr / 10.0 for s in sv):
                break
        with mp.workdps(DPS):
            mu = float(sum(mp_x(S, K0)) / n)
            m = mp_moments(mp_x(S, K0, mu), b, b2, nb)
        out.append(dict(id=f"nb{nb}-centred-{name}", nb=nb, name=name, S=S, b=b, b2=b2, K=K0, mu=mu, spread=spread, moments=m,
                        fit=fit, fit2=fit2, sv=sv, threshold=thr, rank=sum(s > thr for s in sv), moves=move,
                        group=(nb, spread_decade(spread))))
    return out


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------
def solve_nb_numpy(m, nb, min_count, K, mutate=None):
    """lsm_solve_nb<nb> line for line in binary64, with true division and sqrt where the device takes lsm_rcp / lsm_rsqrt and
    no fused multiply-add.  Returns the 20 doubles of the coefficient block.  mutate: one of the deliberate errors of
    test_mutations_are_caught."""
    coef = np.zeros(20)
    count = float(m[0])
    coef[C_COUNT] = count
    if not (count >= min_count) or not (count > 0.0):
        return coef
    d = [1.0 / math.sqrt(m[2 * a]) if m[2 * a] > 0.0 else 0.0 for a in range(nb)]
    rhs = [m[2 * nb - 1 + a] * d[a] for a in range(nb)]
    if mutate == "equilibrate-once":
        G = [[m[a + b] * d[a] for b in range(nb)] for a in range(nb)]
    else:
        G = [[m[a + b] * d[a] * d[b] for b in range(nb)] for a in range(nb)]
    Q = [[0.0] * nb for _ in range(nb)]
    inv_piv = [0.0] * nb
    ok, piv_min = True, 1.0
    for j in range(nb):
        dj = G[j][j]
        for k in range(j):
            dj -= Q[j][k] * Q[j][k] * Q[k][k]
        good = dj > 1e-10
        if ok and good:
            piv_min = min(piv_min, dj)
        ok = ok and good
        Q[j][j] = dj
        inv = 1.0 / (dj if good else 1.0)
        inv_piv[j] = inv
        for i in range(j + 1, nb):
            v = G[i][j]
            for k in range(j):
                v -= Q[i][k] * Q[j][k] * Q[k][k]
            Q[i][j] = v * inv
    if nb > 1 and K > 0.0:
        inv_count = 1.0 / count
        mean_x = m[1] * inv_count
        var_x = max(m[2] * inv_count - mean_x * mean_x, 0.0)
        mean_s = K * (1.0 + mean_x)
        scale = max(abs(mean_s), 1.0)
        ratio = K * math.sqrt(var_x) / (scale * scale) if var_x > 0.0 else 0.0
        est = 1.0
        for _ in range(1, nb + 1 if mutate == "est-power-nb" else nb):
            est *= ratio
        bar = 1e-4 if mutate == "pivot-bar-1e-4" else 1e-6
        trusted = ok and piv_min > bar and est > 1e4 * nb * 2.220446049250313e-16
        if not trusted:
            coef[C_REFINE] = 1.0
            coef[C_HINT] = mean_x
    if ok:
        sol = [0.0] * nb
        for i in range(nb):
            v = rhs[i]
            for k in range(i):
                v -= Q[i][k] * sol[k]
            sol[i] = v
        for i in range(nb):
            sol[i] *= inv_piv[i]
        for i in range(nb - 1, -1, -1):
            v = sol[i]
            for k in range(i + 1, nb):
                v -= Q[k][i] * sol[k]
            sol[i] = v
        for a in range(nb):
            coef[a] = sol[a] * d[a]
    return coef


def solve_centred_numpy(mc, nb, mu, K, mutate=None, info=None):
    """lsm_solve_centered line for line in binary64 (plain products and sums in the device's order)."""
    coef = np.zeros(20)
    count = float(mc[0])
    coef[C_COUNT], coef[C_CENTER] = count, mu
    if not (count > 0.0):
        return coef
    sqrt = math.sqrt
    d = [1.0 / sqrt(mc[2 * a]) if mc[2 * a] > 0.0 else 0.0 for a in range(nb)]
    G = np.array([[mc[a + b] * d[a] * d[b] for b in range(nb)] for a in range(nb)], dtype=np.float64)
    Q = np.eye(nb)
    for _ in range(60):
        off = 0.0
        for p in range(nb):
            for q in range(p + 1, nb):
                off += G[p, q] * G[p, q]
        if off < 1e-60:
            break
        for p in range(nb - 1):
            for q in range(p + 1, nb):
                apq = float(G[p, q])
                if apq == 0.0:
                    continue
                theta = (float(G[q, q]) - float(G[p, p])) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + sqrt(theta * theta + 1.0))
                cs = 1.0 / sqrt(t * t + 1.0)
                sn = t * cs
                gp, gq = G[:, p].copy(), G[:, q].copy()
                G[:, p], G[:, q] = cs * gp - sn * gq, sn * gp + cs * gq
                gp, gq = G[p, :].copy(), G[q, :].copy()
                G[p, :], G[q, :] = cs * gp - sn * gq, sn * gp + cs * gq
                qp, qq = Q[:, p].copy(), Q[:, q].copy()
                Q[:, p], Q[:, q] = cs * qp - sn * qq, sn * qp + cs * qq
    lmax = 0.0
    for a in range(nb):
        lmax = max(lmax, float(G[a, a]))
    F, Fi, z = np.zeros((nb, nb)), np.zeros((nb, nb)), [0.0] * nb
    kk = 0
    for e in range(nb):
        lam = float(G[e, e])
        if not (lam > 1e-13 * lmax):
            continue
        sq = sqrt(lam)
        ze = 0.0
        for a in range(nb):
            F[kk, a] = sq * Q[a, e] / d[a] if d[a] > 0.0 else 0.0
            Fi[a, kk] = d[a] * Q[a, e] / sq
            ze += Fi[a, kk] * mc[2 * nb - 1 + a]
        z[kk] = ze
        kk += 1
    if info is not None:
        info["kept_eigen"] = kk
    if kk == 0:
        return coef
    c0 = K * (1.0 + mu)
    T = np.zeros((nb, nb))
    for k in range(nb):
        binom = 1.0
        for i in range(k + 1):
            v = binom
            for _ in range(k - i):
                v *= c0
            for _ in range(i):
                v *= K
            T[i, k] = v
            binom = binom * float(k - i) / float(i + 1)
    B = np.zeros((kk, nb))
    for e in range(kk):
        for k in range(nb):
            v = 0.0
            for i in range(nb):
                v += F[e, i] * T[i, k]
            B[e, k] = v
    W = np.eye(kk)

    def dot(u, w):
        s = 0.0
        for k in range(nb):
            s += float(u[k]) * float(w[k])
        return s

    for _ in range(60):
        worst = 0.0
        for p in range(kk - 1):
            for q in range(p + 1, kk):
                a2, c2, g = dot(B[p], B[p]), dot(B[q], B[q]), dot(B[p], B[q])
                lim = sqrt(a2 * c2)
                if not (abs(g) > 1e-19 * lim):
                    continue
                worst = max(worst, abs(g) / lim)
                zeta = (c2 - a2) / (2.0 * g)
                t = (1.0 if zeta >= 0.0 else -1.0) / (abs(zeta) + sqrt(1.0 + zeta * zeta))
                cs = 1.0 / sqrt(1.0 + t * t)
                sn = cs * t
                bp, bq = B[p].copy(), B[q].copy()
                B[p], B[q] = cs * bp - sn * bq, sn * bp + cs * bq
                wp, wq = W[:, p].copy(), W[:, q].copy()
                W[:, p], W[:, q] = cs * wp - sn * wq, sn * wp + cs * wq
        if worst < 1e-15:
            break
    sig = [sqrt(dot(B[e], B[e])) for e in range(kk)]
    smax = max([0.0] + sig)
    rows = float(nb) if mutate == "threshold-nb" else min(count, float(nb))
    thr = rows * 2.220446049250313e-16 * smax
    pz = [0.0] * kk
    kept = 0
    for e in range(kk):
        if not (sig[e] > thr):
            continue
        kept += 1
        proj = 0.0
        for a in range(kk):
            proj += W[a, e] * z[a]
        for a in range(kk):
            pz[a] += proj * W[a, e]
    if info is not None:
        info["rank"] = kept
        info["sigma"] = sorted((s / smax for s in sig), reverse=True) if smax > 0.0 else []
    for a in range(nb):
        v = 0.0
        for e in range(kk):
            v += Fi[a, e] * pz[e]
        coef[a] = v
    return coef


# ---- the probe of the threshold mutation ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def probe_threshold():
    """Two prices a few ulp apart at nb = 16: the second singular value of the raw design lies between Eigen's threshold for
    two rows (2 eps sigma_max: kept) and the mutated one (16 eps sigma_max: dropped), a factor >= 2 from both."""
    nb, base = 16, 1.5
    for ulps in range(1, 400):
        S = np.array([base, base + ulps * np.spacing(base)])
        b, b2 = np.array([0.3, 0.7]), np.array([1.0, -1.0])
        (fit, _), sv = _exact_eigen_rule(S, [b, b2], nb - 1)
        if 4.0 * EPS <= sv[1] <= 8.0 * EPS:
            with mp.workdps(DPS):
                mu = float(sum(mp_x(S, 1.0)) / 2)
                m = mp_moments(mp_x(S, 1.0, mu), b, b2, nb)
            return dict(nb=nb, S=S, b=b, K=1.0, mu=mu, moments=m, fit=fit, sv=sv)
    raise AssertionError("no probe found")


# ---- lsm_rcp / lsm_rsqrt and lsm_continuation: inputs and references --------------------------------------------------------------
def rcp_rsqrt_inputs():
    """What the solves can feed the two routines: pivots in (1e-10, 1], counts 1..1e9, moments 1e-300..1e300, both sides of
    the powers of two and four, the smallest and the largest mantissa."""
    rs = np.random.RandomState(5)
    x = [10.0 ** rs.uniform(-10.0, 0.0, 600), np.arange(1.0, 65.0), np.floor(10.0 ** rs.uniform(0.0, 9.0, 300)),
         10.0 ** rs.uniform(-300.0, 300.0, 600), 1.0 + rs.uniform(0.0, 1.0, 300), 2.0 + 2.0 * rs.uniform(0.0, 1.0, 300)]
    edges = []
    for e in (-996, -300, -101, -100, -34, -33, -3, -2, -1, 0, 1, 2, 3, 29, 30, 100, 101, 300, 996):
        p = 2.0 ** e
        edges += [np.nextafter(p, 0.0), p, np.nextafter(p, np.inf), np.nextafter(2.0 * p, 0.0), np.nextafter(np.nextafter(p, 0.0), 0.0),
                  np.nextafter(np.nextafter(p, np.inf), np.inf), p * (1.0 + 2.0 ** -26), p * 1.5, p * math.sqrt(2.0)]
    x.append(np.array(edges))
    return np.concatenate(x)


def ulp_errors(got, want_mp):
    """|got - want| in units of the spacing of binary64 at want."""
    out = np.empty(len(got))
    for i, (g, w) in enumerate(zip(got, want_mp)):
        out[i] = float(abs(mp.mpf(float(g)) - w) / mp.mpf(float(np.spacing(abs(float(w))))))
    return out


def rcp_rsqrt_reference(x):
    with mp.workdps(DPS):
        return [1 / mp.mpf(float(v)) for v in x], [1 / mp.sqrt(mp.mpf(float(v))) for v in x]


def continuation_cases(nb):
    """[n][nb + 2] = {c[0..nb), centre, x}: coefficients of mixed sign, a non-zero centre, x on both sides of it."""
    rs = np.random.RandomState(40 + nb)
    n = 40
    c = rs.uniform(-1.0, 1.0, (n, nb)) * 10.0 ** rs.uniform(-3.0, 3.0, (n, nb))
    centre = rs.uniform(-0.3, 0.3, (n, 1))
    x = rs.uniform(-0.9, 0.9, (n, 1))
    return np.ascontiguousarray(np.hstack([c, centre, x]))


def continuation_reference(e, nb):
    """(Horner in 60 digits of y = x - centre as binary64 forms it, the bound 2 nb eps sum |c_t| |y|^t) per element."""
    want, bound = [], []
    with mp.workdps(DPS):
        for row in e:
            y = mp.mpf(float(row[nb + 1] - row[nb]))
            want.append(mp_poly(list(row[:nb]), y))
            bound.append(float(2 * nb * mp.mpf(EPS) * sum(abs(mp.mpf(float(row[t]))) * abs(y) ** t for t in range(nb))))
    return want, np.array(bound)


# ---- the restatement's recorded error per group ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restatement_centred(nb):
    """{case id: (coefficient block, info)} of solve_centred_numpy on the centred cases of one basis size"""
    out = {}
    for c in centred_cases(nb):
        info = {}
        out[c["id"]] = (solve_centred_numpy(c["moments"], nb, c["mu"], c["K"], info=info), info)
    return out


@functools.lru_cache(maxsize=None)
def restatement_centred_errors(nb):
    """{(nb, decade of spread): the largest error of solve_centred_numpy against Eigen's rule in exact arithmetic} at one nb"""
    table = {}
    for c in centred_cases(nb):
        e = fitted_error(restatement_centred(nb)[c["id"]][0], c["mu"], c)
        table[c["group"]] = max(table.get(c["group"], 0.0), e)
    return table


def restatement_centred_table():
    table = {}
    for nb in CENTRED_NB:
        table.update(restatement_centred_errors(nb))
    return table


def centred_bound(group):
    """Ten times the restatement's recorded error of the group, at least 64 eps, never above the 2e-5 the oracle's own solver
    is held to in tests/test_oracle_models.py."""
    return min(max(10.0 * restatement_centred_errors(group[0])[group], 64.0 * EPS), 2e-5)


# ---- tests -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", FAST_NB)
def test_decision_distances_fast(nb):
    for c in fast_cases(nb):
        assert c["distance_ok"], (c["id"], c["pivots"], c["est"], est_threshold(nb))
        assert c["noise_decided"], (c["id"], c["pivots"], c["est"])
        if c["K_param"] <= 0.0 or nb == 1:
            assert not c["refine"], c["id"]
        if not c["zero"] and not c["ok"]:
            assert c["refine"] == (nb > 1 and c["K_param"] > 0.0), c["id"]


def test_fast_cases_cover_what_they_must():
    for nb in FAST_NB:
        cs = fast_cases(nb)
        names = {c["name"]: c for c in cs}
        assert {len(c["S"]) for c in cs} >= {0, 1, nb, nb + 1, 40, 5000} | ({nb - 1} if nb >= 2 else set())
        assert names["count-0"]["zero"] and not names["single"]["zero"] and (names["single"]["ok"] == (nb == 1))
        assert any((c["x"][0] > 0) for c in cs if len(c["S"])) and any((c["x"][0] < 0) for c in cs if len(c["S"]))
        assert {c["spread"] for c in cs} >= {0.5, 0.3, 0.1, 1e-2, 1e-4, 1e-6, 1e-8}
        assert {c["min_count"] for c in cs} >= {1.0, float(nb)}
        if nb >= 2:
            assert names["too-few"]["zero"] and not names["count-nb-1"]["zero"] and not names["count-nb-1"]["ok"]
            assert not names["duplicates"]["ok"] and len(set(names["duplicates"]["S"])) == nb - 1
            assert any(c["refine"] and c["ok"] for c in cs) and any(c["refine"] and not c["ok"] for c in cs)
        assert any(c["K_param"] <= 0.0 and not c["ok"] for c in cs if not c["zero"]) or nb == 1
        assert any(c["K_param"] <= 0.0 and c["ok"] for c in cs)


@pytest.mark.parametrize("nb", FAST_NB)
def test_restatement_fast_path(nb):
    """The restatement against the exact solution: within 1 eps kappa wherever every pivot exceeds 1e-6; its decisions are the
    expected ones on every case."""
    worst, n_trusted, n_piv = (0.0, None), 0, 0
    for c in fast_cases(nb):
        got = solve_nb_numpy(c["moments"][:3 * nb - 1], nb, c["min_count"], c["K_param"])
        assert got[C_COUNT] == len(c["S"]) and got[C_CENTER] == 0.0
        assert got[C_REFINE] == (1.0 if c["refine"] else 0.0), (c["id"], c["pivots"], c["est"])
        if c["zero"] or not c["ok"]:
            assert (got[:MAX_NB] == 0.0).all(), c["id"]
            continue
        n_trusted += c["trusted"] and c["K_param"] > 0.0
        if not c["pivots_trusted"]:
            continue
        n_piv += 1
        e = poly_error(got[:nb], c["exact"], c["x"]) / (EPS * c["kappa"])
        if e > worst[0]:
            worst = (e, c["id"], c["kappa"], min(c["pivots"]))
        assert e <= 1.0, (c["id"], e, c["kappa"], c["pivots"])
    print(f"nb {nb}: {n_piv} cases with every pivot > 1e-6, {n_trusted} of them trusted with K > 0; worst error {worst[0]:.3f} eps kappa "
          f"at {worst[1:]}" + ("" if n_trusted else "  -- NO trusted case at this size: tested for its decisions only"))


def test_trusted_sizes():
    """Which basis sizes have a trusted case (fast path taken for good, K > 0).  The wide spreads are there to find one at
    nb = 8 and 9; a size without one is tested for its decisions only, and this test says which."""
    have = {nb: [c["id"] for c in fast_cases(nb) if c["trusted"] and c["K_param"] > 0.0 and not c["zero"]] for nb in FAST_NB}
    print("trusted cases per nb: " + ", ".join(f"{nb}: {len(v)}" for nb, v in have.items()))
    print("sizes with none: " + (", ".join(str(nb) for nb, v in have.items() if not v) or "none"))
    assert all(have[nb] for nb in range(1, 8))


@pytest.mark.parametrize("nb", CENTRED_NB)
def test_decision_distances_centred(nb):
    for c in centred_cases(nb):
        thr = c["threshold"]
        assert all(s > 10.0 * thr or s < thr / 10.0 for s in c["sv"]), (c["id"], c["sv"], thr)
    cs = {c["name"]: c for c in centred_cases(nb)}
    assert len(set(cs["duplicates-1e-2"]["S"])) == max(nb // 2, 1) and len(cs["single"]["S"]) == 1
    if nb >= 2:
        assert len(cs["count-nb-1-1e-4"]["S"]) == nb - 1


def test_restatement_centred_table():
    """The restatement of lsm_solve_centered against Eigen's rule in exact arithmetic, per (nb, decade of spread); the rank it
    keeps is Eigen's on every case.  tests/test_gpu_lsm_solve.py takes the device's bound from this table."""
    table = restatement_centred_table()
    print("\nrestatement of lsm_solve_centered: largest error of the fitted values per (nb, decade of spread; 0 = no spread)")
    decades = sorted({g[1] for g in table})
    print("nb   " + "".join(f"{('1e%d' % d) if d else 'none':>10}" for d in decades))
    for nb in CENTRED_NB:
        print(f"{nb:<5}" + "".join(f"{table[(nb, d)]:>10.1e}" if (nb, d) in table else f"{'-':>10}" for d in decades))
    wrong = []
    for nb in CENTRED_NB:
        for c in centred_cases(nb):
            info = restatement_centred(nb)[c["id"]][1]
            if info.get("rank", 0) != c["rank"]:
                wrong.append((c["id"], info.get("rank"), c["rank"], info.get("kept_eigen")))
    print("cases whose kept rank differs from Eigen's:", wrong or "none")
    assert not wrong
    assert max(table.values()) <= 2e-5


def test_mutations_are_caught():
    """Each deliberate error in the restatement pushes a case over its bound or flips a decision."""
    caught = {}
    for nb in FAST_NB:
        for c in fast_cases(nb):
            m = c["moments"][:3 * nb - 1]
            for mutation in ("equilibrate-once", "pivot-bar-1e-4", "est-power-nb"):
                got = solve_nb_numpy(m, nb, c["min_count"], c["K_param"], mutate=mutation)
                flipped = got[C_REFINE] != (1.0 if c["refine"] else 0.0)
                over = False
                if c["pivots_trusted"] and not c["zero"] and not flipped:
                    over = not poly_error(got[:nb], c["exact"], c["x"]) <= EPS * c["kappa"]
                if flipped or over:
                    caught.setdefault(mutation, []).append(c["id"] + (" (decision)" if flipped else " (bound)"))
    p = probe_threshold()
    info, mutated = {}, {}
    good = solve_centred_numpy(p["moments"], p["nb"], p["mu"], p["K"], info=info)
    bad = solve_centred_numpy(p["moments"], p["nb"], p["mu"], p["K"], mutate="threshold-nb", info=mutated)
    print(f"threshold probe: sigma_2 / sigma_max = {p['sv'][1] / EPS:.2f} eps; restatement keeps rank {info['rank']}, "
          f"mutated {mutated['rank']}; fitted error {fitted_error(good, p['mu'], p):.2e} against {fitted_error(bad, p['mu'], p):.2e}")
    assert info["rank"] == 2 and fitted_error(good, p["mu"], p) <= 2e-5
    if mutated["rank"] != 2 and fitted_error(bad, p["mu"], p) > 2e-5:
        caught["threshold-nb"] = ["probe (decision and bound)"]
    # and on no regular case (the factor 10 of their distances is more than the factor 8 the two thresholds can differ by)
    for nb in CENTRED_NB:
        for c in centred_cases(nb):
            if len(c["S"]) < nb:
                mutated = {}
                solve_centred_numpy(c["moments"], nb, c["mu"], c["K"], mutate="threshold-nb", info=mutated)
                if mutated.get("rank", 0) != c["rank"]:
                    caught.setdefault("threshold-nb", []).append(c["id"] + " (decision)")
    for k, v in caught.items():
        print(f"{k}: caught by {len(v)} cases, e.g. {v[:3]}")
    assert set(caught) == {"equilibrate-once", "pivot-bar-1e-4", "est-power-nb", "threshold-nb"}, sorted(caught)


def test_rcp_rsqrt_inputs_cover_their_ranges():
    x = rcp_rsqrt_inputs()
    assert (x > 0.0).all() and np.isfinite(x).all() and x.min() <= 1e-299 and x.max() >= 1e299
    assert ((x > 1e-10) & (x <= 1.0)).sum() >= 500 and 1.0 in x and 4.0 in x and np.nextafter(4.0, 0.0) in x


def test_continuation_reference_against_plain_horner():
    for nb in FAST_NB:
        e = continuation_cases(nb)
        want, bound = continuation_reference(e, nb)
        y = e[:, nb + 1] - e[:, nb]
        cont = e[:, nb - 1].copy()
        for t in range(nb - 2, -1, -1):
            cont = cont * y + e[:, t]
        assert all(abs(float(mp.mpf(float(g)) - w)) <= b for g, w, b in zip(cont, want, bound)), nb
        assert (e[:, :nb] > 0).any() and (e[:, :nb] < 0).any() and (e[:, nb] != 0.0).all()
