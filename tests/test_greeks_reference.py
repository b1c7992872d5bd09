"""CPU reference for the LSM Greeks (mcg_greeks_lsm): a numpy K-tangent of LSM::PredictOptionPrice on raw monomials with
the oracle's minimum-norm rule (one-sided Jacobi, Eigen's threshold), checked here against the oracle's price and against
central differences in K.  tests/test_gpu_greeks.py compares the GPU with it.  Runs without a GPU."""
import math

import numpy as np
import pytest

from oracle.binding import Oracle

EPS = np.finfo(float).eps


def minnorm_fit(S, B, nb):
    """Fitted values A c of the minimum-norm least-squares solutions of A c = B[:, k] for every column of B, A = [S^0 ..
    S^(nb-1)]: the oracle's minnorm_lstsq (one-sided Jacobi on the columns of A, singular values <= min(rows, cols) eps
    sigma_max dropped), vectorised over the rows.  One factorisation serves every right-hand side."""
    rows = len(S)
    cols = [S ** q for q in range(nb)]
    A = np.stack(cols, axis=1)
    V = np.eye(nb)
    # At high orders, and on a sample of one repeated price (date 0), apq can be tiny against aqq - app: zeta * zeta
    # overflows to inf, t = 0 and that rotation is skipped.  The fits still match the oracle to ~2e-11 (tested below),
    # so the overflow is expected and silenced rather than reported as a RuntimeWarning.
    with np.errstate(over="ignore"):
        for _ in range(60):
            rotated = False
            for p in range(nb - 1):
                for q in range(p + 1, nb):
                    cp, cq = cols[p], cols[q]
                    app, aqq, apq = cp @ cp, cq @ cq, cp @ cq
                    if apq == 0.0 or abs(apq) <= 1e-17 * math.sqrt(app * aqq):
                        continue
                    rotated = True
                    zeta = (aqq - app) / (2.0 * apq)
                    t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                    cs = 1.0 / math.sqrt(1.0 + t * t)
                    sn = cs * t
                    cols[p], cols[q] = cs * cp - sn * cq, sn * cp + cs * cq
                    V[p], V[q] = cs * V[p] - sn * V[q], sn * V[p] + cs * V[q]
            if not rotated:
                break
    sig = np.array([math.sqrt(c @ c) for c in cols])
    thr = max(sig.max() * min(rows, nb) * EPS, 2.2250738585072014e-308)
    coef = np.zeros((nb, B.shape[1]))
    for j in range(nb):
        if sig[j] > thr:
            coef += np.outer(V[j], (cols[j] @ B) / (sig[j] * sig[j]))
    return A @ coef


def lsm_tangent_numpy(paths_sm, r, K, maturity, dt, is_call, poly):
    """LSMPricer.cpp:19-102 on a step-major matrix [steps + 1][paths] with the K-tangent dV carried alongside: exercise
    decisions held fixed, the tangent of the fitted continuation is the same projection of disc dV.  Returns (V_0, dV_0)."""
    S = np.asarray(paths_sm, dtype=np.float64)
    M = S.shape[0]
    sgn = -1.0 if is_call else 1.0

    def pay(s):
        return np.maximum(0.0, s - K) if is_call else np.maximum(0.0, K - s)

    V = pay(S[M - 1])
    dV = np.where(V > 0.0, sgn, 0.0)
    disc = math.exp(-r * dt)
    for j in range(M - 2, -1, -1):
        if j * dt > maturity:
            V, dV = V * disc, dV * disc
            continue
        s = S[j]
        p = pay(s)
        itm = p > 1e-14
        Vn, dVn = np.zeros_like(V), np.zeros_like(V)
        if itm.any():
            fit = minnorm_fit(s[itm], np.stack([V[itm] * disc, dV[itm] * disc], axis=1), poly + 1)
            cont, dcont = fit[:, 0], fit[:, 1]
            Vn[itm] = np.where(cont > p[itm], cont, p[itm])
            dVn[itm] = np.where(cont > p[itm], dcont, sgn)
        otm = p < 1e-14
        Vn[otm] = V[otm] * disc
        dVn[otm] = dV[otm] * disc
        V, dV = Vn, dVn
    return V, dV


def mean_se(x):
    """Mean and Monte Carlo std error (ddof 1, over sqrt n) of per-path estimates; one path: se 0 (mcg_greeks)."""
    n = len(x)
    return float(x.mean()), float(x.std(ddof=1) / math.sqrt(n)) if n > 1 else 0.0


def lsm_greeks_numpy(paths_sm, r, K, maturity, dt, is_call, poly):
    """{price, dual_delta, delta} of lsm_tangent_numpy and their std errors {price_se, dual_delta_se, delta_se} from the
    per-path V_0, dV_0 and (V_0 - K dV_0) / S0 (delta by homogeneity; NaN, with its se, unless row 0 is one positive
    constant S0 -- mcg_greeks_lsm's rule)."""
    V, dV = lsm_tangent_numpy(paths_sm, r, K, maturity, dt, is_call, poly)
    return greeks_of(V, dV, paths_sm[0], K)


def greeks_of(V, dV, row0, K):
    """lsm_greeks_numpy's dict from the per-path V_0 and dV_0 and row 0 of the matrix."""
    row0 = np.asarray(row0, dtype=np.float64)
    S0 = float(row0[0])
    g = {}
    g["price"], g["price_se"] = mean_se(V)
    g["dual_delta"], g["dual_delta_se"] = mean_se(dV)
    g["delta"] = g["delta_se"] = math.nan
    if S0 > 0.0 and (row0 == S0).all():
        g["delta"] = (g["price"] - K * g["dual_delta"]) / S0
        g["delta_se"] = mean_se((V - K * dV) / S0)[1]
    return g


def fd_step(paths_sm, K):
    """Central-difference step in K for the LSM price: half the distance from K to the nearest price in rows 1 .. M-1, so
    that no path enters or leaves an in-the-money set within +-h (the regression sample changes there and the price
    jumps; row 0 is one constant, and crossing it moves no path's V_0).  A fixed step is wrong both ways: 1e-7 K .. 1e-4 K
    crosses such jumps at 20 000 x 30 (2 % - 15 % off), 1e-9 K divides the oracle's ~1e-11 absolute solve noise at orders
    >= 4 by too small an h (2.5e-4 - 4.5e-4 off).  The rule does not see exercise decisions that flip within +-h (a kink,
    not a jump): rBergomi put K = 80 at order 2 takes one at this h (1.2e-4 off; 1e-8 at h / 10).  Shrinking h to the
    smallest |continuation - payoff| instead lets the oracle's noise through (6e-5 off at order 2 with date 0 in the
    money), so the deep strikes are checked at orders where this h is clean."""
    S = np.asarray(paths_sm, dtype=np.float64)
    return 0.5 * float(np.min(np.abs(S[1:] - K)))


N_PATHS, STEPS, DT, K, R = 20_000, 29, 0.02, 100.0, 0.04   # 30 columns
MAT = STEPS * DT


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def matrices(orc):
    gbm = orc.paths_gbm(11, 100.0, R, 0.2, DT, STEPS, 0, N_PATHS)
    rb = orc.paths_rbergomi(12, 100.0, R, 0.04, 0.1, 1.9, -0.9, DT, STEPS, 0, N_PATHS)
    return {"gbm": gbm, "rbergomi": rb}


@pytest.mark.parametrize("which", ["gbm", "rbergomi"])
@pytest.mark.parametrize("is_call", [False, True])
@pytest.mark.parametrize("poly", [1, 2, 3])
def test_numpy_tangent_price_matches_oracle_and_central_difference(orc, matrices, which, is_call, poly):
    P = matrices[which]
    g = lsm_greeks_numpy(P, R, K, MAT, DT, is_call, poly)
    want = orc.lsm_price(P, R, K, MAT, DT, is_call, poly)
    assert abs(g["price"] - want) <= 1e-10 * abs(want), (g["price"], want)
    h = 1e-9 * K
    up = orc.lsm_price(P, R, K + h, MAT, DT, is_call, poly)
    dn = orc.lsm_price(P, R, K - h, MAT, DT, is_call, poly)
    fd = (up - dn) / (2 * h)
    assert abs(g["dual_delta"] - fd) <= 1e-4 * abs(fd), (g["dual_delta"], fd)
    assert abs(g["delta"] * P[0][0] + K * g["dual_delta"] - g["price"]) <= 1e-12 * abs(g["price"])
    assert (g["dual_delta"] < 0) == is_call and (g["delta"] > 0) == is_call


def test_numpy_tangent_edge_cases():
    """Dates past maturity only discount V and dV; an all out-of-the-money matrix has price and tangent 0; a lone path
    whose fit is exact carries the discounted tangent of its future."""
    rs = np.random.RandomState(3)
    otm = (150.0 + rs.rand(50, 6)).T
    V, dV = lsm_tangent_numpy(otm, R, K, 1.0, 0.2, False, 2)
    assert not V.any() and not dV.any()
    itm_end = np.full((4, 10), 150.0)
    itm_end[-1] = 90.0
    V, dV = lsm_tangent_numpy(itm_end, R, K, 1.0, 0.25, False, 2)
    assert np.allclose(V, 10.0 * math.exp(-R * 0.75), rtol=1e-14) and np.allclose(dV, math.exp(-R * 0.75), rtol=1e-14)
    assert lsm_tangent_numpy(itm_end, R, K, 0.3, 0.25, False, 2)[1][0] == pytest.approx(math.exp(-R * 0.75), rel=1e-14)


def fd_tol(poly):
    """Dual delta vs the oracle's central difference at fd_step (measured at 20 000 x 30, every strike below): <= 4e-6 at
    orders <= 3, where the oracle's solve is exact to rounding; <= 5e-5 at orders >= 4, where its rank-truncated solve is
    good to ~1e-11 absolute only and that noise over h remains."""
    return 2e-5 if poly <= 3 else 1e-4


def price_tol(poly, want):
    """Numpy vs oracle price: 1e-10 relative; at orders >= 4 plus 1e-10 absolute (the truncated solve's noise, ~1e-11 per
    date, is not relative to a small deep out-of-the-money price)."""
    return 1e-10 * abs(want) + (1e-10 if poly >= 4 else 0.0)


def check_tangent(orc, P, K_, mat, is_call, poly):
    """The numpy K-tangent on P against the oracle's price and its central difference in K; returns (V_0, dV_0, greeks)."""
    V, dV = lsm_tangent_numpy(P, R, K_, mat, DT, is_call, poly)
    g = greeks_of(V, dV, P[0], K_)
    want = orc.lsm_price(P, R, K_, mat, DT, is_call, poly)
    assert abs(g["price"] - want) <= price_tol(poly, want), (g["price"], want)
    h = fd_step(P, K_)
    fd = (orc.lsm_price(P, R, K_ + h, mat, DT, is_call, poly) - orc.lsm_price(P, R, K_ - h, mat, DT, is_call, poly)) / (2 * h)
    assert abs(g["dual_delta"] - fd) <= fd_tol(poly) * abs(fd), (g["dual_delta"], fd, h)
    assert abs(g["delta"] * P[0][0] + K_ * g["dual_delta"] - g["price"]) <= 1e-12 * abs(g["price"])
    assert (g["dual_delta"] < 0) == is_call
    assert g["price_se"] > 0 or np.ptp(V) == 0.0
    return V, dV, g


ORDERS = list(range(9))


@pytest.mark.parametrize("which", ["gbm", "rbergomi"])
@pytest.mark.parametrize("poly", ORDERS)
def test_numpy_tangent_every_order_at_the_money(orc, matrices, which, poly):
    """Orders 0-8 (every k_lsm_date<NB, true> the GPU has), K = S0: date 0 out of the money.  Puts on GBM at even orders and
    on rBergomi at odd ones, calls the other way round (both kinds at every order, half the oracle time)."""
    check_tangent(orc, matrices[which], K, MAT, (poly % 2 == 0) == (which == "rbergomi"), poly)


# date 0 in the money (put 110, call 90): every path regresses on the one price S0 -- the fit is the mean, V_0 one number
DATE0_ITM = [(False, 110.0), (True, 90.0)]


@pytest.mark.parametrize("which", ["gbm", "rbergomi"])
@pytest.mark.parametrize("is_call,K_", DATE0_ITM)
@pytest.mark.parametrize("poly", [0, 3, 5])
def test_numpy_tangent_date0_in_the_money(orc, matrices, which, is_call, K_, poly):
    V, dV, g = check_tangent(orc, matrices[which], K_, MAT, is_call, poly)
    assert np.ptp(V) == 0.0 and np.ptp(dV) == 0.0
    assert g["price_se"] <= 1e-12 * g["price"] and g["dual_delta_se"] <= 1e-12 * abs(g["dual_delta"])


# deep out of / in the money: put 80 / 130, call 120 / 70 (date 0 in the money for the deep ITM ones)
DEEP = [(False, 80.0), (False, 130.0), (True, 120.0), (True, 70.0)]


@pytest.mark.parametrize("which", ["gbm", "rbergomi"])
@pytest.mark.parametrize("is_call,K_", DEEP)
@pytest.mark.parametrize("poly", [1, 4])
def test_numpy_tangent_deep_strikes(orc, matrices, which, is_call, K_, poly):
    check_tangent(orc, matrices[which], K_, MAT, is_call, poly)


@pytest.mark.parametrize("which", ["gbm", "rbergomi"])
@pytest.mark.parametrize("poly", [2, 4])
def test_numpy_tangent_maturity_before_horizon(orc, matrices, which, poly):
    """Maturity 0.37 on a 0.58 matrix: dates 19 .. 28 are not regressed, V and dV only discounted there."""
    check_tangent(orc, matrices[which], K, 0.37, poly % 4 == 0, poly)
