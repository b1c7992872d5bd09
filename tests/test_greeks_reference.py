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


def lsm_greeks_numpy(paths_sm, r, K, maturity, dt, is_call, poly):
    """{price, dual_delta, delta} of lsm_tangent_numpy (delta by homogeneity: row 0 must be one constant S0)."""
    V, dV = lsm_tangent_numpy(paths_sm, r, K, maturity, dt, is_call, poly)
    S0 = float(paths_sm[0][0])
    price, dual = V.mean(), dV.mean()
    return {"price": price, "dual_delta": dual, "delta": (price - K * dual) / S0}


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
