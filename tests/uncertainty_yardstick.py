"""Yardsticks of the uncertainty tests (test infrastructure, written from the oracle's public pieces).

The covariance yardstick deliberately does not share the engine's Schur route: the dense Jacobian
(orc.jacobianDense) with the fixed columns deleted, R of its QR factorisation, C = sigma2 R^-1 R^-T with sigma2 from
orc.reprojectionError. The per-view yardstick is np.add.reduceat / np.maximum.reduceat over sensor -
orc.projectAllPoints.

Tolerance (derived, not chosen): standard deviations are compared relatively and covariances as correlations,
C_ij / sqrt(C_ii C_jj), absolutely, both within tol = 1e3 eps kappa, kappa = cond(Jf D)^2 with D scaling the columns of
the free Jacobian to unit norm -- the sensitivity of (Jf^T Jf)^-1, which neither route can beat, times 1e3 for the
constants of two different factorisations. sigma2 and the per-view sums get the project's sse tolerance, 1e-9 relative
above 1e-13 absolute. Because sigma2 has that absolute floor (on noise-free goldens sse(Pfinal) ~ 1e-20 is rounding
noise of the sums, equal in no two implementations), a standard deviation is compared after division by its own
side's sigma: std / sigma = sqrt(diag (Jf^T Jf)^-1) carries the whole of the covariance's content and none of that
noise; sigma2 itself is held to its own bar."""
import numpy as np

from oracle import calib_oracle as orc

EPS = np.finfo(np.float64).eps


def bitsOf(mask):
    return [i for i in range(32) if mask >> i & 1]


def covarianceYardstick(model, P, offs, s, m, F=()):
    """-> dict sigma2, dof, sse, C (K,K; zero rows / columns for F), unit (K,K) = (Jf^T Jf)^-1 likewise, kappa, tol"""
    P = np.asarray(P, dtype=np.float64).ravel()
    J = orc.jacobianDense(model, P, offs, m)
    K = J.shape[1]
    free = np.setdiff1d(np.arange(K), np.asarray(list(F), dtype=np.int64))
    Jf = J[:, free]
    sse = float(orc.reprojectionError(model, P, offs, s, m))
    dof = J.shape[0] - free.shape[0]
    sigma2 = sse / dof
    R = np.linalg.qr(Jf, mode="r")
    Rinv = np.linalg.solve(R, np.eye(R.shape[0]))
    unit = np.zeros((K, K))
    unit[np.ix_(free, free)] = Rinv @ Rinv.T
    # cond(Jf D) = cond(R D): Jf D = Q (R D), and the columns of R have the norms of the columns of Jf
    kappa = float(np.linalg.cond(R / np.linalg.norm(R, axis=0)) ** 2)
    return {"sigma2": sigma2, "dof": dof, "sse": sse, "C": sigma2 * unit, "unit": unit, "kappa": kappa,
            "tol": 1e3 * EPS * kappa, "free": free}


def correlation(C):
    d = np.sqrt(np.diagonal(C))
    safe = np.where(d > 0, d, 1.0)
    return C / np.outer(safe, safe)


def closeSse(a, b):
    """the project's sse tolerance: 1e-9 relative above 1e-13 absolute"""
    return abs(a - b) <= max(1e-9 * abs(b), 1e-13)


def checkCovariance(res, yard, L, F, label, tol=None, viewSlice=None):
    """res: dict of RefineEngine.covariance / covFinish (or the sharded result); yard: covarianceYardstick of the same
    problem (viewSlice = (v0, v1): res covers all views, the yardstick only those). Prints every figure, then asserts."""
    tol = yard["tol"] if tol is None else tol
    F = list(F)
    M = res["covViews"].shape[0]
    v0, v1 = viewSlice if viewSlice is not None else (0, M)
    sigD, sigY = np.sqrt(res["sigma2"]), np.sqrt(yard["sigma2"])
    stdD = np.concatenate((res["std"][:L], res["std"][L + 6 * v0:L + 6 * v1]))
    covViews = res["covViews"][v0:v1]
    stdY = np.sqrt(np.diagonal(yard["C"]))
    uD, uY = stdD / sigD, np.sqrt(np.diagonal(yard["unit"]))
    free = uY > 0
    relStd = np.abs(uD[free] - uY[free]) / uY[free]
    corrS = np.abs(correlation(res["covShared"]) - correlation(yard["C"][:L, :L])).max() if len(F) < L else 0.0
    corrV = 0.0
    for i in range(v1 - v0):
        a = L + 6 * i
        corrV = max(corrV, np.abs(correlation(covViews[i]) - correlation(yard["C"][a:a + 6, a:a + 6])).max())
    print(f"{label}: kappa {yard['kappa']:.3e} tol {tol:.3e} | sigma2 {res['sigma2']:.12e} (yardstick "
          f"{yard['sigma2']:.12e}) dof {res['dof']} | max rel d(std/sigma) {relStd.max():.3e} | max |d corr| shared "
          f"{corrS:.3e} views {corrV:.3e}")
    if viewSlice is None:
        assert res["dof"] == yard["dof"], label
        assert closeSse(res["sigma2"] * res["dof"], yard["sse"]), label
    assert np.array_equal(stdD[~free], np.zeros(int((~free).sum()))), label
    for i in F:                                  # rows and columns of fixed parameters are exactly 0.0
        assert not res["covShared"][i].any() and not res["covShared"][:, i].any(), (label, i)
        if res.get("covCross") is not None:
            assert not res["covCross"][:, i, :].any(), (label, i)
    assert relStd.max() <= tol, (label, relStd.max(), tol)
    assert corrS <= tol, (label, corrS, tol)
    assert corrV <= tol, (label, corrV, tol)
    if res.get("covCross") is not None and viewSlice is None:
        # the cross block as correlations between each shared parameter and each pose parameter
        worst = 0.0
        for i in range(M):
            a = L + 6 * i
            d = np.outer(np.where(stdD[:L] > 0, stdD[:L], 1.0), stdD[a:a + 6])
            dY = np.outer(np.where(stdY[:L] > 0, stdY[:L], 1.0), stdY[a:a + 6])
            worst = max(worst, np.abs(res["covCross"][i] / d - yard["C"][:L, a:a + 6] / dY).max())
        print(f"{label}: max |d corr| cross {worst:.3e}")
        assert worst <= tol, (label, worst, tol)
    return {"relStd": float(relStd.max()), "corrShared": float(corrS), "corrViews": float(corrV)}


def viewErrorsYardstick(model, P, offs, s, m):
    """-> (sse (M,), rms (M,), max (M,)) with NaN rms and 0 max for an empty view"""
    offs = np.asarray(offs, dtype=np.int64)
    M = offs.shape[0] - 1
    r = np.asarray(s, dtype=np.float64) - orc.projectAllPoints(model, np.asarray(P, dtype=np.float64).ravel(), offs, m)
    e = np.sum(r * r, axis=1)
    n = np.diff(offs)
    sse, mx = np.zeros(M), np.zeros(M)
    full = n > 0
    if e.shape[0]:
        starts = offs[:-1][full]
        sse[full] = np.add.reduceat(e, starts)
        mx[full] = np.sqrt(np.maximum.reduceat(e, starts))
    with np.errstate(invalid="ignore", divide="ignore"):
        rms = np.where(full, np.sqrt(sse / np.where(full, n, 1)), np.nan)
    return sse, rms, mx
