"""Yardstick of the joint stereo tests (test infrastructure, not a test file): stereo_yardstick's problem with the two
cameras free, in numpy fp64 on the oracle's camera model.

Pj = (shared_a[La], shared_b[Lb], rig[6], pose_0[6], .., pose_{M-1}[6]) = (shared_a, shared_b, Ps). A problem is
stereo_yardstick's dict; its shared_a / shared_b are ignored here, the cameras travel in Pj. The dense Jacobian is
stereo_yardstick.jacobianDense at those cameras plus the shared columns orc.jacobianCompact already returns: camera a's
rows carry d/d shared_a, camera b's rows d/d shared_b. A fixed mask (bit s = shared unknown s) removes the columns of the
fixed unknowns from the dense problem, which is what editing the reduced system (unit row, zero column, right-hand side
0) solves; their step is 0."""
import numpy as np

import stereo_yardstick as sy
from oracle import calib_oracle as orc


def sizes(prob):
    La, Lb = orc.numShared(prob["model_a"]), orc.numShared(prob["model_b"])
    return La, Lb, La + Lb + 6


def split(prob, Pj):
    """-> (the problem at Pj's cameras, Ps)"""
    La, Lb, _ = sizes(prob)
    Pj = np.asarray(Pj, dtype=np.float64).ravel()
    return dict(prob, shared_a=Pj[:La].copy(), shared_b=Pj[La:La + Lb].copy()), Pj[La + Lb:]


def join(prob, Ps):
    """Pj of the problem's own cameras and Ps"""
    return np.concatenate((prob["shared_a"], prob["shared_b"], np.asarray(Ps, dtype=np.float64).ravel()))


def residualVector(prob, Pj):
    return sy.residualVector(*split(prob, Pj))


def error(prob, Pj):
    return sy.error(*split(prob, Pj))


def sharedJacobians(prob, Pj):
    """-> (Jsa (na,2,La) d/d shared_a of camera a's rows, Jsb (nb,2,Lb) d/d shared_b of camera b's rows)"""
    p, Ps = split(prob, Pj)
    La, Lb, _ = sizes(prob)
    rig, poses = Ps[:6], Ps[6:]
    Jca = orc.jacobianCompact(p["model_a"], np.concatenate((p["shared_a"], poses)), p["offs_a"], p["xyz_a"])
    Xa, _, _ = sy.pointsInA(p, Ps, "b")
    Jcb = orc.jacobianCompact(p["model_b"], np.concatenate((p["shared_b"], rig)), [0, Xa.shape[0]], Xa)
    return Jca[:, :, :La], Jcb[:, :, :Lb]


def jacobianDense(prob, Pj):
    """(2 (na + nb), S + 6 M): d(projection)/d(Pj), rows as stereo_yardstick.jacobianDense"""
    p, Ps = split(prob, Pj)
    La, Lb, S = sizes(prob)
    Jd = sy.jacobianDense(p, Ps)
    Jsa, Jsb = sharedJacobians(prob, Pj)
    na = Jsa.shape[0]
    J = np.zeros((Jd.shape[0], La + Lb + Jd.shape[1]))
    J[:2 * na, :La] = Jsa.reshape(2 * na, La)
    J[2 * na:, La:La + Lb] = Jsb.reshape(-1, Lb)
    J[:, La + Lb:] = Jd
    return J


def freeColumns(prob, Pj, mask):
    _, _, S = sizes(prob)
    n = np.asarray(Pj).size
    return np.array([c for c in range(n) if c >= S or not mask >> c & 1], dtype=int)


def stepDense(prob, Pj, lam, mask=0):
    """delta = (J^T J + lam diag J^T J)^-1 J^T r over the free columns, 0 at the fixed ones; dense solve"""
    free = freeColumns(prob, Pj, mask)
    J = jacobianDense(prob, Pj)[:, free]
    JTJ = J.T @ J
    delta = np.zeros(np.asarray(Pj).size)
    delta[free] = np.linalg.solve(JTJ + lam * np.diag(np.diagonal(JTJ)), J.T @ residualVector(prob, Pj))
    return delta


def normalBlocks(prob, Pj):
    """View-vectorised, without the dense Jacobian -> dict B (S,S), E (M,S,6) [shared row, view column], V (M,6,6),
    g (S + 6 M,), sseA, sseB. Per point the row block is [shared columns (S) | view columns (6)]; np.add.at sums the
    points of a view."""
    p, Ps = split(prob, Pj)
    La, Lb, S = sizes(prob)
    M = sy.numViews(prob)
    Jva, Jrb, Jvb = sy.compactJacobians(p, Ps)
    Jsa, Jsb = sharedJacobians(prob, Pj)
    ra, rb = sy.residuals(p, Ps)
    via, vib = orc.pointViewIndex(prob["offs_a"]), orc.pointViewIndex(prob["offs_b"])
    na, nb = Jva.shape[0], Jrb.shape[0]
    Sa = np.zeros((na, 2, S))
    Sa[:, :, :La] = Jsa
    Sb = np.zeros((nb, 2, S))
    Sb[:, :, La:La + Lb] = Jsb
    Sb[:, :, La + Lb:] = Jrb
    B = np.einsum("nki,nkj->ij", Sa, Sa) + np.einsum("nki,nkj->ij", Sb, Sb)
    E, V, g = np.zeros((M, S, 6)), np.zeros((M, 6, 6)), np.zeros(S + 6 * M)
    np.add.at(E, via, np.einsum("nki,nkj->nij", Sa, Jva))
    np.add.at(E, vib, np.einsum("nki,nkj->nij", Sb, Jvb))
    np.add.at(V, via, np.einsum("nki,nkj->nij", Jva, Jva))
    np.add.at(V, vib, np.einsum("nki,nkj->nij", Jvb, Jvb))
    g[:S] = np.einsum("nki,nk->i", Sa, ra) + np.einsum("nki,nk->i", Sb, rb)
    gv = np.zeros((M, 6))
    np.add.at(gv, via, np.einsum("nki,nk->ni", Jva, ra))
    np.add.at(gv, vib, np.einsum("nki,nk->ni", Jvb, rb))
    g[S:] = gv.ravel()
    return {"B": B, "E": E, "V": V, "g": g, "sseA": float(np.sum(ra * ra)), "sseB": float(np.sum(rb * rb))}


def stepFromBlocks(nb, lam, mask=0):
    """the LM step through the Schur complement of the view blocks, all views at once: any M"""
    B, E, V, g = nb["B"], nb["E"], nb["V"], nb["g"]
    S, M = B.shape[0], V.shape[0]
    eye = np.eye(6)
    Vd = V + lam * V * eye
    gv = g[S:].reshape(M, 6)
    VinvEt = np.linalg.solve(Vd, np.transpose(E, (0, 2, 1)))                  # (M,6,S)
    Vinvg = np.linalg.solve(Vd, gv[:, :, None])[:, :, 0]                       # (M,6)
    A = B + lam * np.diag(np.diagonal(B)) - np.einsum("mij,mjk->ik", E, VinvEt)
    b = g[:S] - np.einsum("mij,mj->i", E, Vinvg)
    free = np.array([s for s in range(S) if not mask >> s & 1], dtype=int)
    ds = np.zeros(S)
    ds[free] = np.linalg.solve(A[np.ix_(free, free)], b[free])
    dv = Vinvg - np.einsum("mis,s->mi", VinvEt, ds)
    return np.concatenate((ds, dv.ravel()))


def stepBlocks(prob, Pj, lam, mask=0):
    return stepFromBlocks(normalBlocks(prob, Pj), lam, mask)


def refineDense(prob, Pj0, maxIters, mask=0, lamInit=orc.LAMBDA_INITIAL, lamMin=orc.LAMBDA_MIN, lamMax=orc.LAMBDA_MAX,
                errMin=orc.PT_ERROR_MIN, step=stepDense):
    """the loop of src/calibrate.py:143-171 on Pj -> (err before the last update, Pj, trace rows (iter, err(P),
    err(P + delta), lambda, accepted, the S shared unknowns before the update))"""
    _, _, S = sizes(prob)
    Pt = np.array(Pj0, dtype=np.float64).ravel()
    lam, trace, err0 = lamInit, [], None
    for it in range(maxIters):
        delta = step(prob, Pt, lam, mask)
        err0 = sum(error(prob, Pt))
        err1 = sum(error(prob, Pt + delta))
        accepted = bool(err1 < err0)
        trace.append([it, err0, err1, lam, float(accepted)] + list(Pt[:S]))
        if accepted:
            Pt = Pt + delta
            lam /= 10
        else:
            lam *= 10
        if not (lamMin < lam < lamMax) or err0 < errMin:
            break
    return err0, Pt, np.array(trace)


def covarianceDense(prob, Pj, mask=0):
    """the shared (S,S) block of sigma^2 (Jf^T Jf)^-1 over the free columns, rows and columns of the fixed unknowns
    zero; sigma^2 = sse / (rows - free columns)"""
    _, _, S = sizes(prob)
    free = freeColumns(prob, Pj, mask)
    J = jacobianDense(prob, Pj)[:, free]
    C = sum(error(prob, Pj)) / (J.shape[0] - J.shape[1]) * np.linalg.inv(J.T @ J)
    nfree = int(np.sum(free < S))
    out = np.zeros((S, S))
    out[np.ix_(free[:nfree], free[:nfree])] = C[:nfree, :nfree]
    return out


def perturbedJoint(prob, PsTrue, rigDeg, rigFrac, poseDeg, poseFrac, intrinsics=0.02, distortion=0.10, seed=5):
    """Pj with the rig and the poses off as sy.perturbed puts them, alpha beta uc vc of both cameras off by `intrinsics`
    (relative, random signs; a gamma of 0 stays 0) and the distortion coefficients by `distortion` (relative)"""
    La, Lb, _ = sizes(prob)
    rng = np.random.default_rng(seed)
    out = []
    for sh in (prob["shared_a"], prob["shared_b"]):
        sh = np.array(sh, dtype=np.float64)
        sign = rng.choice([-1.0, 1.0], sh.shape[0])
        frac = np.where(np.arange(sh.shape[0]) < 5, intrinsics, distortion)
        new = sh * (1.0 + sign * frac)
        out.append(new)
    return np.concatenate(out + [sy.perturbed(PsTrue, rigDeg, rigFrac, poseDeg, poseFrac)])


def engineCameras(prob):
    return sy.engineCameras(prob)
