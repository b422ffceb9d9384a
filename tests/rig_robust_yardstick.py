"""Yardstick of the robust rig tests (test infrastructure, not a test file): rig_joint_yardstick's problem under a robust
loss per point, in numpy fp64.

A loss is (name, delta): "huber" or "cauchy", delta in pixels; None is the plain problem. With s = rx^2 + ry^2 of a point's
2-vector residual,
    huber   rho(s) = s for s <= delta^2, 2 delta sqrt(s) - delta^2 above;   w = rho'(s) = 1, delta / sqrt(s) above
    cauchy  rho(s) = delta^2 log1p(s / delta^2);                            w = 1 / (1 + s / delta^2)
The problem minimised is sum rho(s_p) over all points of all cameras. The step is the LM step of the re-weighted problem:
both Jacobian rows of a point and its residual times sqrt(w) at the current point (first order; Triggs' second-order term
is left out), the accept rule on sum rho. Everything else -- Pq, the mask, the loop -- is rig_joint_yardstick's."""
import numpy as np

import rig_joint_yardstick as qy
import rig_yardstick as ry
import stereo_joint_yardstick as jy
from oracle import calib_oracle as orc


def rho(loss, s):
    s = np.asarray(s, dtype=np.float64)
    if loss is None:
        return s.copy()
    name, d = loss
    if name == "huber":
        return np.where(s <= d * d, s, 2.0 * d * np.sqrt(s) - d * d)
    assert name == "cauchy"
    return d * d * np.log1p(s / (d * d))


def weight(loss, s):
    s = np.asarray(s, dtype=np.float64)
    if loss is None:
        return np.ones_like(s)
    name, d = loss
    if name == "huber":
        with np.errstate(divide="ignore"):
            return np.where(s <= d * d, 1.0, d / np.sqrt(s))
    assert name == "cauchy"
    return 1.0 / (1.0 + s / (d * d))


def residuals(prob, Pq):
    """-> [res_c (n_c,2)]: sensor - projection"""
    return ry.residuals(*qy.split(prob, Pq))


def squares(prob, Pq):
    """-> [s_c (n_c,)]"""
    return [np.sum(r * r, axis=1) for r in residuals(prob, Pq)]


def weights(prob, Pq, loss):
    """-> [w_c (n_c,)]"""
    return [weight(loss, s) for s in squares(prob, Pq)]


def costCam(prob, Pq, loss):
    """-> (N,) sum rho per camera"""
    return np.array([float(np.sum(rho(loss, s))) for s in squares(prob, Pq)])


def cost(prob, Pq, loss):
    """the cameras' sums of rho added in index order"""
    e = costCam(prob, Pq, loss)
    s = e[0]
    for x in e[1:]:
        s = s + x
    return s


def rowWeights(prob, Pq, loss):
    """sqrt(w) of every row of the dense problem (2 sum n_c,): a point's two rows carry its weight"""
    return np.repeat(np.sqrt(np.concatenate(weights(prob, Pq, loss))), 2)


def stepDense(prob, Pq, lam, loss, mask=0):
    """rig_joint_yardstick.stepDense on the rows and the residual times sqrt(w)"""
    free = qy.freeColumns(prob, Pq, mask)
    sw = rowWeights(prob, Pq, loss)
    J = qy.jacobianDense(prob, Pq)[:, free] * sw[:, None]
    r = qy.residualVector(prob, Pq) * sw
    JTJ = J.T @ J
    delta = np.zeros(np.asarray(Pq).size)
    delta[free] = np.linalg.solve(JTJ + lam * np.diag(np.diagonal(JTJ)), J.T @ r)
    return delta


def normalBlocks(prob, Pq, loss):
    """rig_joint_yardstick.normalBlocks of the weighted problem -> dict B, E, V, g, costCam (N,) = sum rho per camera"""
    p, Pr = qy.split(prob, Pq)
    S, off, L = qy.layout(prob)
    M, N = ry.numViews(prob), ry.numCameras(prob)
    Jv0, rest = ry.compactJacobians(p, Pr)
    Js = qy.sharedJacobians(prob, Pq)
    res = ry.residuals(p, Pr)
    B, E, V, g, gv = np.zeros((S, S)), np.zeros((M, S, 6)), np.zeros((M, 6, 6)), np.zeros(S + 6 * M), np.zeros((M, 6))
    for c in range(N):
        sw = np.sqrt(weight(loss, np.sum(res[c] * res[c], axis=1)))
        vi = orc.pointViewIndex(prob["offs"][c])
        Jv = (Jv0 if c == 0 else rest[c - 1][1]) * sw[:, None, None]
        Jc = (Js[c] if c == 0 else np.concatenate((Js[c], rest[c - 1][0]), axis=2)) * sw[:, None, None]
        rc = res[c] * sw[:, None]
        sl = slice(off[c], off[c] + Jc.shape[2])
        B[sl, sl] = np.einsum("nki,nkj->ij", Jc, Jc)
        Ec = np.zeros((M, Jc.shape[2], 6))
        np.add.at(Ec, vi, np.einsum("nki,nkj->nij", Jc, Jv))
        E[:, sl] = Ec
        np.add.at(V, vi, np.einsum("nki,nkj->nij", Jv, Jv))
        g[sl] = np.einsum("nki,nk->i", Jc, rc)
        np.add.at(gv, vi, np.einsum("nki,nk->ni", Jv, rc))
    g[S:] = gv.ravel()
    return {"B": B, "E": E, "V": V, "g": g, "costCam": costCam(prob, Pq, loss)}


def stepBlocks(prob, Pq, lam, loss, mask=0):
    """through the Schur complement of the weighted view blocks: any M"""
    return jy.stepFromBlocks(normalBlocks(prob, Pq, loss), lam, mask)


def refineDense(prob, Pq0, maxIters, loss, mask=0, lamInit=orc.LAMBDA_INITIAL, lamMin=orc.LAMBDA_MIN, lamMax=orc.LAMBDA_MAX,
                errMin=orc.PT_ERROR_MIN, step=stepDense):
    """rig_joint_yardstick.refineDense with sum rho in the place of the error -> (cost before the last update, Pq, trace)"""
    S = qy.layout(prob)[0]
    Pt = np.array(Pq0, dtype=np.float64).ravel()
    lam, trace, err0 = lamInit, [], None
    for it in range(maxIters):
        delta = step(prob, Pt, lam, loss, mask)
        err0 = cost(prob, Pt, loss)
        err1 = cost(prob, Pt + delta, loss)
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


def covarianceDense(prob, Pq, loss, mask=0):
    """the shared (S,S) block of sigma^2 (Jw^T Jw)^-1 over the free columns, Jw the rows times sqrt(w); sigma^2 =
    sum_p w_p s_p / dof with the plain problem's dof = rows - free columns; rows and columns of the fixed unknowns zero"""
    S = qy.layout(prob)[0]
    free = qy.freeColumns(prob, Pq, mask)
    sw = rowWeights(prob, Pq, loss)
    J = qy.jacobianDense(prob, Pq)[:, free] * sw[:, None]
    wss = float(np.sum((qy.residualVector(prob, Pq) * sw) ** 2))
    C = wss / (J.shape[0] - J.shape[1]) * np.linalg.inv(J.T @ J)
    nfree = int(np.sum(free < S))
    out = np.zeros((S, S))
    out[np.ix_(free[:nfree], free[:nfree])] = C[:nfree, :nfree]
    return out


def rigError(prob, Pq, PqTrue):
    """largest distance of a rig parameter from the truth (degrees / metres)"""
    cols = qy.columnsOfPr(prob)
    return float(np.abs(np.asarray(Pq)[cols] - np.asarray(PqTrue)[cols]).max())


OUTLIER_SEED = 23
_cache = {}


def outlierCase():
    """rig_joint_yardstick.noisyCase's problem (three cameras, eight views, 0.3 px noise) with 5 % of each camera's corners
    (at least one) displaced by 15 to 40 px at a uniform angle, fixed seed -> dict: clean (the problem without the
    outliers), prob, PqTrue, PrTrue, Pq0 (noisyCase's joint start point), PqRig0 (the true cameras, rigs and poses off as
    there), displaced [bool (n_c,)]"""
    if "outlier" not in _cache:
        clean, PqTrue, Pq0, _ = qy.noisyCase()
        rng = np.random.default_rng(OUTLIER_SEED)
        uv, displaced = [], []
        for u in clean["uv"]:
            n = u.shape[0]
            k = max(1, int(round(0.05 * n)))
            idx = np.sort(rng.permutation(n)[:k])
            length, angle = rng.uniform(15.0, 40.0, k), rng.uniform(0.0, 2.0 * np.pi, k)
            u = np.array(u, dtype=np.float64)
            u[idx] += np.stack((length * np.cos(angle), length * np.sin(angle)), axis=1)
            uv.append(np.ascontiguousarray(u))
            flag = np.zeros(n, dtype=bool)
            flag[idx] = True
            displaced.append(flag)
        prob = dict(clean, uv=uv)
        PrTrue = qy.split(clean, PqTrue)[1]
        PqRig0 = qy.join(clean, ry.perturbed(clean, PrTrue, 1.0, 0.03, 1.0, 0.01))
        _cache["outlier"] = {"clean": clean, "prob": prob, "PqTrue": PqTrue, "PrTrue": PrTrue, "Pq0": Pq0, "PqRig0": PqRig0,
                             "displaced": displaced}
    return _cache["outlier"]


LOOP_LOSSES = (("huber", 1.0), ("cauchy", 1.0))


def outlierLoops(joint):
    """The chain of the public surface on the outlier case, in the yardstick, once per mode: a plain loop from the start
    point (rig-only: the true cameras held by the camera mask; joint: every unknown free), then one robust loop per loss
    of LOOP_LOSSES from its result; beside them the plain loop on the clean problem. -> dict: mask, start, plain
    (refineDense's triple), clean (the same on the clean problem), robust {loss: triple}"""
    key = ("loops", bool(joint))
    if key not in _cache:
        oc = outlierCase()
        prob, clean = oc["prob"], oc["clean"]
        mask = 0 if joint else qy.cameraMask(prob)
        start = oc["Pq0"] if joint else oc["PqRig0"]
        plain = qy.refineDense(prob, start, 50, mask)
        _cache[key] = {"mask": mask, "start": start, "plain": plain, "clean": qy.refineDense(clean, start, 50, mask),
                       "robust": {loss: refineDense(prob, plain[1], 50, loss, mask) for loss in LOOP_LOSSES}}
    return _cache[key]
