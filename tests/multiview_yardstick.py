"""Yardstick of the N-view triangulation tests (a helper, not a test): the contract of calib_triangulate_multi in
include/calib_lm.h restated in numpy fp64, slow and plain. The forward model is rectify_yardstick.projectCamera (the
oracle's distortion), the inverse rectify_yardstick.newtonInverse, the Jacobian central differences as in
rectify_yardstick.triJacobian. Scenes are rig_yardstick.makeRig with every corner kept and a random mask per point.

A camera is (modelName, A (3,3), k); T (N,4,4) takes the frame of X into each camera's, X_c = T[c] X; uv is (N,n,2),
camera-major; seen is (N,n) bool here and an (n,) uint32 word per point at the library's door (maskWords)."""
import functools

import numpy as np

import rectify_yardstick as ry
import rig_yardstick as rk

MAX_ITERS, LAMBDA0, PARALLEL = 20, 1e-3, 1e-12
STEP_LEAVE, STEP_DONE, PIXEL_ULPS = 1e-14, 1e-9, 2.0**-44


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def maskWords(seen):
    """(N,n) bool -> (n,) uint32, bit c set where camera c saw the point"""
    seen = np.asarray(seen, dtype=bool)
    return (seen.astype(np.uint32) << np.arange(seen.shape[0], dtype=np.uint32)[:, None]).sum(axis=0, dtype=np.uint32)


def randomMasks(N, n, seed, p=0.7):
    """(N,n) bool: each camera sees each point with probability p; a point seen by fewer than two cameras gets cameras
    added, in a random order, until two see it"""
    rng = np.random.default_rng(seed)
    seen = rng.random((N, n)) < p
    for i in np.flatnonzero(seen.sum(axis=0) < 2):
        for c in rng.permutation(N):
            if seen[:, i].sum() >= 2:
                break
            seen[c, i] = True
    return seen


# The noisy scenes' seed. A test that compares a squared error to 1e-9 RELATIVE presumes residuals far above the rounding
# of a projected pixel: two fp64 forward models differ by some 4 ulp of a coordinate of ~500 px, delta = 4.5e-13 px, which
# moves sse by 2 sqrt(sse) delta -- below 1e-9 sse only where sse >= (2 delta / 1e-9)^2 = 8e-7 px^2. Two cameras leave
# one degree of freedom per point, so 0.3 px noise now and then agrees to 1e-5 px: makeRig's default seed 7 has a point
# with sse 3.3e-10 px^2 at N = 2, where no fp64 code can meet that bar. Seed 8 is the first from 7 upward whose scenes
# (N in 2, 3, 8; M = 3) keep every point's error above 1e-6 px^2 in the yardstick's own loop; test_multiview_cpu.py holds
# that. The kernel's behaviour on nearly consistent pixels is test_gpu_rectify's subject (the flat rule).
NOISE_SEED = 8


@functools.lru_cache(maxsize=None)
def scene(N, M, noiseSigma=0.0, seed=11):
    """-> dict cameras [(name, A, k)], T (N,4,4), uv (N,n,2), seen (N,n) bool, X (n,3) the true points in camera 0's
    frame: M views of the 9 x 6 board in front of makeRig's N cameras (radtan and fisheye alternating), n = 54 M; seed
    is the masks', the noise has NOISE_SEED"""
    prob, PrTrue = rk.makeRig(N, M, noiseSigma=noiseSigma, seed=NOISE_SEED)
    names = [("radtan", "fisheye")[c % 2] for c in range(N)]
    out = {"cameras": rk.cameraTuples(prob, names), "T": rk.rigTransforms(prob, PrTrue), "uv": np.stack(prob["uv"]),
           "X": rk.pointsIn0(prob, PrTrue, 0)[0]}
    out["seen"] = randomMasks(N, out["X"].shape[0], seed)
    for a in (out["T"], out["uv"], out["X"], out["seen"]):
        a.setflags(write=False)
    return out


# ---- the contract -----------------------------------------------------------------------------------------------------------
def inverse(cameras, uv):
    """-> (xy (N,n,2) ideal normalised points, status (N,n)) by the numpy Newton"""
    got = [ry.newtonInverse(cam, p) for cam, p in zip(cameras, uv)]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def rays(T, xy):
    """-> (o (N,3) the cameras' centres -R^T t, d (N,n,3) the rays R^T (x, y, 1), both in the frame of X)"""
    T = np.asarray(T, dtype=np.float64)
    o = -np.einsum("cji,cj->ci", T[:, :3, :3], T[:, :3, 3])
    d = np.einsum("cji,cnj->cni", T[:, :3, :3], np.concatenate((xy, np.ones(xy.shape[:2] + (1,))), axis=2))
    return o, d


def closestPoint(T, xy, seen):
    """(n,3): the point closest in least squares to the seen rays, sum_c (I - dd^T / |d|^2) (X - o_c) = 0"""
    o, d = rays(T, xy)
    with np.errstate(all="ignore"):
        P = np.eye(3) - np.einsum("cni,cnj->cnij", d, d) / (d * d).sum(axis=2)[:, :, None, None]
        P = np.where(np.asarray(seen)[:, :, None, None], P, 0.0)
        A, b = P.sum(axis=0), np.einsum("cnij,cj->ni", P, o)
        X = np.full(b.shape, np.nan)
        for i in range(b.shape[0]):
            if np.isfinite(A[i]).all() and np.linalg.matrix_rank(A[i]) == 3:
                X[i] = np.linalg.solve(A[i], b[i])
    return X


def maxPairSin2(T, xy, seen):
    """(n,): the largest sin^2 of the angle between two seen rays, (aa bb - ab^2) / (aa bb); -inf without a pair"""
    _, d = rays(T, xy)
    N = d.shape[0]
    best = np.full(d.shape[1], -np.inf)
    with np.errstate(all="ignore"):
        for a in range(N):
            for b in range(a):
                aa, bb, ab = (d[a] * d[a]).sum(1), (d[b] * d[b]).sum(1), (d[a] * d[b]).sum(1)
                s = (aa * bb - ab * ab) / (aa * bb)
                both = seen[a] & seen[b] & np.isfinite(s)
                best = np.where(both, np.maximum(best, s), best)
    return best


def inCameras(T, X):
    """(N,n,3): X in every camera's frame"""
    T = np.asarray(T, dtype=np.float64)
    return np.einsum("cij,nj->cni", T[:, :3, :3], X) + T[:, None, :3, 3]


def residuals(cameras, T, X, uv):
    """(N,n,2): uv_c - project_c(T[c] X), whatever was seen"""
    Xc = inCameras(T, np.asarray(X, dtype=np.float64))
    with np.errstate(all="ignore"):
        return np.stack([p - ry.projectCamera(cam, x) for cam, p, x in zip(cameras, uv, Xc)])


def jacobian(cameras, T, X, rel=1e-5):
    """(N,n,2,3): d(projection)/dX by central differences with step rel |X| per point (rectify_yardstick.triJacobian)"""
    X = np.asarray(X, dtype=np.float64)
    zero = np.zeros((len(cameras), X.shape[0], 2))
    h = rel * np.linalg.norm(X, axis=1)
    J = np.empty((len(cameras), X.shape[0], 2, 3))
    for c in range(3):
        d = np.zeros_like(X)
        d[:, c] = h
        J[:, :, :, c] = -(residuals(cameras, T, X + d, zero) - residuals(cameras, T, X - d, zero)) / (2 * h)[None, :, None]
    return J


def seenOnly(a, seen):
    """a (N,n,...) with the entries of unseen cameras set to 0"""
    seen = np.asarray(seen)
    return np.where(seen.reshape(seen.shape + (1,) * (a.ndim - 2)), a, 0.0)


def evaluate(cameras, T, X, uv, seen, rel=1e-5):
    """-> (err (n,), N (n,3,3) = J^T J, g (n,3) = J^T r, front (n,) bool, r (N,n,2) with unseen 0, J (N,n,2,3) with
    unseen 0) over the seen cameras"""
    with np.errstate(all="ignore"):
        r = seenOnly(residuals(cameras, T, X, uv), seen)
        J = seenOnly(jacobian(cameras, T, X, rel), seen)
        front = np.where(seen, inCameras(T, X)[:, :, 2] > 0.0, True).all(axis=0)
        return (r * r).sum(axis=(0, 2)), np.einsum("cnki,cnkj->nij", J, J), np.einsum("cnki,cnk->ni", J, r), front, r, J


def covariance(cameras, T, X, seen, rel=1e-5):
    """(n,3,3): the undamped (J^T J)^-1 at X; NaN where it is not positive definite"""
    X = np.asarray(X, dtype=np.float64)
    zero = np.zeros((len(cameras), X.shape[0], 2))
    Nm = evaluate(cameras, T, X, zero, seen, rel)[1]
    out = np.full(Nm.shape, np.nan)
    for i in range(Nm.shape[0]):
        if np.isfinite(Nm[i]).all() and (np.linalg.eigvalsh(Nm[i]) > 0).all():
            out[i] = np.linalg.inv(Nm[i])
    return out


def positiveDefinite(A):
    """(n,) bool: the pivots of the Cholesky factorisation of A (n,3,3) are positive (leading minors)"""
    with np.errstate(all="ignore"):
        m1 = A[:, 0, 0]
        m2 = A[:, 0, 0] * A[:, 1, 1] - A[:, 1, 0] ** 2
        return (m1 > 0) & (m2 > 0) & (np.linalg.det(A) > 0)


def triangulate(cameras, T, uv, seen):
    """The whole contract -> dict X (n,3), sse (n,), status (n,), X0 (n,3) the start, sin2 (n,), sse0 (n,) the error at
    the start: closest-point start, max-pair sin^2 rule, the damped loop with the flat rule, the statuses in their
    order of precedence"""
    uv, seen = np.asarray(uv, dtype=np.float64), np.asarray(seen, dtype=bool)
    n = uv.shape[1]
    xy, inv = inverse(cameras, np.where(seen[:, :, None], uv, 0.0))
    enough = seen.sum(axis=0) >= 2
    solved = ~((inv != 0) & seen).any(axis=0)
    X0 = closestPoint(T, xy, seen)
    sin2 = maxPairSin2(T, xy, seen)
    with np.errstate(all="ignore"):
        eta = PIXEL_ULPS * np.maximum(1.0, np.where(seen[:, :, None], np.abs(uv), 0.0).max(axis=(0, 2)))
        X = X0.copy()
        err, Nm, g, front, _, _ = evaluate(cameras, T, X, uv, seen)
        sse0 = err.copy()
        geometry = (sin2 >= PARALLEL) & np.isfinite(X).all(axis=1) & front
        live = enough & solved & geometry
        lam, last = np.full(n, LAMBDA0), np.zeros(n)
        for _ in range(MAX_ITERS):
            if not live.any():
                break
            A = Nm + lam[:, None, None] * (Nm * np.eye(3))
            pd = positiveDefinite(A)
            geometry &= ~(live & ~pd)
            live &= pd
            dl = np.zeros((n, 3))
            idx = np.flatnonzero(live)
            if idx.size == 0:
                break
            dl[idx] = np.linalg.solve(A[idx], g[idx][:, :, None])[:, :, 0]
            Xn = X + dl
            errN, NmN, gN, frontN, _, _ = evaluate(cameras, T, np.where(live[:, None], Xn, X), uv, seen)
            pred = (dl * g).sum(axis=1)
            flat = eta * (2.0 * np.sqrt(err) + eta)
            accept = live & frontN & ((errN < err) | ((pred <= flat) & (errN <= err + flat)))
            step = np.linalg.norm(dl, axis=1)
            X = np.where(accept[:, None], Xn, X)
            err, g = np.where(accept, errN, err), np.where(accept[:, None], gN, g)
            Nm = np.where(accept[:, None, None], NmN, Nm)
            front = np.where(accept, frontN, front)
            last = np.where(accept, step, last)
            lam = np.where(live, np.where(accept, lam * 0.1, lam * 10.0), lam)
            live &= ~(step <= STEP_LEAVE * np.linalg.norm(X, axis=1))
        geometry &= front
        status = np.where(~enough, 4, np.where(~solved, 1, np.where(~geometry, 2, np.where(
            ~(last <= STEP_DONE * np.linalg.norm(X, axis=1)), 3, 0)))).astype(np.int32)
    bad = status != 0
    return {"X": np.where(bad[:, None], np.nan, X), "sse": np.where(bad, np.nan, err), "status": status, "X0": X0,
            "sin2": sin2, "sse0": sse0}


def gradientCheck(cameras, T, X, uv, seen):
    """-> (|J^T r| (n,), |J|_2 |r| (n,), sse (n,), r (N,n,2) with unseen 0) at X, by the yardstick's own model"""
    err, _, g, _, r, J = evaluate(cameras, T, X, uv, seen)
    Jd = J.transpose(1, 0, 2, 3).reshape(J.shape[1], -1, 3)
    scale = np.linalg.norm(Jd, ord=2, axis=(1, 2)) * np.sqrt(err)
    return np.linalg.norm(g, axis=1), scale, err, r
