"""Stereo calibration: where camera b sits relative to camera a -- both cameras known, or refined together with the rig.

The reference stops at one camera; this is surface beside it, like uncertainty.py and undistort.py. Two calibrated
cameras see M views of one board. Unknowns are the rig (Xb = R Xa + t, camera a's frame into camera b's) and the M board
poses in camera a's frame; each camera's A and k stay as given. The start point is host arithmetic on per-view poses
(estimatePoses per camera, on the device), the refinement is the LM loop of the reference on the device
(calib_refine_stereo, csrc/stereo.hpp), and the rig's covariance is host arithmetic on the M 6x6 blocks of
calib_stereo_normal_eq. With refineCameras the result of that refinement is the start point of the joint one
(calib_refine_stereo_joint, csrc/stereo_joint.hpp): intrinsics, distortion, rig and poses in one problem, and a covariance
that counts the cameras' uncertainty.
"""
import numpy as np

from . import calibrate, engine, fixed
from . import mathutils as mu
from .main import _MODELS, calibrateCamera


def _camera(camera, tag):
    """(distortionType, A, k) -> (distortionType, modelId, A (3,3), k, shared (L,) in the order of P)"""
    distortionType, A, k = camera
    if distortionType not in _MODELS:
        raise ValueError(f"camera {tag}: distortion type {distortionType!r} unknown")
    modelId = engine.MODEL_IDS[distortionType]
    A = np.asarray(A, dtype=np.float64).reshape(3, 3)
    k = np.asarray(k, dtype=np.float64).ravel()
    if k.shape[0] != engine.NUM_SHARED[modelId] - 5:
        raise ValueError(f"camera {tag}: expected {engine.NUM_SHARED[modelId] - 5} distortion coefficients, got {k.shape[0]}")
    shared = np.concatenate(([A[0, 0], A[1, 1], A[0, 1], A[0, 2], A[1, 2]], k))
    return distortionType, modelId, A, k, shared


def _views(detections, tag):
    """list of (sensor (n,2), model (n,3)) | None | empty -> list of ((n,2), (n,3)) float64 pairs, n = 0 where unseen"""
    out = []
    for i, d in enumerate(detections):
        if d is None or len(d) == 0 or d[0] is None or len(d[0]) == 0:
            out.append((np.empty((0, 2)), np.empty((0, 3))))
            continue
        s = np.asarray(d[0], dtype=np.float64)
        m = np.asarray(d[1], dtype=np.float64)
        if s.ndim != 2 or s.shape[1] != 2 or m.shape != (s.shape[0], 3):
            raise ValueError(f"camera {tag}, view {i}: expected sensor (N,2) and model (N,3), got {s.shape} and {m.shape}")
        out.append((np.ascontiguousarray(s), np.ascontiguousarray(m)))
    return out


def invertPoses(W):
    """(M,4,4) rigid transforms -> their inverses"""
    W = np.asarray(W, dtype=np.float64).reshape(-1, 4, 4)
    Rt = np.transpose(W[:, :3, :3], (0, 2, 1))
    return mu.posesFromRT(Rt, -np.einsum("nij,nj->ni", Rt, W[:, :3, 3]))


def averageTransform(Wa, Wb):
    """Wa, Wb (n,4,4) board in camera a / b, n >= 1 -> (4,4) camera a's frame into camera b's: T_i = Wb_i Wa_i^-1, the
    rotation nearest sum R_i (SVD, determinant fixed) and the mean t_i"""
    T = Wb @ invertPoses(Wa)
    U, _, Vt = np.linalg.svd(T[:, :3, :3].sum(axis=0))
    R0 = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    return mu.poseFromRT(R0, T[:, :3, 3].mean(axis=0))


def rigStartPoint(Wa, Wb, okA, okB):
    """Start point of the stereo refinement from per-view board poses: Wa, Wb (M,4,4) board in camera a / b, okA, okB
    (M,) which of them are solved. T_i = Wb_i Wa_i^-1 over the views both cameras solved; R0 = the rotation nearest
    sum R_i (SVD, determinant fixed), t0 = mean t_i. A view's start pose is Wa_i where camera a solved it, else
    T0^-1 Wb_i. -> (T0 (4,4), W0 (M,4,4)). ValueError for a view neither camera solved, or when no view has both."""
    Wa = np.asarray(Wa, dtype=np.float64).reshape(-1, 4, 4)
    Wb = np.asarray(Wb, dtype=np.float64).reshape(-1, 4, 4)
    okA, okB = np.asarray(okA, dtype=bool), np.asarray(okB, dtype=bool)
    none = np.flatnonzero(~(okA | okB))
    if none.size:
        raise ValueError(f"view {int(none[0])}: neither camera has a solved board pose")
    both = okA & okB
    if not both.any():
        raise ValueError("no view has a solved board pose in both cameras: the rig has no start point")
    T0 = averageTransform(Wa[both], Wb[both])
    W0 = Wa.copy()
    onlyB = ~okA
    if onlyB.any():
        W0[onlyB] = invertPoses(T0[None])[0] @ Wb[onlyB]
    return T0, W0


def posesToParameters(W):
    """(M,4,4) -> (M,6) rows (rho_x, rho_y, rho_z [degrees], t): the view blocks of P"""
    W = np.asarray(W, dtype=np.float64).reshape(-1, 4, 4)
    return np.hstack((mu.rotationMatricesToEuler(W[:, :3, :3]), W[:, :3, 3]))


def parametersToPoses(e):
    e = np.asarray(e, dtype=np.float64).reshape(-1, 6)
    return mu.posesFromRT(mu.eulerToRotationMatrices(e[:, :3]), e[:, 3:])


RIG_NAMES = ("rx", "ry", "rz", "tx", "ty", "tz")


def jointCovarianceFromBlocks(B, E, V, sse, numPoints, fixedMask=0):
    """sigma^2 S_free^-1 (S,S) of the joint problem: S_free the undamped Schur complement B - sum_i E_i V_i^-1 E_i^T of
    the view blocks restricted to the free shared unknowns, rows and columns of the fixed ones exact zeros, sigma^2 =
    sse / dof with dof = 2 numPoints - (S - |F|) - 6 M. ValueError when dof <= 0."""
    B = np.asarray(B, dtype=np.float64)
    S = B.shape[0]
    E = np.asarray(E, dtype=np.float64).reshape(-1, S, 6)
    V = np.asarray(V, dtype=np.float64).reshape(-1, 6, 6)
    free = np.array([s for s in range(S) if not fixedMask >> s & 1], dtype=int)
    dof = 2 * int(numPoints) - free.size - 6 * V.shape[0]
    if dof <= 0:
        raise ValueError(f"{numPoints} points give {2 * int(numPoints)} equations for {free.size + 6 * V.shape[0]} free "
                         "unknowns: no degrees of freedom are left for the covariance")
    Sc = B - np.einsum("mij,mjk->ik", E, np.linalg.solve(V, np.transpose(E, (0, 2, 1))))
    C = np.zeros((S, S))
    C[np.ix_(free, free)] = (sse / dof) * np.linalg.inv(Sc[np.ix_(free, free)])
    return C


def rigCovarianceFromBlocks(B, E, V, sse, numPoints):
    """sigma^2 S^-1 (6,6; Euler angles in degrees, then t) with S = B - sum_i E_i V_i^-1 E_i^T the undamped Schur
    complement of the view blocks and sigma^2 = sse / (2 numPoints - 6 - 6 M). ValueError when dof <= 0."""
    return jointCovarianceFromBlocks(np.asarray(B, dtype=np.float64).reshape(6, 6), E, V, sse, numPoints)


def camerasOf(problem):
    """the cameras of an engine problem (tuples that begin with modelId, shared) as (distortionType, A, k) each"""
    names = {v: n for n, v in engine.MODEL_IDS.items()}
    return tuple((names[modelId], np.array([[s[0], s[2], s[3]], [0.0, s[1], s[4]], [0.0, 0.0, 1.0]]), s[5:].copy())
                 for modelId, s in ((c[0], np.asarray(c[1], dtype=np.float64)) for c in problem))


class StereoCalibration:
    """Result of stereoCalibrate: sse the error AT the result (= sseA + sseB, the error per camera), R (3,3), t (3,),
    T (4,4) camera a's frame into camera b's, W list of (4,4) board in camera a, iters, rmsA / rmsB per point (NaN for a
    camera without points), trace (iters, 5 + 6). sseBeforeLastUpdate is what the refinement itself returns, the
    reference's convention (src/calibrate.py:171); Ps the parameter vector (rig, pose_0, ..).
    From a joint run (stereoCalibrate(refineCameras=True)): Pj = (shared_a, shared_b, Ps) the joint parameter vector,
    fixedMask over its S shared unknowns, trace (iters, 5 + S) the joint loop's, rigOnly the StereoCalibration of the
    rig-only refinement it continued from; cameras(), rectify and triangulate use the refined cameras."""

    def __init__(self, sseBeforeLastUpdate, Ps, iters, trace, sseA, sseB, numA, numB, problem, device, Pj=None,
                 fixedMask=0, rigOnly=None):
        self.Pj, self.fixedMask, self.rigOnly = Pj, fixedMask, rigOnly
        self.sse, self.sseBeforeLastUpdate, self.iters, self.trace = sseA + sseB, sseBeforeLastUpdate, iters, trace
        self.Ps = Ps
        self.T = parametersToPoses(Ps[:6])[0]
        self.R, self.t = self.T[:3, :3].copy(), self.T[:3, 3].copy()
        self.W = list(parametersToPoses(Ps[6:]))
        self.sseA, self.sseB = sseA, sseB
        self.numPointsA, self.numPointsB = numA, numB
        self.rmsA = np.sqrt(sseA / numA) if numA else np.nan
        self.rmsB = np.sqrt(sseB / numB) if numB else np.nan
        self._problem, self._device = problem, device

    def rigCovariance(self):
        """Covariance (6,6) of the rig parameters (rho_x, rho_y, rho_z in DEGREES, then t) at the result:
        sigma^2 S^-1, sigma^2 = (sseA + sseB) / (2 n - 6 - 6 M), the units of CalibrationUncertainty. From a joint run:
        the rig block of covariance(), which counts the cameras' uncertainty."""
        if self.Pj is not None:
            return self.covariance()[-6:, -6:].copy()
        ne = engine.stereoNormalEquations(*self._problem, self.Ps, self._device)
        return rigCovarianceFromBlocks(ne["B"], ne["E"], ne["V"], ne["sseA"] + ne["sseB"],
                                       self.numPointsA + self.numPointsB)

    def covariance(self):
        """Joint runs only: covariance (S,S) of the shared unknowns (jointParameterNames) at the result, sigma^2 S_free^-1
        with dof = 2 n - (S - |F|) - 6 M; rows and columns of fixed parameters are exact zeros."""
        if self.Pj is None:
            raise ValueError("covariance() needs a joint run (refineCameras=True); rigCovariance() serves the rig-only one")
        ne = engine.stereoJointNormalEquations(*self._problem, self.Pj, self._device)
        return jointCovarianceFromBlocks(ne["B"], ne["E"], ne["V"], ne["sseA"] + ne["sseB"],
                                         self.numPointsA + self.numPointsB, self.fixedMask)

    def jointParameterNames(self):
        """names of the S shared unknowns of the joint problem: a.alpha .. a.k.., b.alpha .. b.k.., rig.rx .. rig.tz"""
        return jointParameterNames(self._problem[0][0], self._problem[1][0])

    def cameras(self):
        """(cameraA, cameraB), each (distortionType, A, k) as stereoCalibrate took it"""
        return camerasOf(self._problem)

    def rectify(self, size, **kw):
        """rectify.stereoRectify for this rig: size = (width, height) of the images -> StereoRectification"""
        from . import rectify
        kw.setdefault("device", self._device)
        return rectify.stereoRectify(*self.cameras(), self.R, self.t, size, **kw)

    def triangulate(self, uvA, uvB, returnStatus=False, returnError=False):
        """rectify.triangulate for this rig: matched pixels (N,2) of the two cameras -> X (N,3) in camera a's frame"""
        from . import rectify
        return rectify.triangulate(*self.cameras(), self.R, self.t, uvA, uvB, returnStatus, returnError, self._device)


def _solvedPoses(camera, views, maxIters, device):
    """estimatePoses on the views this camera can solve (at least 4 points) -> (W (M,4,4), ok (M,))"""
    distortionType, _, A, k, _ = camera
    M = len(views)
    W, ok = np.tile(np.eye(4), (M, 1, 1)), np.zeros(M, dtype=bool)
    idx = [i for i, (s, _) in enumerate(views) if s.shape[0] >= 4]
    if idx:
        cal = calibrate.Calibrator(_MODELS[distortionType](), device=device)
        try:
            _, Wi, _, status = cal.estimatePoses(A, k, [views[i] for i in idx], maxIters)
        finally:
            cal.close()
        W[idx] = np.asarray(Wi)
        ok[idx] = np.asarray(status) == 0
    return W, ok


def jointParameterNames(modelIdA, modelIdB):
    return tuple([f"a.{n}" for n in fixed.sharedNames(modelIdA)] + [f"b.{n}" for n in fixed.sharedNames(modelIdB)] +
                 [f"rig.{n}" for n in RIG_NAMES])


def jointFixed(modelIdA, modelIdB, fixedA, fixedB):
    """fixedA / fixedB as Calibrator(fixed=...) takes them, per camera model -> (mask over the S joint shared unknowns,
    {index into Pj: value})"""
    La = engine.NUM_SHARED[modelIdA]
    maskA, valuesA = fixed.resolveFixed(fixed.sharedNames(modelIdA), fixedA)
    maskB, valuesB = fixed.resolveFixed(fixed.sharedNames(modelIdB), fixedB)
    values = dict(valuesA)
    values.update({La + i: v for i, v in valuesB.items()})
    return maskA | maskB << La, values


def stereoCalibrate(detectionsA, detectionsB, cameraA, cameraB, maxIters=50, device=0, refineCameras=False, fixedA=None,
                    fixedB=None):
    """The rig between two KNOWN cameras. camera = (distortionType, A (3,3), k); detectionsA / detectionsB: lists of
    equal length M, entry i a (sensor (n,2), model (n,3)) pair of view i in that camera, or None / empty where the
    camera did not see the board (the cameras may see different corners). -> StereoCalibration.
    refineCameras=True continues from that result with the cameras free: intrinsics, distortion, rig and poses refined
    together. fixedA / fixedB hold shared parameters of a camera fixed there (what Calibrator(fixed=...) takes; values of
    a {name: value} mapping are written into the joint start point)."""
    if not refineCameras and (fixedA is not None or fixedB is not None):
        raise ValueError("fixedA / fixedB apply to the joint refinement: pass refineCameras=True")
    camA, camB = _camera(cameraA, "a"), _camera(cameraB, "b")
    viewsA, viewsB = _views(detectionsA, "a"), _views(detectionsB, "b")
    if len(viewsA) != len(viewsB) or not viewsA:
        raise ValueError(f"expected two detection lists of one length >= 1, got {len(viewsA)} and {len(viewsB)}")
    Wa, okA = _solvedPoses(camA, viewsA, 20, device)
    Wb, okB = _solvedPoses(camB, viewsB, 20, device)
    T0, W0 = rigStartPoint(Wa, Wb, okA, okB)
    Ps0 = np.concatenate((posesToParameters(T0[None]).ravel(), posesToParameters(W0).ravel()))
    problem = tuple((cam[1], cam[4]) + engine.packDetections(views) for cam, views in ((camA, viewsA), (camB, viewsB)))
    sse, Ps, iters, trace, (sseA, sseB) = engine.refineStereo(*problem, Ps0, maxIters, device=device)
    result = StereoCalibration(sse, Ps, iters, trace, sseA, sseB, int(problem[0][2][-1]), int(problem[1][2][-1]), problem,
                               device)
    if not refineCameras:
        return result
    mask, values = jointFixed(camA[1], camB[1], fixedA, fixedB)
    Pj0 = fixed.applyFixedValues(np.concatenate((camA[4], camB[4], Ps)), values)
    sse, Pj, iters, trace, (sseA, sseB) = engine.refineStereoJoint(*problem, Pj0, maxIters, mask, device=device)
    La, Lab = camA[4].shape[0], camA[4].shape[0] + camB[4].shape[0]
    refined = ((problem[0][0], Pj[:La].copy()) + problem[0][2:], (problem[1][0], Pj[La:Lab].copy()) + problem[1][2:])
    return StereoCalibration(sse, Pj[Lab:].copy(), iters, trace, sseA, sseB, result.numPointsA, result.numPointsB, refined,
                             device, Pj=Pj, fixedMask=mask, rigOnly=result)


def calibrateStereo(detectionsA, detectionsB, typeA, typeB, maxIters, device=0, joint=False):
    """Both cameras from scratch, then the rig: calibrateCamera on each camera's own non-empty views, then
    stereoCalibrate with the two results held fixed. -> (resultA, resultB, stereo), resultX = (sse, A, W, k) as
    calibrateCamera returns it (W over that camera's non-empty views, in order). joint=True passes refineCameras=True:
    stereo.cameras() then holds the jointly refined (A, k); resultA / resultB stay the mono ones."""
    results = []
    for dets, distortionType, tag in ((detectionsA, typeA, "a"), (detectionsB, typeB, "b")):
        own = [v for v in _views(dets, tag) if v[0].shape[0] > 0]
        results.append(calibrateCamera(own, distortionType, maxIters, device=device))
    (_, Aa, _, ka), (_, Ab, _, kb) = results
    stereo = stereoCalibrate(detectionsA, detectionsB, (typeA, Aa, ka), (typeB, Ab, kb), maxIters, device,
                             refineCameras=bool(joint))
    return results[0], results[1], stereo
