"""Multi-camera rig calibration: where N known cameras sit relative to camera 0.

stereo.py for N cameras, 2 <= N <= 8. The cameras see M views of one board; each camera's A and k stay as given. Unknowns
are the N - 1 rigs (rig_c takes camera 0's frame into camera c's, Xc = R_c X0 + t_c) and the M board poses in camera 0's
frame: ONE set of poses and one covariance tie the cameras together, which N - 1 stereoCalibrate calls pair by pair do
not give. The start point is host arithmetic on per-view poses (estimatePoses per camera, on the device; a spanning tree
over the camera pairs that share solved views), the refinement is the LM loop of the reference on the device
(calib_refine_rig, csrc/rig.hpp), the covariance host arithmetic on the blocks of calib_rig_normal_eq. With refineCameras
the result of that refinement is the start point of the joint one (calib_refine_rig_joint, csrc/rig_joint.hpp): every
camera's intrinsics and distortion, the rigs and the poses in one problem, and a covariance that counts the cameras'
uncertainty.
"""
from collections import deque

import numpy as np

from . import engine, fixed
from .main import calibrateCamera
from .stereo import (RIG_NAMES, _camera, _solvedPoses, _views, averageTransform, camerasOf, invertPoses, jointCovarianceFromBlocks,
                     parametersToPoses, posesToParameters)


def rigStartPoints(W, ok):
    """Start point of the rig refinement from per-camera, per-view board poses: W (N,M,4,4) board in camera c, ok (N,M)
    which of them are solved. A breadth-first spanning tree from camera 0 over the camera pairs with at least one view
    solved by both, neighbours tried in index order; an edge's transform is stereo.averageTransform over the views both
    solved (rigStartPoint's average), composed along the tree. A view's start pose comes from the lowest-indexed camera
    that solved it, carried into camera 0's frame. -> (T (N,4,4) camera 0's frame into camera c's, T[0] = I; W0 (M,4,4)).
    ValueError naming the first view that no camera solved, or the first camera that no chain of shared views connects
    to camera 0."""
    W = np.asarray(W, dtype=np.float64)
    ok = np.asarray(ok, dtype=bool)
    if W.ndim != 4 or W.shape[2:] != (4, 4) or ok.shape != W.shape[:2]:
        raise ValueError(f"expected W (N,M,4,4) and ok (N,M), got {W.shape} and {ok.shape}")
    N, M = ok.shape
    none = np.flatnonzero(~ok.any(axis=0))
    if none.size:
        raise ValueError(f"view {int(none[0])}: no camera has a solved board pose")
    T = np.tile(np.eye(4), (N, 1, 1))
    reached = np.zeros(N, dtype=bool)
    reached[0] = True
    queue = deque([0])
    while queue:
        a = queue.popleft()
        for b in range(N):
            both = ok[a] & ok[b]
            if reached[b] or not both.any():
                continue
            T[b] = averageTransform(W[a][both], W[b][both]) @ T[a]
            reached[b] = True
            queue.append(b)
    if not reached.all():
        raise ValueError(f"camera {int(np.flatnonzero(~reached)[0])}: no chain of views that two cameras both solved "
                         "connects it to camera 0: its rig has no start point")
    first = np.argmax(ok, axis=0)                                  # the lowest-indexed camera that solved the view
    W0 = invertPoses(T)[first] @ W[first, np.arange(M)]
    return T, W0


class RigCalibration:
    """Result of rigCalibrate: T (N,4,4) camera 0's frame into camera c's (T[0] = I), W list of (4,4) board in camera 0,
    Pr the parameter vector (rig_1, .., rig_{N-1}, pose_0, ..), sse the error AT the result (= sseCam.sum()), sseCam /
    numPoints / rms (N,) per camera (rms NaN for a camera without points), iters, trace (iters, 5 + S).
    sseBeforeLastUpdate is what the refinement itself returns, the reference's convention (src/calibrate.py:171).
    From a joint run (rigCalibrate(refineCameras=True)): Pq = (shared_0 | shared_1, rig_1 | .. | pose_0, ..) the joint
    parameter vector, fixedMask (a Python int) over its S shared unknowns, trace (iters, 5 + S) the joint loop's, rigOnly
    the RigCalibration of the rig-only refinement it continued from; cameras(), rectify, triangulate and triangulateAll
    use the refined cameras.
    From a robust run (rigCalibrate(loss=...)): loss the parsed (name, scale), cost / costCam the sums of rho(|r|^2) at
    the result and sseBeforeLastUpdate the robust loop's own return (a sum of rho), trace the robust loop's; sseCam, sse
    and rms stay the plain sums of |r|^2 at the result, comparable with an L2 run; Pq, fixedMask and rigOnly as from a
    joint run (with refineCameras=False the mask holds every camera bit). Without a loss: loss None, cost = sse."""

    def __init__(self, sseBeforeLastUpdate, Pr, iters, trace, sseCam, problem, device, Pq=None, fixedMask=0, rigOnly=None,
                 loss=None, costCam=None, camerasHeld=False):
        N = len(problem)
        S = 6 * (N - 1)
        self.Pq, self.fixedMask, self.rigOnly = Pq, fixedMask, rigOnly
        self.loss, self._camerasHeld = loss, camerasHeld
        self.costCam = np.asarray(sseCam if costCam is None else costCam, dtype=np.float64)
        self.cost = float(self.costCam.sum())
        self.Pr, self.iters, self.trace, self.sseBeforeLastUpdate = Pr, iters, trace, sseBeforeLastUpdate
        self.sseCam = np.asarray(sseCam, dtype=np.float64)
        self.sse = float(self.sseCam.sum())
        self.T = np.concatenate((np.eye(4)[None], parametersToPoses(Pr[:S])))
        self.W = list(parametersToPoses(Pr[S:]))
        self.numPoints = np.array([int(cam[2][-1]) for cam in problem], dtype=np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.rms = np.where(self.numPoints > 0, np.sqrt(self.sseCam / self.numPoints), np.nan)
        self._problem, self._device = problem, device

    @property
    def numCameras(self):
        return len(self._problem)

    def transform(self, a, b):
        """(4,4) camera a's frame into camera b's: Xb = R Xa + t"""
        return self.T[b] @ invertPoses(self.T[a][None])[0]

    def covariance(self):
        """Covariance (S,S) of the rig parameters (parameterNames) at the result: sigma^2 S_undamped^-1 with
        sigma^2 = sse / (2 n - S - 6 M), the units of CalibrationUncertainty. From a joint run: of the S shared unknowns
        of the joint problem (jointParameterNames), sigma^2 S_free^-1 with dof = 2 n - (S - |F|) - 6 M; rows and columns
        of fixed parameters are exact zeros. From a robust run: of the WEIGHTED blocks (every point's rows times
        sqrt(rho'), first order), sigma^2 = sum_p w_p |r_p|^2 / dof with the plain run's dof; a run that held the cameras
        (refineCameras=False) returns the rig rows and columns only, in parameterNames() order."""
        if self.loss is not None:
            ne = engine.rigRobustNormalEquations(self._problem, self.Pq, self.loss, self._device)
            wss = sum(float(np.sum(w * np.sum(r * r, axis=1))) for w, r in zip(self.weights(), self.residuals()))
            C = jointCovarianceFromBlocks(ne["B"], ne["E"], ne["V"], wss, int(self.numPoints.sum()), self.fixedMask)
            if not self._camerasHeld:
                return C
            rigs = self._rigColumns()
            return C[np.ix_(rigs, rigs)].copy()
        if self.Pq is not None:
            ne = engine.rigJointNormalEquations(self._problem, self.Pq, self._device)
            return jointCovarianceFromBlocks(ne["B"], ne["E"], ne["V"], float(ne["sseCam"].sum()),
                                             int(self.numPoints.sum()), self.fixedMask)
        ne = engine.rigNormalEquations(self._problem, self.Pr, self._device)
        return jointCovarianceFromBlocks(ne["B"], ne["E"], ne["V"], float(ne["sseCam"].sum()), int(self.numPoints.sum()))

    def rigCovariance(self, c):
        """the 6 x 6 block of covariance() of camera c >= 1 (rho_x, rho_y, rho_z in DEGREES, then t)"""
        if not 1 <= c < self.numCameras:
            raise ValueError(f"camera {c!r} has no rig: expected 1 <= c < {self.numCameras}")
        if self.Pq is not None and not self._camerasHeld:
            _, off, L = engine.rigJointLayout([cam[0] for cam in self._problem])
            r = slice(off[c] + L[c], off[c] + L[c] + 6)
            return self.covariance()[r, r].copy()
        return self.covariance()[6 * (c - 1):6 * c, 6 * (c - 1):6 * c].copy()

    def _rigColumns(self):
        """the rig unknowns' places among Pq's shared ones, in parameterNames() order"""
        _, off, L = engine.rigJointLayout([cam[0] for cam in self._problem])
        return np.concatenate([np.arange(off[c] + L[c], off[c] + L[c] + 6) for c in range(1, self.numCameras)])

    def residuals(self):
        """list of (n_c, 2): sensor - projection of every point at the result, on the device (a robust run's)"""
        if self.Pq is None:
            raise ValueError("residuals() belongs to a result with a joint parameter vector: pass loss= or refineCameras=True")
        return engine.rigResiduals(self._problem, self.Pq, self._device)

    def weights(self):
        """list of (n_c,): rho'(|r|^2) of residuals() under the run's loss, 1 without one -- small where the loss took a
        point for an outlier"""
        return [engine.lossWeight(self.loss, np.sum(r * r, axis=1)) for r in self.residuals()]

    def parameterNames(self):
        """names of the S rig unknowns: rig1.rx .. rig{N-1}.tz"""
        return tuple(f"rig{c}.{n}" for c in range(1, self.numCameras) for n in RIG_NAMES)

    def jointParameterNames(self):
        """names of the S shared unknowns of the joint problem: cam0.alpha .. cam0.k.., cam1.alpha .. cam1.k.., rig1.rx ..
        rig1.tz, cam2.alpha .."""
        return jointParameterNames([cam[0] for cam in self._problem])

    def cameras(self):
        """the cameras, each (distortionType, A, k) as rigCalibrate took it -- from a joint run, as it refined them"""
        return camerasOf(self._problem)

    def rectify(self, a, b, size, **kw):
        """rectify.stereoRectify for the pair (a, b): size = (width, height) of the images -> StereoRectification"""
        from . import rectify
        kw.setdefault("device", self._device)
        cams, T = self.cameras(), self.transform(a, b)
        return rectify.stereoRectify(cams[a], cams[b], T[:3, :3].copy(), T[:3, 3].copy(), size, **kw)

    def triangulate(self, a, b, uvA, uvB, returnStatus=False, returnError=False):
        """rectify.triangulate for the pair (a, b): matched pixels (n,2) of the two cameras -> X (n,3) in camera a's frame"""
        from . import rectify
        cams, T = self.cameras(), self.transform(a, b)
        return rectify.triangulate(cams[a], cams[b], T[:3, :3].copy(), T[:3, 3].copy(), uvA, uvB, returnStatus, returnError,
                                   self._device)

    def triangulateAll(self, uv, seen=None, **kw):
        """rectify.triangulateMulti with the rig's own cameras and T: uv (N,n,2), or a list of N (n,2) arrays, the pixels
        of n points in every camera (not finite, or masked out by seen, where a camera did not see the point) -> X (n,3)
        in camera 0's frame, from all the cameras that saw each point at once"""
        from . import rectify
        kw.setdefault("device", self._device)
        return rectify.triangulateMulti(self.cameras(), self.T, uv, seen, **kw)


def jointParameterNames(modelIds):
    """names of Pq's shared unknowns for cameras of these model ids"""
    names = []
    for c, modelId in enumerate(modelIds):
        names += [f"cam{c}.{n}" for n in fixed.sharedNames(modelId)]
        if c:
            names += [f"rig{c}.{n}" for n in RIG_NAMES]
    return tuple(names)


def jointFixed(modelIds, fixedSpecs=None, fixedRigs=()):
    """fixedSpecs: None, or one Calibrator(fixed=...)-style spec per camera; fixedRigs: the cameras c >= 1 whose rig is
    held -> (mask, a Python int over the S shared unknowns of Pq, {index into Pq: value})"""
    N = len(modelIds)
    _, off, L = engine.rigJointLayout(modelIds)
    if fixedSpecs is None:
        fixedSpecs = [None] * N
    fixedSpecs = list(fixedSpecs)
    if len(fixedSpecs) != N:
        raise ValueError(f"expected one fixed spec per camera ({N}), got {len(fixedSpecs)}")
    mask, values = 0, {}
    for c, spec in enumerate(fixedSpecs):
        m, v = fixed.resolveFixed(fixed.sharedNames(modelIds[c]), spec)
        mask |= m << off[c]
        values.update({off[c] + i: x for i, x in v.items()})
    for c in fixedRigs:
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 1 <= c < N:
            raise ValueError(f"fixedRigs: camera {c!r} has no rig: expected 1 <= c < {N}")
        mask |= 0x3f << (off[c] + L[c])
    return mask, values


def packJoint(shared, Pr):
    """the cameras' shared vectors and Pr = (rig_1, .., rig_{N-1}, pose_0, ..) -> Pq, camera-major"""
    N = len(shared)
    Pr = np.asarray(Pr, dtype=np.float64).ravel()
    parts = [np.asarray(shared[0], dtype=np.float64)]
    for c in range(1, N):
        parts += [np.asarray(shared[c], dtype=np.float64), Pr[6 * (c - 1):6 * c]]
    return np.concatenate(parts + [Pr[6 * (N - 1):]])


def unpackJoint(modelIds, Pq):
    """Pq -> (the cameras' shared vectors, Pr)"""
    S, off, L = engine.rigJointLayout(modelIds)
    Pq = np.asarray(Pq, dtype=np.float64).ravel()
    shared = [Pq[off[c]:off[c] + L[c]].copy() for c in range(len(modelIds))]
    rigs = [Pq[off[c] + L[c]:off[c] + L[c] + 6] for c in range(1, len(modelIds))]
    return shared, np.concatenate(rigs + [Pq[S:]])


def rigCalibrate(detections, cameras, maxIters=50, device=0, refineCameras=False, fixed=None, fixedRigs=(), loss=None):
    """The rigs between N KNOWN cameras, 2 <= N <= 8. cameras[c] = (distortionType, A (3,3), k); detections[c]: a list of
    length M, entry i a (sensor (n,2), model (n,3)) pair of view i in camera c, or None / empty where the camera did not
    see the board (the cameras may see different corners). -> RigCalibration.
    refineCameras=True continues from that result with the cameras free: every camera's intrinsics and distortion, the
    rigs and the poses refined together. fixed: one Calibrator(fixed=...)-style spec per camera (values of a {name: value}
    mapping are written into the joint start point); fixedRigs: the cameras c >= 1 whose rig is held there.
    loss: None, "huber", "cauchy" or (name, scale in pixels, default 1.0) -- a robust loss per point. The plain rig-only
    refinement runs as without one (kept as result.rigOnly); ONE robust loop (calib_refine_rig_robust) continues from its
    result, with every camera held unless refineCameras, then with fixed / fixedRigs. Two cameras go through here too:
    stereoCalibrate has no loss."""
    fixedSpecs = fixed
    loss = engine.parseLoss(loss)
    if not refineCameras and (fixedSpecs is not None or len(tuple(fixedRigs))):
        raise ValueError("fixed / fixedRigs apply to the joint refinement: pass refineCameras=True")
    if len(detections) != len(cameras) or not 2 <= len(cameras) <= 8:
        raise ValueError(f"expected 2 to 8 cameras and a detection list for each, got {len(cameras)} and {len(detections)}")
    cams = [_camera(cam, c) for c, cam in enumerate(cameras)]
    views = [_views(dets, c) for c, dets in enumerate(detections)]
    M = len(views[0])
    if M < 1 or any(len(v) != M for v in views):
        raise ValueError(f"expected detection lists of one length >= 1, got {[len(v) for v in views]}")
    solved = [_solvedPoses(cam, v, 20, device) for cam, v in zip(cams, views)]
    T0, W0 = rigStartPoints(np.stack([W for W, _ in solved]), np.stack([ok for _, ok in solved]))
    Pr0 = np.concatenate((posesToParameters(T0[1:]).ravel(), posesToParameters(W0).ravel()))
    problem = tuple((cam[1], cam[4]) + engine.packDetections(v) for cam, v in zip(cams, views))
    sse, Pr, iters, trace, sseCam = engine.refineRig(problem, Pr0, maxIters, device=device)
    result = RigCalibration(sse, Pr, iters, trace, sseCam, problem, device)
    if not refineCameras and loss is None:
        return result
    from . import fixed as fixedModule
    modelIds = [cam[1] for cam in cams]
    if refineCameras:
        mask, values = jointFixed(modelIds, fixedSpecs, tuple(fixedRigs))
    else:                                                          # the robust rig-only problem: every camera bit
        _, off, L = engine.rigJointLayout(modelIds)
        mask, values = sum(((1 << L[c]) - 1) << off[c] for c in range(len(cams))), {}
    Pq0 = fixedModule.applyFixedValues(packJoint([cam[4] for cam in cams], Pr), values)
    if loss is not None:
        cost, Pq, iters, trace, costCam = engine.refineRigRobust(problem, Pq0, maxIters, loss, mask, device=device)
        shared, PrJ = unpackJoint(modelIds, Pq)
        refined = tuple((p[0], sh) + p[2:] for p, sh in zip(problem, shared))
        sseCam = [float(np.sum(r * r)) for r in engine.rigResiduals(refined, Pq, device)]
        return RigCalibration(cost, PrJ, iters, trace, sseCam, refined, device, Pq=Pq, fixedMask=mask, rigOnly=result,
                              loss=loss, costCam=costCam, camerasHeld=not refineCameras)
    sse, Pq, iters, trace, sseCam = engine.refineRigJoint(problem, Pq0, maxIters, mask, device=device)
    shared, PrJ = unpackJoint(modelIds, Pq)
    refined = tuple((p[0], sh) + p[2:] for p, sh in zip(problem, shared))
    return RigCalibration(sse, PrJ, iters, trace, sseCam, refined, device, Pq=Pq, fixedMask=mask, rigOnly=result)


def calibrateRig(detections, types, maxIters, device=0, joint=False, loss=None):
    """Every camera from scratch, then the rigs: calibrateCamera on each camera's own non-empty views, then rigCalibrate
    with the results held fixed. -> (results, rig), results[c] = (sse, A, W, k) as calibrateCamera returns it (W over that
    camera's non-empty views, in order). joint=True passes refineCameras=True: rig.cameras() then holds the jointly refined
    (A, k); results stay the mono ones. loss: rigCalibrate's -- the mono calibrations stay plain."""
    if len(detections) != len(types):
        raise ValueError(f"expected a distortion type per camera, got {len(types)} for {len(detections)} cameras")
    results = []
    for c, (dets, distortionType) in enumerate(zip(detections, types)):
        own = [v for v in _views(dets, c) if v[0].shape[0] > 0]
        results.append(calibrateCamera(own, distortionType, maxIters, device=device))
    rig = rigCalibrate(detections, [(t, A, k) for t, (_, A, _, k) in zip(types, results)], maxIters, device,
                       refineCameras=bool(joint), loss=loss)
    return results, rig
