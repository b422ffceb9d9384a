"""Using a calibrated rig: stereo rectification, and 3-D points from matched pixels.

The reference stops at one camera; this is surface beside it, like undistort.py and stereo.py. stereoCalibrate finds
the rig (Xb = R Xa + t); here that rig is used. The rectifying rotations, the projection matrices and the choice of the
focal length are host arithmetic (numpy); what runs per pixel or per point runs on the device: the maps
(calib_rectify_maps), the inverse model under rectifyPoints and under the focal length's sample grid
(calib_undistort_points), the resampling (calib_remap) and the triangulation (calib_triangulate, csrc/rectify.hpp; from
every camera of a rig at once: calib_triangulate_multi, csrc/triangulate_multi.hpp).
"""
import numpy as np

from . import engine
from .stereo import _camera
from .undistort import _MODELS, remap

GRID = 17      # samples per side of the grid that measures a camera's field of view (stereoRectify, alpha)


# ---- rotations ---------------------------------------------------------------------------------------------------------
def rotationFromVector(w):
    """Rodrigues: the rotation by |w| radians about w; exactly I for w = 0"""
    w = np.asarray(w, dtype=np.float64).ravel()
    theta = float(np.linalg.norm(w))
    if theta == 0.0:
        return np.eye(3)
    x, y, z = w / theta
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def rotationVector(R):
    """the rotation vector of R (angle below 180 degrees): axis from the antisymmetric part, angle = atan2(sin, cos)"""
    R = np.asarray(R, dtype=np.float64)
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = float(np.linalg.norm(v)), 0.5 * (float(np.trace(R)) - 1.0)
    if s == 0.0:
        return np.zeros(3)
    return v * (np.arctan2(s, c) / s)


def rectifyRotations(R, t):
    """Bouguet's construction for a rig Xb = R Xa + t -> (R1, R2, axis): R1 rotates camera a's frame and R2 camera b's
    so that both look the same way (R1 = R2 R) with the baseline R2 t along e_axis, axis = 0 (a horizontal rig) or 1 (a
    vertical one). Each camera turns by half of R, then both turn by the smallest rotation that lays the baseline on
    the axis. ValueError for t = 0 and for a relative rotation of 90 degrees or more. A rig that is rectified already
    (R = I, t along +-x or +-y) returns R1 = R2 = I exactly."""
    R = np.asarray(R, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64).ravel()
    if R.shape != (3, 3) or t.shape != (3,):
        raise ValueError(f"expected R (3, 3) and t (3,), got {R.shape} and {t.shape}")
    if not np.all(np.isfinite(R)) or not np.all(np.isfinite(t)) or not np.any(t != 0.0):
        raise ValueError("t = 0 (or a value that is not finite): the cameras share a centre and there is no baseline")
    if not np.trace(R) - 1.0 > 0.0:
        raise ValueError("the cameras are rotated against each other by 90 degrees or more: they cannot be rectified")
    om = rotationVector(R)
    rr = rotationFromVector(-0.5 * om)
    tt = rr @ t
    axis = 0 if abs(tt[0]) > abs(tt[1]) else 1
    uu = np.zeros(3)
    uu[axis] = 1.0 if tt[axis] > 0 else -1.0
    ww = np.cross(tt, uu)
    nw = float(np.linalg.norm(ww))
    if nw > 0.0:
        ww *= np.arctan2(nw, abs(tt[axis])) / nw          # = acos(|tt[axis]| / |tt|), without its loss near 0
    wR = rotationFromVector(ww)
    return wR @ rr.T, wR @ rr, axis


# ---- the focal length from the cameras' fields of view ---------------------------------------------------------------------
def sampleGrid(size):
    """(GRID, GRID, 2) source pixels (col j (w - 1) / 16, row i (h - 1) / 16), indexed [i, j]"""
    w, h = size
    jj, ii = np.meshgrid(np.arange(GRID) * ((w - 1) / (GRID - 1.0)), np.arange(GRID) * ((h - 1) / (GRID - 1.0)))
    return np.stack((jj, ii), axis=-1)


_ALPHA_HINT = "pass alpha=None and choose the focal length yourself (focal=)"


def rectifiedGrid(xy, status, Rc, tag=""):
    """The grid's ideal normalised points xy (GRID, GRID, 2) rotated by Rc and divided by Z -> (GRID, GRID, 2).
    ValueError where the model has no inverse at a sample (status 1) or a rotated sample has Z <= 0."""
    xy = np.asarray(xy, dtype=np.float64).reshape(GRID, GRID, 2)
    if np.any(np.asarray(status) != 0):
        raise ValueError(f"camera {tag}: the distortion model has no inverse at {int(np.count_nonzero(status))} of the "
                         f"{GRID * GRID} samples of its image, so its field of view cannot be measured: {_ALPHA_HINT}")
    X = np.concatenate((xy, np.ones((GRID, GRID, 1))), axis=-1) @ np.asarray(Rc, dtype=np.float64).T
    if not np.all(X[..., 2] > 0.0):
        raise ValueError(f"camera {tag}: part of its image looks backwards after the rectifying rotation: {_ALPHA_HINT}")
    return X[..., :2] / X[..., 2:]


def innerRectangle(p):
    """(lo (2,), hi (2,)): the largest rectangle inside the grid's outline as its border samples show it -- the max over
    the left column, the min over the right column, the max over the top row, the min over the bottom row"""
    return (np.array([p[:, 0, 0].max(), p[0, :, 1].max()]), np.array([p[:, -1, 0].min(), p[-1, :, 1].min()]))


def outerRectangle(p):
    """(lo (2,), hi (2,)): the bounding box of all samples"""
    return p.reshape(-1, 2).min(axis=0), p.reshape(-1, 2).max(axis=0)


def focalRange(grids, qs, os_, newSize):
    """-> (f_in, f_out). A rectified pixel is f (p - q) + o. f_in is the smallest f at which every camera's INNER
    rectangle covers [0, W' - 1] x [0, H' - 1] (every destination pixel shows the source: alpha = 0), f_out the largest
    at which every OUTER rectangle lies inside it (every source pixel is kept: alpha = 1): the max, respectively the
    min, over the cameras and the four sides of o / (q - lo) and (W' - 1 - o) / (hi - q)."""
    far = np.array([newSize[0] - 1.0, newSize[1] - 1.0])
    fin, fout = [], []
    for p, q, o in zip(grids, qs, os_):
        lo, hi = innerRectangle(p)
        if not (np.all(lo < q) and np.all(q < hi)):
            raise ValueError(f"a camera's inner rectangle does not contain its centre: {_ALPHA_HINT}")
        fin += list(o / (q - lo)) + list((far - o) / (hi - q))
        lo, hi = outerRectangle(p)
        fout += list(o / (q - lo)) + list((far - o) / (hi - q))
    return float(max(fin)), float(min(fout))


def _deviceInverse(device):
    def inverse(camera, uv):
        _, modelId, A, k, _ = camera
        return engine.undistortPoints(modelId, A, k, uv, device=device)
    return inverse


def _size(size, name):
    try:
        w, h = size
        w, h = int(w), int(h)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: expected (width, height), got {size!r}") from None
    if w < 1 or h < 1:
        raise ValueError(f"{name}: width and height must be positive, got ({w}, {h})")
    return w, h


def _focal(cams, sizes, rotations, qs, os_, newSize, alpha, inverse):
    grids = [rectifiedGrid(*inverse(cam, sampleGrid(sz).reshape(-1, 2)), Rc, tag)
             for cam, sz, Rc, tag in zip(cams, sizes, rotations, "ab")]
    fin, fout = focalRange(grids, qs, os_, newSize)
    return (1.0 - alpha) * fin + alpha * fout


def _rectification(cameraA, cameraB, R, t, size, sizeB, newSize, alpha, focal, zeroDisparity, inverse):
    """stereoRectify's arithmetic -> dict of the fields of StereoRectification; inverse(camera, uv (N,2)) -> (xy, status)
    is what takes the grid's pixels to ideal normalised points (on the device in stereoRectify)"""
    cams = (_camera(cameraA, "a"), _camera(cameraB, "b"))
    sizes = (_size(size, "size"), _size(size if sizeB is None else sizeB, "sizeB"))
    newSize = _size(sizes[0] if newSize is None else newSize, "newSize")
    t = np.asarray(t, dtype=np.float64).ravel()
    R1, R2, axis = rectifyRotations(R, t)
    rotations = (R1, R2)
    qs = [Rc[:2, 2] / Rc[2, 2] for Rc in rotations]                 # where each optical axis points after the rotation
    os_ = [np.array([cam[2][0, 2] * newSize[0] / sz[0], cam[2][1, 2] * newSize[1] / sz[1]])
           for cam, sz in zip(cams, sizes)]                         # .. and the pixel it keeps
    for c in ((0, 1) if zeroDisparity else (1 - axis,)):           # the coordinates both cameras share
        qs[0][c] = qs[1][c] = 0.5 * (qs[0][c] + qs[1][c])
        os_[0][c] = os_[1][c] = 0.5 * (os_[0][c] + os_[1][c])
    if focal is not None:
        f = float(focal)
    elif alpha is None:
        f = float(min(cam[2][1 - axis, 1 - axis] for cam in cams))  # beta for a horizontal rig, alpha for a vertical one
    else:
        f = _focal(cams, sizes, rotations, qs, os_, newSize, float(alpha), inverse)
    if not (np.isfinite(f) and f > 0.0):
        raise ValueError(f"the focal length of the rectified pair must be positive, got {f!r}")
    centres = [o - f * q for q, o in zip(qs, os_)]
    P1, P2 = (np.array([[f, 0.0, c[0], 0.0], [0.0, f, c[1], 0.0], [0.0, 0.0, 1.0, 0.0]]) for c in centres)
    T = float((R2 @ t)[axis])
    P2[axis, 3] = f * T
    Q = np.zeros((4, 4))
    Q[0, 0] = Q[1, 1] = 1.0
    Q[0, 3], Q[1, 3], Q[2, 3] = -centres[0][0], -centres[0][1], f
    Q[3, 2], Q[3, 3] = -1.0 / T, (centres[0][axis] - centres[1][axis]) / T
    return dict(R1=R1, R2=R2, P1=P1, P2=P2, Q=Q, axis=axis, baseline=float(np.linalg.norm(t)), newSize=newSize,
                cameras=tuple((cam[0], cam[2], cam[3]) for cam in cams))


class StereoRectification:
    """Result of stereoRectify. R1, R2 (3,3) rotate camera a's / b's frame into the common rectified one; P1, P2 (3,4)
    project a point of the rectified frame of camera a into the rectified images (P2[axis, 3] = f times the baseline);
    Q (4,4) takes (u, v, d, 1), d = u_a - u_b (v_a - v_b for a vertical rig, axis = 1), to homogeneous X in the
    rectified frame of camera a; baseline = |t|; newSize = (width, height) of the rectified images."""

    def __init__(self, fields, device=0):
        self.__dict__.update(fields)
        self._device = device
        self._maps = {}

    def _side(self, which):
        if which not in ("a", "b"):
            raise ValueError(f"which: expected 'a' or 'b', got {which!r}")
        i = "ab".index(which)
        distortionType, A, k = self.cameras[i]
        return _MODELS[distortionType](), A, k, (self.R1, self.R2)[i], (self.P1, self.P2)[i]

    def maps(self, which):
        """(mapx, mapy), float32 (height, width) of newSize, for camera 'a' or 'b'; built once and kept"""
        if which not in self._maps:
            model, A, k, Rc, P = self._side(which)
            self._maps[which] = engine.rectifyMaps(model.modelId, A, k, Rc, P, *self.newSize, device=self._device)
        return self._maps[which]

    def rectifyPoints(self, which, uv, returnStatus=False):
        """uv (N,2) pixels of camera 'a' or 'b' -> (N,2) pixels of its rectified image (NaN rows: see
        DistortionModel.rectifyPoints)"""
        model, A, k, Rc, P = self._side(which)
        out, status = engine.rectifyPoints(model.modelId, A, k, uv, Rc, P, device=self._device)
        return (out, status) if returnStatus else out

    def reproject(self, uvd):
        """(N,3) rows (u, v, d) of the rectified image of camera a -> (N,3) points of its rectified frame: Q applied"""
        uvd = np.asarray(uvd, dtype=np.float64)
        if uvd.ndim != 2 or uvd.shape[1] != 3:
            raise ValueError(f"uvd: expected shape (None, 3), got {uvd.shape}")
        X = np.concatenate((uvd, np.ones((uvd.shape[0], 1))), axis=1) @ self.Q.T
        with np.errstate(divide="ignore", invalid="ignore"):
            return X[:, :3] / X[:, 3:]

    def apply(self, imageA, imageB, border=0):
        """the rectified pair: each image resampled through its camera's maps (remap's rules)"""
        return remap(imageA, *self.maps("a"), border), remap(imageB, *self.maps("b"), border)


def stereoRectify(cameraA, cameraB, R, t, size, sizeB=None, newSize=None, alpha=None, focal=None, zeroDisparity=True,
                  device=0):
    """Rectify a calibrated rig: camera = (distortionType, A (3,3), k) as in stereoCalibrate, Xb = R Xa + t, size =
    (width, height) of camera a's images (sizeB: camera b's, default the same; newSize: the rectified images', default
    size). -> StereoRectification.

    A rectified pixel of camera c is f (p - q_c) + o_c, p = (X / Z, Y / Z) of the rotated ray: q_c is where the
    camera's own optical axis points after the rotation and o_c its principal point scaled to newSize, so each axis
    keeps its pixel -- except that the coordinates both images share are set to the mean over the two cameras: both
    with zeroDisparity (a point at infinity has disparity 0), else only the one across the baseline (rows for a
    horizontal rig). The common focal length f is `focal` if given; else, with alpha=None, the smaller of the cameras'
    beta (alpha for a vertical rig); else (1 - alpha) f_in + alpha f_out, where at f_in every rectified pixel shows
    the source (alpha = 0) and at f_out every source pixel is kept (alpha = 1), both measured on a 17 x 17 grid of
    each image (focalRange). ValueError where that grid cannot be measured (a sample without an inverse, or behind
    the rectified camera)."""
    return StereoRectification(_rectification(cameraA, cameraB, R, t, size, sizeB, newSize, alpha, focal, zeroDisparity,
                                              _deviceInverse(device)), device)


def _newCameraMatrix(model, A, k, size, alpha, newSize, inverse):
    model = model if isinstance(model, str) else model.modelName
    cam = _camera((model, A, k), "")
    size = _size(size, "size")
    newSize = _size(size if newSize is None else newSize, "newSize")
    q = np.zeros(2)
    o = np.array([cam[2][0, 2] * newSize[0] / size[0], cam[2][1, 2] * newSize[1] / size[1]])
    f = _focal((cam,), (size,), (np.eye(3),), (q,), (o,), newSize, float(alpha), inverse)
    return np.array([[f, 0.0, o[0]], [0.0, f, o[1]], [0.0, 0.0, 1.0]])


def optimalNewCameraMatrix(model, A, k, size, alpha, newSize=None, device=0):
    """The camera matrix for Undistorter(..., newA=): stereoRectify's rule for one camera without a rotation. alpha = 0:
    every pixel of the undistorted image shows the source; alpha = 1: every source pixel is kept; between: the focal
    lengths interpolated. The principal point is A's, scaled to newSize (default size)."""
    return _newCameraMatrix(model, A, k, size, alpha, newSize, _deviceInverse(device))


# ---- triangulation ---------------------------------------------------------------------------------------------------------
def triangulate(cameraA, cameraB, R, t, uvA, uvB, returnStatus=False, returnError=False, device=0):
    """3-D points from matched pixels uvA, uvB (N,2) of two calibrated cameras joined by Xb = R Xa + t, under each
    camera's full model: -> X (N,3) in camera a's frame, the minimiser of the four pixel residuals (start: the midpoint
    of the two rays' common perpendicular; then damped Gauss-Newton on the device). returnStatus adds the (N,) int32
    status -- 0 ok, 1 a pixel without an inverse, 2 degenerate geometry (parallel or diverging rays), 3 not converged;
    X is NaN where it is not 0 -- and returnError the (N,) squared pixel error at X."""
    camA, camB = _camera(cameraA, "a"), _camera(cameraB, "b")
    X, sse, status = engine.triangulate(camA[1], camA[2], camA[3], camB[1], camB[2], camB[3], R, t, uvA, uvB, device)
    out = (X,) + ((status,) if returnStatus else ()) + ((sse,) if returnError else ())
    return out[0] if len(out) == 1 else out


def seenMasks(uv):
    """(N,n,2) pixels -> (n,) uint32: bit c set where both coordinates of camera c's pixel are finite"""
    ok = np.isfinite(uv).all(axis=2)
    return (ok.astype(np.uint32) << np.arange(uv.shape[0], dtype=np.uint32)[:, None]).sum(axis=0, dtype=np.uint32)


def triangulateMulti(cameras, T, uv, seen=None, returnStatus=False, returnError=False, returnCovariance=False,
                     returnResiduals=False, sigma=1.0, device=0):
    """One 3-D point from every camera that saw it: cameras[c] = (distortionType, A (3,3), k), 2 to 8 of them; T (N,4,4)
    with X_c = T[c] X (RigCalibration.T: X in camera 0's frame); uv (N,n,2), or a list of N (n,2) arrays, the pixels of
    the n points in each camera; seen (n,) unsigned integers, bit c set where camera c saw the point -- None: a camera
    saw a point where both coordinates of its pixel are finite. A camera that did not see a point adds nothing to it.
    -> X (n,3), the minimiser of the pixel residuals of the cameras that saw the point under each camera's full model
    (start: the point closest to the rays; then damped Gauss-Newton on the device). returnStatus adds the (n,) int32
    status -- 0 ok, 1 a seen pixel without an inverse, 2 degenerate geometry, 3 not converged, 4 fewer than two cameras
    saw the point; every output is NaN where it is not 0 --, returnError the (n,) squared pixel error at X,
    returnCovariance the (n,3,3) covariance sigma^2 (J^T J)^-1 of X for pixel noise of standard deviation sigma, and
    returnResiduals the (N,n,2) residuals at X, NaN for a camera that did not see the point."""
    cams = [_camera(cam, c) for c, cam in enumerate(cameras)]
    if isinstance(uv, (list, tuple)):
        if len(uv) != len(cams):
            raise ValueError(f"uv: expected a pixel array per camera ({len(cams)}), got {len(uv)}")
        parts = [np.asarray(p, dtype=np.float64) for p in uv]
        if any(p.ndim != 2 or p.shape != parts[0].shape or p.shape[1] != 2 for p in parts):
            raise ValueError(f"uv: expected arrays of one shape (None, 2), got {[p.shape for p in parts]}")
        uv = np.stack(parts)
    uv = np.asarray(uv, dtype=np.float64)
    if uv.ndim != 3 or uv.shape[0] != len(cams) or uv.shape[2] != 2:
        raise ValueError(f"uv: expected shape ({len(cams)}, None, 2), got {uv.shape}")
    if seen is None:
        seen = seenMasks(uv)
    X, sse, status, cov, res = engine.triangulateMulti([(cam[1], cam[2], cam[3]) for cam in cams], T, uv, seen,
                                                       returnCovariance, returnResiduals, device)
    out = (X,) + ((status,) if returnStatus else ()) + ((sse,) if returnError else ())
    if returnCovariance:
        full = cov[:, [0, 1, 3, 1, 2, 4, 3, 4, 5]].reshape(-1, 3, 3)
        out += (float(sigma) ** 2 * full,)
    if returnResiduals:
        out += (res,)
    return out[0] if len(out) == 1 else out
