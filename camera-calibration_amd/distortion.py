"""Distortion / projection models: the numeric half of the reference's src/distortion.py.

The reference builds its Jacobian by running these formulas on sympy symbols
(src/distortion.py:13-40); here the derivatives are closed-form device code
(csrc/point_model.hpp), so nothing symbolic ships. The forward model itself
(projectWithDistortion / distortPoints) is evaluated by the HIP library too.
"""
import numpy as np

from . import _native as nat
from . import engine
from . import fixed


class DistortionModel:
    _maxFOV = 179.5              # src/distortion.py:11 (the NaN-by-FOV branch is disabled there, :12)
    _shouldNaNByFOV = False
    modelName = None
    modelId = None

    def getIntrinsicSymbols(self):
        """names, in parameter-vector order (src/distortion.py:61-62)"""
        return ("α", "β", "γ", "uc", "vc")

    def getDistortionSymbols(self):
        raise NotImplementedError()

    def sharedParameterNames(self):
        """names of the L shared parameters in the order of the parameter vector P: what Calibrator(fixed=...)
        and RefineEngine.setFixedShared take (fixed.py lists the aliases)"""
        return fixed.INTRINSIC_NAMES + tuple(self.getDistortionSymbols())

    def projectWithDistortion(self, A, X, k):
        """A (3,3), X (N,3) camera-frame points, k -> (N,2) sensor points (src/distortion.py:42-59)"""
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[1] != 3:
            raise ValueError(f"Expected shape (None, 3), got {X.shape}")
        return engine.projectWithDistortion(self.modelId, A, X, self._checkK(k))

    def distortPoints(self, x, k):
        """x (N,2) normalised points -> (N,2) distorted normalised points"""
        x = np.asarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != 2:
            raise ValueError(f"Expected shape (None, 2), got {x.shape}")
        return engine.distortPoints(self.modelId, x, self._checkK(k))

    def undistortPoints(self, A, k, uv, newA=None, returnStatus=False):
        """uv (N,2) pixels of the distorted image -> (N,2) ideal points: normalised (x, y), or pixels of the camera
        matrix newA. The inverse of projectWithDistortion's distortion step, by Newton on the device. Where the model
        has no inverse (past the turning point of its radial polynomial, a folded-over root, a non-finite pixel) the
        row is NaN; returnStatus=True also returns the (N,) int32 status, 0 = solved, 1 = not."""
        uv = np.asarray(uv, dtype=np.float64)
        if uv.ndim != 2 or uv.shape[1] != 2:
            raise ValueError(f"Expected shape (None, 2), got {uv.shape}")
        xy, status = engine.undistortPoints(self.modelId, A, self._checkK(k), uv, newA)
        return (xy, status) if returnStatus else xy

    def undistortMaps(self, A, k, size, newA=None):
        """size = (width, height) of the undistorted image -> (mapx, mapy), float32 (height, width): the position in
        the distorted image that each pixel of the undistorted one (camera matrix newA, default A) shows."""
        try:
            width, height = size
        except (TypeError, ValueError):
            raise ValueError(f"size: expected (width, height), got {size!r}") from None
        return engine.undistortMaps(self.modelId, A, self._checkK(k), width, height, newA)

    def rectifyMaps(self, A, k, R, P, size):
        """undistortMaps with a rotation: size = (width, height) of the rectified image, R (3,3) or None the rotation
        from the camera's frame into the rectified one, P its camera matrix ((3,3), or the (3,4) projection matrix of
        stereoRectify) -> (mapx, mapy), float32 (height, width); NaN where the pixel's ray does not enter the camera's
        front half space (remap turns that into the border value)."""
        try:
            width, height = size
        except (TypeError, ValueError):
            raise ValueError(f"size: expected (width, height), got {size!r}") from None
        return engine.rectifyMaps(self.modelId, A, self._checkK(k), R, P, width, height)

    def rectifyPoints(self, A, k, uv, R, P, returnStatus=False):
        """uv (N,2) pixels of the distorted image -> (N,2) pixels of the rectified one (R, P as in rectifyMaps). A row
        is NaN where the model has no inverse or the point lies behind the rectified camera; returnStatus=True also
        returns the (N,) int32 status, 0 = ok, 1 = not."""
        out, status = engine.rectifyPoints(self.modelId, A, self._checkK(k), uv, R, P)
        return (out, status) if returnStatus else out

    def estimateDistortion(self, A, allDetections, allBoardPosesInCamera, device=0):
        """Linear least-squares start value of k given A and the board poses (src/distortion.py:70,
        110-191 radial-tangential, 222-271 fisheye): D^T D and D^T Ddot are formed on the device
        (calib_distortion_normal_equations), the |k| x |k| system is solved on the host."""
        from . import linearcalibrate
        offs, sensor, model = engine.packDetections(allDetections)
        DtD, Dtd = engine.distortionNormalEquations(self.modelId, offs, sensor, model, A,
                                                    np.asarray(allBoardPosesInCamera, dtype=np.float64), device)
        return linearcalibrate.solveDistortionNormalEquations(DtD, Dtd)

    def _checkK(self, k):
        k = np.asarray(k, dtype=np.float64).ravel()
        n = len(self.getDistortionSymbols())
        if k.shape[0] != n:
            raise ValueError(f"not enough values to unpack (expected {n}, got {k.shape[0]})")
        return k


class RadialTangentialModel(DistortionModel):
    """k = (k1, k2, p1, p2, k3)  (src/distortion.py:74-108)"""
    modelName = "radtan"
    modelId = nat.MODEL_RADTAN

    def getDistortionSymbols(self):
        return ("k1", "k2", "p1", "p2", "k3")


class FisheyeModel(DistortionModel):
    """k = (k1, k2, k3, k4), theta = atan(r) polynomial  (src/distortion.py:194-220).

    At r = 0 the reference evaluates 0/0 (NaN); this engine returns the analytic
    limit (xd, yd) = (0, 0)."""
    modelName = "fisheye"
    modelId = nat.MODEL_FISHEYE

    def getDistortionSymbols(self):
        return ("k1", "k2", "k3", "k4")
