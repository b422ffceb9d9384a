"""How far to trust a calibration: standard deviations, covariance and per-view reprojection errors.

The numbers come from the device (RefineEngine.covariance / viewErrors, include/calib_lm.h: calib_covariance,
calib_view_errors); this module only holds them. The covariance is sigma^2 (Jf^T Jf)^-1 at the estimate, with Jf
the Jacobian without the columns of the fixed shared parameters; fixed parameters have zero rows and columns.
Pose entries are in the units of the parameter vector: Euler angles in DEGREES, then t.
"""
from dataclasses import dataclass

import numpy as np


@dataclass
class CalibrationUncertainty:
    sigma: float                # noise estimate sqrt(sse / dof), in pixels
    dof: int                    # 2 n - number of free parameters
    rms: float                  # overall per-point RMS reprojection error sqrt(sse / n)
    names: tuple                # the L shared parameter names, in the order of P
    stdShared: np.ndarray       # (L,)
    covShared: np.ndarray       # (L, L)
    stdPoses: np.ndarray        # (M, 6): rho_x, rho_y, rho_z [degrees], t_x, t_y, t_z
    covPoses: np.ndarray        # (M, 6, 6)
    perViewRms: np.ndarray      # (M,) per-point RMS of each view (NaN for an empty view)
    perViewMax: np.ndarray      # (M,) largest point error of each view
    values: np.ndarray = None   # (L,) the shared parameters the uncertainty belongs to (for summary())
    fixedMask: int = 0          # bit i: shared parameter i was held fixed

    def isFixed(self, i):
        return bool(self.fixedMask >> i & 1)

    def correlationShared(self):
        """(L, L) correlation matrix of the shared parameters: C_ij / sqrt(C_ii C_jj), unit diagonal. Rows and
        columns of fixed parameters (zero variance) are 0 off the diagonal."""
        d = np.sqrt(np.diagonal(self.covShared))
        safe = np.where(d > 0, d, 1.0)
        R = self.covShared / np.outer(safe, safe)
        np.fill_diagonal(R, 1.0)
        return R

    def summary(self):
        """one `name = value ± std` line per shared parameter (`(fixed)` for a fixed one), then the noise estimate"""
        vals = self.values if self.values is not None else np.full(len(self.names), np.nan)
        lines = []
        for i, n in enumerate(self.names):
            if self.isFixed(i):
                lines.append(f"{n} = {vals[i]:.6g} (fixed)")
            else:
                lines.append(f"{n} = {vals[i]:.6g} ± {self.stdShared[i]:.3g}")
        lines.append(f"sigma {self.sigma:.4g} px, rms {self.rms:.4g} px, dof {self.dof}")
        return "\n".join(lines)


def fromEngineResults(names, cov, errs, numPoints, values=None, fixedMask=0):
    """CalibrationUncertainty from RefineEngine.covariance() and RefineEngine.viewErrors() of one problem"""
    L = len(names)
    M = cov["covViews"].shape[0]
    sse = cov["sigma2"] * cov["dof"]
    return CalibrationUncertainty(
        sigma=float(np.sqrt(cov["sigma2"])), dof=int(cov["dof"]), rms=float(np.sqrt(sse / numPoints)),
        names=tuple(names), stdShared=cov["std"][:L].copy(), covShared=cov["covShared"],
        stdPoses=cov["std"][L:].reshape(M, 6).copy(), covPoses=cov["covViews"],
        perViewRms=errs["rms"], perViewMax=errs["max"],
        values=None if values is None else np.asarray(values, dtype=np.float64).ravel()[:L].copy(),
        fixedMask=int(fixedMask))
