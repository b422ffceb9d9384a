"""Yardsticks of the undistortion tests (a helper, not a test): numpy fp64 restatements of what include/calib_lm.h
states for calib_undistort_points / calib_undistort_maps / calib_remap -- the pixel <-> normalised conversions and the
bilinear rule -- and the model's 2 x 2 Jacobian by central differences. The forward model is never restated here: it is
always oracle.calib_oracle.distortPoints."""
import numpy as np

from oracle import calib_oracle as orc


def pixelsToNormalised(A, uv):
    """yd = (v - vc) / beta, xd = (u - uc - gamma yd) / alpha"""
    A = np.asarray(A, dtype=np.float64)
    uv = np.asarray(uv, dtype=np.float64)
    y = (uv[..., 1] - A[1, 2]) / A[1, 1]
    x = (uv[..., 0] - A[0, 2] - A[0, 1] * y) / A[0, 0]
    return np.stack((x, y), axis=-1)


def normalisedToPixels(A, xy):
    """u = alpha x + gamma y + uc, v = beta y + vc"""
    A = np.asarray(A, dtype=np.float64)
    xy = np.asarray(xy, dtype=np.float64)
    u = A[0, 0] * xy[..., 0] + A[0, 1] * xy[..., 1] + A[0, 2]
    v = A[1, 1] * xy[..., 1] + A[1, 2]
    return np.stack((u, v), axis=-1)


def distort(model, xy, k):
    """orc.distortPoints on an (..., 2) array"""
    xy = np.asarray(xy, dtype=np.float64)
    xd, yd = orc.distortPoints(model, xy[..., 0], xy[..., 1], k)
    return np.stack((xd, yd), axis=-1)


def modelJacobian(model, xy, k, h=1e-5):
    """(N, 2, 2) d(xd, yd) / d(x, y) by central differences of orc.distortPoints. Truncation h^2 f''' / 6 ~ 1e-10 and
    rounding eps / h ~ 1e-11 per entry: ample for a condition number that is asserted to one digit."""
    xy = np.asarray(xy, dtype=np.float64)
    J = np.empty(xy.shape[:-1] + (2, 2))
    for c in range(2):
        d = np.zeros(2)
        d[c] = h
        J[..., :, c] = (distort(model, xy + d, k) - distort(model, xy - d, k)) / (2 * h)
    return J


def inverseNorm(J):
    """||J^-1||_2 = 1 / sigma_min(J), per point"""
    return 1.0 / np.linalg.svd(J, compute_uv=False)[..., -1]


def mapsYardstick(model, A, k, newA, width, height):
    """fp64 (mapx, mapy), each (height, width): destination pixel -> normalised (newA) -> orc.distortPoints -> A.
    A destination pixel exactly on the fisheye axis comes out NaN (the oracle's 0 / 0); the caller puts the limit."""
    jj, ii = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    xy = pixelsToNormalised(A if newA is None else newA, np.stack((jj, ii), axis=-1))
    uv = normalisedToPixels(A, distort(model, xy, k))
    return uv[..., 0], uv[..., 1]


def bilinear(image, mapx, mapy, border=0.0):
    """fp64 (h, w, C): x0 = floor(sx), fx = sx - x0, likewise y; taps a (y0, x0), b (y0, x0 + 1), c (y0 + 1, x0),
    d (y0 + 1, x0 + 1), each `border` where it lies outside the image; top = a + fx (b - a), bot = c + fx (d - c),
    out = top + fy (bot - top). A NaN or infinite map entry gives `border`. No rounding to the image's dtype."""
    img = np.asarray(image, dtype=np.float64)
    if img.ndim == 2:
        img = img[:, :, None]
    H, W, C = img.shape
    sx, sy = np.asarray(mapx, dtype=np.float64), np.asarray(mapy, dtype=np.float64)
    finite = np.isfinite(sx) & np.isfinite(sy)
    sx, sy = np.where(finite, sx, -10.0), np.where(finite, sy, -10.0)
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = (sx - x0)[..., None], (sy - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        return np.where(inside[..., None], v, float(border))

    a, b, c, d = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    top = a + fx * (b - a)
    bot = c + fx * (d - c)
    out = top + fy * (bot - top)
    return np.where(finite[..., None], out, float(border))
