#!/usr/bin/env python3
"""Writes tests/golden/point_model/{radtan,fisheye}.npz: the per-point camera model of csrc/point_model.hpp evaluated
with mpmath at 420 digits on its whole domain, with a magnitude beside every value (tests/point_model_yardstick.py says
what a magnitude is and holds the layout). Needs mpmath; the tests that read the fixtures do not.

    python tools/make_point_model_golden.py            # rewrites both files

Every stored number is the float64 rounding of a 420-digit value: (g' - s) / r^2 is evaluated as it stands down to
r = 1e-150, where the difference loses 300 digits and keeps 120. The value and its magnitude come out of one pass: the
model is written once, in the order of the kernel's chain rule, over a number type that carries both.

Shared parameters are synthetic's c2 / c3 cameras with a skew of 0.75, every one rounded to fp32: the same fixture then
serves the fp32 engine, which converts the parameters to fp32 on load, without an input rounding to account for.
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import point_model_yardstick as pmy                      # noqa: E402
from camera_calibration_amd import synthetic             # noqa: E402

mp.mp.dps = 420
SKEW = 0.75
MONOTONE_K = (-0.02, 0.003, -0.0004, 0.00005)            # theta poly(theta) increases on [0, pi/2): the inverse exists
NOISE_PX = 0.3
INVERSE_POINTS = 512


# ---------------------------------------------------------------- a number with its magnitude
class V:
    """value v and magnitude m >= |v|: additions add magnitudes; a product a b takes max(|a| m_b, |b| m_a), the
    first-order rule (a relative excess m / |v| is carried through products and powers, not compounded by them)"""
    __slots__ = ("v", "m")

    def __init__(self, v, m=None):
        self.v = mp.mpf(v)
        self.m = abs(self.v) if m is None else mp.mpf(m)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def __add__(self, o):
        o = V.of(o)
        return V(self.v + o.v, self.m + o.m)
    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return V(self.v - o.v, self.m + o.m)

    def __rsub__(self, o):
        return V.of(o) - self

    def __mul__(self, o):
        o = V.of(o)
        return V(self.v * o.v, max(abs(self.v) * o.m, abs(o.v) * self.m))
    __rmul__ = __mul__

    def __neg__(self):
        return V(-self.v, self.m)


def fn(g, dg, a):
    """a function of a: |g|, or |g'| magnitude(a) where the argument's own cancellation makes that larger"""
    return V(g, max(abs(g), abs(dg) * a.m))



def rcp(a):
    return fn(1 / a.v, -1 / a.v ** 2, a)


def sqrtV(a):
    s = mp.sqrt(a.v)
    return fn(s, 1 / (2 * s), a)


def atanV(a):
    return fn(mp.atan(a.v), 1 / (1 + a.v ** 2), a)


ZERO, ONE = V(0), V(1)
DEG = V(mp.pi / 180)


def trig(rhoDeg):
    """(sin, cos) of an angle in degrees; 0 is the identity exactly (the fixture uses 0 or whole degrees)"""
    if rhoDeg == 0.0:
        return ZERO, ONE
    th = V(rhoDeg) * DEG
    return fn(mp.sin(th.v), mp.cos(th.v), th), fn(mp.cos(th.v), mp.sin(th.v), th)


def distortV(name, k, x, y):
    """-> xd, yd, xd_x, xd_y, yd_y, dkx[NK], dky[NK] (the factor f_j in both for a radial coefficient)"""
    r2 = x * x + y * y
    if name == "radtan":
        k1, k2, p1, p2, k3 = k
        rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        drad = k1 + r2 * (2 * k2 + 3 * k3 * r2)
        r4 = r2 * r2
        r6 = r4 * r2
        xy, xx, yy = x * y, x * x, y * y
        xd = rad * x + 2 * p1 * xy + p2 * (r2 + 2 * xx)
        yd = rad * y + p1 * (r2 + 2 * yy) + 2 * p2 * xy
        xd_x = rad + 2 * xx * drad + 2 * p1 * y + 6 * p2 * x
        xd_y = 2 * xy * drad + 2 * p1 * x + 2 * p2 * y
        yd_y = rad + 2 * yy * drad + 6 * p1 * y + 2 * p2 * x
        return (xd, yd, xd_x, xd_y, yd_y, [r2, r4, 2 * xy, r2 + 2 * xx, r6], [r2, r4, r2 + 2 * yy, 2 * xy, r6])
    k1, k2, k3, k4 = k
    if r2.v == 0:                                      # the axis: the analytic limit, not the reference's 0 / 0
        s, thr, sror, t2 = ONE, ONE, 2 * k1 - V(2) * rcp(V(3)), ZERO
    else:
        r = sqrtV(r2)
        th = atanV(r)
        t2 = th * th
        poly = 1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))
        gp = (1 + t2 * (3 * k1 + t2 * (5 * k2 + t2 * (7 * k3 + 9 * k4 * t2)))) * rcp(1 + r2)
        ir = rcp(r)
        thr = th * ir
        s = thr * poly
        sror = (gp - s) * ir * ir
    xd, yd = s * x, s * y
    xd_x = s + x * x * sror
    xd_y = x * y * sror
    yd_y = s + y * y * sror
    f = [thr * t2]
    for j in range(3):
        f.append(f[-1] * t2)
    return xd, yd, xd_x, xd_y, yd_y, f, f


def pointBlock(name, shared, pose, X):
    """one point -> uv [2], xd [2], J [2][C] of V, Zc"""
    L = pmy.NUM_SHARED[name]
    C = L + 6
    al, be, ga, uc, vc = (V(float(a)) for a in shared[:5])
    k = [V(float(a)) for a in shared[5:L]]
    (sx, cx), (sy, cy), (sz, cz) = (trig(float(a)) for a in pose[:3])
    t = [V(float(a)) for a in pose[3:6]]
    R = [[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
         [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
         [-sy, cy * sx, cy * cx]]
    Pw = [V(float(a)) for a in X]
    q = [R[i][0] * Pw[0] + R[i][1] * Pw[1] + R[i][2] * Pw[2] for i in range(3)]
    Zc = q[2] + t[2]
    iz = rcp(Zc)
    x, y = (q[0] + t[0]) * iz, (q[1] + t[1]) * iz
    xd, yd, xd_x, xd_y, yd_y, dkx, dky = distortV(name, k, x, y)
    yd_x = xd_y
    u = al * xd + ga * yd + uc
    v = be * yd + vc
    J = [[ZERO] * C, [ZERO] * C]
    J[0][0], J[1][1], J[0][2], J[0][3], J[1][4] = xd, yd, yd, ONE, ONE
    axy, by = al * x + ga * y, be * y
    for j in range(L - 5):
        if name == "fisheye" or j < 2 or j == 4:
            J[0][5 + j], J[1][5 + j] = axy * dkx[j], by * dkx[j]
        else:
            J[0][5 + j], J[1][5 + j] = al * dkx[j] + ga * dky[j], be * dky[j]
    ux, uy = (al * xd_x + ga * yd_x) * iz, (al * xd_y + ga * yd_y) * iz
    vx, vy = be * yd_x * iz, be * yd_y * iz
    ax = [DEG * cz * cy, DEG * sz * cy, -(DEG * sy)]
    ay = [-(DEG * sz), DEG * cz]

    def col(c, dx, dy):
        J[0][c], J[1][c] = ux * dx + uy * dy, vx * dx + vy * dy
    dX, dY, dZ = ax[1] * q[2] - ax[2] * q[1], ax[2] * q[0] - ax[0] * q[2], ax[0] * q[1] - ax[1] * q[0]
    col(L + 0, dX - x * dZ, dY - y * dZ)
    dX, dY, dZ = ay[1] * q[2], -(ay[0] * q[2]), ay[0] * q[1] - ay[1] * q[0]
    col(L + 1, dX - x * dZ, dY - y * dZ)
    col(L + 2, -(DEG * q[1]), DEG * q[0])
    J[0][L + 3], J[1][L + 3] = ux, vx
    J[0][L + 4], J[1][L + 4] = uy, vy
    J[0][L + 5], J[1][L + 5] = -(ux * x + uy * y), -(vx * x + vy * y)
    return [u, v], [xd, yd], J, Zc


def projectMp(name, params, X):
    """(u, v) as plain mpf from a flat list of mpf parameters (L shared, then the pose): what the CPU test
    differentiates numerically, written apart from pointBlock"""
    L = pmy.NUM_SHARED[name]
    al, be, ga, uc, vc = params[:5]
    k = params[5:L]
    rho, t = params[L:L + 3], params[L + 3:L + 6]
    sx, sy, sz = (mp.sin(a * mp.pi / 180) for a in rho)
    cx, cy, cz = (mp.cos(a * mp.pi / 180) for a in rho)
    R = mp.matrix([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                   [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx], [-sy, cy * sx, cy * cx]])
    Pc = R * mp.matrix([mp.mpf(float(a)) for a in X]) + mp.matrix(t)
    x, y = Pc[0] / Pc[2], Pc[1] / Pc[2]
    r = mp.sqrt(x * x + y * y)
    if name == "radtan":
        k1, k2, p1, p2, k3 = k
        rad = 1 + k1 * r ** 2 + k2 * r ** 4 + k3 * r ** 6
        xd = rad * x + 2 * p1 * x * y + p2 * (r ** 2 + 2 * x * x)
        yd = rad * y + p1 * (r ** 2 + 2 * y * y) + 2 * p2 * x * y
    else:
        th = mp.atan(r)
        s = th / r * (1 + sum(kj * th ** (2 * j + 2) for j, kj in enumerate(k))) if r != 0 else mp.mpf(1)
        xd, yd = s * x, s * y
    return al * xd + ga * yd + uc, be * yd + vc


# ---------------------------------------------------------------- inputs
def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def sharedOf(name):
    cfg = synthetic.CONFIGS["c2" if name == "radtan" else "c3"]
    A = np.asarray(cfg["A"], dtype=np.float64)
    return f32([A[0, 0], A[1, 1], SKEW, A[0, 2], A[1, 2]] + list(cfg["k"]))


def radtanCap(k):
    """largest r at which the radial polynomial 1 + k1 r^2 + k2 r^4 + k3 r^6 stays below 1e6 (bisection)"""
    k1, k2, _, _, k3 = (float(a) for a in k)
    lo, hi = 1.0, 1e3
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        r2 = mid * mid
        lo, hi = (mid, hi) if 1 + r2 * (k1 + r2 * (k2 + r2 * k3)) < 1e6 else (lo, mid)
    return lo


def radii(name, shared, count):
    """-> list of (r, mode): the radii of the identity-posed points. mode 2: on an axis, so that r is that number
    exactly; 1: two in three on an axis, the third at a random angle; 0: a sweep point, the quadrants in turn"""
    out = []
    if name == "fisheye":
        out.append((0.0, 2))
    near = [2.0 ** -e for e in (50, 40, 30, 20, 10, 3)]
    below = [1e-8 * (1 - d) for d in near] + [9e-9, 5e-9, 3e-9, 1e-9, 1e-10, 1e-12, 1e-20, 1e-50, 1e-100, 1e-150]
    above = [1e-8 * (1 + d) for d in near] + [1e-8, 1.0000001e-8, 1.001e-8, 1.01e-8, 1.1e-8, 1.5e-8, 2e-8, 3e-8, 5e-8,
                                               7e-8]
    out += [(r, 1) for r in below + above]
    out += [(float(r), 0) for r in np.logspace(-8, -1, 57)]                      # decades, 8 per decade
    one = [1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)]
    one += [1.0 + s * 1e-3 * 2.0 ** -j for j in range(16) for s in (-1.0, 1.0)]       # 32 within 1e-3 of 1
    out += [(float(r), 2 if j < 3 else 1) for j, r in enumerate(one)]
    top = 1e3 if name == "fisheye" else radtanCap(shared[5:])
    far = [float(r) for r in np.logspace(np.log10(3.0), np.log10(top), 48)[1:]]
    far[-1] = top
    out += [(r, 1) for r in far]
    left = count - len(out)
    nLow = left * 4 // 9
    out += [(float(r), 0) for r in np.linspace(0.1, 1.0, nLow, endpoint=False)]
    out += [(float(r), 0) for r in np.linspace(1.0, 3.0, left - nLow + 1)[1:]]
    assert len(out) == count
    return out


def buildInputs(name):
    """everything but the yardstick values -> dict of float64 / int64 arrays"""
    rng = np.random.default_rng(20 if name == "radtan" else 21)
    shared = sharedOf(name)
    sizes = np.array(pmy.VIEW_SIZES, dtype=np.int64)
    offs = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    M, n = sizes.shape[0], int(offs[-1])
    vi = np.repeat(np.arange(M), sizes)
    general = np.isin(vi, pmy.GENERAL_VIEWS)
    ident = np.flatnonzero(~general)
    pts = np.zeros((n, 3))
    exact = np.zeros(n, dtype=bool)                                  # x, y, z are fp32 numbers
    # identity-posed views: (x, y, 0) with t = (0, 0, 1) is the normalised point itself
    rs = radii(name, shared, ident.shape[0])
    order = rng.permutation(ident.shape[0])
    axes = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))
    for j, (r, mode) in enumerate(rs):
        p = ident[order[j]]
        if mode == 2 or (mode == 1 and j % 3 != 2):
            c, s = axes[(j // 3) % 4]                                # three in a row share a half-axis
            pts[p, :2] = (r * c, r * s)
        elif mode == 1:                                              # off the axes at the special radii too
            phi = rng.uniform(0.0, 2 * np.pi)
            pts[p, :2] = (r * np.cos(phi), r * np.sin(phi))
        else:
            phi = (j % 4) * np.pi / 2 + rng.uniform(0.05, np.pi / 2 - 0.05)       # the quadrants in turn
            xy = np.array([r * np.cos(phi), r * np.sin(phi)])
            if r >= 1e-8:
                xy = f32(xy)
                exact[p] = True
            pts[p, :2] = xy
    poses = np.tile(np.array([0.0, 0.0, 0.0, 0.0, 0.0, 1.0]), (M, 1))
    angles = ((60.0, -35.0, 20.0), (-45.0, 60.0, -170.0), (10.0, -20.0, 95.0), (30.0, 50.0, -60.0), (-60.0, -60.0, 45.0))
    depth = (0.0625, 0.25, 1.0, 2.5, 4.0)
    for v, ang, tz in zip(pmy.GENERAL_VIEWS, angles, depth):
        poses[v] = (*ang, 0.25 * tz, -0.125 * tz, tz)
        a, b = int(offs[v]), int(offs[v + 1])
        pts[a:b] = f32(np.column_stack((rng.uniform(-0.3, 0.3, b - a), rng.uniform(-0.3, 0.3, b - a),
                                        rng.uniform(-0.1, 0.1, b - a))) * tz)
    streamIndex = ident[rng.integers(0, ident.shape[0], int(np.sum(pmy.STREAM_SIZES)))].astype(np.int64)
    return {"shared": shared, "poses": poses, "offs": offs, "pts": pts, "general": general, "f32_exact": exact,
            "noise": rng.uniform(-NOISE_PX, NOISE_PX, (n, 2)), "stream_index": streamIndex,
            "stream_noise": rng.uniform(-NOISE_PX, NOISE_PX, (streamIndex.shape[0], 2))}


def evaluatePoints(name, inp, indices):
    """the yardstick at the given points -> dict y, y_mag, xd, xd_mag, J, J_mag, zc (float64 roundings)"""
    C = pmy.NUM_SHARED[name] + 6
    m = len(indices)
    out = {"y": np.empty((m, 2)), "y_mag": np.empty((m, 2)), "xd": np.empty((m, 2)), "xd_mag": np.empty((m, 2)),
           "J": np.empty((m, 2, C)), "J_mag": np.empty((m, 2, C)), "zc": np.empty(m)}
    vi = pmy.pointViews(inp["offs"])
    for j, p in enumerate(indices):
        uv, xd, J, Zc = pointBlock(name, inp["shared"], inp["poses"][vi[p]], inp["pts"][p])
        out["zc"][j] = float(Zc.v)
        for a in range(2):
            out["y"][j, a], out["y_mag"][j, a] = float(uv[a].v), float(uv[a].m)
            out["xd"][j, a], out["xd_mag"][j, a] = float(xd[a].v), float(xd[a].m)
            for c in range(C):
                out["J"][j, a, c], out["J_mag"][j, a, c] = float(J[a][c].v), float(J[a][c].m)
    return out


# ---------------------------------------------------------------- the inverse at wide angles (fisheye)
def thetaD(k, th):
    return th * (1 + sum(mp.mpf(float(kj)) * th ** (2 * j + 2) for j, kj in enumerate(k)))


def foldOf(k):
    """the first angle at which d(theta poly)/dtheta = 0 -> (theta, theta_d) as mpf"""
    d = lambda th: 1 + sum((2 * j + 3) * mp.mpf(float(kj)) * th ** (2 * j + 2) for j, kj in enumerate(k))   # noqa: E731
    lo, hi = mp.mpf(0), mp.mpf(0)
    while d(hi) > 0:
        lo, hi = hi, hi + mp.mpf("0.01")
        assert hi < 2
    th = mp.findroot(d, (lo, hi), solver="illinois")
    return th, thetaD(k, th)


def inversePoints():
    """the monotone coefficients and 512 normalised points with theta in [0.7, 1.55], the quadrants in turn"""
    rng = np.random.default_rng(22)
    th = np.linspace(0.7, 1.55, INVERSE_POINTS)
    phi = (np.arange(INVERSE_POINTS) % 4) * np.pi / 2 + rng.uniform(0.0, np.pi / 2, INVERSE_POINTS)
    return f32(MONOTONE_K), np.stack((np.tan(th) * np.cos(phi), np.tan(th) * np.sin(phi)), axis=1)


def inverseValues(kM, x):
    """the distorted points and the symmetric 2 x 2 derivative (xd_x, xd_y, yd_y) at x under the monotone coefficients;
    the fold of synthetic.FISHEYE_K (rounded to fp32 as the fixture's shared parameters are)"""
    xd, der = np.empty_like(x), np.empty((x.shape[0], 3))
    kV = [V(float(a)) for a in kM]
    for i in range(x.shape[0]):
        o = distortV("fisheye", kV, V(float(x[i, 0])), V(float(x[i, 1])))
        xd[i] = float(o[0].v), float(o[1].v)
        der[i] = float(o[2].v), float(o[3].v), float(o[4].v)
    kF = f32(synthetic.FISHEYE_K)
    thF, tdF = foldOf(kF)
    return {"inv_xd": xd, "inv_der": der, "fold_k": kF, "fold_theta": np.float64(float(thF)),
            "fold_theta_d": np.float64(float(tdF))}


def build(name):
    inp = buildInputs(name)
    fx = dict(inp)
    fx.update(evaluatePoints(name, inp, range(int(inp["offs"][-1]))))
    if name == "fisheye":
        kM, x = inversePoints()
        fx.update({"inv_k": kM, "inv_x": x})
        fx.update(inverseValues(kM, x))
    return fx


def main():
    os.makedirs(pmy.FIXTURES, exist_ok=True)
    for name in pmy.MODELS:
        fx = build(name)
        path = os.path.join(pmy.FIXTURES, name + ".npz")
        np.savez_compressed(path, **fx)
        print(f"{path}: {fx['pts'].shape[0]} points, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
