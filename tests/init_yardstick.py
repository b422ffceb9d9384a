"""Yardstick of the initialisation-kernel tests (test infrastructure, not a test file): inputs and host references for
dlt_kernel, homography_lm_kernel, extrinsics_kernel, distortion_normal_kernel and compose_views_kernel /
decompose_views_kernel. numpy only; imported by tests/test_init_yardstick_cpu.py (the guard, no GPU) and
tests/test_gpu_init_kernels.py.

The shared problem R: 83 views of a 13 x 10 board whose point counts cycle through R_COUNT_CYCLE, in both camera
models at the noise levels of R_SIGMAS. dlt_kernel and homography_lm_kernel run 16 views per 256-thread workgroup with
16 lanes per view, so 83 views are five full workgroups and one with 3 views, and the counts meet every pattern of the
lane stride `for (q = lane; q < n; q += 16)`.

A "views" dict: model (name), offs (M+1,), s (MN,2), m (MN,3), W (M,4,4 true poses), A, k (the goldens' true camera)."""
import functools

import numpy as np

from camera_calibration_amd import linearcalibrate as lc
from conftest import loadGolden
from oracle import calib_oracle as orc

MODEL_IDS = {"radtan": orc.RADTAN, "fisheye": orc.FISHEYE}
# 130 corners. The spacing sets how far the views reach into the distortion, and with it lambda_1 / lambda_2 of M^T M, the
# convergence rate of dlt_kernel's inverse iteration: the guard wants it near 1e-2 on some view of every variant
# ((1e-2)^4 = 1e-8, the bar on H) and nowhere so large that 8 iterations leave 1e-10. The radtan camera (k1 = -0.5) gets
# there on a 0.48 m x 0.36 m board, the milder fisheye camera on a 0.54 m x 0.405 m one.
BOARDS = {"radtan": (13, 10, 0.04), "fisheye": (13, 10, 0.045)}
R_COUNT_CYCLE = (4, 5, 7, 15, 16, 17, 31, 33, 54, 64, 65, 88, 130)
R_NUM_VIEWS = 83
# Noise per variant, nominally 0, 0.3 and 2 px. The host polish must agree with itself on 95 % of a variant's views
# (undecidedViews); its 20 accept / reject decisions leave H reproducible to about 3e-6 and the reprojections to 3e-7 px,
# just past a tenth of the bars, so a variant has 0..13 undecided views almost independently of sigma. R_SEED is the first
# seed from 0 at which both models meet the condition at 0 and 0.3 px (and the DLT conditions of the guard); the 2 px
# variants did not meet it there and were lowered in steps of 0.25 px until they did: 1.5 px radtan, 1.25 px fisheye.
R_SIGMAS = {"radtan": (0.0, 0.3, 1.5), "fisheye": (0.0, 0.3, 1.25)}
R_VARIANTS = [(model, sigma) for model in ("radtan", "fisheye") for sigma in R_SIGMAS[model]]
R_SEED = 22
LANES, VIEWS_PER_WORKGROUP = 16, 16          # dlt_kernel / homography_lm_kernel
H_BAR, REPROJ_BAR = 1e-5, 1e-6               # test_homography_lm_on_device_vs_reference
BIG_VIEWS, BIG_BOARD = 4855, (9, 6, 0.05)    # 262 170 points: 1 025 workgroups of 256, the grid is capped at 1 024


def rCounts():
    return [R_COUNT_CYCLE[i % len(R_COUNT_CYCLE)] for i in range(R_NUM_VIEWS)]


def lanePatterns(n):
    """what a view of n points does to the 16-lane stride loop"""
    out = set()
    trips, rest = divmod(n, LANES)
    if n < LANES:
        out.add("fewer points than lanes")
    if n == LANES:
        out.add("exactly one per lane")
    if n == LANES + 1:
        out.add("one past one per lane")
    if n in (2 * LANES - 1, 2 * LANES + 1):
        out.add("around two trips")
    if n in (4 * LANES, 4 * LANES + 1):
        out.add("around four trips")
    if trips >= 1 and rest == 1:
        out.add("last trip with one live lane")
    if n == 4:
        out.add("exact fit")
    return out


R_REQUIRED = {"fewer points than lanes", "exactly one per lane", "one past one per lane", "around two trips",
              "around four trips", "last trip with one live lane", "exact fit"}


@functools.lru_cache(maxsize=None)
def trueCamera(modelName):
    g = loadGolden(f"g2_config1_{modelName}.npz")
    return np.array(g["Atrue"]), np.array(g["ktrue"])


def makeViews(model, counts, sigma, seed, board=None):
    """Packed views of a board: poses from orc.syntheticBoardPoses (view indices seed, seed + 1, ..), points through
    orc.projectAllPoints with the goldens' true camera of `model`, Gaussian noise sigma. A view of fewer points than
    the board has keeps the four outer corners and draws the others without replacement, so no view is collinear.
    The subsets and the noise directions depend on (counts, seed) only: the same problem at another sigma."""
    numW, numH, spacing = board or BOARDS[model]
    corners = orc.checkerboardCorners(numW, numH, spacing)
    full = corners.shape[0]
    outer = np.array([0, numW - 1, full - numW, full - 1])
    inner = np.setdiff1d(np.arange(full), outer)
    rng = np.random.default_rng(seed)
    picks = []
    for n in counts:
        if not 4 <= n <= full:
            raise ValueError(f"a view has 4..{full} points, got {n}")
        picks.append(np.arange(full) if n == full else
                     np.sort(np.concatenate((outer, rng.choice(inner, n - 4, replace=False)))))
    offs = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    m = np.ascontiguousarray(np.vstack([corners[p] for p in picks]))
    # the generator aims the camera at one of the corners it is given; aimed at the middle of a square instead, no
    # corner lies on the optical axis, where the fisheye rows (th / r) are 0 / 0 in the reference too
    aim = corners + np.array([spacing / 2, spacing / 2, 0.0])
    W = orc.syntheticBoardPoses(aim, [seed + i for i in range(len(counts))])
    A, k = trueCamera(model)
    P = orc.composeParameterVector(A, W, k)
    s = orc.projectAllPoints(MODEL_IDS[model], P, offs, m) + sigma * rng.standard_normal((m.shape[0], 2))
    return dict(model=model, offs=offs, s=np.ascontiguousarray(s), m=m, W=W, A=A, k=k)


@functools.lru_cache(maxsize=None)
def problemR(model, sigma):
    return makeViews(model, rCounts(), sigma, R_SEED)


def detections(v):
    return [(v["s"][a:b], v["m"][a:b]) for a, b in zip(v["offs"][:-1], v["offs"][1:])]


def permuted(v, seed=1):
    """the same views with each view's points in another order: every sum of the host path in another order"""
    rng = np.random.default_rng(seed)
    idx = np.concatenate([a + rng.permutation(b - a) for a, b in zip(v["offs"][:-1], v["offs"][1:])])
    return dict(v, s=np.ascontiguousarray(v["s"][idx]), m=np.ascontiguousarray(v["m"][idx]))


def withEmptyViews(v, Hs=None):
    """empty views spliced in at the front, in the middle and at the end -> (views, indices of the old views in it,
    indices of the empty ones). W (and Hs, if given) get a row for each empty view: the next view's, scaled."""
    M = len(v["offs"]) - 1
    at = (0, M // 2, M)
    offs, keep, empty = [0], [], []
    for i in range(M + 1):
        if i in at:
            empty.append(len(offs) - 1)
            offs.append(offs[-1])
        if i < M:
            keep.append(len(offs) - 1)
            offs.append(offs[-1] + int(v["offs"][i + 1] - v["offs"][i]))
    keep, empty = np.array(keep), np.array(empty)
    W = np.empty((M + 3, 4, 4))
    W[keep] = v["W"]
    W[empty] = v["W"][[0, M // 2, M - 1]]
    out = dict(v, offs=np.array(offs, dtype=np.int64), W=W)
    if Hs is None:
        return out, keep, empty
    H = np.empty((M + 3, 3, 3))
    H[keep] = Hs
    H[empty] = np.asarray(Hs)[[0, M // 2, M - 1]] * np.array([2.0, -0.5, 3.0])[:, None, None]
    return out, keep, empty, H


def project(H, m):
    """H (3,3), model points (n,>=2) -> (n,2)"""
    y = np.column_stack((m[:, :2], np.ones(m.shape[0]))) @ np.asarray(H).T
    return y[:, :2] / y[:, 2:3]


# ---------------------------------------------------------------- DLT
def hostSvdRoute(v):
    """True when lc.estimateHomographies takes the reference's SVD route for every group of views"""
    counts = np.diff(v["offs"])
    return all(int(n) * int((counts == n).sum()) <= lc._SVD_POINT_LIMIT for n in np.unique(counts))


def dltSvd(s, m):
    """one view by the reference's route restated on its own: the right singular vector of M's smallest singular
    value, of the full 9 x 9 V (with 4 points M is 8 x 9 and the null vector is V's ninth row)"""
    s, m = np.asarray(s, dtype=np.float64), np.asarray(m, dtype=np.float64)[:, :2]
    Na, Nb = lc.computeNormalizationMatrices(s[None])[0], lc.computeNormalizationMatrices(m[None])[0]
    a = s * Na[[0, 1], [0, 1]] + Na[:2, 2]
    b = m * Nb[[0, 1], [0, 1]] + Nb[:2, 2]
    n = s.shape[0]
    M = np.zeros((2 * n, 9))
    M[0::2, 0], M[0::2, 1], M[0::2, 2] = -b[:, 0], -b[:, 1], -1.0
    M[0::2, 6], M[0::2, 7], M[0::2, 8] = a[:, 0] * b[:, 0], a[:, 0] * b[:, 1], a[:, 0]
    M[1::2, 3], M[1::2, 4], M[1::2, 5] = -b[:, 0], -b[:, 1], -1.0
    M[1::2, 6], M[1::2, 7], M[1::2, 8] = a[:, 1] * b[:, 0], a[:, 1] * b[:, 1], a[:, 1]
    Vt = np.linalg.svd(M, full_matrices=True)[2]
    H = np.linalg.inv(Na) @ Vt[-1].reshape(3, 3) @ Nb
    return H / H[2, 2]


def dltInverseIteration(s, m, iters, wantRatio=False):
    """dlt_kernel's algorithm for one view (the algorithm, not the kernel's order of operations): centroid / mean
    distance normalisation, M^T M from its 3 x 3 blocks, shift 1e-15 tr, `iters` solves from x = 1 with x /= max|x|,
    de-normalisation, H /= H[2,2]. wantRatio: also lambda_1 / lambda_2 of M^T M, which sets the convergence rate."""
    s, m = np.asarray(s, dtype=np.float64), np.asarray(m, dtype=np.float64)[:, :2]
    mu_, mX = s.mean(axis=0), m.mean(axis=0)
    sa = np.sqrt(2.0) / np.linalg.norm(s - mu_, axis=1).mean()
    sb = np.sqrt(2.0) / np.linalg.norm(m - mX, axis=1).mean()
    u, v = (sa * (s - mu_)).T
    X, Y = (sb * (m - mX)).T
    Pm = np.stack((X, Y, np.ones_like(X)), axis=1)
    S0 = Pm.T @ Pm
    Su, Sv, Se = (Pm * u[:, None]).T @ Pm, (Pm * v[:, None]).T @ Pm, (Pm * (u * u + v * v)[:, None]).T @ Pm
    MtM = np.zeros((9, 9))
    MtM[0:3, 0:3] = MtM[3:6, 3:6] = S0
    MtM[0:3, 6:9] = MtM[6:9, 0:3] = -Su
    MtM[3:6, 6:9] = MtM[6:9, 3:6] = -Sv
    MtM[6:9, 6:9] = Se
    shifted = MtM + 1e-15 * np.trace(MtM) * np.eye(9)
    x = np.ones(9)
    for _ in range(iters):
        x = np.linalg.solve(shifted, x)
        x = x / np.abs(x).max()
    Hp = x.reshape(3, 3)
    Na = np.array([[sa, 0, -sa * mu_[0]], [0, sa, -sa * mu_[1]], [0, 0, 1]])
    Nb = np.array([[sb, 0, -sb * mX[0]], [0, sb, -sb * mX[1]], [0, 0, 1]])
    H = np.linalg.inv(Na) @ Hp @ Nb
    H = H / H[2, 2]
    if wantRatio:
        lam = np.linalg.eigvalsh(MtM)
        return H, max(lam[0], 0.0) / lam[1]
    return H


@functools.lru_cache(maxsize=None)
def hostHomographies(model, sigma):
    """lc.estimateHomographies of R (the SVD route) -> (M,3,3)"""
    return np.array(lc.estimateHomographies(detections(problemR(model, sigma))))


# ---------------------------------------------------------------- LM polish
@functools.lru_cache(maxsize=None)
def hostPolish(model, sigma):
    """lc.refineHomographies of R from the host SVD start -> (M,3,3)"""
    v = problemR(model, sigma)
    return np.array(lc.refineHomographies(list(hostHomographies(model, sigma)), detections(v)))


def viewError(H, s, m):
    return float(np.sum((np.asarray(s) - project(H, m)) ** 2))


@functools.lru_cache(maxsize=None)
def undecidedViews(model, sigma):
    """Views of R on which the host polish does not agree with itself once each view's points are permuted (the same
    sums in another order), to a tenth of the bars the device is held to: 1e-6 on H, 1e-7 px on the reprojections of
    the view's own model points. The 20-iteration LM has accept/reject branches, so on a view where a decision hangs
    on the last bits two correct implementations part ways; there a comparison says nothing. -> tuple of indices"""
    v = problemR(model, sigma)
    Ha = hostPolish(model, sigma)
    vp = permuted(v)
    detsP = detections(vp)
    Hb = np.array(lc.refineHomographies(list(hostHomographies(model, sigma)), detsP))
    out = []
    for i, (sv, mv) in enumerate(detections(v)):
        dH = np.abs(Ha[i] - Hb[i]).max()
        dy = np.abs(project(Ha[i], mv) - project(Hb[i], mv)).max()
        if not (dH <= H_BAR / 10 and dy <= REPROJ_BAR / 10):
            out.append(i)
    return tuple(out)


# ---------------------------------------------------------------- extrinsics
EXT_VIEWS = 4099                             # 16 blocks of 256 and 3


def extrinsicsInput():
    """The host-polished homographies of R at its largest sigma (radtan), tiled to EXT_VIEWS, each copy times its own
    non-zero scale in [0.25, 4], negative on every third: -> (H (EXT_VIEWS,3,3), scale, A)"""
    H = hostPolish("radtan", R_SIGMAS["radtan"][-1])
    idx = np.arange(EXT_VIEWS) % H.shape[0]
    scale = 0.25 * 16.0 ** np.random.default_rng(3).random(EXT_VIEWS)
    scale[::3] *= -1.0
    return H[idx] * scale[:, None, None], scale, trueCamera("radtan")[0]


# ---------------------------------------------------------------- distortion normal equations
def distortionRows(modelName, A, W, offs, s, m):
    """D (2N x nk) and Ddot (2N,) of the linear distortion estimate in np.longdouble: the row formulas of
    lc.estimateDistortion (src/distortion.py:110-191 radtan, :222-271 fisheye), rows (u_j, v_j) interleaved.
    Also returns r (N,), the normalised radius the fisheye rows divide by."""
    ld = np.longdouble
    A = np.asarray(A, dtype=ld)
    fx, fy, uc, vc = A[0, 0], A[1, 1], A[0, 2], A[1, 2]
    offs = np.asarray(offs, dtype=np.int64)
    Udot = np.asarray(s, dtype=ld).reshape(-1, 2)
    bX = np.asarray(m, dtype=ld).reshape(-1, 3)
    W = np.asarray(W, dtype=ld).reshape(-1, 4, 4)
    vi = np.repeat(np.arange(offs.shape[0] - 1), np.diff(offs))
    Wp = W[vi]
    c = (Wp[:, :3, 0] * bX[:, 0:1] + Wp[:, :3, 1] * bX[:, 1:2] + Wp[:, :3, 2] * bX[:, 2:3]) + Wp[:, :3, 3]
    xn, yn = c[:, 0] / c[:, 2], c[:, 1] / c[:, 2]
    r = np.sqrt(xn * xn + yn * yn)
    u = fx * xn + A[0, 1] * yn + uc
    v = fy * yn + vc
    if modelName == "radtan":
        Du = np.stack(((u - uc) * r**2, (u - uc) * r**4, fx * (2 * xn * yn),
                       fx * (r**2 + 2 * xn**2), (u - uc) * r**6), axis=1)
        Dv = np.stack(((v - vc) * r**2, (v - vc) * r**4, fy * (r**2 + 2 * yn**2),
                       fy * (2 * xn * yn), (v - vc) * r**6), axis=1)
    else:
        th = np.arctan(r)
        tr = th / r
        Du = np.stack([fx * (u - uc) * tr * th**(2 * j) for j in (1, 2, 3, 4)], axis=1)
        Dv = np.stack([fy * (v - vc) * tr * th**(2 * j) for j in (1, 2, 3, 4)], axis=1)
    D = np.empty((2 * Du.shape[0], Du.shape[1]), dtype=ld)
    D[0::2], D[1::2] = Du, Dv
    Ddot = np.empty(2 * Du.shape[0], dtype=ld)
    Ddot[0::2], Ddot[1::2] = Udot[:, 0] - u, Udot[:, 1] - v
    return D, Ddot, r


def normalEquationsYardstick(v):
    """-> D^T D, D^T Ddot (longdouble), and the two bars: 1e-11 sqrt(DtD[a,a] DtD[b,b]) and 1e-11 sum |D[i,a] Ddot[i]|
    (1e-11 is the project's bar for B, E, V, g; per entry, because the columns span r^2 .. r^6)"""
    D, Ddot, r = distortionRows(v["model"], v["A"], v["W"], v["offs"], v["s"], v["m"])
    DtD, Dtd = D.T @ D, D.T @ Ddot
    d = np.sqrt(np.diagonal(DtD))
    return DtD, Dtd, 1e-11 * d[:, None] * d[None, :], 1e-11 * (np.abs(D) * np.abs(Ddot)[:, None]).sum(axis=0), r


def _smallMotion(rng, n):
    """n poses near the identity: up to 0.2 degrees about each axis and 2 mm along each, which moves no point of a
    board aimed at the middle of a square (makeViews) onto the optical axis"""
    T = np.tile(np.eye(4), (n, 1, 1))
    T[:, :3, :3] = orc.eulerToR(rng.uniform(-0.2, 0.2, (n, 3)))
    T[:, :3, 3] = rng.uniform(-0.002, 0.002, (n, 3))
    return T


@functools.lru_cache(maxsize=None)
def distortionCaseEmpty(model):
    """(a) R at sigma = 0.3 with empty views at the front, in the middle and at the end; every view has its own W"""
    return withEmptyViews(problemR(model, 0.3))[0]


@functools.lru_cache(maxsize=None)
def distortionCaseBig(model):
    """(b) BIG_VIEWS full 54-point views: 83 noisy views tiled, each copy's poses perturbed on their own. The second
    trip of the kernel's grid-stride loop is taken by the 26 points past 1 024 x 256."""
    base = makeViews(model, [BIG_BOARD[0] * BIG_BOARD[1]] * R_NUM_VIEWS, 0.3, R_SEED + 1000, board=BIG_BOARD)
    idx = np.arange(BIG_VIEWS) % R_NUM_VIEWS
    n = BIG_BOARD[0] * BIG_BOARD[1]
    W = _smallMotion(np.random.default_rng(5), BIG_VIEWS) @ base["W"][idx]
    pts = (idx[:, None] * n + np.arange(n)[None, :]).ravel()
    return dict(base, offs=np.arange(BIG_VIEWS + 1, dtype=np.int64) * n, s=np.ascontiguousarray(base["s"][pts]),
                m=np.ascontiguousarray(base["m"][pts]), W=W)


# ---------------------------------------------------------------- compose / decompose
def composeAngles():
    """EXT_VIEWS rows of Euler angles uniform in (-180, 180)^3 degrees, then -- in the last, partial block of 256, at
    indices >= 4096 -- the g0 golden's gimbal-lock rows (ry = +-90) with their neighbours, and rows with an angle of
    at most 1e-8 rad, which the reference's numeric Rodrigues path turns into the identity. -> (angles (n,3), t (n,3))"""
    rng = np.random.default_rng(11)
    g0 = np.array(loadGolden("g0_mathutils.npz")["angles"])
    special = [g0[40:50],
               [[0.0, 89.9, 0.0], [0.0, -89.9, 0.0], [25.0, 89.999, -40.0], [25.0, 90.001, -40.0],
                [12.0, 89.75, 50.0], [12.0, 89.7, -50.0], [12.0, -89.7, -50.0],      # the isclose band ends at 0.256 degrees
                [5e-7, 0.0, 0.0], [0.0, -5.7e-7, 0.0], [0.0, 0.0, 5.8e-7], [3e-7, -3e-7, 3e-7], [30.0, 5e-7, -5e-7]]]
    angles = np.vstack([rng.uniform(-180.0, 180.0, (EXT_VIEWS, 3))] + [np.asarray(a, dtype=np.float64) for a in special])
    return angles, rng.uniform(-2.0, 2.0, angles.shape)


# ---------------------------------------------------------------- the whole stage
STAGE_SIGMA = 0.3
STAGE_EXISTING_BARS = (1e-5, 1e-6, 1e-5)     # A, W, k in test_device_initialisation_stages_vs_reference


def stageDifference(a, b):
    """(A relative to its largest entry, W, k) differences of two (A, W, k) results"""
    return (float(np.abs(a[0] - b[0]).max() / np.abs(b[0]).max()), float(np.abs(np.array(a[1]) - np.array(b[1])).max()),
            float(np.abs(np.array(a[2]) - np.array(b[2])).max()))


def _distortionModel(model):
    import camera_calibration_amd as cca
    return cca.RadialTangentialModel() if model == "radtan" else cca.FisheyeModel()


@functools.lru_cache(maxsize=None)
def hostStage(model, sigma=STAGE_SIGMA):
    """-> (host result (A, W, k), its self-difference under a permutation of every view's points, the bars: 100 x
    the self-difference, floored at 1e-12 -- the device sums in a third order and may part from the host on an
    undecided view)"""
    v = problemR(model, sigma)
    dm = _distortionModel(model)
    res = lc.estimateCalibrationParameters(dm, detections(v))
    resP = lc.estimateCalibrationParameters(dm, detections(permuted(v)))
    selfDiff = stageDifference(resP, res)
    return res, selfDiff, tuple(max(100.0 * d, 1e-12) for d in selfDiff)
