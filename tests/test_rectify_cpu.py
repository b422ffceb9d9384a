"""Rectification and triangulation, the parts that need no GPU: the C ABI declares and exports the new entry points and
rejects bad arguments before it needs a device, and the host arithmetic of camera_calibration_amd/rectify.py -- the
rectifying rotations, the projection matrices, Q, the focal length from the cameras' fields of view -- against
tests/rectify_yardstick.py. Wherever rectify.py would ask the device for the inverse of the model, these tests hand it
the yardstick's numpy Newton instead (rectify._rectification / _newCameraMatrix take the inverse as an argument).

Bars: 1e-14 on the rotations' identities (a handful of fp64 roundings on entries <= 1), 1e-9 px on pixels that must
agree (the numpy Newton leaves 1e-13 of a normalised coordinate, times a focal length of some hundred pixels), 0.5 px
for the overshoot of the alpha = 0 maps (a condition the issue sets, not a measurement)."""
import functools
import os
import re

import numpy as np
import pytest

import camera_calibration_amd as cca
import rectify_yardstick as ry
import stereo_yardstick as sy
from camera_calibration_amd import _native as nat
from camera_calibration_amd import engine, rectify, synthetic
from conftest import ROOT
from oracle import calib_oracle as orc

NEW_SYMBOLS = ("calib_rectify_maps", "calib_rectify_points", "calib_triangulate")
SIZE = (640, 480)
CAM_A = ("radtan", np.asarray(synthetic.RADTAN_A, dtype=np.float64), synthetic.RADTAN_K)
CAM_B = ("fisheye", sy.A_B, sy.K_B["fisheye"])
CAM_B_RADTAN = ("radtan", sy.A_B, sy.K_B["radtan"])


def yardstickInverse(cam, uv):
    """rectify.py's inverse hook, served by the numpy Newton"""
    return ry.newtonInverse((cam[0], cam[2], cam[3]), uv)


@functools.lru_cache(maxsize=None)
def rig(which):
    """(R, t, Xa): the rig of stereo_yardstick.makeStereo (2, -3, 1.5 degrees, baseline along -x), or the same rotation
    with the baseline along y; Xa the board corners of 6 views in camera a's frame"""
    prob, PsTrue = sy.makeStereo(6)
    R, t = orc.eulerToR(PsTrue[:3])[0], PsTrue[3:6].copy()
    if which == "vertical":
        t = np.array([0.1 * t[1], -t[0], t[2]])
    Xa, _, _ = sy.pointsInA(prob, PsTrue, "a")
    for a in (R, t, Xa):
        a.setflags(write=False)
    return R, t, Xa


def packageRectification(which, **kw):
    R, t, _ = rig(which)
    return rectify._rectification(CAM_A, CAM_B, R, t, SIZE, None, None, kw.pop("alpha", None), kw.pop("focal", None),
                                  kw.pop("zeroDisparity", True), yardstickInverse)


# ---- symbols, version, arguments -----------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_new_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "calib_lm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(calib_[a-z0-9_]+)\s*\(", text))
    lib = nat.loadLibrary()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/calib_lm.h"
        assert n in nat.SIGNATURES, f"{n} has no ctypes signature"
        assert hasattr(lib, n), f"{n} is not exported by the library"
    assert lib.calib_version() >= 450


def test_python_surface_is_exported():
    for name in ("rectify", "rectifyRotations", "stereoRectify", "StereoRectification", "optimalNewCameraMatrix",
                 "triangulate"):
        assert hasattr(cca, name), name
    for name in ("rectifyMaps", "rectifyPoints", "triangulate"):
        assert callable(getattr(engine, name)), name
    for cls in (cca.RadialTangentialModel, cca.FisheyeModel):
        assert callable(cls.rectifyMaps) and callable(cls.rectifyPoints)
    for name in ("maps", "rectifyPoints", "reproject", "apply"):
        assert callable(getattr(cca.StereoRectification, name)), name
    assert callable(cca.StereoCalibration.rectify) and callable(cca.StereoCalibration.triangulate)


def test_c_abi_rejects_bad_arguments_before_it_needs_a_device():
    lib = nat.loadLibrary()
    A = np.ascontiguousarray(synthetic.RADTAN_A, dtype=np.float64)
    flat = A.copy()
    flat[0, 0] = 0.0                                                            # alpha = 0
    k = np.array(synthetic.RADTAN_K, dtype=np.float64)
    R, t = np.eye(3), np.array([-0.1, 0.0, 0.0])
    scaled = 1.01 * np.eye(3)                                                   # det = 1.03
    mirror = np.diag([1.0, 1.0, -1.0])                                          # det = -1
    uv, out, X = np.zeros((3, 2)), np.zeros((3, 2)), np.zeros((3, 3))
    mx, my = np.zeros((4, 6), dtype=np.float32), np.zeros((4, 6), dtype=np.float32)
    d, f = nat.dptr, nat.f32ptr
    maps = lib.calib_rectify_maps
    assert maps(0, d(A), d(k), None, d(A), 6, 0, f(mx), f(my), 0) == nat.E_INVALID
    assert maps(0, d(A), d(k), None, d(A), -6, 4, f(mx), f(my), 0) == nat.E_INVALID
    assert maps(0, d(A), d(k), None, None, 6, 4, f(mx), f(my), 0) == nat.E_INVALID
    assert maps(0, d(A), d(k), None, d(A), 6, 4, None, f(my), 0) == nat.E_INVALID
    assert maps(0, None, d(k), None, d(A), 6, 4, f(mx), f(my), 0) == nat.E_INVALID
    assert maps(0, d(flat), d(k), None, d(A), 6, 4, f(mx), f(my), 0) == nat.E_INVALID
    assert maps(0, d(A), d(k), None, d(flat), 6, 4, f(mx), f(my), 0) == nat.E_INVALID
    assert maps(2, d(A), d(k), None, d(A), 6, 4, f(mx), f(my), 0) == nat.E_INVALID
    assert maps(0, d(A), d(k), d(scaled), d(A), 6, 4, f(mx), f(my), 0) == nat.E_INVALID
    assert maps(0, d(A), d(k), d(mirror), d(A), 6, 4, f(mx), f(my), 0) == nat.E_INVALID
    assert maps(0, d(A), d(k), None, d(A), 65536, 32768, f(mx), f(my), 0) == nat.E_INVALID      # 2^31 pixels
    pts = lib.calib_rectify_points
    assert pts(0, 0, d(A), d(k), None, None, d(A), None, None, 0) == 0                          # n == 0
    assert pts(0, -1, d(A), d(k), d(uv), None, d(A), d(out), None, 0) == nat.E_INVALID
    assert pts(0, 3, d(A), d(k), None, None, d(A), d(out), None, 0) == nat.E_INVALID
    assert pts(0, 3, d(A), d(k), d(uv), None, None, d(out), None, 0) == nat.E_INVALID
    assert pts(0, 3, d(A), d(k), d(uv), None, d(flat), d(out), None, 0) == nat.E_INVALID
    assert pts(0, 3, d(A), d(k), d(uv), d(mirror), d(A), d(out), None, 0) == nat.E_INVALID
    assert pts(5, 3, d(A), d(k), d(uv), None, d(A), d(out), None, 0) == nat.E_INVALID
    tri = lib.calib_triangulate
    assert tri(0, d(A), d(k), 0, d(A), d(k), d(R), d(t), 0, None, None, None, None, None, 0) == 0    # n == 0
    assert tri(0, d(A), d(k), 0, d(A), d(k), d(R), d(t), -2, d(uv), d(uv), d(X), None, None, 0) == nat.E_INVALID
    assert tri(0, d(A), d(k), 0, d(A), d(k), d(R), d(t), 3, d(uv), None, d(X), None, None, 0) == nat.E_INVALID
    assert tri(0, d(A), d(k), 0, d(A), d(k), d(R), d(t), 3, d(uv), d(uv), None, None, None, 0) == nat.E_INVALID
    assert tri(0, d(A), d(k), 0, d(A), d(k), None, d(t), 3, d(uv), d(uv), d(X), None, None, 0) == nat.E_INVALID
    assert tri(0, d(A), d(k), 0, d(A), d(k), d(R), None, 3, d(uv), d(uv), d(X), None, None, 0) == nat.E_INVALID
    assert tri(0, d(A), d(k), 3, d(A), d(k), d(R), d(t), 3, d(uv), d(uv), d(X), None, None, 0) == nat.E_INVALID
    assert tri(0, d(flat), d(k), 0, d(A), d(k), d(R), d(t), 3, d(uv), d(uv), d(X), None, None, 0) == nat.E_INVALID
    assert tri(0, d(A), d(k), 0, d(A), d(k), d(scaled), d(t), 3, d(uv), d(uv), d(X), None, None, 0) == nat.E_INVALID
    assert nat.lastError()


@pytest.fixture
def noNativeCalls(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the wrapper reached the native library")
    monkeypatch.setattr(nat, "loadLibrary", refuse)
    monkeypatch.setattr(nat, "requireDevice", refuse)


def test_wrappers_reject_bad_shapes_before_any_native_call(noNativeCalls):
    name, A, k = CAM_A
    model = cca.RadialTangentialModel()
    R, t, _ = rig("horizontal")
    with pytest.raises(ValueError):
        model.rectifyMaps(A, k, None, A, (0, 5))
    with pytest.raises(ValueError):
        model.rectifyMaps(A, k, None, A, 640)
    with pytest.raises(ValueError):
        model.rectifyMaps(A, k, np.eye(4), A, (6, 5))
    with pytest.raises(ValueError):
        model.rectifyMaps(A, k, 2.0 * np.eye(3), A, (6, 5))
    with pytest.raises(ValueError):
        model.rectifyMaps(A, k, None, np.eye(4), (6, 5))
    with pytest.raises(ValueError):
        model.rectifyPoints(A, k, np.zeros((4, 3)), None, A)
    with pytest.raises(ValueError):
        model.rectifyPoints(A, k[:4], np.zeros((4, 2)), None, A)
    with pytest.raises(ValueError):
        cca.triangulate(CAM_A, CAM_B, R, t, np.zeros((4, 2)), np.zeros((5, 2)))
    with pytest.raises(ValueError):
        cca.triangulate(CAM_A, CAM_B, R, t[:2], np.zeros((4, 2)), np.zeros((4, 2)))
    with pytest.raises(ValueError):
        cca.triangulate(("pinhole", A, k), CAM_B, R, t, np.zeros((4, 2)), np.zeros((4, 2)))
    with pytest.raises(ValueError):
        cca.stereoRectify(CAM_A, CAM_B, R, t, (640, 0), focal=400.0)
    rect = cca.stereoRectify(CAM_A, CAM_B, R, t, SIZE)                          # alpha=None: host arithmetic only
    with pytest.raises(ValueError):
        rect.maps("c")
    with pytest.raises(ValueError):
        rect.reproject(np.zeros((3, 2)))


# ---- rotations -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["horizontal", "vertical"])
def test_rectifying_rotations(which):
    R, t, _ = rig(which)
    R1, R2, axis = cca.rectifyRotations(R, t)
    assert axis == (0 if which == "horizontal" else 1)
    ortho = max(np.abs(Rc.T @ Rc - np.eye(3)).max() for Rc in (R1, R2))
    det = max(abs(np.linalg.det(Rc) - 1.0) for Rc in (R1, R2))
    chain = np.abs(R1 - R2 @ R).max()
    b = R2 @ t
    off = np.abs(np.delete(b, axis)).max()
    print(f"{which}: |R^T R - I| {ortho:.2e}, |det - 1| {det:.2e}, |R1 - R2 R| {chain:.2e} (bar 1e-14), off-axis "
          f"baseline {off:.2e} (bar {1e-14 * np.linalg.norm(t):.2e})")
    assert ortho <= 1e-14 and det <= 1e-14 and chain <= 1e-14
    assert off <= 1e-14 * np.linalg.norm(t)
    assert np.sign(b[axis]) == np.sign((ry.rot(-ry.rotVec(R) / 2) @ t)[axis])
    yR1, yR2, yaxis = ry.rectifyRotations(R, t)
    assert yaxis == axis and np.abs(R1 - yR1).max() <= 1e-14 and np.abs(R2 - yR2).max() <= 1e-14


def test_a_rectified_rig_returns_the_identity_bit_for_bit():
    for t in ([-0.2, 0.0, 0.0], [0.3, 0.0, 0.0], [0.0, 0.1, 0.0], [0.0, -7.0, 0.0]):
        R1, R2, axis = cca.rectifyRotations(np.eye(3), t)
        assert R1.tobytes() == np.eye(3).tobytes() and R2.tobytes() == np.eye(3).tobytes()
        assert axis == (0 if t[0] != 0.0 else 1)


def test_rotations_that_cannot_be_rectified_raise():
    R, t, _ = rig("horizontal")
    with pytest.raises(ValueError):
        cca.rectifyRotations(R, [0.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        cca.rectifyRotations(ry.rot([0.0, np.pi / 2, 0.0]), t)                  # 90 degrees
    with pytest.raises(ValueError):
        cca.rectifyRotations(ry.rot([0.0, 2.0, 1.0]), t)                        # 128 degrees
    cca.rectifyRotations(ry.rot([0.0, 1.5, 0.0]), t)                            # 86 degrees: fine
    with pytest.raises(ValueError):
        cca.rectifyRotations(np.eye(4), t)


# ---- the epipolar property, through the yardstick ---------------------------------------------------------------------
@pytest.mark.parametrize("zeroDisparity", [True, False])
@pytest.mark.parametrize("which", ["horizontal", "vertical"])
def test_rectified_points_share_a_row_and_Q_returns_them(which, zeroDisparity):
    R, t, Xa = rig(which)
    rect = packageRectification(which, zeroDisparity=zeroDisparity)
    yard = ry.rectification(CAM_A, CAM_B, R, t, SIZE, zeroDisparity=zeroDisparity)
    for key in ("R1", "R2", "P1", "P2", "Q"):
        assert np.abs(rect[key] - yard[key]).max() <= 1e-12 * max(1.0, np.abs(yard[key]).max()), key
    axis = rect["axis"]
    uvA, uvB = ry.projectCamera(CAM_A, Xa), ry.projectCamera(CAM_B, Xa @ R.T + t)
    xyA, stA = ry.newtonInverse(CAM_A, uvA)
    xyB, stB = ry.newtonInverse(CAM_B, uvB)
    assert not stA.any() and not stB.any()
    ra, za = ry.rectifyNormalised(xyA, rect["R1"], rect["P1"])
    rb, zb = ry.rectifyNormalised(xyB, rect["R2"], rect["P2"])
    assert (za > 0).all() and (zb > 0).all()
    across = 1 - axis
    rows = np.abs(ra[:, across] - rb[:, across]).max()
    Xr = Xa @ rect["R1"].T                                                      # the rectified frame of camera a
    f = rect["P1"][0, 0]
    centre = rect["P1"][axis, 2] - rect["P2"][axis, 2]
    d = ra[:, axis] - rb[:, axis]
    want = -f * (rect["R2"] @ t)[axis] / Xr[:, 2] + centre
    disp = np.abs(d - want).max()
    StereoRectification = cca.StereoRectification(rect)
    back = StereoRectification.reproject(np.column_stack((ra, d)))
    rel = (np.linalg.norm(back - Xr, axis=1) / np.linalg.norm(Xr, axis=1)).max()
    print(f"{which}, zeroDisparity={zeroDisparity}: rows differ by {rows:.2e} px, disparity off by {disp:.2e} px, "
          f"Q off by {rel:.2e} relative (bars 1e-9); centre difference {centre:.3f} px")
    assert rows <= 1e-9 and disp <= 1e-9 and rel <= 1e-9
    assert (centre == 0.0) == zeroDisparity
    assert rect["P2"][axis, 3] == f * (rect["R2"] @ t)[axis] and rect["baseline"] == np.linalg.norm(t)


def test_default_focal_length_and_given_focal_length():
    for which, want in (("horizontal", min(CAM_A[1][1, 1], CAM_B[1][1, 1])), ("vertical", min(CAM_A[1][0, 0], CAM_B[1][0, 0]))):
        rect = packageRectification(which)
        assert rect["P1"][0, 0] == rect["P1"][1, 1] == rect["P2"][0, 0] == rect["P2"][1, 1] == want
        assert packageRectification(which, focal=321.5, alpha=0.3)["P1"][0, 0] == 321.5
    # each optical axis keeps its pixel in the coordinate the cameras do not share
    R, t, _ = rig("horizontal")
    rect = packageRectification("horizontal", zeroDisparity=False)
    for Rc, P, cam in ((rect["R1"], rect["P1"], CAM_A), (rect["R2"], rect["P2"], CAM_B)):
        px = P[:, :3] @ (Rc @ np.array([0.0, 0.0, 1.0]))
        assert abs(px[0] / px[2] - cam[1][0, 2]) <= 1e-9


# ---- the alpha rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["horizontal", "vertical"])
def test_alpha_one_keeps_every_sample_and_touches_the_border(which):
    R, t, _ = rig(which)
    rect = packageRectification(which, alpha=1.0)
    lowest, highest = np.inf, -np.inf
    touch = np.inf
    for cam, Rc, P in ((CAM_A, rect["R1"], rect["P1"]), (CAM_B, rect["R2"], rect["P2"])):
        p = ry.gridInRectifiedFrame(cam, SIZE, Rc).reshape(-1, 2)
        assert p.shape == (289, 2)
        px = p * P[0, 0] + P[:2, 2]
        lo, hi = px.min(axis=0), np.array([SIZE[0] - 1.0, SIZE[1] - 1.0]) - px.max(axis=0)
        lowest, highest = min(lowest, lo.min(), hi.min()), max(highest, lo.max(), hi.max())
        touch = min(touch, np.abs(lo).min(), np.abs(hi).min())
    print(f"{which}: the samples keep at least {lowest:.3e} px from the border, the nearest is {touch:.3e} px from it")
    assert lowest >= -1e-9 and touch <= 1e-9


@pytest.mark.parametrize("which", ["horizontal", "vertical"])
def test_alpha_zero_maps_stay_inside_the_source(which):
    rect = packageRectification(which, alpha=0.0)
    worst = 0.0
    for cam, Rc, P in ((CAM_A, rect["R1"], rect["P1"]), (CAM_B, rect["R2"], rect["P2"])):
        mx, my, z = ry.rectifyMaps(cam, Rc, P, *SIZE)
        assert (z > 0).all()
        over = max(-mx.min(), mx.max() - (SIZE[0] - 1), -my.min(), my.max() - (SIZE[1] - 1))
        worst = max(worst, over)
    print(f"{which}: the alpha = 0 maps overshoot the source by {worst:.3f} px (cap 0.5)")
    assert worst <= 0.5


def test_alpha_interpolates_the_focal_lengths():
    f0, f1 = (packageRectification("horizontal", alpha=a)["P1"][0, 0] for a in (0.0, 1.0))
    fh = packageRectification("horizontal", alpha=0.5)["P1"][0, 0]
    R, t, _ = rig("horizontal")
    yard = ry.rectification(CAM_A, CAM_B, R, t, SIZE, alpha=0.5)
    print(f"f_in {f0:.4f}, f_out {f1:.4f}, alpha = 0.5: {fh:.4f}; yardstick {yard['fin']:.4f}, {yard['fout']:.4f}")
    assert f0 > f1 > 0
    assert abs(fh - 0.5 * (f0 + f1)) <= 1e-12 * f0
    assert abs(f0 - yard["fin"]) <= 1e-9 * f0 and abs(f1 - yard["fout"]) <= 1e-9 * f0 and abs(fh - yard["f"]) <= 1e-9 * f0


@pytest.mark.parametrize("cam", [CAM_A, CAM_B, CAM_B_RADTAN], ids=["radtan_a", "fisheye_b", "radtan_b"])
def test_optimal_new_camera_matrix(cam):
    newSize = (800, 600)
    got = {a: rectify._newCameraMatrix(cam[0], cam[1], cam[2], SIZE, a, newSize, yardstickInverse) for a in (0.0, 0.5, 1.0)}
    yard0, fin, fout, grid = ry.newCameraMatrix(cam, SIZE, 0.0, newSize)
    for a, newA in got.items():
        want = ry.newCameraMatrix(cam, SIZE, a, newSize)[0]
        assert np.abs(newA - want).max() <= 1e-9 * fin
        assert newA[0, 0] == newA[1, 1] and newA[0, 1] == 0.0
        assert abs(newA[0, 2] - cam[1][0, 2] * 800 / 640) <= 1e-12 * 800 and abs(newA[1, 2] - cam[1][1, 2] * 600 / 480) <= 1e-12 * 600
    assert abs(got[0.5][0, 0] - 0.5 * (got[0.0][0, 0] + got[1.0][0, 0])) <= 1e-12 * fin
    # alpha = 1: all 289 samples inside the destination, one on its border
    px = grid.reshape(-1, 2) * got[1.0][0, 0] + got[1.0][:2, 2]
    lo, hi = px.min(axis=0), np.array([799.0, 599.0]) - px.max(axis=0)
    touch = min(np.abs(lo).min(), np.abs(hi).min())
    # alpha = 0: the map of the undistorted image stays within 0.5 px of the source
    mx, my, _ = ry.rectifyMaps(cam, None, got[0.0], *newSize)
    over = max(-mx.min(), mx.max() - (SIZE[0] - 1), -my.min(), my.max() - (SIZE[1] - 1))
    print(f"{cam[0]}: f_in {fin:.3f}, f_out {fout:.3f}; alpha = 1 margin {min(lo.min(), hi.min()):.2e}, touches within "
          f"{touch:.2e}; alpha = 0 overshoot {over:.3f} px (cap 0.5)")
    assert min(lo.min(), hi.min()) >= -1e-9 and touch <= 1e-9
    assert over <= 0.5


def test_a_camera_whose_corners_have_no_inverse_raises():
    fish = ("fisheye", np.asarray(synthetic.FISHEYE_A, dtype=np.float64), synthetic.FISHEYE_K)
    _, status = ry.newtonInverse(fish, np.array([[0.0, 0.0], [639.0, 479.0], [700.0, 529.0]]))
    assert status.tolist() == [1, 0, 0]                                         # the corner (0, 0) is out of the model's reach
    R, t, _ = rig("horizontal")
    with pytest.raises(ValueError, match="alpha=None"):
        rectify._rectification(fish, CAM_B, R, t, SIZE, None, None, 0.0, None, True, yardstickInverse)
    with pytest.raises(ValueError, match="alpha=None"):
        rectify._newCameraMatrix("fisheye", fish[1], fish[2], SIZE, 1.0, None, yardstickInverse)
    with pytest.raises(ValueError, match="alpha=None"):                         # a rotation that turns samples backwards
        rectify.rectifiedGrid(np.zeros((289, 2)) + [2.0, 0.0], np.zeros(289, dtype=np.int32), ry.rot([0.0, 0.6, 0.0]), "a")
    rectify._rectification(fish, CAM_B, R, t, SIZE, None, None, None, None, True, yardstickInverse)     # alpha=None: fine


# ---- the yardstick's own pieces ------------------------------------------------------------------------------------------
def test_yardstick_inverse_and_midpoint_on_known_points():
    R, t, Xa = rig("horizontal")
    for cam in (CAM_A, CAM_B, CAM_B_RADTAN):
        xy, st = ry.newtonInverse(cam, ry.projectCamera(cam, Xa))
        assert not st.any() and np.abs(xy - Xa[:, :2] / Xa[:, 2:]).max() <= 1e-12
    Xb = Xa @ R.T + t
    X0, sin2, (s, u) = ry.midpoint(Xa[:, :2] / Xa[:, 2:], Xb[:, :2] / Xb[:, 2:], R, t)
    assert (np.linalg.norm(X0 - Xa, axis=1) / np.linalg.norm(Xa, axis=1)).max() <= 1e-12
    assert np.abs(s - Xa[:, 2]).max() <= 1e-11 and np.abs(u - Xb[:, 2]).max() <= 1e-11
    print(f"sin^2 of the rays' angle: {sin2.min():.4f} .. {sin2.max():.4f}")
    J = ry.triJacobian(CAM_A, CAM_B, R, t, Xa[:5])
    r0 = ry.triResiduals(CAM_A, CAM_B, R, t, Xa[:5], np.zeros((5, 2)), np.zeros((5, 2)))
    d = 1e-6 * np.array([1.0, -2.0, 0.5])
    r1 = ry.triResiduals(CAM_A, CAM_B, R, t, Xa[:5] + d, np.zeros((5, 2)), np.zeros((5, 2)))
    assert np.abs((r0 - r1) - J @ d).max() <= 1e-6                              # first order in a 1e-6 step
