"""N-view triangulation without a device: guards of tests/multiview_yardstick.py (what the GPU tests measure the kernel
against), the C ABI's argument checks, and the Python wrappers' own.

Where the bars come from:
  start        for two cameras the closest point to two rays IS the midpoint of their common perpendicular; the two
               formulas differ in rounding only, amplified by 1 / sin^2 ~ 200 of the rays' angle: 1e-12 of |X|.
  sin^2        the GPU tests' scenes must be far from the kernel's parallel rule (1e-12): >= 1e-3.
  loop         the yardstick's own loop must reach a stationary point on the noisy scenes, |J^T r| <= 1e-8 |J| |r|, the
               bar test_gpu_rectify holds the pair kernel to (central differences resolve ~1e-10); and every point's error
               stays above 1e-6 px^2, where a relative bar of 1e-9 on it is above the rounding of a projected pixel
               (multiview_yardstick.NOISE_SEED).
  covariance   (J^T J)^-1 from central differences with steps 1e-5 and 3e-5 |X| agree within 1e-8 of the largest entry
               (truncation (3e-5)^2 ~ 1e-9 relative, rounding 1e-16 / 1e-5 ~ 1e-11)."""
import os
import re

import numpy as np
import pytest

import camera_calibration_amd as cca
import multiview_yardstick as my
import rectify_yardstick as ry
from camera_calibration_amd import _native as nat
from camera_calibration_amd import engine, rectify, synthetic
from conftest import ROOT

GPU_SCENES = [(2, 3, 0.0), (3, 3, 0.0), (8, 3, 0.0), (2, 3, 0.3), (3, 3, 0.3), (8, 3, 0.3), (3, 10, 0.0)]


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def test_two_camera_start_is_the_midpoint_of_the_common_perpendicular():
    sc = my.scene(2, 3)
    both = np.ones_like(sc["seen"])
    xy, status = my.inverse(sc["cameras"], sc["uv"])
    assert not status.any()
    X0 = my.closestPoint(sc["T"], xy, both)
    mid, sin2, _ = ry.midpoint(xy[0], xy[1], sc["T"][1][:3, :3], sc["T"][1][:3, 3])
    rel = np.linalg.norm(X0 - mid, axis=1) / np.linalg.norm(mid, axis=1)
    dsin = np.abs(my.maxPairSin2(sc["T"], xy, both) - sin2)
    print(f"|closest point - midpoint| / |X| {rel.max():.2e}, |sin^2 - midpoint's| {dsin.max():.2e} (bars 1e-12)")
    assert rel.max() <= 1e-12 and dsin.max() <= 1e-12


@pytest.mark.parametrize("N,M,sigma", GPU_SCENES)
def test_scenes_of_the_gpu_tests_are_well_posed(N, M, sigma):
    sc = my.scene(N, M, sigma)
    assert (sc["seen"].sum(axis=0) >= 2).all() and sc["seen"].shape == (N, 54 * M)
    if N > 2:
        assert (sc["seen"].sum(axis=0) < N).any()                               # the masks do hide cameras
    xy, status = my.inverse(sc["cameras"], sc["uv"])
    assert not status.any()
    sin2 = my.maxPairSin2(sc["T"], xy, sc["seen"])
    X0 = my.closestPoint(sc["T"], xy, sc["seen"])
    front = my.inCameras(sc["T"], X0)[:, :, 2] > 0
    print(f"N {N} M {M} sigma {sigma}: max-pair sin^2 {sin2.min():.2e} .. {sin2.max():.2e}")
    assert sin2.min() >= 1e-3
    assert front.all()


@pytest.mark.parametrize("N", [2, 3, 8])
def test_yardstick_loop_reaches_a_stationary_point(N):
    sc = my.scene(N, 3, 0.3)
    got = my.triangulate(sc["cameras"], sc["T"], sc["uv"], sc["seen"])
    assert not got["status"].any()
    grad, scale, sse, _ = my.gradientCheck(sc["cameras"], sc["T"], got["X"], sc["uv"], sc["seen"])
    print(f"N {N}: max |J^T r| / (|J| |r|) {(grad / scale).max():.2e} (bar 1e-8), sse / sse(start) up to "
          f"{(got['sse'] / got['sse0']).max():.6f}")
    assert (grad <= 1e-8 * scale).all()
    assert (got["sse"] <= got["sse0"]).all()
    print(f"N {N}: smallest sse {got['sse'].min():.2e} px^2 (floor 1e-6: multiview_yardstick.NOISE_SEED)")
    assert got["sse"].min() >= 1e-6
    assert np.abs(got["sse"] - sse).max() <= 1e-12 * sse.max()


@pytest.mark.parametrize("N", [2, 3, 8])
def test_yardstick_covariance_does_not_depend_on_its_step(N):
    sc = my.scene(N, 3, 0.3)
    a = my.covariance(sc["cameras"], sc["T"], sc["X"], sc["seen"], 1e-5)
    b = my.covariance(sc["cameras"], sc["T"], sc["X"], sc["seen"], 3e-5)
    rel = np.abs(a - b).max(axis=(1, 2)) / np.abs(a).max(axis=(1, 2))
    print(f"N {N}: the two steps differ by {rel.max():.2e} of the largest entry (bar 1e-8)")
    assert np.isfinite(a).all() and rel.max() <= 1e-8


def test_mask_words():
    seen = np.array([[True, False, True], [False, False, True], [True, False, True]])
    assert my.maskWords(seen).tolist() == [5, 0, 7] and my.maskWords(seen).dtype == np.uint32
    uv = np.zeros((3, 3, 2))
    uv[~seen] = np.nan
    assert rectify.seenMasks(uv).tolist() == [5, 0, 7]
    uv[0, 0, 1] = np.inf                                                        # one coordinate not finite: not seen
    assert rectify.seenMasks(uv).tolist() == [4, 0, 7]


# ---- symbols, version, arguments -----------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "calib_lm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(calib_[a-z0-9_]+)\s*\(", text))
    lib = nat.loadLibrary()
    assert "calib_triangulate_multi" in declared and "calib_view_camera_t" in text
    assert "calib_triangulate_multi" in nat.SIGNATURES and hasattr(lib, "calib_triangulate_multi")
    assert lib.calib_version() >= 480
    for name in ("triangulateMulti",):
        assert callable(getattr(cca, name)) and callable(getattr(engine, name))
    assert callable(cca.RigCalibration.triangulateAll)


def viewCameras(cams):
    """[(model, A, k, R, t)] -> (ctypes array, what it points into)"""
    arr = (nat.ViewCamera * len(cams))()
    keep = []
    for c, (model, A, k, R, t) in enumerate(cams):
        keep.append([None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (A, k, R, t)])
        arr[c] = nat.ViewCamera(model, *[nat.dptr(a) for a in keep[-1]])
    return arr, keep


def test_c_abi_rejects_bad_arguments_before_it_needs_a_device():
    lib = nat.loadLibrary()
    tri = lib.calib_triangulate_multi
    A = np.ascontiguousarray(synthetic.RADTAN_A, dtype=np.float64)
    flat = A.copy()
    flat[1, 1] = 0.0                                                            # beta = 0
    k = np.array(synthetic.RADTAN_K, dtype=np.float64)
    R, t = np.eye(3), np.array([-0.1, 0.0, 0.0])
    scaled = 1.01 * np.eye(3)                                                   # det = 1.03
    good = (0, A, k, R, t)
    uv, X = np.zeros((3, 4, 2)), np.zeros((4, 3))
    d = nat.dptr

    def call(cams, n=4, num=None, uvp=d(uv), seen=None, Xp=d(X)):
        arr, keep = viewCameras(cams)
        sp = None if seen is None else np.asarray(seen, dtype=np.uint32).ctypes.data_as(nat._c_uint32_p)
        return tri(len(cams) if num is None else num, arr, n, uvp, sp, Xp, None, None, None, None, 0)

    assert call([good, good], n=0, uvp=None, Xp=None) == 0                     # n == 0 touches no device
    assert call([good] * 8, n=0) == 0
    assert call([good]) == nat.E_INVALID                                        # N = 1
    assert call([good] * 9) == nat.E_INVALID                                    # N = 9
    assert tri(2, None, 4, d(uv), None, d(X), None, None, None, None, 0) == nat.E_INVALID
    assert call([good, good], uvp=None) == nat.E_INVALID
    assert call([good, good], Xp=None) == nat.E_INVALID
    assert call([good, (0, None, k, R, t)]) == nat.E_INVALID
    assert call([good, (0, A, None, R, t)]) == nat.E_INVALID
    assert call([good, (2, A, k, R, t)]) == nat.E_INVALID                       # model id
    assert call([good, (-1, A, k, R, t)]) == nat.E_INVALID
    assert call([good, (0, flat, k, R, t)]) == nat.E_INVALID
    assert call([(0, A, k, scaled, t), good]) == nat.E_INVALID
    assert call([good, (0, A, k, np.diag([1.0, 1.0, -1.0]), t)]) == nat.E_INVALID
    assert call([good, good], n=-1) == nat.E_INVALID
    assert call([good, good], seen=[3, 3, 4, 3]) == nat.E_INVALID               # bit 2 of a two-camera call
    assert call([good, good, good], seen=[7, 0, 8, 1]) == nat.E_INVALID
    assert nat.lastError()
    assert call([good, (0, A, k, None, None)], n=0) == 0                        # R NULL = identity, t NULL = 0
    assert call([good, good, good], n=0, seen=[]) == 0


@pytest.fixture
def noNativeCalls(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the wrapper reached the native library")
    monkeypatch.setattr(nat, "loadLibrary", refuse)
    monkeypatch.setattr(nat, "requireDevice", refuse)


def test_wrappers_reject_bad_arguments_before_any_native_call(noNativeCalls):
    sc = my.scene(3, 3)
    cams, T, uv = sc["cameras"], sc["T"], sc["uv"]
    n = uv.shape[1]
    with pytest.raises(ValueError, match="cameras"):
        cca.triangulateMulti(cams[:1], T[:1], uv[:1])
    with pytest.raises(ValueError, match="cameras"):
        cca.triangulateMulti(cams * 3, np.tile(T, (3, 1, 1)), np.tile(uv, (3, 1, 1)))
    with pytest.raises(ValueError, match="T"):
        cca.triangulateMulti(cams, T[:2], uv)
    with pytest.raises(ValueError, match="T"):
        cca.triangulateMulti(cams, T[:, :3, :3], uv)
    with pytest.raises(ValueError, match="uv"):
        cca.triangulateMulti(cams, T, uv[:2])
    with pytest.raises(ValueError, match="uv"):
        cca.triangulateMulti(cams, T, uv[:, :, :1])
    with pytest.raises(ValueError, match="uv"):
        cca.triangulateMulti(cams, T, [uv[0], uv[1]])
    with pytest.raises(ValueError, match="uv"):
        cca.triangulateMulti(cams, T, [uv[0], uv[1], uv[2][:5]])
    with pytest.raises(ValueError, match="seen"):
        cca.triangulateMulti(cams, T, uv, seen=np.ones(n - 1, dtype=np.uint32))
    with pytest.raises(ValueError, match="seen"):
        cca.triangulateMulti(cams, T, uv, seen=np.full(n, 8, dtype=np.uint32))
    with pytest.raises(ValueError, match="seen"):
        cca.triangulateMulti(cams, T, uv, seen=np.ones(n))                      # floats are not masks
    bad = T.copy()
    bad[1, :3, :3] *= 1.01
    with pytest.raises(ValueError, match=r"T\[1\]"):
        cca.triangulateMulti(cams, bad, uv)
    with pytest.raises(ValueError, match="camera 2"):
        cca.triangulateMulti(cams[:2] + [("radtan", cams[2][1], cams[2][2][:3])], T, uv)
    with pytest.raises(ValueError, match="camera 0"):
        cca.triangulateMulti([("pinhole",) + tuple(cams[0][1:])] + cams[1:], T, uv)
    with pytest.raises(ValueError, match="A of camera 1"):
        engine.triangulateMulti([(0, cams[0][1], cams[0][2]), (1, np.eye(2), cams[1][2])], T[:2], uv[:2])
