"""Undistortion, the parts that need no GPU: the C ABI declares and exports the three entry points, the Python
wrappers reject bad shapes before they touch the library, and the bilinear yardstick the GPU tests compare with
(tests/undistort_yardstick.py) reproduces a 2 x 2 image worked out by hand."""
import os
import re

import numpy as np
import pytest

import camera_calibration_amd as cca
from camera_calibration_amd import _native as nat
from camera_calibration_amd import engine, synthetic, undistort
from conftest import ROOT
from undistort_yardstick import bilinear, normalisedToPixels, pixelsToNormalised

NEW_SYMBOLS = ("calib_undistort_points", "calib_undistort_maps", "calib_remap")


def test_header_declares_and_library_exports_the_undistortion_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "calib_lm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(calib_[a-z0-9_]+)\s*\(", text))
    lib = nat.loadLibrary()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/calib_lm.h"
        assert n in nat.SIGNATURES, f"{n} has no ctypes signature"
        assert hasattr(lib, n), f"{n} is not exported by the library"
    assert "CALIB_IMAGE_U8" in text and "CALIB_IMAGE_F32" in text
    assert lib.calib_version() >= 430


def test_python_surface_is_exported():
    for name in ("remap", "undistortImage", "Undistorter", "undistort"):
        assert hasattr(cca, name), name
    for name in ("undistortPoints", "undistortMaps", "remap"):
        assert callable(getattr(engine, name)), name
    for cls in (cca.RadialTangentialModel, cca.FisheyeModel):
        assert callable(cls.undistortPoints) and callable(cls.undistortMaps)


@pytest.fixture
def noNativeCalls(monkeypatch):
    """the wrappers must raise before they reach the library or ask for a device"""
    def refuse(*a, **k):
        raise AssertionError("the wrapper reached the native library")
    monkeypatch.setattr(nat, "loadLibrary", refuse)
    monkeypatch.setattr(nat, "requireDevice", refuse)


def test_wrappers_reject_bad_shapes_before_any_native_call(noNativeCalls):
    A, k = synthetic.RADTAN_A, synthetic.RADTAN_K
    model = cca.RadialTangentialModel()
    f32 = np.zeros((4, 6), dtype=np.float32)
    for bad in (np.zeros((5, 3)), np.zeros(4), np.zeros((2, 2, 2))):            # uv is not (N, 2)
        with pytest.raises(ValueError):
            model.undistortPoints(A, k, bad)
        with pytest.raises(ValueError):
            engine.undistortPoints(nat.MODEL_RADTAN, A, k, bad)
    with pytest.raises(ValueError):                                             # a 5-channel image
        undistort.remap(np.zeros((8, 9, 5), dtype=np.uint8), f32, f32)
    with pytest.raises(ValueError):
        engine.remap(np.zeros((8, 9, 5), dtype=np.float32), f32, f32)
    with pytest.raises(ValueError):                                             # maps whose shapes differ
        undistort.remap(np.zeros((8, 9, 3), dtype=np.uint8), f32, np.zeros((6, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        undistort.remap(np.zeros((8, 9), dtype=np.uint8), f32, f32[:, :5])
    with pytest.raises(ValueError):                                             # what the library could not read
        undistort.remap(np.zeros((8, 9, 3), dtype=np.float64), f32, f32)
    with pytest.raises(ValueError):
        undistort.remap(np.zeros((8, 9, 3), dtype=np.uint8), f32.astype(np.float64), f32.astype(np.float64))
    with pytest.raises(ValueError):
        model.undistortMaps(A, k, (0, 5))
    with pytest.raises(ValueError):
        model.undistortMaps(A, k, 640)
    with pytest.raises(ValueError):
        model.undistortMaps(np.eye(4), k, (6, 5))
    with pytest.raises(ValueError):
        model.undistortPoints(A, k[:4], np.zeros((3, 2)))
    with pytest.raises(ValueError):
        undistort.undistortImage(np.zeros(7, dtype=np.uint8), "radtan", A, k)
    with pytest.raises(ValueError):
        undistort.Undistorter("pinhole", A, k, (6, 5))


def test_bilinear_yardstick_on_a_hand_computed_image():
    img = np.array([[10.0, 20.0], [30.0, 50.0]])
    # (sx, sy) -> value, border 7:
    #   (0.25, 0.5)   top = 10 + .25 * 10 = 12.5, bot = 30 + .25 * 20 = 35, out = 12.5 + .5 * 22.5 = 23.75
    #   (1, 1)        on the last pixel: a = 50, fx = fy = 0 -> 50 whatever the outside taps are
    #   (1.5, 0)      a = 20, b outside = 7: 20 + .5 * (7 - 20) = 13.5 (only the outside TAP is border)
    #   (-0.5, -0.5)  a, b, c outside, d = 10: top = 7, bot = 7 + .5 * 3 = 8.5, out = 7 + .5 * 1.5 = 7.75
    #   (0, 1.25)     a = 30, c outside: 30 + .25 * (7 - 30) = 24.25
    #   (-1, 0), (2, 0), (5, 5)  every tap outside -> 7;  NaN, inf -> 7
    sx = np.array([[0.25, 1.0, 1.5, -0.5, 0.0], [-1.0, 2.0, 5.0, np.nan, np.inf]], dtype=np.float32)
    sy = np.array([[0.5, 1.0, 0.0, -0.5, 1.25], [0.0, 0.0, 5.0, 0.0, 0.0]], dtype=np.float32)
    want = np.array([[23.75, 50.0, 13.5, 7.75, 24.25], [7.0, 7.0, 7.0, 7.0, 7.0]])
    got = bilinear(img, sx, sy, border=7.0)
    assert got.shape == (2, 5, 1)
    assert np.array_equal(got[:, :, 0], want)
    rgb = np.stack((img, 2 * img, img + 1), axis=2)
    got = bilinear(rgb, sx[:1, :1], sy[:1, :1], border=0.0)
    assert np.array_equal(got[0, 0], [23.75, 47.5, 24.75])


def test_pixel_conversions_of_the_yardstick_invert_each_other():
    A = np.array([[400.0, 0.3, 320.0], [0.0, 410.0, 240.0], [0.0, 0.0, 1.0]])
    xy = np.array([[0.0, 0.0], [0.5, -0.25], [-0.8, 0.8]])
    uv = normalisedToPixels(A, xy)
    assert np.array_equal(uv[0], [320.0, 240.0])
    assert np.allclose(uv[1], [400 * 0.5 + 0.3 * -0.25 + 320, 410 * -0.25 + 240], rtol=0, atol=1e-12)
    assert np.abs(pixelsToNormalised(A, uv) - xy).max() < 1e-15


def test_c_abi_rejects_bad_arguments_before_it_needs_a_device():
    import ctypes
    lib = nat.loadLibrary()
    A = np.ascontiguousarray(synthetic.RADTAN_A, dtype=np.float64)
    flat = A.copy()
    flat[1, 1] = 0.0                                                            # beta = 0
    k = np.array(synthetic.RADTAN_K, dtype=np.float64)
    uv, xy = np.zeros((3, 2)), np.zeros((3, 2))
    mx, my = np.zeros((4, 6), dtype=np.float32), np.zeros((4, 6), dtype=np.float32)
    src, dst = np.zeros((5, 7, 3), dtype=np.uint8), np.zeros((4, 6, 3), dtype=np.uint8)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                            # noqa: E731
    pts = lib.calib_undistort_points
    assert pts(nat.MODEL_RADTAN, 0, nat.dptr(A), nat.dptr(k), None, None, None, None, 0) == 0          # n == 0
    assert pts(nat.MODEL_RADTAN, 3, nat.dptr(A), nat.dptr(k), None, None, nat.dptr(xy), None, 0) == nat.E_INVALID
    assert pts(nat.MODEL_RADTAN, 3, None, nat.dptr(k), nat.dptr(uv), None, nat.dptr(xy), None, 0) == nat.E_INVALID
    assert pts(7, 3, nat.dptr(A), nat.dptr(k), nat.dptr(uv), None, nat.dptr(xy), None, 0) == nat.E_INVALID
    assert pts(nat.MODEL_RADTAN, 3, nat.dptr(flat), nat.dptr(k), nat.dptr(uv), None, nat.dptr(xy), None, 0) == nat.E_INVALID
    assert pts(nat.MODEL_RADTAN, 3, nat.dptr(A), nat.dptr(k), nat.dptr(uv), nat.dptr(flat), nat.dptr(xy), None, 0) == nat.E_INVALID
    maps = lib.calib_undistort_maps
    assert maps(nat.MODEL_FISHEYE, nat.dptr(A), nat.dptr(k), None, 6, 0, nat.f32ptr(mx), nat.f32ptr(my), 0) == nat.E_INVALID
    assert maps(nat.MODEL_FISHEYE, nat.dptr(A), nat.dptr(k), None, 6, 4, None, nat.f32ptr(my), 0) == nat.E_INVALID
    assert maps(nat.MODEL_FISHEYE, nat.dptr(flat), nat.dptr(k), None, 6, 4, nat.f32ptr(mx), nat.f32ptr(my), 0) == nat.E_INVALID
    assert maps(nat.MODEL_FISHEYE, nat.dptr(A), nat.dptr(k), nat.dptr(flat), 6, 4, nat.f32ptr(mx), nat.f32ptr(my), 0) == nat.E_INVALID
    assert maps(2, nat.dptr(A), nat.dptr(k), None, 6, 4, nat.f32ptr(mx), nat.f32ptr(my), 0) == nat.E_INVALID
    remap = lib.calib_remap
    assert remap(nat.IMAGE_U8, vp(src), 5, 7, 5, nat.f32ptr(mx), nat.f32ptr(my), 4, 6, 0.0, vp(dst), 0) == nat.E_INVALID
    assert remap(nat.IMAGE_U8, vp(src), 5, 7, 0, nat.f32ptr(mx), nat.f32ptr(my), 4, 6, 0.0, vp(dst), 0) == nat.E_INVALID
    assert remap(2, vp(src), 5, 7, 3, nat.f32ptr(mx), nat.f32ptr(my), 4, 6, 0.0, vp(dst), 0) == nat.E_INVALID
    assert remap(nat.IMAGE_U8, vp(src), 5, 0, 3, nat.f32ptr(mx), nat.f32ptr(my), 4, 6, 0.0, vp(dst), 0) == nat.E_INVALID
    assert remap(nat.IMAGE_U8, vp(src), 5, 7, 3, nat.f32ptr(mx), nat.f32ptr(my), -4, 6, 0.0, vp(dst), 0) == nat.E_INVALID
    assert remap(nat.IMAGE_U8, None, 5, 7, 3, nat.f32ptr(mx), nat.f32ptr(my), 4, 6, 0.0, vp(dst), 0) == nat.E_INVALID
    assert remap(nat.IMAGE_U8, vp(src), 5, 7, 3, nat.f32ptr(mx), None, 4, 6, 0.0, vp(dst), 0) == nat.E_INVALID
    assert nat.lastError()                                                      # a message is left for the caller
