"""Applying a calibration to images: remap through a rectify map, undistort one image, or many of one size.

The reference stops at the estimate; this is surface beside it, like uncertainty.py. The maps come from
DistortionModel.undistortMaps (the forward model evaluated per destination pixel, csrc/undistort.hpp), the resampling
is bilinear with a constant border, and both run on the device. Images and maps are host arrays.
"""
import numpy as np

from . import engine
from .distortion import FisheyeModel, RadialTangentialModel

_MODELS = {"radtan": RadialTangentialModel, "fisheye": FisheyeModel}


def _model(model):
    """a DistortionModel instance, or its name"""
    if isinstance(model, str):
        if model not in _MODELS:
            raise ValueError(f"unknown distortion model {model!r} (expected one of {sorted(_MODELS)})")
        return _MODELS[model]()
    return model


def remap(image, mapx, mapy, border=0):
    """image (H, W) or (H, W, C), uint8 or float32, C <= 4; mapx, mapy float32 (h, w) -> (h, w) or (h, w, C).

    out[i, j] is the image sampled bilinearly at column mapx[i, j], row mapy[i, j]. A tap outside the image counts
    as `border`; a NaN or infinite map entry gives `border`. uint8 results are rounded to nearest (ties to even)."""
    image = np.asarray(image)
    if image.ndim == 2:
        return engine.remap(image[:, :, None], mapx, mapy, border)[:, :, 0]
    return engine.remap(image, mapx, mapy, border)


class Undistorter:
    """The maps of one camera and image size, built once: Undistorter(model, A, k, (width, height)).apply(image).

    newA is the camera matrix of the undistorted image (default: A itself). mapx, mapy are float32 (height, width)."""

    def __init__(self, model, A, k, size, newA=None):
        self.model = _model(model)
        self.size = tuple(int(v) for v in size)
        self.mapx, self.mapy = self.model.undistortMaps(A, k, self.size, newA)

    def apply(self, image, border=0):
        return remap(image, self.mapx, self.mapy, border)


def undistortImage(image, model, A, k, newA=None, border=0):
    """The image a pinhole camera newA (default A) would have taken: maps for the image's own size, then remap."""
    image = np.asarray(image)
    if image.ndim not in (2, 3):
        raise ValueError(f"image: expected shape (H, W) or (H, W, C), got {image.shape}")
    return Undistorter(model, A, k, (image.shape[1], image.shape[0]), newA).apply(image, border)
