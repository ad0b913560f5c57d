"""Declarative server-side input preprocessing for ``Servable``.

A ``Servable`` takes ``preprocess={alias: callable}``; each callable turns
the tensor a client sent for that alias into what the model eats.
``ImagePreprocess`` is the image case: clients ship ``uint8`` NHWC pixels
(1 byte per value on the wire and over H2D instead of 4) and the server
runs the fused dequantize + normalize + NCHW kernel
(``ops.image_u8_to_float``), or, with ``resize`` / ``center_crop`` set, the
fused bilinear resize + crop + normalize + NCHW kernel
(``ops.image_u8_resize_to_float``) on images of any size; ``antialias=True``
selects the antialiased resize kernels for downscaled photos.
"""
from __future__ import annotations

import warnings

import numpy as np

try:
    import torch
except ImportError:  # pragma: no cover
    torch = None

from . import ops

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def _positive_int(value, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{what} must be a positive int, got {value!r}")
    if value < 1:
        raise ValueError(f"{what} must be a positive int, got {value!r}")
    return int(value)


def _int_or_pair(value, what):
    """None, an int, or an (H, W) pair of positive ints."""
    if value is None:
        return None
    if isinstance(value, (tuple, list)):
        if len(value) != 2:
            raise ValueError(f"{what} must be an int or (H, W), got {value!r}")
        return (_positive_int(value[0], what), _positive_int(value[1], what))
    return _positive_int(value, what)


class ImagePreprocess:
    """uint8 ``[N,H,W,C]`` pixels -> normalized float tensor.

    Accepts a numpy array or a torch tensor, on CPU or device. With
    ``device`` set, the **uint8** tensor is moved there first, so the H2D
    copy is 4x smaller than shipping fp32 and the kernel runs on the GPU.
    Wrong dtype / rank / channel count raise ``ValueError`` (servers answer
    INVALID_ARGUMENT). Semantics: see ``ops.image_u8_to_float``.

    ``resize`` and ``center_crop`` (both ``None`` by default: the input is
    normalized at its own size) add a bilinear resize and a centre crop in
    the same kernel; semantics: see ``ops.image_u8_resize_to_float``.

    * ``resize=(H, W)`` resizes to exactly that size. ``resize=s`` (an int)
      sets the shorter side to ``s`` and the longer side to
      ``s * long_in // short_in`` (integer arithmetic, aspect ratio kept), so
      the resized size follows each request's input shape.
    * ``center_crop=c`` or ``(Hc, Wc)`` keeps the window that starts at
      ``top = (Hr - Hc) // 2``, ``left = (Wr - Wc) // 2`` of the resized
      ``(Hr, Wr)`` image. A crop larger than the resized image raises
      ``ValueError``. Without ``resize`` the input is cropped at its own
      size.
    * ``antialias=True`` resizes with the antialiased triangle filter (what
      PIL and torchvision ``Resize`` do when they shrink an image) instead of
      the 2-tap bilinear. It needs ``resize`` or ``center_crop``."""

    def __init__(self, mean, std, out_dtype=None, layout: str = "nchw",
                 pixel_scale: float = 1.0 / 255.0, device=None,
                 resize=None, center_crop=None, antialias: bool = False):
        self.mean = tuple(float(m) for m in mean)
        self.std = tuple(float(s) for s in std)
        self.out_dtype = torch.float32 if out_dtype is None else out_dtype
        self.layout = layout
        self.pixel_scale = pixel_scale
        self.device = device
        # fail at construction, not on the first request
        ops.normalization_constants(self.mean, self.std, pixel_scale)
        if layout not in ("nchw", "nhwc"):
            raise ValueError(
                f"layout must be 'nchw' or 'nhwc', got {layout!r}")
        self.resize = _int_or_pair(resize, "resize")
        crop = _int_or_pair(center_crop, "center_crop")
        self.center_crop = (crop, crop) if isinstance(crop, int) else crop
        self.antialias = bool(antialias)
        if self.antialias and self.resize is None and self.center_crop is None:
            raise ValueError(
                "antialias=True needs resize or center_crop: without them "
                "the input is not resized")

    def resized_size(self, height: int, width: int):
        """``(Hr, Wr)`` of the resized image for an input of this size."""
        if self.resize is None:
            return height, width
        if isinstance(self.resize, tuple):
            return self.resize
        s = self.resize
        if height <= width:
            return s, s * width // height
        return s * height // width, s

    def crop_window(self, resized_height: int, resized_width: int):
        """``(top, left, Hc, Wc)`` inside the resized image, or ``None``."""
        if self.center_crop is None:
            return None
        hc, wc = self.center_crop
        if hc > resized_height or wc > resized_width:
            raise ValueError(
                f"center_crop {hc}x{wc} is larger than the resized image "
                f"{resized_height}x{resized_width}")
        return ((resized_height - hc) // 2, (resized_width - wc) // 2,
                hc, wc)

    def __call__(self, x):
        if not isinstance(x, torch.Tensor):
            arr = np.asarray(x)
            if arr.dtype.kind in ("S", "U", "O"):
                raise ValueError(
                    f"image input must be uint8 pixels, got {arr.dtype}")
            with warnings.catch_warnings():
                # decoded request arrays are read-only views of the wire
                # bytes; they are only read here
                warnings.simplefilter("ignore", UserWarning)
                x = torch.from_numpy(arr)
        if self.device is not None and x.dtype == torch.uint8:
            x = x.to(self.device)
        if self.resize is None and self.center_crop is None:
            return ops.image_u8_to_float(
                x, self.mean, self.std, out_dtype=self.out_dtype,
                layout=self.layout, pixel_scale=self.pixel_scale)
        if x.dim() != 4 or x.shape[1] < 1 or x.shape[2] < 1:
            raise ValueError(
                "image input must be [N,H,W,C] with non-empty images, got "
                f"shape {list(x.shape)}")
        size = self.resized_size(int(x.shape[1]), int(x.shape[2]))
        return ops.image_u8_resize_to_float(
            x, size, self.mean, self.std, crop=self.crop_window(*size),
            out_dtype=self.out_dtype, layout=self.layout,
            pixel_scale=self.pixel_scale, antialias=self.antialias)
