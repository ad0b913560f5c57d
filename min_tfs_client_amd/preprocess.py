"""Declarative server-side input preprocessing for ``Servable``.

A ``Servable`` takes ``preprocess={alias: callable}``; each callable turns
the tensor a client sent for that alias into what the model eats.
``ImagePreprocess`` is the image case: clients ship ``uint8`` NHWC pixels
(1 byte per value on the wire and over H2D instead of 4) and the server
runs the fused dequantize + normalize + NCHW kernel
(``ops.image_u8_to_float``).
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


class ImagePreprocess:
    """uint8 ``[N,H,W,C]`` pixels -> normalized float tensor.

    Accepts a numpy array or a torch tensor, on CPU or device. With
    ``device`` set, the **uint8** tensor is moved there first, so the H2D
    copy is 4x smaller than shipping fp32 and the kernel runs on the GPU.
    Wrong dtype / rank / channel count raise ``ValueError`` (servers answer
    INVALID_ARGUMENT). Semantics: see ``ops.image_u8_to_float``."""

    def __init__(self, mean, std, out_dtype=None, layout: str = "nchw",
                 pixel_scale: float = 1.0 / 255.0, device=None):
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
        return ops.image_u8_to_float(
            x, self.mean, self.std, out_dtype=self.out_dtype,
            layout=self.layout, pixel_scale=self.pixel_scale)
