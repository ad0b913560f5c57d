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
``Yuv420ImagePreprocess`` takes what decoders emit, NV12 or I420 frames at
1.5 bytes per pixel, and converts them to RGB inside the same bilinear
resize kernel (``ops.image_yuv420_resize_to_float``); with ``antialias=True``
the conversion happens inside the horizontal pass of the antialiased resize
instead, so downscaled decoder frames get the PIL / torchvision filter
without an RGB copy.
``RaggedImagePreprocess`` is the mixed-size case: one request carries N
images of N different sizes packed back to back (``pack_ragged_images``) and
one kernel launch (``ops.image_u8_ragged_resize_to_float``) turns them into
one batch; ``AntialiasedRaggedImagePreprocess`` does the same with the
antialiased filter, in two launches.
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


def _as_tensor(x):
    if isinstance(x, torch.Tensor):
        return x
    arr = np.asarray(x)
    if arr.dtype.kind in ("S", "U", "O"):
        raise ValueError(
            f"image input must be uint8 pixels, got {arr.dtype}")
    with warnings.catch_warnings():
        # decoded request arrays are read-only views of the wire bytes;
        # they are only read here
        warnings.simplefilter("ignore", UserWarning)
        return torch.from_numpy(arr)


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
        x = _as_tensor(x)
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


class Yuv420ImagePreprocess:
    """uint8 ``[N,H*3/2,W]`` YUV 4:2:0 frames -> normalized float tensor.

    Clients ship what a video or JPEG decoder emits, NV12
    (``chroma="nv12"``) or I420 (``chroma="i420"``) frames, 1.5 bytes per
    pixel instead of RGB's 3, and the server converts, resizes, crops and
    normalizes in one kernel (``ops.image_yuv420_resize_to_float``; frame
    layout and ``matrix``: ``ops.yuv420_to_rgb_u8``). The result is exactly
    what :class:`ImagePreprocess` with the same arguments gives for the
    converted RGB frames, bit for bit, ``antialias=True`` included (two
    kernels then: the horizontal pass converts, the vertical pass is the RGB
    one).

    Accepts a numpy array or a torch tensor, on CPU or device. With
    ``device`` set, the **uint8** bytes are moved there first. ``resize``,
    ``center_crop`` and ``antialias`` follow the rules of
    :class:`ImagePreprocess`, applied to the frame's ``(H, W)``;
    ``antialias=True`` needs ``resize`` or ``center_crop``. Wrong dtype, rank
    or frame geometry raise ``ValueError`` (servers answer
    INVALID_ARGUMENT)."""

    def __init__(self, mean, std, out_dtype=None, layout: str = "nchw",
                 pixel_scale: float = 1.0 / 255.0, device=None,
                 resize=None, center_crop=None, chroma: str = "nv12",
                 matrix: str = "bt601", antialias: bool = False):
        self._rule = ImagePreprocess(
            mean, std, out_dtype=out_dtype, layout=layout,
            pixel_scale=pixel_scale, device=device, resize=resize,
            center_crop=center_crop, antialias=antialias)
        rule = self._rule
        self.mean, self.std = rule.mean, rule.std
        self.out_dtype, self.layout = rule.out_dtype, rule.layout
        self.pixel_scale, self.device = rule.pixel_scale, rule.device
        self.resize, self.center_crop = rule.resize, rule.center_crop
        self.antialias = rule.antialias
        if len(self.mean) != 3 or len(self.std) != 3:
            raise ValueError(
                "mean/std need 3 entries (R, G, B), got "
                f"{len(self.mean)}/{len(self.std)}")
        if chroma not in ops.YUV_CHROMA_LAYOUTS:
            raise ValueError(
                f"chroma must be 'nv12' or 'i420', got {chroma!r}")
        if matrix not in ops.YUV_MATRICES:
            raise ValueError(
                f"matrix must be one of {sorted(ops.YUV_MATRICES)}, got "
                f"{matrix!r}")
        self.chroma, self.matrix = chroma, matrix

    def resized_size(self, height: int, width: int):
        """``(Hr, Wr)`` of the resized image for a frame of this size."""
        return self._rule.resized_size(height, width)

    def crop_window(self, resized_height: int, resized_width: int):
        """``(top, left, Hc, Wc)`` inside the resized image, or ``None``."""
        return self._rule.crop_window(resized_height, resized_width)

    def __call__(self, x):
        x = _as_tensor(x)
        if self.device is not None and x.dtype == torch.uint8:
            x = x.to(self.device)
        if x.dim() != 3 or x.shape[1] < 3 or x.shape[1] % 3 != 0 or \
                x.shape[2] < 2:
            raise ValueError(
                "YUV 4:2:0 input must be [N,H*3/2,W] with non-empty frames, "
                f"got shape {list(x.shape)}")
        size = self.resized_size(int(x.shape[1]) // 3 * 2, int(x.shape[2]))
        return ops.image_yuv420_resize_to_float(
            x, size, self.mean, self.std, crop=self.crop_window(*size),
            out_dtype=self.out_dtype, layout=self.layout,
            pixel_scale=self.pixel_scale, chroma=self.chroma,
            matrix=self.matrix, antialias=self.antialias)


class RaggedImagePreprocess:
    """N uint8 images of N different sizes -> one normalized float batch.

    Called as ``pre(images, image_shapes)``: ``images`` is the flat uint8
    ``[total_bytes]`` buffer of the images in HWC order, back to back with no
    padding, and ``image_shapes`` the integer ``[N,2]`` rows ``(H_i, W_i)``
    (see :func:`pack_ragged_images`). Numpy arrays or torch tensors, on CPU or
    device; with ``device`` set the **uint8** data is moved there first and
    one kernel launch resizes, crops and normalizes every image
    (``ops.image_u8_ragged_resize_to_float``). ``image_shapes`` is read on
    the host.

    Every image goes through the rules of :class:`ImagePreprocess` for its
    own size (``resize=s`` sets its shorter side to ``s``; ``center_crop``
    starts at ``((Hr-Hc)//2, (Wr-Wc)//2)`` of its resized size), and all
    images must end at one output size, known at construction:

    * ``resize=(H, W)``, with or without ``center_crop``;
    * ``resize=s`` (an int) with ``center_crop``;
    * ``center_crop`` alone (each image is cropped at its own size).

    Anything else raises ``ValueError`` at construction; a crop larger than
    some image's resized size raises ``ValueError`` at call time and names
    the image. This class resizes with the 2-tap bilinear filter
    (``pre.antialias`` is ``False``) and ``antialias=True`` raises
    ``ValueError``: the antialiased filter is
    :class:`AntialiasedRaggedImagePreprocess`."""

    antialias = False

    def __init__(self, mean, std, out_dtype=None, layout: str = "nchw",
                 pixel_scale: float = 1.0 / 255.0, device=None,
                 resize=None, center_crop=None, antialias: bool = False):
        if antialias:
            raise ValueError(
                "RaggedImagePreprocess is bilinear and takes no "
                "antialias=True: use AntialiasedRaggedImagePreprocess")
        self._rule = ImagePreprocess(
            mean, std, out_dtype=out_dtype, layout=layout,
            pixel_scale=pixel_scale, device=device, resize=resize,
            center_crop=center_crop)
        rule = self._rule
        self.mean, self.std = rule.mean, rule.std
        self.out_dtype, self.layout = rule.out_dtype, rule.layout
        self.pixel_scale, self.device = rule.pixel_scale, rule.device
        self.resize, self.center_crop = rule.resize, rule.center_crop
        if self.center_crop is not None:
            self.out_size = self.center_crop
        elif isinstance(self.resize, tuple):
            self.out_size = self.resize
        else:
            raise ValueError(
                "RaggedImagePreprocess needs one output size for all images: "
                "resize=(H, W), or center_crop with resize=int or alone; "
                f"got resize={resize!r}, center_crop={center_crop!r}")

    def __call__(self, images, image_shapes):
        x = _as_tensor(images)
        if self.device is not None and x.dtype == torch.uint8:
            x = x.to(self.device)
        shapes = image_shapes
        if isinstance(shapes, torch.Tensor):
            shapes = shapes.cpu().numpy()  # device tensor: synchronizing D2H
        shapes = np.asarray(shapes)
        if shapes.dtype.kind not in "iu" or shapes.ndim != 2 or \
                shapes.shape[1] != 2:
            raise ValueError(
                "image_shapes must be integer [N,2] rows of (H, W), got "
                f"dtype {shapes.dtype} shape {list(shapes.shape)}")
        n = shapes.shape[0]
        sizes = np.zeros((n, 2), dtype=np.int64)
        origins = np.zeros((n, 2), dtype=np.int64)
        for i in range(n):
            h, w = int(shapes[i, 0]), int(shapes[i, 1])
            if h < 1 or w < 1:
                raise ValueError(
                    f"image {i}: sides must be positive, got {h}x{w}")
            size = self._rule.resized_size(h, w)
            try:
                window = self._rule.crop_window(*size)
            except ValueError as e:
                raise ValueError(f"image {i} ({h}x{w}): {e}") from None
            sizes[i] = size
            if window is not None:
                origins[i] = window[:2]
        return ops.image_u8_ragged_resize_to_float(
            x, shapes, sizes, self.out_size, self.mean, self.std,
            origins=origins, out_dtype=self.out_dtype, layout=self.layout,
            pixel_scale=self.pixel_scale, antialias=self.antialias)


class AntialiasedRaggedImagePreprocess(RaggedImagePreprocess):
    """:class:`RaggedImagePreprocess` with the antialiased triangle filter
    (``ImagePreprocess(..., antialias=True)`` per image; what PIL and
    torchvision ``Resize`` do when they shrink a photo): the same call, the
    same construction rules without the ``antialias`` parameter, and two
    kernel launches for the batch. ``pre.antialias`` is ``True``."""

    antialias = True

    def __init__(self, mean, std, out_dtype=None, layout: str = "nchw",
                 pixel_scale: float = 1.0 / 255.0, device=None,
                 resize=None, center_crop=None):
        super().__init__(mean, std, out_dtype=out_dtype, layout=layout,
                         pixel_scale=pixel_scale, device=device,
                         resize=resize, center_crop=center_crop)


def pack_ragged_images(images):
    """Client side of the ragged layout: a list of ``[H_i,W_i,C]`` uint8
    arrays -> ``(data, shapes)``, the flat uint8 ``[total_bytes]`` buffer of
    the images back to back and the int32 ``[N,2]`` rows ``(H_i, W_i)``.
    All images must share ``C``. Numpy only."""
    arrays = []
    channels = None
    for i, img in enumerate(images):
        arr = np.asarray(img)
        if arr.dtype != np.uint8 or arr.ndim != 3:
            raise ValueError(
                f"image {i} must be a uint8 [H,W,C] array, got dtype "
                f"{arr.dtype} shape {list(arr.shape)}")
        if channels is None:
            channels = arr.shape[2]
        elif arr.shape[2] != channels:
            raise ValueError(
                f"image {i} has {arr.shape[2]} channels but image 0 has "
                f"{channels}: all images of one request share C")
        arrays.append(arr)
    shapes = np.array([a.shape[:2] for a in arrays],
                      dtype=np.int32).reshape(len(arrays), 2)
    if not arrays:
        return np.zeros((0,), dtype=np.uint8), shapes
    return np.concatenate([a.reshape(-1) for a in arrays]), shapes
