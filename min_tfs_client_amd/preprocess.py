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
``PatchEmbedPreprocess`` is the Vision Transformer case: uint8 pixels go
straight to encoder tokens, normalization, patch projection, class token and
position embedding in one matrix-core kernel (``ops.image_u8_patch_embed``);
``Yuv420PatchEmbedPreprocess`` feeds the same kernel NV12 or I420 frames,
converted while the tile is filled (``ops.image_yuv420_patch_embed``), and
``ResizePatchEmbedPreprocess`` images of any size, resized and centre-cropped
while the tile is filled (``ops.image_u8_resize_patch_embed``);
``RaggedResizePatchEmbedPreprocess`` does that for a packed request of N
images of N sizes in one launch (``ops.image_u8_ragged_resize_patch_embed``).
"""
from __future__ import annotations

import threading
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


def _resized_size(resize, height, width):
    """The ``resize`` rule of :class:`ImagePreprocess`: ``(Hr, Wr)`` for an
    input of ``height x width``."""
    if resize is None:
        return height, width
    if isinstance(resize, tuple):
        return resize
    if height <= width:
        return resize, resize * width // height
    return resize * height // width, resize


def _crop_window(center_crop, resized_height, resized_width):
    """The ``center_crop`` rule of :class:`ImagePreprocess`: ``(top, left,
    Hc, Wc)`` inside the resized image, or ``None``."""
    if center_crop is None:
        return None
    hc, wc = center_crop
    if hc > resized_height or wc > resized_width:
        raise ValueError(
            f"center_crop {hc}x{wc} is larger than the resized image "
            f"{resized_height}x{resized_width}")
    return ((resized_height - hc) // 2, (resized_width - wc) // 2, hc, wc)


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
        return _resized_size(self.resize, height, width)

    def crop_window(self, resized_height: int, resized_width: int):
        """``(top, left, Hc, Wc)`` inside the resized image, or ``None``."""
        return _crop_window(self.center_crop, resized_height, resized_width)

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


def _ragged_windows(resize, center_crop, image_shapes):
    """The per-image rules of the ragged hooks: ``(shapes, sizes, origins)``,
    integer ``[N,2]`` arrays of every image's own size, its resized size and
    the origin of its crop window (``resize`` / ``center_crop`` as
    :class:`ImagePreprocess` keeps them)."""
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
        size = _resized_size(resize, h, w)
        try:
            window = _crop_window(center_crop, *size)
        except ValueError as e:
            raise ValueError(f"image {i} ({h}x{w}): {e}") from None
        sizes[i] = size
        if window is not None:
            origins[i] = window[:2]
    return shapes, sizes, origins


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
        shapes, sizes, origins = _ragged_windows(
            self.resize, self.center_crop, image_shapes)
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


class PatchEmbedPreprocess:
    """uint8 ``[N,H,W,3]`` pixels -> ViT tokens ``[N,T,D]``: normalization,
    patch projection, class token and position embedding in one kernel
    (``ops.image_u8_patch_embed``).

    ``weight`` ``[D,3,P,P]`` and ``bias`` are the patch convolution's
    parameters, ``pos_embed`` (``T*D`` values) and ``cls_token`` (``D``
    values) the model's, any float dtype; ``None`` leaves a term out. The
    hook keeps references to them and folds lazily (``ops.patch_embed_fold``;
    position and class embeddings as fp32): on the first call, and again
    whenever one of them has changed since the last fold. In-place updates
    such as ``load_state_dict`` bump ``tensor._version``, so a servable that
    loads its weights after construction serves the loaded ones.

    Accepts a numpy array or a torch tensor, on CPU or device. With
    ``device`` set, the **uint8** bytes are moved there first and the folded
    operands live there. The projection uses bf16 weights with fp32
    accumulation whatever ``out_dtype`` is. Invalid input raises
    ``ValueError`` (servers answer INVALID_ARGUMENT)."""

    def __init__(self, weight, bias, mean, std, pos_embed=None,
                 cls_token=None, out_dtype=None,
                 pixel_scale: float = 1.0 / 255.0, device=None):
        self.weight, self.bias = weight, bias
        self.pos_embed, self.cls_token = pos_embed, cls_token
        self.mean = tuple(float(m) for m in mean)
        self.std = tuple(float(s) for s in std)
        self.out_dtype = torch.float32 if out_dtype is None else out_dtype
        self.pixel_scale = pixel_scale
        self.device = device
        self.patch = int(weight.shape[-1])
        self._lock = threading.Lock()
        self._key = None
        self._folded = None
        # fail at construction, not on the first request
        ops.normalization_constants(self.mean, self.std, pixel_scale)

    def _sources(self):
        return (self.weight, self.bias, self.pos_embed, self.cls_token)

    def folded(self):
        """``(wk, bias_f, pos, cls)`` for the parameters as they are now."""
        key = tuple(None if t is None else (t._version, t.data_ptr(), t.device)
                    for t in self._sources())
        with self._lock:
            if key != self._key:
                wk, bias_f = ops.patch_embed_fold(
                    self.weight, self.bias, self.mean, self.std,
                    self.pixel_scale)
                dev = self.weight.device if self.device is None \
                    else self.device
                D = wk.shape[0]
                pos = cls = None
                if self.pos_embed is not None:
                    pos = self.pos_embed.detach().float().reshape(
                        -1, D).to(dev).contiguous()
                if self.cls_token is not None:
                    cls = self.cls_token.detach().float().reshape(
                        D).to(dev).contiguous()
                self._folded = (wk.to(dev), bias_f.to(dev), pos, cls)
                self._key = key
            return self._folded

    def __call__(self, x):
        x = _as_tensor(x)
        if self.device is not None and x.dtype == torch.uint8:
            x = x.to(self.device)
        wk, bias_f, pos, cls = self.folded()
        return ops.image_u8_patch_embed(
            x, wk, bias_f, self.patch, pos_embed=pos, cls_token=cls,
            out_dtype=self.out_dtype)


class Yuv420PatchEmbedPreprocess(PatchEmbedPreprocess):
    """uint8 ``[N,H*3/2,W]`` YUV 4:2:0 frames -> ViT tokens ``[N,T,D]``:
    the conversion to RGB happens inside the patch-embedding kernel
    (``ops.image_yuv420_patch_embed``), from half the request bytes.

    ``chroma`` (``"nv12"`` or ``"i420"``) and ``matrix`` are those of
    ``ops.yuv420_to_rgb_u8``; everything else, the lazy refold included, is
    :class:`PatchEmbedPreprocess`, and the tokens are exactly what that class
    gives for the converted RGB frames, bit for bit. The patch is 16 or 32."""

    def __init__(self, weight, bias, mean, std, pos_embed=None,
                 cls_token=None, out_dtype=None,
                 pixel_scale: float = 1.0 / 255.0, device=None,
                 chroma: str = "nv12", matrix: str = "bt601"):
        super().__init__(weight, bias, mean, std, pos_embed=pos_embed,
                         cls_token=cls_token, out_dtype=out_dtype,
                         pixel_scale=pixel_scale, device=device)
        if self.patch not in ops.YUV420_PATCH_EMBED_PATCHES:
            raise ValueError(
                f"patch must be one of {ops.YUV420_PATCH_EMBED_PATCHES} for "
                f"YUV 4:2:0 input, got {self.patch}")
        if chroma not in ops.YUV_CHROMA_LAYOUTS:
            raise ValueError(
                f"chroma must be 'nv12' or 'i420', got {chroma!r}")
        if matrix not in ops.YUV_MATRICES:
            raise ValueError(
                f"matrix must be one of {sorted(ops.YUV_MATRICES)}, got "
                f"{matrix!r}")
        self.chroma, self.matrix = chroma, matrix

    def __call__(self, x):
        x = _as_tensor(x)
        if self.device is not None and x.dtype == torch.uint8:
            x = x.to(self.device)
        wk, bias_f, pos, cls = self.folded()
        return ops.image_yuv420_patch_embed(
            x, wk, bias_f, self.patch, pos_embed=pos, cls_token=cls,
            out_dtype=self.out_dtype, chroma=self.chroma, matrix=self.matrix)


class ResizePatchEmbedPreprocess(PatchEmbedPreprocess):
    """uint8 ``[N,H,W,3]`` pixels of any size -> ViT tokens ``[N,T,D]``: the
    bilinear resize and the centre crop happen inside the patch-embedding
    kernel (``ops.image_u8_resize_patch_embed``), which resamples while it
    fills its tile.

    ``resize`` and ``center_crop`` follow the rules of
    :class:`ImagePreprocess` (an int ``resize`` sets the shorter side and
    keeps the aspect ratio); at least one is needed, and the window they give
    must be a multiple of the patch, which is 16 or 32. Every image of one
    request has the same size; requests may differ. Everything else, the lazy
    refold included, is :class:`PatchEmbedPreprocess`. The resized pixel is
    an fp32 blend and reaches the matrix cores as two bf16 pieces, within
    ``2**-16`` of its value."""

    def __init__(self, weight, bias, mean, std, pos_embed=None,
                 cls_token=None, out_dtype=None,
                 pixel_scale: float = 1.0 / 255.0, device=None,
                 resize=None, center_crop=None):
        super().__init__(weight, bias, mean, std, pos_embed=pos_embed,
                         cls_token=cls_token, out_dtype=out_dtype,
                         pixel_scale=pixel_scale, device=device)
        if self.patch not in ops.RESIZE_PATCH_EMBED_PATCHES:
            raise ValueError(
                f"patch must be one of {ops.RESIZE_PATCH_EMBED_PATCHES} for "
                f"resized input, got {self.patch}")
        self.resize = _int_or_pair(resize, "resize")
        crop = _int_or_pair(center_crop, "center_crop")
        self.center_crop = (crop, crop) if isinstance(crop, int) else crop
        if self.resize is None and self.center_crop is None:
            raise ValueError(
                "ResizePatchEmbedPreprocess needs resize or center_crop; "
                "PatchEmbedPreprocess serves images at their own size")

    def resized_size(self, height: int, width: int):
        """``(Hr, Wr)`` of the resized image for an input of this size."""
        return _resized_size(self.resize, height, width)

    def crop_window(self, resized_height: int, resized_width: int):
        """``(top, left, Hc, Wc)`` inside the resized image, or ``None``."""
        return _crop_window(self.center_crop, resized_height, resized_width)

    def __call__(self, x):
        x = _as_tensor(x)
        if self.device is not None and x.dtype == torch.uint8:
            x = x.to(self.device)
        if x.dim() != 4 or x.shape[1] < 1 or x.shape[2] < 1:
            raise ValueError(
                "image input must be [N,H,W,3] with non-empty images, got "
                f"shape {list(x.shape)}")
        size = self.resized_size(int(x.shape[1]), int(x.shape[2]))
        wk, bias_f, pos, cls = self.folded()
        return ops.image_u8_resize_patch_embed(
            x, size, wk, bias_f, self.patch, crop=self.crop_window(*size),
            pos_embed=pos, cls_token=cls, out_dtype=self.out_dtype)


class RaggedResizePatchEmbedPreprocess(PatchEmbedPreprocess):
    """N uint8 RGB images of N different sizes -> ViT tokens ``[N,T,D]``, in
    one launch of the patch-embedding kernel
    (``ops.image_u8_ragged_resize_patch_embed``), whose resampling loader
    takes the source geometry per tile row.

    Called as ``pre(images, image_shapes)``, the packed buffer and the
    ``[N,2]`` rows ``(H_i, W_i)`` of :class:`RaggedImagePreprocess`
    (:func:`pack_ragged_images`); ``image_shapes`` is read on the host.
    ``resize`` and ``center_crop`` follow that class's per-image rules and
    must give one output size for all images, a multiple of the patch, which
    is 16 or 32. Every image gets exactly the tokens that
    :class:`ResizePatchEmbedPreprocess` gives it alone, bit for bit.
    Everything else, the lazy refold included, is
    :class:`PatchEmbedPreprocess`."""

    def __init__(self, weight, bias, mean, std, pos_embed=None,
                 cls_token=None, out_dtype=None,
                 pixel_scale: float = 1.0 / 255.0, device=None,
                 resize=None, center_crop=None):
        super().__init__(weight, bias, mean, std, pos_embed=pos_embed,
                         cls_token=cls_token, out_dtype=out_dtype,
                         pixel_scale=pixel_scale, device=device)
        if self.patch not in ops.RESIZE_PATCH_EMBED_PATCHES:
            raise ValueError(
                f"patch must be one of {ops.RESIZE_PATCH_EMBED_PATCHES} for "
                f"resized input, got {self.patch}")
        self.resize = _int_or_pair(resize, "resize")
        crop = _int_or_pair(center_crop, "center_crop")
        self.center_crop = (crop, crop) if isinstance(crop, int) else crop
        if self.center_crop is not None:
            self.out_size = self.center_crop
        elif isinstance(self.resize, tuple):
            self.out_size = self.resize
        else:
            raise ValueError(
                "RaggedResizePatchEmbedPreprocess needs one output size for "
                "all images: resize=(H, W), or center_crop with resize=int "
                f"or alone; got resize={resize!r}, "
                f"center_crop={center_crop!r}")

    def __call__(self, images, image_shapes):
        x = _as_tensor(images)
        if self.device is not None and x.dtype == torch.uint8:
            x = x.to(self.device)
        shapes, sizes, origins = _ragged_windows(
            self.resize, self.center_crop, image_shapes)
        wk, bias_f, pos, cls = self.folded()
        return ops.image_u8_ragged_resize_patch_embed(
            x, shapes, sizes, self.out_size, wk, bias_f, self.patch,
            origins=origins, pos_embed=pos, cls_token=cls,
            out_dtype=self.out_dtype)


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


def pack_ragged_tokens(sequences):
    """Client side of the ragged token layout (``bert_servable``'s
    ``"ids_ragged"``): a list of id lists -> ``(input_ids,
    sequence_lengths)``, the int32 ``[total]`` ids back to back and the int32
    ``[B]`` lengths. Every sequence has at least one id. Numpy only."""
    arrays = []
    for i, seq in enumerate(sequences):
        arr = np.asarray(seq)
        if arr.ndim != 1 or arr.size == 0 or arr.dtype.kind not in "iu":
            raise ValueError(
                f"sequence {i} must be a non-empty 1-D list of integer ids, "
                f"got dtype {arr.dtype} shape {list(arr.shape)}")
        arrays.append(arr.astype(np.int32))
    lengths = np.array([a.size for a in arrays], dtype=np.int32)
    if not arrays:
        return np.zeros((0,), dtype=np.int32), lengths
    return np.concatenate(arrays), lengths
