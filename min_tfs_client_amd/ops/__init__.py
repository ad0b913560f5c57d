"""Native ops: C++ wire codec + CDNA4 HIP pack kernels.

Loads the in-tree ``_native`` extension (built by ``setup.py build_ext
--inplace`` / ``__graft_entry__.build()``). On a GPU machine the extension
is REQUIRED — device-tensor paths raise rather than silently falling back
to eager PyTorch, so a passing GPU test means the HIP path actually ran.
"""
from __future__ import annotations

import functools
import math
import operator
from typing import Optional

try:
    import torch
except ImportError:  # pragma: no cover
    torch = None

_native = None
_import_error: Optional[BaseException] = None
try:
    from min_tfs_client_amd import _native  # type: ignore
except Exception as e:  # pragma: no cover - exercised on unbuilt trees
    _import_error = e


def native_available() -> bool:
    return _native is not None


def require_native():
    """The GPU path must run the HIP extension; fail loudly otherwise."""
    if _native is None:
        raise RuntimeError(
            "min_tfs_client_amd._native extension is not built "
            "(run `python setup.py build_ext --inplace`); the HIP pack path "
            f"is mandatory on GPU machines. Import error: {_import_error}")
    return _native


def get_native():
    """Native module or None (CPU-only paths may fall back to the python
    codec)."""
    return _native


# ---------------------------------------------------------------------------
# public op wrappers
# ---------------------------------------------------------------------------

def cast(tensor, out_dtype):
    """Vectorized dtype cast on device (bf16/f16/f32 matrix)."""
    return require_native().cast(tensor, out_dtype)


def nchw_to_nhwc(tensor, out_dtype=None):
    """Fused NCHW->NHWC + cast in one CDNA4 kernel (BASELINE config 5)."""
    if out_dtype is None:
        out_dtype = tensor.dtype
    return require_native().nchw_to_nhwc(tensor, out_dtype)


def nhwc_to_nchw(tensor, out_dtype=None):
    """Inverse fused layout transform (unpack direction)."""
    if out_dtype is None:
        out_dtype = tensor.dtype
    return require_native().nhwc_to_nchw(tensor, out_dtype)


def quantize_q8(tensor, scale, zero_point=0.0):
    return require_native().quantize_q8(tensor, scale, zero_point)


def dequantize_q8(tensor, scale, zero_point=0.0):
    return require_native().dequantize_q8(tensor, scale, zero_point)


def normalization_constants(mean, std, pixel_scale=1.0 / 255.0):
    """Per-channel ``(scale, bias)`` lists for :func:`image_u8_to_float`.

    ``scale_c = float32(pixel_scale / std_c)`` and ``bias_c =
    float32(-mean_c / std_c)``: computed in Python double, then rounded once
    to fp32 (the returned floats are exactly those fp32 values)."""
    scale, bias = _normalization_constants(
        tuple(float(m) for m in mean), tuple(float(s) for s in std),
        float(pixel_scale))
    return list(scale), list(bias)


@functools.lru_cache(maxsize=64)
def _normalization_constants(mean, std, pixel_scale):
    # cached: a serving process applies the same few constants to every
    # request, and the kernel itself runs in microseconds
    import numpy as np

    if len(mean) != len(std):
        raise ValueError(
            f"mean has {len(mean)} entries but std has {len(std)}")
    if any(s == 0.0 for s in std):
        raise ValueError("std must be non-zero for every channel")
    scale = tuple(float(np.float32(pixel_scale / s)) for s in std)
    bias = tuple(float(np.float32(-m / s)) for m, s in zip(mean, std))
    return scale, bias


def image_u8_to_float(tensor, mean, std, out_dtype=None, layout="nchw",
                      pixel_scale=1.0 / 255.0):
    """Fused uint8 image ingest: dequantize + per-channel normalize (+ NHWC
    -> NCHW) of a contiguous ``[N,H,W,C]`` uint8 tensor, ``C`` in 1..4.

        y[n,c,h,w] = out_dtype(float(x[n,h,w,c]) * scale_c + bias_c)

    with ``(scale, bias) = normalization_constants(mean, std, pixel_scale)``,
    an unfused fp32 multiply then add, and unsigned bytes (200 is 200.0).
    The result is bit-identical to the eager expression
    ``(x.permute(0,3,1,2).float() * scale.view(1,C,1,1) +
    bias.view(1,C,1,1)).to(out_dtype)``; it can differ from
    ``(x/255 - mean)/std`` by a few ulp, because the constants are folded
    before the pixel is touched.

    Device tensors run the gfx950 kernel (one pass, no eager fallback);
    CPU tensors use the eager expression, so CPU-only servers work too.
    ``layout`` selects the output layout, ``"nchw"`` or ``"nhwc"``. Invalid
    arguments raise ``ValueError`` on both paths."""
    if out_dtype is None:
        out_dtype = torch.float32
    if layout not in ("nchw", "nhwc"):
        raise ValueError(f"layout must be 'nchw' or 'nhwc', got {layout!r}")
    if out_dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(
            f"out_dtype must be float32, bfloat16 or float16, got {out_dtype}")
    if not isinstance(tensor, torch.Tensor):
        raise ValueError("image_u8_to_float expects a torch tensor")
    if tensor.dtype != torch.uint8:
        raise ValueError(
            f"image_u8_to_float expects uint8 pixels, got {tensor.dtype}")
    if tensor.dim() != 4:
        raise ValueError(
            f"image_u8_to_float expects [N,H,W,C], got rank {tensor.dim()}")
    if not tensor.is_contiguous():
        raise ValueError("image_u8_to_float expects a contiguous tensor")
    C = int(tensor.shape[3])
    if not 1 <= C <= 4:
        raise ValueError(f"image_u8_to_float supports 1..4 channels, got {C}")
    if len(mean) != C or len(std) != C:
        raise ValueError(
            f"mean/std need {C} entries (one per channel), got "
            f"{len(mean)}/{len(std)}")
    scale, bias = normalization_constants(mean, std, pixel_scale)
    if tensor.is_cuda:
        return require_native().u8_nhwc_normalize(
            tensor, scale, bias, out_dtype, layout == "nchw")
    s = torch.tensor(scale, dtype=torch.float32)
    b = torch.tensor(bias, dtype=torch.float32)
    if layout == "nchw":
        x = tensor.permute(0, 3, 1, 2).float()
        y = x * s.view(1, C, 1, 1) + b.view(1, C, 1, 1)
    else:
        y = tensor.float() * s.view(1, 1, 1, C) + b.view(1, 1, 1, C)
    return y.to(out_dtype).contiguous()


RESIZE_MAX_SIDE = 16384


def _resize_taps(n_out, offset, ratio, n_in):
    """Source indices and weights of ``n_out`` output coordinates starting
    at ``offset`` of the resized axis: fp32 tensor ops, one rounding each."""
    o = torch.arange(offset, offset + n_out, dtype=torch.float32)
    s = (((o + 0.5) * ratio) - 0.5).clamp(min=0.0)
    i0 = s.floor().to(torch.int64).clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    return i0, i1, s - i0.float()


def _resize_aa_taps(n_out, offset, ratio, n_in):
    """Antialiased taps of ``n_out`` output coordinates starting at
    ``offset`` of the resized axis: ``(lo, size, idx, w)`` with ``idx`` and
    ``w`` of shape ``[n_out, K]``, ``K`` the longest tap count. Taps past a
    coordinate's own ``size`` have weight 0 and its last index. fp32 tensor
    ops, one rounding each."""
    import numpy as np

    support = ratio if ratio >= 1.0 else 1.0
    inv = float(np.float32(1.0 / ratio)) if ratio >= 1.0 else 1.0
    o = torch.arange(offset, offset + n_out, dtype=torch.float32)
    c = (o + 0.5) * ratio
    # .to(int64) truncates toward zero
    lo = ((c - support) + 0.5).to(torch.int64).clamp(0, n_in - 1)
    hi = ((c + support) + 0.5).to(torch.int64).clamp(max=n_in)
    size = (hi - lo).clamp(min=1)
    j = torch.arange(int(size.max()), dtype=torch.int64).view(1, -1)
    idx = lo.view(-1, 1) + j
    x = ((idx.float() - c.view(-1, 1)) + 0.5) * inv
    w = (1.0 - x.abs()).clamp(min=0.0)
    w = torch.where(j < size.view(-1, 1), w, torch.zeros_like(w))
    idx = torch.minimum(idx, (lo + size - 1).view(-1, 1))
    return lo, size, idx, w


def _resize_aa_eager(p, rh, rw, top, left, Hc, Wc):
    """The antialiased recipe on a CPU fp32 ``[N,Hin,Win,C]`` tensor: fp32
    ``[N,Hc,Wc,C]`` before normalization. Taps are added one at a time in
    ascending order; a padded tap adds ``0 * p``, which is exact."""
    _, Hin, Win, _ = p.shape
    ylo, ysize, yidx, wy = _resize_aa_taps(Hc, top, rh, Hin)
    _, _, xidx, wx = _resize_aa_taps(Wc, left, rw, Win)
    y_base = int(ylo[0])
    p = p[:, y_base:int(ylo[-1] + ysize[-1])]      # the rows the crop needs
    acc = torch.zeros((p.shape[0], p.shape[1], Wc, p.shape[3]),
                      dtype=torch.float32)
    tot = torch.zeros(Wc, dtype=torch.float32)
    for k in range(wx.shape[1]):
        wk = wx[:, k]
        acc = acc + wk.view(1, 1, Wc, 1) * p[:, :, xidx[:, k]]
        tot = tot + wk
    h = acc / tot.view(1, 1, Wc, 1)
    acc = torch.zeros((p.shape[0], Hc, Wc, p.shape[3]), dtype=torch.float32)
    tot = torch.zeros(Hc, dtype=torch.float32)
    for k in range(wy.shape[1]):
        wk = wy[:, k]
        acc = acc + wk.view(1, Hc, 1, 1) * h[:, yidx[:, k] - y_base]
        tot = tot + wk
    return acc / tot.view(1, Hc, 1, 1)


def _resize_window(name, Hin, Win, size, crop):
    """The ``size`` / ``crop`` checks of the ops that resize ``Hin x Win``
    images: ``(Hr, Wr, top, left, Hc, Wc, rh, rw)``, the ratios rounded once
    to fp32."""
    import numpy as np

    try:
        Hr, Wr = (int(d) for d in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (H, W), got {size!r}") from None
    for label, v in (("input height", Hin), ("input width", Win),
                     ("resized height", Hr), ("resized width", Wr)):
        if not 1 <= v <= RESIZE_MAX_SIDE:
            raise ValueError(
                f"{name}: {label} must be in 1..{RESIZE_MAX_SIDE}, got {v}")
    if crop is None:
        top, left, Hc, Wc = 0, 0, Hr, Wr
    else:
        try:
            top, left, Hc, Wc = (int(d) for d in crop)
        except (TypeError, ValueError):
            raise ValueError(
                f"crop must be (top, left, height, width), got {crop!r}"
            ) from None
        if Hc < 1 or Wc < 1:
            raise ValueError(f"crop extent must be positive, got {Hc}x{Wc}")
        if top < 0 or left < 0 or top + Hc > Hr or left + Wc > Wr:
            raise ValueError(
                f"crop window (top={top}, left={left}, {Hc}x{Wc}) is not "
                f"inside the resized image {Hr}x{Wr}")
    return (Hr, Wr, top, left, Hc, Wc, float(np.float32(Hin / Hr)),
            float(np.float32(Win / Wr)))


def image_u8_resize_to_float(tensor, size, mean, std, crop=None,
                             out_dtype=None, layout="nchw",
                             pixel_scale=1.0 / 255.0, _variant=0, *,
                             antialias=False, _ws_cap_bytes=None):
    """Fused uint8 image ingest with bilinear resize and crop: a contiguous
    ``[N,Hin,Win,C]`` uint8 tensor, ``C`` in 1..4, is resized to a virtual
    ``size=(Hr,Wr)`` image, the window ``crop=(top,left,Hc,Wc)`` of that image
    (``None``: all of it) is normalized as in :func:`image_u8_to_float` and
    returned as ``[N,C,Hc,Wc]`` (``layout="nhwc"``: ``[N,Hc,Wc,C]``).

    Half-pixel-centre bilinear without antialiasing, the family of
    ``F.interpolate(mode="bilinear", align_corners=False, antialias=False)``,
    pinned to these fp32 operations (each rounded once, none fused)::

        rw = float32(Win / Wr)    rh = float32(Hin / Hr)
        sx = max(((float(ox + left) + 0.5) * rw) - 0.5, 0)
        x0 = min(int(floor(sx)), Win-1)   x1 = min(x0+1, Win-1)
        wx = sx - float(x0)                  # rows likewise: top, rh, Hin
        t  = p[y0,x0] + wx * (p[y0,x1] - p[y0,x0])
        b  = p[y1,x0] + wx * (p[y1,x1] - p[y1,x0])
        v  = t + wy * (b - t)
        y  = out_dtype((v * scale_c) + bias_c)

    With ``size == (Hin,Win)`` the weights are exactly 0 and the result is
    bit-identical to :func:`image_u8_to_float`; a cropped call equals the
    same window sliced out of the uncropped call, bit for bit. Against
    ``F.interpolate`` the result differs by rounding only.

    ``antialias=True`` (keyword only) switches to the antialiased member of
    the family, ``F.interpolate(..., antialias=True)``, what PIL and
    torchvision ``Resize`` do: a separable triangle filter whose width
    follows the downscale ratio, horizontal pass then vertical pass. For one
    axis (``o`` the output index plus the crop offset, ``r`` the ``rw`` /
    ``rh`` above), again one fp32 rounding per operation::

        support = r if r >= 1 else 1
        inv  = float32(1.0 / r) if r >= 1 else 1
        c    = (float(o) + 0.5) * r
        lo   = clamp(int((c - support) + 0.5), 0, n_in - 1)   # truncating
        hi   = min(int((c + support) + 0.5), n_in)
        size = max(hi - lo, 1)
        for j in 0 .. size-1:                   # ascending, acc = tot = 0
            x   = ((float(lo + j) - c) + 0.5) * inv
            w   = max(1 - |x|, 0)
            acc = acc + w * p[lo + j]
            tot = tot + w
        value = acc / tot

    The horizontal pass reads the uint8 pixels, the vertical pass its fp32
    results; then ``y = out_dtype((value * scale_c) + bias_c)``. The identity
    and crop properties above hold here too. This follows ATen's index rule
    with one division by ``tot`` instead of normalized weights, so it differs
    from ``F.interpolate`` by rounding only. An upscaled axis (``r < 1``)
    keeps support 1, which is plain bilinear.

    Device tensors run the gfx950 kernels (one pass, or two for
    ``antialias=True``; no eager fallback); CPU
    tensors use an eager expression of exactly these operations, so both are
    bit-identical and CPU-only servers work too. All sides (``Hin``, ``Win``,
    ``Hr``, ``Wr``) must be in 1..16384. Invalid arguments raise
    ``ValueError`` on both paths; ``N == 0`` returns an empty tensor."""
    name = "image_u8_resize_to_float"
    if out_dtype is None:
        out_dtype = torch.float32
    if layout not in ("nchw", "nhwc"):
        raise ValueError(f"layout must be 'nchw' or 'nhwc', got {layout!r}")
    if out_dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(
            f"out_dtype must be float32, bfloat16 or float16, got {out_dtype}")
    if not isinstance(tensor, torch.Tensor):
        raise ValueError(f"{name} expects a torch tensor")
    if tensor.dtype != torch.uint8:
        raise ValueError(f"{name} expects uint8 pixels, got {tensor.dtype}")
    if tensor.dim() != 4:
        raise ValueError(
            f"{name} expects [N,H,W,C], got rank {tensor.dim()}")
    if not tensor.is_contiguous():
        raise ValueError(f"{name} expects a contiguous tensor")
    N, Hin, Win, C = (int(d) for d in tensor.shape)
    if not 1 <= C <= 4:
        raise ValueError(f"{name} supports 1..4 channels, got {C}")
    if len(mean) != C or len(std) != C:
        raise ValueError(
            f"mean/std need {C} entries (one per channel), got "
            f"{len(mean)}/{len(std)}")
    Hr, Wr, top, left, Hc, Wc, rh, rw = _resize_window(
        name, Hin, Win, size, crop)
    scale, bias = normalization_constants(mean, std, pixel_scale)
    if tensor.is_cuda and antialias:
        return require_native().u8_nhwc_resize_aa_normalize(
            tensor, rh, rw, top, left, Hc, Wc, scale, bias, out_dtype,
            layout == "nchw", int(_ws_cap_bytes or 0))
    if tensor.is_cuda:
        return require_native().u8_nhwc_resize_normalize(
            tensor, rh, rw, top, left, Hc, Wc, scale, bias, out_dtype,
            layout == "nchw", int(_variant))
    if N == 0:
        shape = (0, C, Hc, Wc) if layout == "nchw" else (0, Hc, Wc, C)
        return torch.empty(shape, dtype=out_dtype)
    if antialias:
        v = _resize_aa_eager(tensor.float(), rh, rw, top, left, Hc, Wc)
    else:
        y0, y1, wy = _resize_taps(Hc, top, rh, Hin)
        x0, x1, wx = _resize_taps(Wc, left, rw, Win)
        p = tensor.float()
        wx = wx.view(1, 1, Wc, 1)
        wy = wy.view(1, Hc, 1, 1)
        r0, r1 = p[:, y0], p[:, y1]
        p00, p10 = r0[:, :, x0], r1[:, :, x0]
        t = p00 + wx * (r0[:, :, x1] - p00)
        b = p10 + wx * (r1[:, :, x1] - p10)
        v = t + wy * (b - t)
    s = torch.tensor(scale, dtype=torch.float32)
    bs = torch.tensor(bias, dtype=torch.float32)
    y = (v * s.view(1, 1, 1, C)) + bs.view(1, 1, 1, C)
    if layout == "nchw":
        y = y.permute(0, 3, 1, 2)
    return y.to(out_dtype).contiguous()


# (yoff, yc, rv, gu, gv, bu) of the pinned int32 YUV -> RGB conversion
YUV_MATRICES = {
    "bt601": (16, 298, 409, -100, -208, 516),
    "bt709": (16, 298, 459, -55, -136, 541),
    "bt601_full": (0, 256, 359, -88, -183, 454),
}
YUV_CHROMA_LAYOUTS = ("nv12", "i420")


def _yuv420_frame_size(tensor, chroma, matrix, name):
    """Validate a ``[N,H*3/2,W]`` uint8 batch of 4:2:0 frames; ``(N,H,W)``."""
    if chroma not in YUV_CHROMA_LAYOUTS:
        raise ValueError(
            f"chroma must be 'nv12' or 'i420', got {chroma!r}")
    if matrix not in YUV_MATRICES:
        raise ValueError(
            f"matrix must be one of {sorted(YUV_MATRICES)}, got {matrix!r}")
    if not isinstance(tensor, torch.Tensor):
        raise ValueError(f"{name} expects a torch tensor")
    if tensor.dtype != torch.uint8:
        raise ValueError(f"{name} expects uint8 bytes, got {tensor.dtype}")
    if tensor.dim() != 3:
        raise ValueError(
            f"{name} expects [N,H*3/2,W], got rank {tensor.dim()}")
    if not tensor.is_contiguous():
        raise ValueError(f"{name} expects a contiguous tensor")
    N, rows, W = (int(d) for d in tensor.shape)
    if rows % 3 != 0:
        raise ValueError(
            f"{name}: a 4:2:0 frame has H*3/2 rows, got {rows} (not a "
            "multiple of 3)")
    H = rows // 3 * 2
    if H % 2 != 0 or W % 2 != 0:
        raise ValueError(
            f"{name}: frame height and width must be even, got {H}x{W}")
    for label, v in (("frame height", H), ("frame width", W)):
        if not 2 <= v <= RESIZE_MAX_SIDE:
            raise ValueError(
                f"{name}: {label} must be in 2..{RESIZE_MAX_SIDE}, got {v}")
    return N, H, W


def yuv420_to_rgb_u8(tensor, chroma="nv12", matrix="bt601"):
    """YUV 4:2:0 frames -> RGB uint8 ``[N,H,W,3]``, the pinned integer
    conversion.

    ``tensor`` is a contiguous uint8 ``[N,H*3/2,W]`` batch, ``H`` and ``W``
    even. A frame is its ``H*W`` luma bytes followed by the quarter-size
    chroma: ``chroma="nv12"``: ``H/2`` rows of ``W/2`` interleaved ``(U,V)``
    pairs; ``chroma="i420"``: the flat U plane of ``(H/2)*(W/2)`` bytes, then
    the V plane. Chroma is replicated: pixel ``(y,x)`` uses sample
    ``(y>>1, x>>1)``. In int32, with ``D = U-128``, ``E = V-128`` and
    ``out = clamp((sum + 128) >> 8, 0, 255)``:

    ==============  ====  =========  ==============  =========
    ``matrix``      C     R          G               B
    ==============  ====  =========  ==============  =========
    ``bt601``       Y-16  298C+409E  298C-100D-208E  298C+516D
    ``bt709``       Y-16  298C+459E  298C-55D-136E   298C+541D
    ``bt601_full``  Y     256C+359E  256C-88D-183E   256C+454D
    ==============  ====  =========  ==============  =========

    (the first two are video range, the last is full-range JFIF). A negative
    sum clamps to 0 whichever way the shift rounds. Each channel is within 1
    of the rounded floating-point matrix.

    Plain torch integer ops, on CPU and device tensors: this is the
    reference of :func:`image_yuv420_resize_to_float`, its CPU path, and the
    two-step baseline it is measured against. Invalid arguments raise
    ``ValueError``."""
    N, H, W = _yuv420_frame_size(tensor, chroma, matrix, "yuv420_to_rgb_u8")
    yoff, yc, rv, gu, gv, bu = YUV_MATRICES[matrix]
    hw, q = H * W, (H // 2) * (W // 2)
    flat = tensor.reshape(N, hw + 2 * q)
    Y = flat[:, :hw].reshape(N, H, W).to(torch.int32)
    if chroma == "nv12":
        uv = flat[:, hw:].reshape(N, H // 2, W // 2, 2)
        U, V = uv[..., 0], uv[..., 1]
    else:
        U = flat[:, hw:hw + q].reshape(N, H // 2, W // 2)
        V = flat[:, hw + q:].reshape(N, H // 2, W // 2)

    def up(plane):
        return (plane.to(torch.int32) - 128).repeat_interleave(
            2, dim=1).repeat_interleave(2, dim=2)

    D, E = up(U), up(V)
    base = yc * (Y - yoff) + 128
    rgb = torch.stack((base + rv * E, base + gu * D + gv * E, base + bu * D),
                      dim=-1)
    return (rgb >> 8).clamp_(0, 255).to(torch.uint8)


def image_yuv420_resize_to_float(tensor, size, mean, std, crop=None,
                                 out_dtype=None, layout="nchw",
                                 pixel_scale=1.0 / 255.0, _variant=0, *,
                                 chroma="nv12", matrix="bt601",
                                 antialias=False, _ws_cap_bytes=None):
    """Fused ingest of YUV 4:2:0 frames: conversion to RGB, bilinear resize,
    crop and normalize in one pass. ``tensor`` is a contiguous uint8
    ``[N,H*3/2,W]`` batch of NV12 or I420 frames (layout and ``matrix``: see
    :func:`yuv420_to_rgb_u8`), 1.5 bytes per pixel instead of RGB's 3.

    The contract, bit for bit::

        image_yuv420_resize_to_float(x, size, mean, std, crop, out_dtype,
                                     layout, pixel_scale,
                                     chroma=chroma, matrix=matrix)
          == image_u8_resize_to_float(yuv420_to_rgb_u8(x, chroma, matrix),
                                      size, mean, std, crop, out_dtype,
                                      layout, pixel_scale)

    so every bilinear tap is the converted and clamped uint8 value of its
    source pixel, and the identity-size and crop properties of
    :func:`image_u8_resize_to_float` carry over. ``size=None`` means
    ``(H,W)``; ``mean`` and ``std`` have 3 entries.

    ``antialias=True`` (keyword only) keeps that contract with
    ``antialias=True`` on the right-hand side too, bit for bit::

        image_yuv420_resize_to_float(..., chroma=c, matrix=m, antialias=True)
          == image_u8_resize_to_float(yuv420_to_rgb_u8(x, c, m), ...,
                                      antialias=True)

    Every tap of the horizontal pass is the converted, clamped uint8 value of
    its source pixel, widened to fp32; the tap order, the one division by
    ``tot``, the vertical pass and the normalization are those of the RGB
    antialiased op, whose vertical kernel it reuses.

    Device tensors run the gfx950 kernels: one launch (two for
    ``antialias=True``: a horizontal pass that converts, then the vertical
    pass), the RGB image never exists in device memory, no eager fallback. CPU tensors run exactly the
    two-step expression above, so CPU-only servers work too. ``H`` and ``W``
    must be even and in 2..16384, the resized sides in 1..16384. Invalid
    arguments raise ``ValueError`` on both paths; ``N == 0`` returns an empty
    tensor."""
    import numpy as np

    name = "image_yuv420_resize_to_float"
    if out_dtype is None:
        out_dtype = torch.float32
    if layout not in ("nchw", "nhwc"):
        raise ValueError(f"layout must be 'nchw' or 'nhwc', got {layout!r}")
    if out_dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(
            f"out_dtype must be float32, bfloat16 or float16, got {out_dtype}")
    N, Hin, Win = _yuv420_frame_size(tensor, chroma, matrix, name)
    if len(mean) != 3 or len(std) != 3:
        raise ValueError(
            f"mean/std need 3 entries (R, G, B), got {len(mean)}/{len(std)}")
    if size is None:
        size = (Hin, Win)
    try:
        Hr, Wr = (int(d) for d in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (H, W), got {size!r}") from None
    for label, v in (("resized height", Hr), ("resized width", Wr)):
        if not 1 <= v <= RESIZE_MAX_SIDE:
            raise ValueError(
                f"{name}: {label} must be in 1..{RESIZE_MAX_SIDE}, got {v}")
    if crop is None:
        top, left, Hc, Wc = 0, 0, Hr, Wr
    else:
        try:
            top, left, Hc, Wc = (int(d) for d in crop)
        except (TypeError, ValueError):
            raise ValueError(
                f"crop must be (top, left, height, width), got {crop!r}"
            ) from None
        if Hc < 1 or Wc < 1:
            raise ValueError(f"crop extent must be positive, got {Hc}x{Wc}")
        if top < 0 or left < 0 or top + Hc > Hr or left + Wc > Wr:
            raise ValueError(
                f"crop window (top={top}, left={left}, {Hc}x{Wc}) is not "
                f"inside the resized image {Hr}x{Wr}")
    scale, bias = normalization_constants(mean, std, pixel_scale)
    if tensor.is_cuda:
        rh = float(np.float32(Hin / Hr))
        rw = float(np.float32(Win / Wr))
        if antialias:
            return require_native().yuv420_resize_aa_normalize(
                tensor, chroma == "i420", list(YUV_MATRICES[matrix]), rh, rw,
                top, left, Hc, Wc, scale, bias, out_dtype, layout == "nchw",
                int(_variant), int(_ws_cap_bytes or 0))
        return require_native().yuv420_resize_normalize(
            tensor, chroma == "i420", list(YUV_MATRICES[matrix]), rh, rw,
            top, left, Hc, Wc, scale, bias, out_dtype, layout == "nchw",
            int(_variant))
    return image_u8_resize_to_float(
        yuv420_to_rgb_u8(tensor, chroma, matrix), (Hr, Wr), mean, std,
        crop=(top, left, Hc, Wc), out_dtype=out_dtype, layout=layout,
        pixel_scale=pixel_scale, antialias=bool(antialias))


def _ragged_pairs(value, n, what, name):
    """``value`` as an int64 numpy ``[n,2]``: one pair for every image, or
    one pair per image."""
    import numpy as np

    if isinstance(value, torch.Tensor):
        value = value.cpu().numpy()
    try:
        arr = np.asarray(value)
    except (TypeError, ValueError):
        arr = None
    if arr is None or arr.dtype.kind not in "iu" or \
            arr.shape not in ((2,), (n, 2)):
        raise ValueError(
            f"{name}: {what} must be one integer pair or integer [{n},2], "
            f"got {value!r}")
    arr = arr.astype(np.int64)
    if arr.ndim == 1:
        arr = np.broadcast_to(arr, (n, 2))
    return arr


def _first_bad(mask):
    import numpy as np

    idx = np.nonzero(mask)[0]
    return int(idx[0]) if idx.size else None


def _ragged_data(name, data):
    """The checks of a packed ragged buffer."""
    if not isinstance(data, torch.Tensor):
        raise ValueError(f"{name} expects a torch tensor")
    if data.dtype != torch.uint8:
        raise ValueError(f"{name} expects uint8 pixels, got {data.dtype}")
    if data.dim() != 1:
        raise ValueError(
            f"{name} expects a flat [total_bytes] tensor, got rank "
            f"{data.dim()}")
    if not data.is_contiguous():
        raise ValueError(f"{name} expects a contiguous tensor")


def _ragged_geometry(name, data, shapes, sizes, out_size, origins, C):
    """The per-image checks that the ragged ops share, for ``C`` channels:
    ``(N, Hc, Wc, shp, siz, org, offsets)``, int64 numpy ``[N,2]`` arrays of
    the input sizes, resized sizes and crop origins and the ``[N]`` byte
    offsets of the images in ``data``."""
    import numpy as np

    if isinstance(shapes, torch.Tensor):
        shapes = shapes.cpu().numpy()      # device tensor: synchronizing D2H
    try:
        shp = np.asarray(shapes)
    except (TypeError, ValueError):
        shp = None
    if shp is not None and shp.size == 0 and shp.ndim <= 2:
        shp = np.zeros((0, 2), dtype=np.int64)         # [] or [0,2]
    if shp is None or shp.dtype.kind not in "iu" or shp.ndim != 2 or \
            shp.shape[1] != 2:
        raise ValueError(
            f"{name}: shapes must be integer [N,2] rows of (H, W), got "
            f"{shapes!r}")
    shp = shp.astype(np.int64)
    N = int(shp.shape[0])
    try:
        Hc, Wc = (int(d) for d in out_size)
    except (TypeError, ValueError):
        raise ValueError(
            f"out_size must be (H, W), got {out_size!r}") from None
    if not (1 <= Hc <= RESIZE_MAX_SIDE and 1 <= Wc <= RESIZE_MAX_SIDE):
        raise ValueError(
            f"{name}: out_size sides must be in 1..{RESIZE_MAX_SIDE}, got "
            f"{Hc}x{Wc}")
    siz = _ragged_pairs(sizes, N, "sizes", name)
    org = (np.zeros((N, 2), dtype=np.int64) if origins is None
           else _ragged_pairs(origins, N, "origins", name))

    for label, arr in (("input", shp), ("resized", siz)):
        bad = _first_bad(((arr < 1) | (arr > RESIZE_MAX_SIDE)).any(axis=1))
        if bad is not None:
            raise ValueError(
                f"{name}: image {bad}: {label} sides must be in "
                f"1..{RESIZE_MAX_SIDE}, got {int(arr[bad, 0])}x"
                f"{int(arr[bad, 1])}")
    nbytes = shp[:, 0] * shp[:, 1] * C
    total = int(nbytes.sum())
    if total != data.numel():
        raise ValueError(
            f"{name}: shapes describe {total} bytes ({N} images, {C} "
            f"channels) but data has {data.numel()}")
    bad = _first_bad((org < 0).any(axis=1) | (org[:, 0] + Hc > siz[:, 0]) |
                     (org[:, 1] + Wc > siz[:, 1]))
    if bad is not None:
        raise ValueError(
            f"{name}: image {bad}: crop window (top={int(org[bad, 0])}, "
            f"left={int(org[bad, 1])}, {Hc}x{Wc}) is not inside the resized "
            f"image {int(siz[bad, 0])}x{int(siz[bad, 1])}")
    offsets = np.zeros(N, dtype=np.int64)
    np.cumsum(nbytes[:-1], out=offsets[1:])
    return N, Hc, Wc, shp, siz, org, offsets


def _ragged_table(shp, siz, org, offsets, pinned):
    """The ragged kernels' per-image table, a CPU int32 ``[N,8]`` tensor:
    offset (int64 as two little-endian words), Hin, Win, top, left, bits of
    rh, bits of rw."""
    import numpy as np

    N = int(shp.shape[0])
    table = torch.empty((N, 8), dtype=torch.int32,
                        pin_memory=N > 0 and pinned)
    t = table.numpy()
    t[:, 0:2] = offsets.astype("<i8").view("<i4").reshape(N, 2)
    t[:, 2:4] = shp
    t[:, 4:6] = org
    # Python-double division rounded once to fp32, as the dense op does
    t[:, 6:8] = (shp / siz).astype(np.float32).view(np.int32)
    return table


def image_u8_ragged_resize_to_float(data, shapes, sizes, out_size, mean, std,
                                    origins=None, out_dtype=None,
                                    layout="nchw", pixel_scale=1.0 / 255.0,
                                    *, antialias=False, _ws_cap_bytes=None):
    """Fused uint8 image ingest of a ragged batch: N images of N different
    sizes, packed back to back with no padding, are each resized, cropped to
    one shared output size and normalized into one ``[N,C,Hc,Wc]``
    (``layout="nhwc"``: ``[N,Hc,Wc,C]``) batch, in one kernel launch (two
    with ``antialias=True``).

    * ``data``: contiguous 1-D uint8 torch tensor, on CPU or device. Image
      ``i`` is HWC and starts at byte ``off_i = sum_{j<i} H_j*W_j*C``.
    * ``shapes``: integer ``[N,2]``, row ``i`` is ``(H_i, W_i)``. It is read
      on the **host**: a list, a numpy array or a CPU tensor. A device
      tensor is accepted and copied to the host, which costs a small
      synchronizing D2H copy per call.
    * ``sizes``: the resized size, one ``(Hr,Wr)`` pair for all images or
      ``[N,2]`` per image.
    * ``out_size``: the shared ``(Hc,Wc)``.
    * ``origins``: ``(top,left)`` of the crop window inside the resized
      image, ``[N,2]`` per image, one pair, or ``None`` for zeros.
    * ``C = len(mean)``, in 1..4.

    The contract, bit for bit::

        out[i] == image_u8_resize_to_float(
                      data[off_i : off_i + H_i*W_i*C].view(1,H_i,W_i,C),
                      sizes[i], mean, std,
                      crop=(top_i, left_i, Hc, Wc), out_dtype=out_dtype,
                      layout=layout, pixel_scale=pixel_scale,
                      antialias=antialias)[0]

    CPU tensors run exactly this loop, so CPU-only servers work. Device
    tensors run the gfx950 ragged kernels only (no eager fallback): the host
    builds a per-image table (offset, sizes, origin, ``float32(H_i/Hr_i)``,
    ``float32(W_i/Wr_i)``) and copies it on the current stream from a pinned
    buffer.

    ``antialias=True`` (keyword only) resizes every image with the
    antialiased triangle filter of :func:`image_u8_resize_to_float`, what PIL
    and torchvision ``Resize`` do when they shrink a photo. On the device the
    native entry derives each image's source-row range from the same table
    and runs the horizontal and the vertical pass over one ragged fp32
    workspace, two launches for the whole batch; a batch whose workspace
    exceeds the cap runs in chunks of whole images. ``_ws_cap_bytes``
    overrides that cap (a test hook, as on the dense op).

    Invalid arguments raise ``ValueError`` on both paths, before any launch,
    and name the image at fault: wrong dtype, rank or contiguity of ``data``;
    ``shapes`` not integer ``[N,2]``; ``len(mean) != len(std)`` or C outside
    1..4; a side outside 1..16384; ``sum(H_i*W_i*C) != data.numel()``;
    ``sizes`` / ``origins`` of the wrong shape; a crop window not inside an
    image's resized size; a bad ``layout`` or ``out_dtype``. ``N == 0`` with
    empty ``data`` returns an empty tensor of the output shape."""
    name = "image_u8_ragged_resize_to_float"
    if out_dtype is None:
        out_dtype = torch.float32
    if layout not in ("nchw", "nhwc"):
        raise ValueError(f"layout must be 'nchw' or 'nhwc', got {layout!r}")
    if out_dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(
            f"out_dtype must be float32, bfloat16 or float16, got {out_dtype}")
    _ragged_data(name, data)
    if len(mean) != len(std):
        raise ValueError(
            f"mean has {len(mean)} entries but std has {len(std)}")
    C = len(mean)
    if not 1 <= C <= 4:
        raise ValueError(f"{name} supports 1..4 channels, got {C}")

    N, Hc, Wc, shp, siz, org, offsets = _ragged_geometry(
        name, data, shapes, sizes, out_size, origins, C)
    scale, bias = normalization_constants(mean, std, pixel_scale)

    if data.is_cuda:
        native = require_native()
        table = _ragged_table(shp, siz, org, offsets, not antialias)
        if antialias:
            # the entry reads these rows on the host and ships its own table
            return native.u8_ragged_resize_aa_normalize(
                data, table, C, Hc, Wc, scale, bias, out_dtype,
                layout == "nchw", int(_ws_cap_bytes or 0))
        # pinned source: the copy is queued on the current stream and the
        # caching host allocator keeps the buffer until it has completed
        table_dev = table.to(data.device, non_blocking=True)
        return native.u8_ragged_resize_normalize(
            data, table_dev, C, Hc, Wc, scale, bias, out_dtype,
            layout == "nchw")
    if N == 0:
        shape = (0, C, Hc, Wc) if layout == "nchw" else (0, Hc, Wc, C)
        return torch.empty(shape, dtype=out_dtype)
    outs = []
    for i in range(N):
        h, w = int(shp[i, 0]), int(shp[i, 1])
        off = int(offsets[i])
        outs.append(image_u8_resize_to_float(
            data[off:off + h * w * C].view(1, h, w, C),
            (int(siz[i, 0]), int(siz[i, 1])), mean, std,
            crop=(int(org[i, 0]), int(org[i, 1]), Hc, Wc),
            out_dtype=out_dtype, layout=layout, pixel_scale=pixel_scale,
            antialias=antialias))
    return torch.cat(outs)


PATCH_EMBED_PATCHES = (14, 16, 32)


def patch_embed_fold(weight, bias, mean, std, pixel_scale=1.0 / 255.0):
    """Fold the per-channel normalization into a ViT patch projection, once
    per model, on the host: ``(wk, bias_f)`` for :func:`image_u8_patch_embed`.

    ``weight`` is the conv weight ``[D,3,P,P]``, ``bias`` its ``[D]`` bias or
    ``None``. With ``(scale, bias_c) = normalization_constants(mean, std,
    pixel_scale)``, so that the normalized pixel is ``u8 * scale_c +
    bias_c``::

        wk[d, (py*P + px)*3 + c] = bf16_rne(W[d,c,py,px] * scale_c)
        bias_f[d] = fp32(bias[d] + sum W[d,c,py,px] * bias_c)

    Products and the sum are fp64, from the unrounded ``W``; the bf16
    rounding is one round-to-nearest-even straight from fp64 (normal range).
    ``wk`` is bf16 ``[D,Kp]``, ``Kp`` = ``3*P*P`` rounded up to a multiple of
    32 with a zero tail; ``bias_f`` is fp32 ``[D]``; both are on the device
    of ``weight``. Deterministic."""
    if not isinstance(weight, torch.Tensor) or weight.dim() != 4 or \
            weight.shape[1] != 3 or weight.shape[2] != weight.shape[3] or \
            not weight.is_floating_point():
        raise ValueError(
            "patch_embed_fold expects a float conv weight [D,3,P,P], got "
            f"{getattr(weight, 'shape', weight)!r}")
    D, P = int(weight.shape[0]), int(weight.shape[2])
    if len(mean) != 3 or len(std) != 3:
        raise ValueError(
            f"mean/std need 3 entries (R, G, B), got {len(mean)}/{len(std)}")
    if bias is not None and tuple(bias.shape) != (D,):
        raise ValueError(
            f"bias must have shape {[D]}, got {list(bias.shape)}")
    scale, bias_c = normalization_constants(mean, std, pixel_scale)
    w = weight.detach().cpu().double()
    s = torch.tensor(scale, dtype=torch.float64).view(1, 3, 1, 1)
    b = torch.tensor(bias_c, dtype=torch.float64).view(1, 3, 1, 1)
    K = 3 * P * P
    # 8 significant bits, ties to even; .to(bfloat16) is then exact (a cast
    # of the fp64 product would round twice, through fp32)
    mant, exp = torch.frexp((w * s).permute(0, 2, 3, 1).reshape(D, K))
    wk = torch.zeros((D, (K + 31) // 32 * 32), dtype=torch.bfloat16)
    wk[:, :K] = torch.ldexp(torch.round(mant * 256.0), exp - 8).to(
        torch.bfloat16)
    bias_f = (w * b).sum((1, 2, 3))
    if bias is not None:
        bias_f = bias_f + bias.detach().cpu().double()
    return wk.to(weight.device), bias_f.float().to(weight.device)


def image_u8_patch_embed(images, wk, bias_f, patch, pos_embed=None,
                         cls_token=None, out_dtype=None):
    """Fused ViT patch embedding of raw pixels: contiguous uint8
    ``[N,H,W,3]`` images -> tokens ``[N,T,D]``, normalization, patch
    projection, class token and position embedding in one kernel launch.

    ``(wk, bias_f)`` come from :func:`patch_embed_fold`: bf16 ``[D,Kp]`` and
    fp32 ``[D]``, ``D`` a multiple of 16. ``patch`` is 14, 16 or 32 and
    divides ``H`` and ``W``; ``Hp = H/patch``, ``Wp = W/patch``. ``cls_token``
    is fp32 ``[D]`` or ``None``, ``pos_embed`` fp32 ``[T,D]`` or ``None``,
    with ``T = Hp*Wp + (1 if cls_token is given else 0)``::

        out[n, t0 + hp*Wp + wp, d] = out_dtype(
            sum_k u8(n, hp*P+py, wp*P+px, c) * wk[d, (py*P+px)*3+c]
            + bias_f[d] + pos_embed[t0 + hp*Wp + wp, d])
        out[n, 0, d] = out_dtype(cls_token[d] + pos_embed[0, d])   # t0 = 1

    The pixel operand is exact (every byte is a bf16 number); the products
    run on the bf16 matrix cores with fp32 accumulation, the rest is fp32
    and one round-to-nearest-even conversion to ``out_dtype`` (float32, the
    default, bfloat16 or float16). The only approximation against an fp32
    model on normalized input is the bf16 rounding of the folded weights.
    Deterministic: the same input gives bit-identical output on every run.

    Device tensors run the gfx950 kernel (no eager fallback); CPU tensors
    use an eager fp32 expression with the same semantics, so CPU-only servers
    work too. ``N == 0`` returns an empty tensor. Invalid arguments raise
    ``ValueError`` on both paths. The kernel loads pixels 16 bytes at a time:
    a device ``images`` whose storage is not 16-byte aligned (a view at an
    odd offset; fresh tensors are aligned) is copied once before the
    launch."""
    return _image_u8_patch_embed(images, wk, bias_f, patch, pos_embed,
                                 cls_token, out_dtype, 0)


def _image_u8_patch_embed(images, wk, bias_f, patch, pos_embed, cls_token,
                          out_dtype, tile):
    """:func:`image_u8_patch_embed` with the kernel's tile forced, for tests
    and the bench tool: ``tile`` 0 is the kernel's own rule, 1 the small
    tile, 2 the large one. The CPU path has no tiles."""
    name = "image_u8_patch_embed"
    out_dtype = _patch_embed_out_dtype(out_dtype)
    if isinstance(patch, bool) or patch not in PATCH_EMBED_PATCHES:
        raise ValueError(
            f"patch must be one of {PATCH_EMBED_PATCHES}, got {patch!r}")
    P = int(patch)
    N, H, W = _patch_embed_images(name, images)
    out_dtype, T, D = _patch_embed_operands(
        name, images, H, W, P, wk, bias_f, pos_embed, cls_token, out_dtype)
    if N == 0:
        return torch.empty((0, T, D), dtype=out_dtype, device=images.device)
    if images.is_cuda:
        if images.data_ptr() % 16:      # the kernel loads 16 bytes at a time
            images = images.clone()
        return require_native().u8_patch_embed(
            images, wk, bias_f, P, pos_embed, cls_token, out_dtype,
            int(tile))
    return _patch_embed_eager(images.float(), wk, bias_f, P, pos_embed,
                              cls_token, out_dtype)


def _patch_embed_images(name, images):
    """``(N, H, W)`` of a uint8 ``[N,H,W,3]`` batch, or ``ValueError``."""
    if not isinstance(images, torch.Tensor):
        raise ValueError(f"{name} expects a torch tensor")
    if images.dtype != torch.uint8:
        raise ValueError(f"{name} expects uint8 pixels, got {images.dtype}")
    if images.dim() != 4:
        raise ValueError(f"{name} expects [N,H,W,3], got rank {images.dim()}")
    N, H, W, C = (int(d) for d in images.shape)
    if C != 3:
        raise ValueError(f"{name} expects 3 channels, got {C}")
    return N, H, W


def _patch_embed_eager(a, wk, bias_f, P, pos_embed, cls_token, out_dtype):
    """The CPU expression of the patch embedding for an fp32 operand ``a``
    ``[N,H,W,3]``: fp32 matmul, then the kernel's epilogue."""
    N, H, W, _ = a.shape
    K, Hp, Wp, D = 3 * P * P, H // P, W // P, wk.shape[0]
    a = a.view(N, Hp, P, Wp, P, 3).permute(0, 1, 3, 2, 4, 5).reshape(
        N * Hp * Wp, K)
    y = ((a @ wk[:, :K].float().t()) + bias_f).view(N, Hp * Wp, D)
    if pos_embed is not None:
        y = y + pos_embed[-Hp * Wp:]
    if cls_token is not None:
        row = cls_token if pos_embed is None else cls_token + pos_embed[0]
        y = torch.cat((row.expand(N, 1, D), y), dim=1)
    return y.to(out_dtype).contiguous()


def _patch_embed_out_dtype(out_dtype):
    if out_dtype is None:
        return torch.float32
    if out_dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(
            f"out_dtype must be float32, bfloat16 or float16, got {out_dtype}")
    return out_dtype


def _patch_embed_operands(name, images, H, W, P, wk, bias_f, pos_embed,
                          cls_token, out_dtype):
    """The checks the RGB and the YUV patch embedding share, for ``images``
    of ``H x W`` pixels: ``(out_dtype, T, D)``."""
    out_dtype = _patch_embed_out_dtype(out_dtype)
    if H < P or W < P or H % P or W % P:
        raise ValueError(
            f"{name}: H and W must be positive multiples of patch {P}, got "
            f"{H}x{W}")
    K = 3 * P * P
    Kp = (K + 31) // 32 * 32
    if not isinstance(wk, torch.Tensor) or wk.dtype != torch.bfloat16 or \
            wk.dim() != 2 or wk.shape[1] != Kp or wk.shape[0] < 16 or \
            wk.shape[0] % 16:
        raise ValueError(
            f"wk must be bfloat16 [D,{Kp}] with D a multiple of 16, got "
            f"{getattr(wk, 'dtype', None)} {list(getattr(wk, 'shape', ()))}")
    D = int(wk.shape[0])
    t0 = 0 if cls_token is None else 1
    T = (H // P) * (W // P) + t0
    for label, t, shape in (("bias_f", bias_f, (D,)),
                            ("pos_embed", pos_embed, (T, D)),
                            ("cls_token", cls_token, (D,))):
        if t is None and label != "bias_f":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or \
                tuple(t.shape) != shape:
            raise ValueError(
                f"{label} must be float32 {list(shape)}, got "
                f"{getattr(t, 'dtype', None)} "
                f"{list(getattr(t, 'shape', ()))}")
    for label, t in (("images", images), ("wk", wk), ("bias_f", bias_f),
                     ("pos_embed", pos_embed), ("cls_token", cls_token)):
        if t is None:
            continue
        if not t.is_contiguous():
            raise ValueError(f"{name} expects a contiguous {label}")
        if t.device != images.device:
            raise ValueError(
                f"{label} is on {t.device} but images is on {images.device}")
    return out_dtype, T, D


YUV420_PATCH_EMBED_PATCHES = (16, 32)


def image_yuv420_patch_embed(frames, wk, bias_f, patch, pos_embed=None,
                             cls_token=None, out_dtype=None, *,
                             chroma="nv12", matrix="bt601"):
    """Fused ViT patch embedding of YUV 4:2:0 frames: contiguous uint8
    ``[N,H*3/2,W]`` NV12 or I420 frames (layout, ``chroma`` and ``matrix``:
    see :func:`yuv420_to_rgb_u8`) -> tokens ``[N,T,D]`` in one kernel launch,
    from half the bytes of RGB. The contract, bit for bit::

        image_yuv420_patch_embed(x, wk, bias_f, patch, pos_embed, cls_token,
                                 out_dtype, chroma=chroma, matrix=matrix)
          == image_u8_patch_embed(yuv420_to_rgb_u8(x, chroma, matrix),
                                  wk, bias_f, patch, pos_embed, cls_token,
                                  out_dtype)

    so ``(wk, bias_f)`` are those of :func:`patch_embed_fold`, unchanged, and
    every other argument and property is that of
    :func:`image_u8_patch_embed`: the converted pixel is a uint8 value, exact
    in bf16. ``patch`` is 16 or 32 (14 is not served from YUV) and divides
    ``H`` and ``W``.

    Device tensors run the gfx950 kernel, which converts while it fills its
    tile: the RGB image never exists in device memory, no eager fallback.
    CPU tensors run exactly the two-step expression above. ``N == 0`` returns
    an empty tensor. Invalid arguments raise ``ValueError`` on both paths. A
    device ``frames`` whose storage is not 16-byte aligned is copied once
    before the launch."""
    return _image_yuv420_patch_embed(frames, wk, bias_f, patch, pos_embed,
                                     cls_token, out_dtype, 0, chroma=chroma,
                                     matrix=matrix)


def _image_yuv420_patch_embed(frames, wk, bias_f, patch, pos_embed,
                              cls_token, out_dtype, tile, *, chroma="nv12",
                              matrix="bt601"):
    """:func:`image_yuv420_patch_embed` with the kernel's tile forced, as
    :func:`_image_u8_patch_embed`."""
    name = "image_yuv420_patch_embed"
    if isinstance(patch, bool) or patch not in YUV420_PATCH_EMBED_PATCHES:
        raise ValueError(
            f"{name}: patch must be one of {YUV420_PATCH_EMBED_PATCHES}, got "
            f"{patch!r}")
    P = int(patch)
    N, H, W = _yuv420_frame_size(frames, chroma, matrix, name)
    out_dtype, T, D = _patch_embed_operands(
        name, frames, H, W, P, wk, bias_f, pos_embed, cls_token, out_dtype)
    if N == 0:
        return torch.empty((0, T, D), dtype=out_dtype, device=frames.device)
    if frames.is_cuda:
        if frames.data_ptr() % 16:      # the kernel's loads are aligned
            frames = frames.clone()
        return require_native().yuv420_patch_embed(
            frames, wk, bias_f, P, pos_embed, cls_token, out_dtype,
            int(tile), chroma == "i420", list(YUV_MATRICES[matrix]))
    return _image_u8_patch_embed(
        yuv420_to_rgb_u8(frames, chroma, matrix), wk, bias_f, P, pos_embed,
        cls_token, out_dtype, 0)


RESIZE_PATCH_EMBED_PATCHES = (16, 32)


def image_u8_resize_patch_embed(images, size, wk, bias_f, patch, crop=None,
                                pos_embed=None, cls_token=None,
                                out_dtype=None):
    """Fused ViT patch embedding of images of any size: contiguous uint8
    ``[N,Hin,Win,3]`` images are resized to a virtual ``size=(Hr,Wr)`` image
    and the window ``crop=(top,left,Hc,Wc)`` of it (``None``: all of it) goes
    to tokens ``[N,T,D]``, in one kernel launch. ``size`` and ``crop`` mean
    what they mean in :func:`image_u8_resize_to_float` (bilinear, no
    antialiasing); ``Hc`` and ``Wc`` are positive multiples of ``patch``,
    which is 16 or 32. ``(wk, bias_f)`` are those of :func:`patch_embed_fold`,
    unchanged; ``pos_embed``, ``cls_token``, ``out_dtype`` and ``T`` are those
    of :func:`image_u8_patch_embed` with ``H, W := Hc, Wc``.

    The operand of output pixel ``(oy, ox)`` of the window, channel ``c``, is
    the blend ``v = t + wy*(b - t)`` of :func:`image_u8_resize_to_float`
    before its normalization, from the same fp32 operations. It reaches the
    bf16 matrix cores as two pieces::

        hi = bf16_rne(v)      lo = bf16_rne(v - hi)      a = hi + lo
        out[n, t0 + hp*Wp + wp, d] = out_dtype(
            sum_k a_k * wk[d, k] + bias_f[d] + pos_embed[t0 + hp*Wp + wp, d])

    ``v - hi`` is exact in fp32, so ``|v - a| <= 2**-16 * |v|``. Accumulation
    is fp32: per 32 values of ``k`` the ``hi`` products, then the ``lo``
    products, ascending ``k``, one accumulator; class-token rows and the
    epilogue are those of :func:`image_u8_patch_embed`. Deterministic. With
    ``size == (Hin,Win)`` and ``crop=None`` the weights are exactly 0, ``lo``
    is 0 and the result is bit-identical to :func:`image_u8_patch_embed`; a
    cropped call equals the same tokens of any call whose window holds the
    same pixels of the resized image, since the taps depend on the position
    in the resized image alone.

    Device tensors run the gfx950 kernel, which resamples while it fills its
    tile: neither the resized image nor an fp32 tensor exists in device
    memory, no eager fallback. CPU tensors run an eager expression: the
    blends of :func:`image_u8_resize_to_float`, the split, an fp32 matmul and
    the same epilogue, the same semantics without bit-identity to the device.
    All sides must be in 1..16384. ``N == 0`` returns an empty tensor.
    Invalid arguments raise ``ValueError`` on both paths."""
    return _image_u8_resize_patch_embed(images, size, wk, bias_f, patch, crop,
                                        pos_embed, cls_token, out_dtype, 0)


def _image_u8_resize_patch_embed(images, size, wk, bias_f, patch, crop,
                                 pos_embed, cls_token, out_dtype, tile):
    """:func:`image_u8_resize_patch_embed` with the kernel's tile forced, as
    :func:`_image_u8_patch_embed`."""
    name = "image_u8_resize_patch_embed"
    if isinstance(patch, bool) or patch not in RESIZE_PATCH_EMBED_PATCHES:
        raise ValueError(
            f"{name}: patch must be one of {RESIZE_PATCH_EMBED_PATCHES}, got "
            f"{patch!r}")
    P = int(patch)
    N, Hin, Win = _patch_embed_images(name, images)
    Hr, Wr, top, left, Hc, Wc, rh, rw = _resize_window(
        name, Hin, Win, size, crop)
    out_dtype, T, D = _patch_embed_operands(
        name, images, Hc, Wc, P, wk, bias_f, pos_embed, cls_token, out_dtype)
    if N == 0:
        return torch.empty((0, T, D), dtype=out_dtype, device=images.device)
    if images.is_cuda:
        return require_native().u8_resize_patch_embed(
            images, rh, rw, top, left, Hc, Wc, wk, bias_f, P, pos_embed,
            cls_token, out_dtype, int(tile))
    # mean 0, std 1, pixel_scale 1: v * 1 + (-0) is v
    v = image_u8_resize_to_float(
        images, (Hr, Wr), (0.0,) * 3, (1.0,) * 3, crop=(top, left, Hc, Wc),
        layout="nhwc", pixel_scale=1.0)
    hi = v.bfloat16().float()
    lo = (v - hi).bfloat16().float()
    return _patch_embed_eager(hi + lo, wk, bias_f, P, pos_embed, cls_token,
                              out_dtype)


def image_u8_ragged_resize_patch_embed(data, shapes, sizes, out_size, wk,
                                       bias_f, patch, origins=None,
                                       pos_embed=None, cls_token=None,
                                       out_dtype=None):
    """Fused ViT patch embedding of a ragged batch: N RGB images of N
    different sizes, packed back to back with no padding, are each resized
    and cropped to one shared window and go to tokens ``[N,T,D]``, in one
    kernel launch.

    ``data``, ``shapes``, ``sizes``, ``out_size`` and ``origins`` are those
    of :func:`image_u8_ragged_resize_to_float` with ``C = 3`` (``shapes`` is
    read on the host); ``out_size = (Hc,Wc)`` holds positive multiples of
    ``patch``, which is 16 or 32. Every other argument is that of
    :func:`image_u8_resize_patch_embed`. The contract, on the device and bit
    for bit, for every image ``i`` (and every tile of the kernel)::

        out[i] == image_u8_resize_patch_embed(
                      data[off_i : off_i + H_i*W_i*3].view(1,H_i,W_i,3),
                      sizes[i], wk, bias_f, patch,
                      (top_i, left_i, Hc, Wc), pos_embed, cls_token,
                      out_dtype)[0]

    CPU tensors run exactly this loop over the dense op's eager path. Device
    tensors run the gfx950 kernel only (no eager fallback), whose resampling
    loader reads the source geometry per tile row: the host builds the
    per-image table of :func:`image_u8_ragged_resize_to_float` and copies it
    on the current stream from a pinned buffer. Deterministic.

    Invalid arguments raise ``ValueError`` on both paths, before any launch,
    and name the image at fault, as :func:`image_u8_ragged_resize_to_float`
    does. ``N == 0`` with empty ``data`` returns an empty ``[0,T,D]``."""
    return _image_u8_ragged_resize_patch_embed(
        data, shapes, sizes, out_size, wk, bias_f, patch, origins, pos_embed,
        cls_token, out_dtype, 0)


def _image_u8_ragged_resize_patch_embed(data, shapes, sizes, out_size, wk,
                                        bias_f, patch, origins, pos_embed,
                                        cls_token, out_dtype, tile):
    """:func:`image_u8_ragged_resize_patch_embed` with the kernel's tile
    forced, as :func:`_image_u8_patch_embed`."""
    name = "image_u8_ragged_resize_patch_embed"
    if isinstance(patch, bool) or patch not in RESIZE_PATCH_EMBED_PATCHES:
        raise ValueError(
            f"{name}: patch must be one of {RESIZE_PATCH_EMBED_PATCHES}, got "
            f"{patch!r}")
    P = int(patch)
    _ragged_data(name, data)
    N, Hc, Wc, shp, siz, org, offsets = _ragged_geometry(
        name, data, shapes, sizes, out_size, origins, 3)
    out_dtype, T, D = _patch_embed_operands(
        name, data, Hc, Wc, P, wk, bias_f, pos_embed, cls_token, out_dtype)
    if N == 0:
        return torch.empty((0, T, D), dtype=out_dtype, device=data.device)
    if data.is_cuda:
        native = require_native()
        # pinned source: the copy is queued on the current stream and the
        # caching host allocator keeps the buffer until it has completed
        table_dev = _ragged_table(shp, siz, org, offsets, True).to(
            data.device, non_blocking=True)
        return native.u8_ragged_resize_patch_embed(
            data, table_dev, Hc, Wc, wk, bias_f, P, pos_embed, cls_token,
            out_dtype, int(tile))
    outs = []
    for i in range(N):
        h, w = int(shp[i, 0]), int(shp[i, 1])
        off = int(offsets[i])
        outs.append(_image_u8_resize_patch_embed(
            data[off:off + h * w * 3].view(1, h, w, 3),
            (int(siz[i, 0]), int(siz[i, 1])), wk, bias_f, P,
            (int(org[i, 0]), int(org[i, 1]), Hc, Wc), pos_embed, cls_token,
            out_dtype, 0))
    return torch.cat(outs)


BERT_EMBED_MAX_HIDDEN = 4096
_FLOAT_DTYPES = ("float32", "bfloat16", "float16")


def _bert_embed_operands(name, input_ids, ids_rank, tok, pos, typ, gamma,
                         beta, token_type_ids, out_dtype):
    """The checks that both BERT embedding ops share: ``(token_type_ids,
    out_dtype)``, the types contiguous in the dtype of the ids."""
    tables = (("tok", tok, 2), ("pos", pos, 2), ("typ", typ, 2),
              ("gamma", gamma, 1), ("beta", beta, 1))
    for label, t, rank in tables:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: {label} must be a torch tensor")
        if t.dim() != rank:
            raise ValueError(
                f"{name}: {label} must have rank {rank}, got {t.dim()}")
        if t.dtype != tok.dtype:
            raise ValueError(
                f"{name}: tables, gamma and beta share one dtype, but tok is "
                f"{tok.dtype} and {label} is {t.dtype}")
        if t.device != tok.device:
            raise ValueError(
                f"{name}: {label} is on {t.device} but tok is on "
                f"{tok.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: {label} must be contiguous")
    floats = tuple(getattr(torch, n) for n in _FLOAT_DTYPES)
    if tok.dtype not in floats:
        raise ValueError(
            f"{name}: tables must be float32, bfloat16 or float16, got "
            f"{tok.dtype}")
    H = int(tok.shape[1])
    if H % 8 or not 8 <= H <= BERT_EMBED_MAX_HIDDEN:
        raise ValueError(
            f"{name}: H must be a multiple of 8 in 8.."
            f"{BERT_EMBED_MAX_HIDDEN}, got {H}")
    if tok.shape[0] < 1 or typ.shape[0] < 1:
        raise ValueError(f"{name}: tok and typ must have at least one row")
    for label, t, _ in tables[1:]:
        if t.shape[-1] != H:
            raise ValueError(
                f"{name}: {label} has {t.shape[-1]} columns but tok has {H}")
    if out_dtype is None:
        out_dtype = tok.dtype
    if out_dtype not in floats:
        raise ValueError(
            f"out_dtype must be float32, bfloat16 or float16, got {out_dtype}")

    def ids_like(label, t):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: {label} must be a torch tensor")
        if t.dtype not in (torch.int32, torch.int64):
            raise ValueError(
                f"{name}: {label} must be int32 or int64, got {t.dtype}")
        if t.dim() != ids_rank:
            raise ValueError(
                f"{name}: {label} must have rank {ids_rank}, got {t.dim()}")
        if t.device != tok.device:
            raise ValueError(
                f"{name}: {label} is on {t.device} but tok is on "
                f"{tok.device}")

    ids_like("input_ids", input_ids)
    if not input_ids.is_contiguous():
        raise ValueError(f"{name}: input_ids must be contiguous")
    if token_type_ids is not None:
        ids_like("token_type_ids", token_type_ids)
        if token_type_ids.shape != input_ids.shape:
            raise ValueError(
                f"{name}: token_type_ids has shape "
                f"{list(token_type_ids.shape)} but input_ids has "
                f"{list(input_ids.shape)}")
        # the kernel reads both through one template parameter
        token_type_ids = token_type_ids.to(input_ids.dtype).contiguous()
    return token_type_ids, out_dtype


def _bert_embed_bad(name, kind, where, value, bound):
    what = "token_type_ids" if kind else "input_ids"
    return ValueError(
        f"{name}: {what}{where} = {value} is outside [0, {bound})")


def _bert_embed_first_bad(input_ids, token_type_ids, vocab, type_vocab):
    """CPU path: the lowest row whose id or type is out of range, as the
    kernel reports it (the id first when both are bad): ``(kind, flat
    index)`` or ``None``."""
    bad = (input_ids < 0) | (input_ids >= vocab)
    kind = torch.zeros_like(bad)
    if token_type_ids is not None:
        bad_t = (token_type_ids < 0) | (token_type_ids >= type_vocab)
        kind = bad_t & ~bad
        bad = bad | bad_t
    flat = bad.reshape(-1).nonzero()
    if flat.numel() == 0:
        return None
    i = int(flat[0])
    return int(kind.reshape(-1)[i]), i


def bert_embed(input_ids, tok, pos, typ, gamma, beta, eps,
               attention_mask=None, token_type_ids=None, out_dtype=None):
    """Fused BERT embedding ingest: token ids ``[B,S]`` -> ``(hidden,
    additive_mask)``, the encoder's input ``[B,S,H]`` and its attention mask
    ``[B,1,1,S]`` (``None`` when ``attention_mask`` is), in one launch.

        x      = float(tok[id]) + float(pos[s]) + float(typ[type])   (fp32)
        hidden = out_dtype(LayerNorm(x; gamma, beta, eps))
        mask   = where(attention_mask != 0, +0.0, finfo(out_dtype).min)

    The three rows are summed in fp32 from the values as stored, the
    statistics are two-pass fp32 (mean, then the sum of squared deviations;
    biased variance) with an IEEE ``1 / sqrt(var + eps)``, and the result is
    rounded once, to ``out_dtype`` (default: the tables' dtype). The result
    is deterministic: the same input gives bit-identical output on every run,
    and a row's bits depend on its id, position and type only.

    * ``input_ids``: int32 or int64 ``[B,S]``, contiguous, read as they are
      (no cast). ``S <= pos.shape[0]``.
    * ``tok [vocab,H]``, ``pos [max_pos,H]``, ``typ [type_vocab,H]``,
      ``gamma [H]``, ``beta [H]``: contiguous float32, bfloat16 or float16,
      all of one dtype, on the device of the ids. ``H`` is a multiple of 8
      in 8..4096.
    * ``attention_mask``: integer or bool ``[B,S]``; non-zero keeps.
    * ``token_type_ids``: int32 or int64 ``[B,S]`` (``None``: all zero).

    An id outside ``[0, vocab)`` or a type outside ``[0, type_vocab)`` is a
    ``ValueError`` that names the batch row, the position, the value and the
    bound. On the device such a value never indexes a table: the kernel
    reads row 0 instead and reports the lowest bad row through a 4-byte
    error slot, which this wrapper reads after the launch with one small
    synchronizing D2H copy.

    Device tensors run the gfx950 kernel only (no eager fallback); CPU
    tensors use an eager expression with the same semantics, so CPU-only
    servers work too. ``B == 0`` or ``S == 0`` returns empty tensors. Invalid
    arguments raise ``ValueError`` on both paths."""
    name = "bert_embed"
    token_type_ids, out_dtype = _bert_embed_operands(
        name, input_ids, 2, tok, pos, typ, gamma, beta, token_type_ids,
        out_dtype)
    B, S = (int(d) for d in input_ids.shape)
    H = int(tok.shape[1])
    if S > pos.shape[0]:
        raise ValueError(
            f"{name}: sequence length {S} exceeds max_position_embeddings "
            f"{int(pos.shape[0])}")
    mask = attention_mask
    if mask is not None:
        if not isinstance(mask, torch.Tensor):
            raise ValueError(f"{name}: attention_mask must be a torch tensor")
        if tuple(mask.shape) != (B, S):
            raise ValueError(
                f"{name}: attention_mask must have shape {[B, S]}, got "
                f"{list(mask.shape)}")
        if mask.is_floating_point() or mask.is_complex():
            raise ValueError(
                f"{name}: attention_mask must be an integer or bool tensor, "
                f"got {mask.dtype}")
        if mask.device != tok.device:
            raise ValueError(
                f"{name}: attention_mask is on {mask.device} but tok is on "
                f"{tok.device}")
        if mask.dtype not in (torch.int32, torch.int64, torch.uint8,
                              torch.bool):
            mask = mask != 0
        mask = mask.contiguous()
    vocab, type_vocab = int(tok.shape[0]), int(typ.shape[0])
    if B == 0 or S == 0:
        hidden = torch.empty((B, S, H), dtype=out_dtype, device=tok.device)
        return hidden, (None if mask is None else
                        torch.empty((B, 1, 1, S), dtype=out_dtype,
                                    device=tok.device))
    if tok.is_cuda:
        hidden, add_mask, code = require_native().bert_embed(
            input_ids, None, B, S, mask, token_type_ids, tok, pos, typ,
            gamma, beta, float(eps), 0, out_dtype, True)
        if code >= 0:
            b, s = divmod(code >> 1, S)
            src = token_type_ids if code & 1 else input_ids
            raise _bert_embed_bad(name, code & 1, f"[{b},{s}]",
                                  int(src[b, s]),
                                  type_vocab if code & 1 else vocab)
        return hidden, add_mask
    bad = _bert_embed_first_bad(input_ids, token_type_ids, vocab,
                                type_vocab)
    if bad is not None:
        kind, i = bad
        b, s = divmod(i, S)
        src = token_type_ids if kind else input_ids
        raise _bert_embed_bad(name, kind, f"[{b},{s}]", int(src[b, s]),
                              type_vocab if kind else vocab)
    import torch.nn.functional as F
    x = F.embedding(input_ids, tok).float() + pos[:S].float()
    x = x + (typ[0].float() if token_type_ids is None
             else F.embedding(token_type_ids, typ).float())
    hidden = F.layer_norm(x, (H,), gamma.float(), beta.float(),
                          float(eps)).to(out_dtype)
    if mask is None:
        return hidden, None
    zero = torch.zeros((), dtype=out_dtype)
    low = torch.full((), torch.finfo(out_dtype).min, dtype=out_dtype)
    return hidden, torch.where(mask != 0, zero, low)[:, None, None, :]


def _bert_ragged_lengths(name, lengths, total, max_pos):
    """``lengths`` as int64 numpy ``[B]``, each in 1..max_pos, summing to
    ``total``; read on the host."""
    import numpy as np

    if isinstance(lengths, torch.Tensor):
        lengths = lengths.cpu().numpy()    # device tensor: synchronizing D2H
    try:
        arr = np.asarray(lengths)
    except (TypeError, ValueError):
        arr = None
    if arr is not None and arr.size == 0 and arr.ndim == 1:
        arr = np.zeros((0,), dtype=np.int64)
    if arr is None or arr.dtype.kind not in "iu" or arr.ndim != 1:
        raise ValueError(
            f"{name}: lengths must be integer [B], got {lengths!r}")
    arr = arr.astype(np.int64)
    bad = _first_bad((arr < 1) | (arr > max_pos))
    if bad is not None:
        raise ValueError(
            f"{name}: sequence {bad}: length must be in 1..{max_pos} "
            f"(max_position_embeddings), got {int(arr[bad])}")
    ends = np.cumsum(arr)
    bad = _first_bad(ends > total)
    if bad is not None or int(arr.sum()) != total:
        at = f"sequence {bad} ends past it" if bad is not None else \
            f"sequence {len(arr) - 1} ends before it" if len(arr) else \
            "there are no sequences"
        raise ValueError(
            f"{name}: lengths sum to {int(arr.sum())} but input_ids has "
            f"{total} tokens: {at}")
    return arr


def bert_embed_ragged(input_ids, lengths, tok, pos, typ, gamma, beta, eps,
                      token_type_ids=None, pad_id=0, out_dtype=None,
                      packed=False):
    """:func:`bert_embed` of a ragged batch: B sequences of B lengths, their
    ids back to back in ``input_ids [total]`` with no padding, go to
    ``(hidden [B,S,H], additive_mask [B,1,1,S])`` with ``S = max(lengths)``,
    in one launch of the same kernel.

    * ``lengths``: integer ``[B]``, each in ``1..pos.shape[0]``, summing to
      ``total``. Read on the **host**: a list, a numpy array or a CPU tensor
      (a device tensor costs a small synchronizing D2H copy).
    * ``token_type_ids``: flat like ``input_ids``; padded positions get
      type 0.
    * ``pad_id``: the id of positions at and past a sequence's length.

    The contract, on the device and bit for bit::

        ids  = full((B,S), pad_id);  ids[b, :len_b] = input_ids[off_b:...]
        mask = arange(S)[None] < lengths[:, None]
        out == bert_embed(ids, ..., attention_mask=mask,
                          token_type_ids=<padded with 0>)

    ``packed=True`` returns ``hidden [total,H]`` alone, the kept rows back to
    back in the order of ``input_ids`` and no mask: ``hidden_padded[mask]`` of
    the default call, bit for bit. The kernel skips the padded rows instead
    of computing them.

    CPU tensors run exactly this. Device tensors run the gfx950 kernel only
    (no eager fallback): the host builds an int32 ``(offset, length)`` table
    and copies it on the current stream from a pinned buffer. Invalid
    arguments raise ``ValueError`` on both paths, before any launch; a bad
    length names its sequence, a bad id or type names its sequence, position,
    value and bound, as in :func:`bert_embed`. ``B == 0`` with empty
    ``input_ids`` returns empty tensors."""
    import numpy as np

    name = "bert_embed_ragged"
    token_type_ids, out_dtype = _bert_embed_operands(
        name, input_ids, 1, tok, pos, typ, gamma, beta, token_type_ids,
        out_dtype)
    vocab, type_vocab = int(tok.shape[0]), int(typ.shape[0])
    try:
        if isinstance(pad_id, bool):
            raise TypeError
        pad_id = operator.index(pad_id)
    except TypeError:
        raise ValueError(f"pad_id must be an integer, got {pad_id!r}") \
            from None
    if not 0 <= pad_id < vocab:
        raise ValueError(
            f"{name}: pad_id {pad_id} is outside [0, {vocab})")
    total = int(input_ids.numel())
    lens = _bert_ragged_lengths(name, lengths, total, int(pos.shape[0]))
    B = int(lens.shape[0])
    H = int(tok.shape[1])
    if B == 0 and packed:
        return torch.empty((0, H), dtype=out_dtype, device=tok.device)
    if B == 0:
        return (torch.empty((0, 0, H), dtype=out_dtype, device=tok.device),
                torch.empty((0, 1, 1, 0), dtype=out_dtype, device=tok.device))
    S = int(lens.max())
    offsets = np.zeros(B, dtype=np.int64)
    np.cumsum(lens[:-1], out=offsets[1:])

    def where(code):
        b, s = divmod(code >> 1, S)
        src = token_type_ids if code & 1 else input_ids
        return _bert_embed_bad(
            name, code & 1, f" of sequence {b}, position {s}",
            int(src[int(offsets[b]) + s]), type_vocab if code & 1 else vocab)

    if tok.is_cuda:
        table = torch.empty((B, 2), dtype=torch.int32, pin_memory=True)
        t = table.numpy()
        t[:, 0] = offsets
        t[:, 1] = lens
        # pinned source: the copy is queued on the current stream and the
        # caching host allocator keeps the buffer until it has completed
        table_dev = table.to(tok.device, non_blocking=True)
        hidden, add_mask, code = require_native().bert_embed(
            input_ids, table_dev, B, S, None, token_type_ids, tok, pos, typ,
            gamma, beta, float(eps), pad_id, out_dtype, True, bool(packed))
        if code >= 0:
            raise where(code)
        return hidden if packed else (hidden, add_mask)
    keep = torch.arange(S)[None, :] < torch.from_numpy(lens)[:, None]
    ids = torch.full((B, S), pad_id, dtype=input_ids.dtype)
    ids[keep] = input_ids
    types = None
    if token_type_ids is not None:
        types = torch.zeros((B, S), dtype=input_ids.dtype)
        types[keep] = token_type_ids
    bad = _bert_embed_first_bad(ids, types, vocab, type_vocab)
    if bad is not None:
        raise where(bad[1] * 2 + bad[0])
    hidden, add_mask = bert_embed(ids, tok, pos, typ, gamma, beta, eps, keep,
                                  types, out_dtype)
    return hidden[keep] if packed else (hidden, add_mask)


def masked_mean_pool(hidden, mask=None, normalize=False):
    """Fused masked mean-pool head: ``[B,S,H]`` hidden state (f32, bf16 or
    f16, contiguous) -> fp32 ``[B,H]``, one vector per sequence.

        cnt_b = number of s with mask[b,s] != 0
        y_bh  = (sum of float(hidden[b,s,h]) over kept s) / max(cnt_b, 1)
        normalize:  y_bh = y_bh / max(sqrt(sum_h y_bh**2), 1e-12)

    fp32 accumulation, IEEE division and square root (``F.normalize``
    semantics). Masked positions are selected out, never multiplied in, so a
    NaN or Inf there does not reach the output; a row with nothing kept (or
    ``S == 0``) is zeros. The result is deterministic: the same input gives
    bit-identical output on every run.

    ``mask`` is ``[B,S]`` of an integer or bool dtype on the device of
    ``hidden``; non-zero keeps the position and ``None`` keeps all. int32,
    uint8 and bool go to the kernel as they are, other integer dtypes are
    reduced with ``mask != 0`` first.

    Device tensors run the gfx950 kernels (the hidden state is read once, no
    eager fallback); CPU tensors use an eager expression with the same
    semantics, so CPU-only servers work too. Invalid arguments raise
    ``ValueError`` on both paths."""
    if not isinstance(hidden, torch.Tensor):
        raise ValueError("masked_mean_pool expects a torch tensor")
    if hidden.dim() != 3:
        raise ValueError(
            f"masked_mean_pool expects [B,S,H], got rank {hidden.dim()}")
    if hidden.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(
            "masked_mean_pool expects float32, bfloat16 or float16, got "
            f"{hidden.dtype}")
    if not hidden.is_contiguous():
        raise ValueError("masked_mean_pool expects a contiguous tensor")
    B, S, H = (int(d) for d in hidden.shape)
    if mask is not None:
        if not isinstance(mask, torch.Tensor):
            raise ValueError("masked_mean_pool expects a torch tensor mask")
        if tuple(mask.shape) != (B, S):
            raise ValueError(
                f"mask must have shape {[B, S]}, got {list(mask.shape)}")
        if mask.is_floating_point() or mask.is_complex():
            raise ValueError(
                f"mask must be an integer or bool tensor, got {mask.dtype}")
        if mask.device != hidden.device:
            raise ValueError(
                f"mask is on {mask.device} but hidden is on {hidden.device}")
        if mask.dtype not in (torch.int32, torch.uint8, torch.bool):
            mask = mask != 0   # e.g. int64: 1 << 32 is still "keep"
        mask = mask.contiguous()
    if hidden.is_cuda:
        return require_native().masked_mean_pool(hidden, mask, bool(normalize))
    x = hidden.float()
    if mask is None:
        total = x.sum(1)
        count = torch.full((B, 1), max(S, 1), dtype=torch.float32)
    else:
        keep = mask != 0
        total = torch.where(keep[..., None], x, torch.zeros((), dtype=x.dtype)
                            ).sum(1)
        count = keep.sum(1, keepdim=True).clamp(min=1).float()
    y = total / count
    if normalize:
        y = y / y.norm(dim=1, keepdim=True).clamp(min=1e-12)
    return y.contiguous()


ATTENTION_HEAD_DIM = 64


def attention_tiles(lengths, device=None):
    """The tile table of the packed form of :func:`masked_self_attention`:
    int32 ``[ntiles,4]``, one row ``(row0, L, q0, seq)`` per 64-row query
    tile of every sequence, ``ntiles = sum(ceil(len/64))``. ``row0`` is the
    sequence's first row in the packed ``[total, ...]`` tensor (sequences
    back to back in the order of ``lengths``), ``L`` its length, ``q0`` the
    tile's first query (a multiple of 64 below ``L``) and ``seq`` its index
    in ``lengths``. Every packed row is covered exactly once.

    Rows are longest sequence first (a stable sort: equal lengths keep the
    order of ``lengths``), tiles ascending inside a sequence. A workgroup's
    cost grows with ``L`` and the table's order is the dispatch order, so the
    long sequences start first and do not form the tail; the kernel's file
    header has the measurement behind that order.

    ``lengths`` is read on the **host**: a list, a numpy array or a CPU
    tensor of integers, each at least 1 (a device tensor costs a small
    synchronizing D2H copy). With a device the table is built in a pinned
    buffer and copied on the current stream without synchronization;
    ``device=None`` returns the CPU tensor. An empty list gives ``[0,4]``."""
    import numpy as np

    name = "attention_tiles"
    if isinstance(lengths, torch.Tensor):
        lengths = lengths.cpu().numpy()    # device tensor: synchronizing D2H
    try:
        arr = np.asarray(lengths)
    except (TypeError, ValueError):
        arr = None
    if arr is not None and arr.size == 0 and arr.ndim == 1:
        arr = np.zeros((0,), dtype=np.int64)
    if arr is None or arr.dtype.kind not in "iu" or arr.ndim != 1:
        raise ValueError(
            f"{name}: lengths must be integer [B], got {lengths!r}")
    arr = arr.astype(np.int64)
    bad = _first_bad(arr < 1)
    if bad is not None:
        raise ValueError(
            f"{name}: sequence {bad}: length must be at least 1, got "
            f"{int(arr[bad])}")
    if int(arr.sum()) >= 1 << 30:
        raise ValueError(f"{name}: the lengths must sum to less than 2^30")
    per_seq = (arr + 63) // 64
    n = int(per_seq.sum())
    to_device = device is not None and torch.device(device).type == "cuda"
    table = torch.empty((n, 4), dtype=torch.int32,
                        pin_memory=n > 0 and to_device)
    t = table.numpy()
    order = np.argsort(-arr, kind="stable")
    counts = per_seq[order]
    seq = np.repeat(order, counts)
    t[:, 0] = (np.cumsum(arr) - arr)[seq]
    t[:, 1] = arr[seq]
    t[:, 2] = (np.arange(n) - np.repeat(np.cumsum(counts) - counts,
                                        counts)) * 64
    t[:, 3] = seq
    if device is None:
        return table
    # pinned source: the copy is queued on the current stream and the
    # caching host allocator keeps the buffer until it has completed
    return table.to(device, non_blocking=True)


def attention_keys(mask):
    """The key table of the keys form of :func:`masked_self_attention`:
    ``(index int32 [B,S], count int32 [B])`` of a ``[B,S]`` keep mask.
    ``index[b, :count[b]]`` holds the positions ``s`` with ``mask[b,s] != 0``
    in ascending order; entries at and past ``count[b]`` are unspecified and
    are never read.

    ``mask`` is an integer or bool tensor, the rules of
    :func:`masked_mean_pool`: int32, uint8 and bool go to the kernel as they
    are, other integer dtypes are reduced with ``mask != 0`` first, a float
    mask is a ``ValueError``. A device mask is compacted by one launch (one
    wave per sequence, no host synchronization, deterministic); a CPU mask by
    a stable argsort, with the same result."""
    name = "attention_keys"
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"{name} expects a torch tensor")
    if mask.dim() != 2:
        raise ValueError(f"{name} expects [B,S], got rank {mask.dim()}")
    if mask.is_floating_point() or mask.is_complex():
        raise ValueError(
            f"{name}: mask must be an integer or bool tensor, got "
            f"{mask.dtype}")
    if mask.shape[1] >= 1 << 30:
        raise ValueError(f"{name}: S must be below 2^30")
    if mask.dtype not in (torch.int32, torch.uint8, torch.bool):
        mask = mask != 0       # e.g. int64: 1 << 32 is still "keep"
    mask = mask.contiguous()
    if mask.is_cuda:
        return require_native().attention_keys(mask)
    keep = mask != 0
    # stable: the kept positions first, each group in ascending order
    index = torch.argsort(~keep, dim=1, stable=True).to(torch.int32)
    return index.contiguous(), keep.sum(1, dtype=torch.int32)


def masked_self_attention(qkv, lengths, heads, scale=None, *, tiles=None,
                          keys=None):
    """Fused length-masked multi-head self-attention: the ``[B,S,3*H]`` qkv
    projection (bf16 or f16, contiguous, last axis ordered ``(3, heads,
    head_dim)`` as ``BertLayer.qkv`` emits it, ``head_dim == 64``) ->
    ``[B,S,H]`` of the same dtype, written in that layout directly.

    For sequence ``b`` with ``L = clamp(lengths[b], 0, S)``::

        out[b,s,h*64:(h+1)*64] = softmax_{j<L}((q_s . k_j) * scale) @ v_j   s < L
        out[b,s,:]             = +0.0                                  s >= L

    ``lengths`` is int32 ``[B]`` on the device of ``qkv``; ``None`` means
    every sequence is ``S`` long. ``scale`` defaults to ``1/sqrt(head_dim)``.
    Keys, values and queries at or past ``L`` are selected out, never
    multiplied in: a NaN or Inf stored there does not reach a kept output
    (the rule of :func:`masked_mean_pool`). Products and sums are fp32, the
    softmax is fp32, P is rounded once to the input dtype for ``P @ V`` and
    the result once at the store. Reruns are bit-identical and a sequence's
    output does not depend on its batch neighbours.

    Packed (varlen) form: a rank-2 ``qkv [T,3*H]`` holds the sequences back
    to back with no padding and the result is ``[T,H]``. ``tiles`` (keyword
    only, required, int32 ``[n,4]`` contiguous on the device of ``qkv``, from
    :func:`attention_tiles`) says where each sequence lies and ``lengths``
    must be ``None``. For every sequence ``(row0, L)`` of the table, bit for
    bit on both paths::

        out[row0:row0+L] == masked_self_attention(
                                qkv[row0:row0+L][None], None, heads, scale)[0]

    No row of a neighbouring sequence is loaded and no row past ``row0 + L``
    is stored. The kernel launches exactly ``n * heads`` workgroups. A table
    cannot cause a fault: ``row0`` is clamped to ``0..T``, ``L`` to ``0..T -
    row0`` and ``q0`` to ``>= 0`` on the device, and an entry with ``q0 >=
    L`` does nothing. Rows of ``out`` that no entry covers are unspecified.

    Keys form, for an arbitrary key mask: ``keys=(index, count)`` (keyword
    only, from :func:`attention_keys`: int32 ``[B,S]`` and ``[B]``,
    contiguous, on the device of ``qkv``) with a rank-3 ``qkv`` and neither
    ``lengths`` nor ``tiles``. With ``c = clamp(count[b], 0, S)`` and every
    index clamped to ``0..S-1``::

        c > 0:  out[b,s] = softmax_{j<c}((q_s . k_index[b,j]) * scale)
                           @ v_index[b,j]                     for EVERY s < S
        c == 0: out[b,s] = mean_{j<S} v_j                     for every s < S

    This is what ``scaled_dot_product_attention`` gives with the additive
    ``finfo.min`` mask, padded queries and a row with nothing kept (a uniform
    softmax over all S keys) included. K and V rows of masked positions are
    never loaded, so a NaN there reaches no output; all Q rows are. The cost
    follows the number of kept keys, wherever they lie. A query's result
    depends only on its own row and on the order of the kept keys, so
    ``out[b, kept]`` equals ``masked_self_attention(qkv[b, kept][None], None,
    heads, scale)[0]`` bit for bit when ``c > 0``.

    Device tensors run the gfx950 MFMA kernel only (no eager fallback, no
    host synchronization: the lengths are clamped on the device); CPU tensors
    run an eager fp32 expression with the same semantics (the packed form:
    exactly the loop above over the table's entries), so CPU-only servers
    work too. Invalid arguments raise ``ValueError`` on both paths, before
    any launch: among them a rank other than 2 or 3, a rank-2 ``qkv``
    without ``tiles`` or with ``lengths``, ``tiles`` with a rank-3 ``qkv``,
    ``tiles`` of the wrong dtype, shape or device, ``keys`` together with
    ``lengths`` or ``tiles`` or a rank-2 ``qkv``, either tensor of ``keys``
    of the wrong dtype, shape, device or contiguity. ``B == 0``, ``S == 0``
    or ``T == 0`` returns an empty tensor."""
    name = "masked_self_attention"
    if not isinstance(qkv, torch.Tensor):
        raise ValueError(f"{name} expects a torch tensor")
    if qkv.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(
            f"{name} expects bfloat16 or float16 qkv, got {qkv.dtype}")
    if qkv.dim() not in (2, 3):
        raise ValueError(
            f"{name} expects [B,S,3*H] or [T,3*H], got rank {qkv.dim()}")
    packed = qkv.dim() == 2
    if not qkv.is_contiguous():
        raise ValueError(f"{name} expects a contiguous tensor")
    try:
        if isinstance(heads, bool):
            raise TypeError
        heads = operator.index(heads)
    except TypeError:
        raise ValueError(f"heads must be an integer, got {heads!r}") from None
    S, H3 = (int(d) for d in qkv.shape[-2:])
    B = 1 if packed else int(qkv.shape[0])
    if heads < 1 or H3 % (3 * heads):
        raise ValueError(
            f"{name}: the last axis ({H3}) must be 3 * heads ({heads}) * "
            "head_dim")
    head_dim = H3 // (3 * heads)
    if head_dim != ATTENTION_HEAD_DIM:
        raise ValueError(
            f"{name}: head_dim must be {ATTENTION_HEAD_DIM}, got {head_dim}")
    if qkv.data_ptr() % 16:
        raise ValueError(f"{name}: qkv must be 16-byte aligned")
    if scale is None:
        scale = 1.0 / math.sqrt(head_dim)
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError(f"{name}: scale must be finite, got {scale}")
    if keys is not None:
        if lengths is not None or tiles is not None:
            raise ValueError(
                f"{name}: keys exclude lengths and tiles: the key table is "
                "the mask")
        if packed:
            raise ValueError(
                f"{name}: keys go with a rank-3 qkv, got rank 2")
    if packed:
        if tiles is None:
            raise ValueError(
                f"{name}: a rank-2 (packed) qkv needs tiles, see "
                "attention_tiles")
        if lengths is not None:
            raise ValueError(
                f"{name}: tiles and lengths exclude each other: a packed "
                "qkv takes its lengths from the table")
        if not isinstance(tiles, torch.Tensor) or tiles.dtype != torch.int32:
            raise ValueError(
                f"{name}: tiles must be an int32 tensor, got "
                f"{getattr(tiles, 'dtype', type(tiles))}")
        if tiles.dim() != 2 or tiles.shape[1] != 4:
            raise ValueError(
                f"{name}: tiles must have shape [n,4], got "
                f"{list(tiles.shape)}")
        if tiles.device != qkv.device:
            raise ValueError(
                f"{name}: tiles is on {tiles.device} but qkv is on "
                f"{qkv.device}")
        if not tiles.is_contiguous():
            raise ValueError(f"{name}: tiles must be contiguous")
        if S >= 1 << 30 or tiles.shape[0] * heads >= 1 << 24:
            raise ValueError(
                f"{name}: T must be below 2^30 and n * heads below 2^24, "
                f"got T={S} n={tiles.shape[0]} heads={heads}")
    elif tiles is not None:
        raise ValueError(
            f"{name}: tiles go with a rank-2 (packed) qkv, got rank 3")
    if keys is not None:
        if not isinstance(keys, (tuple, list)) or len(keys) != 2:
            raise ValueError(
                f"{name}: keys must be the (index, count) pair of "
                "attention_keys")
        for what, t, shape in (("index", keys[0], (B, S)),
                               ("count", keys[1], (B,))):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
                raise ValueError(
                    f"{name}: keys {what} must be an int32 tensor, got "
                    f"{getattr(t, 'dtype', type(t))}")
            if tuple(t.shape) != shape:
                raise ValueError(
                    f"{name}: keys {what} must have shape {list(shape)}, "
                    f"got {list(t.shape)}")
            if t.device != qkv.device:
                raise ValueError(
                    f"{name}: keys {what} is on {t.device} but qkv is on "
                    f"{qkv.device}")
            if not t.is_contiguous():
                raise ValueError(f"{name}: keys {what} must be contiguous")
    if lengths is not None:
        if not isinstance(lengths, torch.Tensor) or \
                lengths.dtype != torch.int32:
            raise ValueError(f"{name}: lengths must be an int32 tensor")
        if tuple(lengths.shape) != (B,):
            raise ValueError(
                f"{name}: lengths must have shape {[B]}, got "
                f"{list(lengths.shape)}")
        if lengths.device != qkv.device:
            raise ValueError(
                f"{name}: lengths is on {lengths.device} but qkv is on "
                f"{qkv.device}")
        lengths = lengths.contiguous()
    if qkv.is_cuda:
        if keys is not None:
            return require_native().masked_self_attention(
                qkv, None, heads, scale, None, keys[0], keys[1])
        return require_native().masked_self_attention(qkv, lengths, heads,
                                                      scale, tiles)
    H = H3 // 3
    if keys is not None:
        # the kernel's rule, clamps included: a gather of the kept K and V
        # rows, so a masked row is never read; nothing kept: the plain mean
        out = qkv.new_empty((B, S, H))
        x = qkv.float().view(B, S, 3, heads, head_dim)
        for b in range(B):
            c = min(max(int(keys[1][b]), 0), S)
            kept = keys[0][b, :c].long().clamp(0, S - 1) if c else \
                torch.arange(S)
            q, k, v = x[b, :, 0], x[b, kept, 1], x[b, kept, 2]  # [*,heads,64]
            scores = torch.einsum("shd,jhd->hsj", q, k) * (scale if c else 0.)
            out[b] = torch.einsum("hsj,jhd->shd", torch.softmax(scores, -1),
                                  v).reshape(S, H).to(qkv.dtype)
        return out
    if packed:
        # the kernel's walk over the table, clamps included; uncovered rows
        # are unspecified (zeros here)
        out = qkv.new_zeros((S, H))
        done = {}
        for row0, n, q0, _ in tiles.tolist():
            row0 = min(max(row0, 0), S)
            n = min(max(n, 0), S - row0)
            q0 = max(q0, 0)
            if q0 >= n:
                continue
            if (row0, n) not in done:
                done[row0, n] = masked_self_attention(
                    qkv[row0:row0 + n][None], None, heads, scale)[0]
            q1 = min(q0 + 64, n)
            out[row0 + q0:row0 + q1] = done[row0, n][q0:q1]
        return out
    q, k, v = (t.transpose(1, 2) for t in
               qkv.float().view(B, S, 3, heads, head_dim).unbind(2))
    n = torch.full((B,), S) if lengths is None else lengths.clamp(0, S)
    keep = torch.arange(S)[None, :] < n[:, None]             # [B,S]
    rows, cols = keep[:, None, :, None], keep[:, None, None, :]
    zero = torch.zeros(())
    q, k, v = (torch.where(rows, t, zero) for t in (q, k, v))
    scores = torch.where(cols, (q @ k.transpose(2, 3)) * scale,
                         torch.full((), float("-inf")))
    # a sequence with nothing kept: softmax of all -inf is NaN, selected out
    p = torch.where(rows & cols, torch.softmax(scores, -1), zero)
    return (p @ v).transpose(1, 2).reshape(B, S, H).to(qkv.dtype)


SOFTMAX_TOPK_MAX_K = 64


def softmax_topk(logits, k):
    """Fused classification head: ``[B,C]`` logits (f32, bf16 or f16,
    contiguous) -> ``(scores, classes)``, fp32 ``[B,k]`` and int32 ``[B,k]``,
    the ``k`` most probable classes of every row in rank order.
    ``1 <= k <= min(C, 64)``.

    The order is exact: by ``float(logit)`` descending, equal values lower
    index first, ``-0.0`` equal to ``+0.0``, NaN above ``+Inf`` (NaNs among
    themselves by index) — ``torch.sort(x.float(), 1, descending=True,
    stable=True)`` truncated to ``k``.

        m       = the rank-0 logit
        score_j = exp(x_j - m) / sum_i exp(x_i - m)

    in fp32 with an IEEE divide. A row holding NaN or ``+Inf`` has NaN
    scores (its classes are still ranked), ``-Inf`` logits score exactly 0
    and rank last. The result is deterministic: the same input gives
    bit-identical output on every run.

    Device tensors run the gfx950 kernel (one workgroup per row, the row is
    read once and kept on chip up to 8192 classes; no eager fallback); CPU
    tensors use an eager expression with the same semantics, so CPU-only
    servers work too. ``B == 0`` returns empty tensors. Invalid arguments
    raise ``ValueError`` on both paths."""
    if not isinstance(logits, torch.Tensor):
        raise ValueError("softmax_topk expects a torch tensor")
    if logits.dim() != 2:
        raise ValueError(
            f"softmax_topk expects [B,C], got rank {logits.dim()}")
    if logits.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(
            "softmax_topk expects float32, bfloat16 or float16, got "
            f"{logits.dtype}")
    if not logits.is_contiguous():
        raise ValueError("softmax_topk expects a contiguous tensor")
    B, C = (int(d) for d in logits.shape)
    try:
        if isinstance(k, bool):
            raise TypeError
        k = operator.index(k)
    except TypeError:
        raise ValueError(f"k must be an integer, got {k!r}") from None
    if not 1 <= k <= min(C, SOFTMAX_TOPK_MAX_K):
        raise ValueError(
            f"k must be in 1..min(C, {SOFTMAX_TOPK_MAX_K}), got {k} with "
            f"C = {C}")
    if B == 0:
        return (torch.empty((0, k), dtype=torch.float32,
                            device=logits.device),
                torch.empty((0, k), dtype=torch.int32, device=logits.device))
    if logits.is_cuda:
        scores, classes = require_native().softmax_topk(logits, k)
        return scores, classes
    x = logits.float()
    order = torch.sort(x, dim=1, descending=True,
                       stable=True).indices[:, :k]
    e = torch.exp(x - x.gather(1, order[:, :1]))
    scores = e.gather(1, order) / e.sum(1, keepdim=True)
    return scores.contiguous(), order.to(torch.int32).contiguous()


def pack_tensor_proto(tensor):
    """Device tensor -> python TensorProto message (for the non-turbo
    client path): native D2H pipeline for the payload, proto wrapper around
    it."""
    from ..tensors import tensor_to_tensor_proto
    from ..types import DataType
    from ..wire import messages as pb

    if not tensor.is_cuda:
        return tensor_to_tensor_proto(tensor)
    n = require_native()
    dtype = DataType(tensor.dtype)
    proto = pb.TensorProto()
    proto.dtype = dtype.enum
    for d in tensor.shape:
        proto.tensor_shape.dim.add().size = d
    proto.tensor_content = n.tensor_content_bytes(tensor, 1)
    return proto
