"""Native ops: C++ wire codec + CDNA4 HIP pack kernels.

Loads the in-tree ``_native`` extension (built by ``setup.py build_ext
--inplace`` / ``__graft_entry__.build()``). On a GPU machine the extension
is REQUIRED — device-tensor paths raise rather than silently falling back
to eager PyTorch, so a passing GPU test means the HIP path actually ran.
"""
from __future__ import annotations

import functools
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
    import numpy as np

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
    scale, bias = normalization_constants(mean, std, pixel_scale)
    rh = float(np.float32(Hin / Hr))
    rw = float(np.float32(Win / Wr))
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
    import numpy as np

    name = "image_u8_ragged_resize_to_float"
    if out_dtype is None:
        out_dtype = torch.float32
    if layout not in ("nchw", "nhwc"):
        raise ValueError(f"layout must be 'nchw' or 'nhwc', got {layout!r}")
    if out_dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(
            f"out_dtype must be float32, bfloat16 or float16, got {out_dtype}")
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
    if len(mean) != len(std):
        raise ValueError(
            f"mean has {len(mean)} entries but std has {len(std)}")
    C = len(mean)
    if not 1 <= C <= 4:
        raise ValueError(f"{name} supports 1..4 channels, got {C}")

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
    scale, bias = normalization_constants(mean, std, pixel_scale)
    offsets = np.zeros(N, dtype=np.int64)
    np.cumsum(nbytes[:-1], out=offsets[1:])

    if data.is_cuda:
        native = require_native()
        # the kernel's per-image table, int32 [N,8]: offset (int64 as two
        # little-endian words), Hin, Win, top, left, bits of rh, bits of rw
        table = torch.empty((N, 8), dtype=torch.int32,
                            pin_memory=N > 0 and not antialias)
        t = table.numpy()
        t[:, 0:2] = offsets.astype("<i8").view("<i4").reshape(N, 2)
        t[:, 2:4] = shp
        t[:, 4:6] = org
        # Python-double division rounded once to fp32, as the dense op does
        t[:, 6:8] = (shp / siz).astype(np.float32).view(np.int32)
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
