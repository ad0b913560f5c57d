"""Antialiased resize in the fused uint8 ingest path, CPU side:
``ops.image_u8_resize_to_float(..., antialias=True)`` against the pinned
recipe written out tap by tap in numpy float32, against
``F.interpolate(antialias=True)``, its identity / crop properties, and the
``antialias`` plumbing through ``ImagePreprocess``, the ResNet-50 servable
and ``model.json``.

The recipe, per axis (every operation rounds once to fp32)::

    support = r if r >= 1 else 1      inv = float32(1/r) if r >= 1 else 1
    c    = (float(o) + 0.5) * r
    lo   = clamp(int((c - support) + 0.5), 0, n_in - 1)
    hi   = min(int((c + support) + 0.5), n_in)
    size = max(hi - lo, 1)
    acc += max(1 - |((float(lo + j) - c) + 0.5) * inv|, 0) * p[lo + j]
    value = acc / tot

horizontal pass first, then vertical, then ``(value * scale) + bias``."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from min_tfs_client_amd import ops
from min_tfs_client_amd.models import resnet50_servable
from min_tfs_client_amd.preprocess import ImagePreprocess
from min_tfs_client_amd.repository import default_loader

MEAN = (0.485, 0.456, 0.406, 0.5)
STD = (0.229, 0.224, 0.225, 0.25)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16,
          "f16": torch.float16}
f32 = np.float32


def _pixels(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)


def _op(x, size, crop=None, **kw):
    C = x.shape[3]
    kw.setdefault("mean", MEAN[:C])
    kw.setdefault("std", STD[:C])
    mean, std = kw.pop("mean"), kw.pop("std")
    return ops.image_u8_resize_to_float(x, size, mean, std, crop=crop,
                                        antialias=True, **kw)


def _span(o, n_in, n_r):
    """(c, lo, size, inv) of resized coordinate ``o``, numpy float32."""
    r = f32(n_in / n_r)
    support = r if r >= 1 else f32(1)
    inv = f32(1.0 / float(r)) if r >= 1 else f32(1)
    c = (f32(o) + f32(0.5)) * r
    lo = min(max(int((c - support) + f32(0.5)), 0), n_in - 1)
    hi = min(int((c + support) + f32(0.5)), n_in)
    return c, lo, max(hi - lo, 1), inv


def _longest(n_out, offset, n_in, n_r):
    return max(_span(o, n_in, n_r)[2] for o in range(offset, offset + n_out))


def _axis(values, o, n_in, n_r):
    """One output coordinate of one axis: ``values[i]`` are fp32 arrays."""
    c, lo, size, inv = _span(o, n_in, n_r)
    acc = np.zeros_like(values[0], dtype=f32)
    tot = f32(0)
    for j in range(size):
        x = ((f32(lo + j) - c) + f32(0.5)) * inv
        w = max(f32(1) - abs(x), f32(0))
        acc = acc + w * values[lo + j]
        tot = tot + w
    assert acc.dtype == f32
    return acc / tot


def sequential_reference(x, size, crop=None):
    """The recipe tap by tap, sequentially, numpy float32: fp32 NHWC."""
    x = x.numpy()
    N, Hin, Win, C = x.shape
    Hr, Wr = size
    top, left, Hc, Wc = (0, 0, Hr, Wr) if crop is None else crop
    p = x.astype(f32)
    cols = [p[:, :, i, :] for i in range(Win)]               # [N,Hin,C] each
    h = np.stack([_axis(cols, left + ox, Win, Wr) for ox in range(Wc)],
                 axis=2)                                      # [N,Hin,Wc,C]
    rows = [h[:, i] for i in range(Hin)]                      # [N,Wc,C] each
    v = np.stack([_axis(rows, top + oy, Hin, Hr) for oy in range(Hc)],
                 axis=1)                                      # [N,Hc,Wc,C]
    scale = np.array([f32((1.0 / 255.0) / s) for s in STD[:C]], dtype=f32)
    bias = np.array([f32(-m / s) for m, s in zip(MEAN[:C], STD[:C])],
                    dtype=f32)
    y = (v * scale.reshape(1, 1, 1, C)) + bias.reshape(1, 1, 1, C)
    assert y.dtype == f32
    return torch.from_numpy(y)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape,size,crop", [
    ((2, 11, 13, 3), (4, 5), None),            # downscale on both axes
    ((1, 12, 16, 2), (6, 8), (1, 2, 4, 5)),    # crop offsets
    ((1, 5, 7, 1), (9, 12), None),             # upscale
    ((1, 10, 6, 4), (3, 11), None),            # down on one axis, up on other
], ids=str)
def test_cpu_op_is_the_sequential_recipe(shape, size, crop, dtype, layout):
    x = _pixels(shape, seed=1)
    y = _op(x, size, crop, out_dtype=DTYPES[dtype], layout=layout)
    ref = sequential_reference(x, size, crop)
    if layout == "nchw":
        ref = ref.permute(0, 3, 1, 2)
    ref = ref.to(DTYPES[dtype]).contiguous()
    assert y.dtype == DTYPES[dtype] and y.is_contiguous()
    assert tuple(y.shape) == tuple(ref.shape)
    assert torch.equal(y, ref)


@pytest.mark.parametrize("shape,size", [
    ((2, 37, 53, 3), (16, 20)),
    ((1, 480, 640, 3), (256, 341)),
    ((2, 33, 47, 4), (5, 3)),
    ((2, 20, 30, 1), (40, 45)),
    ((2, 9, 9, 3), (1, 1)),
    ((1, 17, 16384, 1), (3, 7)),               # 4682 taps per column
], ids=str)
def test_close_to_f_interpolate_antialias(shape, size):
    """Against ``F.interpolate(float input, antialias=True)`` with mean 0,
    std 1, pixel_scale 1. Both sides are weighted means of values up to 255
    over at most Kx (then Ky) taps; one rounding per product and per add on
    sums bounded by 255 * tot gives |diff| <= (Kx + Ky + 4) * 2^-23 * 255."""
    x = _pixels(shape, seed=2)
    C = shape[3]
    y = _op(x, size, mean=(0.0,) * C, std=(1.0,) * C, pixel_scale=1.0)
    ref = F.interpolate(x.permute(0, 3, 1, 2).float(), size=size,
                        mode="bilinear", align_corners=False, antialias=True)
    kx = _longest(size[1], 0, shape[2], size[1])
    ky = _longest(size[0], 0, shape[1], size[0])
    bound = (kx + ky + 4) * 2.0 ** -23 * 255
    diff = (y - ref).abs().max().item()
    print(f"{shape}->{size}: Kx={kx} Ky={ky} diff={diff:.3g} "
          f"bound={bound:.3g}")
    assert diff <= bound


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", [(2, 8, 8, 3), (1, 16, 16, 3),
                                   (2, 7, 9, 4), (1, 64, 64, 1)], ids=str)
def test_identity_size_equals_image_u8_to_float(shape, dtype, layout):
    if shape == (1, 16, 16, 3):                   # all 256 byte values
        x = (torch.arange(768) % 256).to(torch.uint8).view(shape)
    else:
        x = _pixels(shape, seed=3)
    C = shape[3]
    y = _op(x, shape[1:3], out_dtype=DTYPES[dtype], layout=layout)
    same = ops.image_u8_to_float(x, MEAN[:C], STD[:C],
                                 out_dtype=DTYPES[dtype], layout=layout)
    assert torch.equal(y, same)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_crop_equals_slice_of_uncropped(dtype, layout):
    x = _pixels((2, 48, 64, 3), seed=4)
    full = _op(x, (24, 32), out_dtype=DTYPES[dtype], layout=layout)
    part = _op(x, (24, 32), (4, 8, 16, 16), out_dtype=DTYPES[dtype],
               layout=layout)
    if layout == "nchw":
        assert torch.equal(part, full[:, :, 4:20, 8:24])
    else:
        assert torch.equal(part, full[:, 4:20, 8:24, :])
    x = _pixels((1, 37, 53, 3), seed=5)           # non-integer ratios
    full = _op(x, (16, 20), out_dtype=DTYPES[dtype], layout="nhwc")
    part = _op(x, (16, 20), (3, 7, 11, 9), out_dtype=DTYPES[dtype],
               layout="nhwc")
    assert torch.equal(part, full[:, 3:14, 7:16, :])


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_antialias_false_is_the_default(dtype, layout):
    x = _pixels((2, 37, 53, 3), seed=6)
    kw = dict(crop=(2, 3, 10, 12), out_dtype=DTYPES[dtype], layout=layout)
    plain = ops.image_u8_resize_to_float(x, (16, 20), MEAN[:3], STD[:3], **kw)
    off = ops.image_u8_resize_to_float(x, (16, 20), MEAN[:3], STD[:3],
                                       antialias=False, **kw)
    on = ops.image_u8_resize_to_float(x, (16, 20), MEAN[:3], STD[:3],
                                      antialias=True, **kw)
    assert torch.equal(plain, off)
    assert not torch.equal(plain, on)


def test_antialias_is_keyword_only():
    x = _pixels((1, 8, 8, 3))
    with pytest.raises(TypeError):
        ops.image_u8_resize_to_float(x, (4, 4), MEAN[:3], STD[:3], None,
                                     None, "nchw", 1.0 / 255.0, 0, True)


def test_downscaled_checkerboard_is_flat_grey():
    """A one-pixel checkerboard shrunk 4x: away from the border, where the
    filter window is whole and symmetric (8 taps per axis), the antialiased
    result is flat grey to rounding, (8 + 8 + 4) * 2^-23 * 255."""
    ij = torch.arange(16).view(16, 1) + torch.arange(16).view(1, 16)
    x = ((ij % 2) * 255).to(torch.uint8).view(1, 16, 16, 1)
    y = ops.image_u8_resize_to_float(x, (4, 4), (0.0,), (1.0,),
                                     pixel_scale=1.0, antialias=True)
    inner = y[0, 0, 1:3, 1:3]
    assert (inner - 127.5).abs().max().item() <= 20 * 2.0 ** -23 * 255


def test_empty_batch():
    x = torch.empty((0, 8, 8, 3), dtype=torch.uint8)
    y = _op(x, (4, 6), out_dtype=torch.bfloat16)
    assert y.shape == (0, 3, 4, 6) and y.dtype == torch.bfloat16
    y = _op(x, (4, 6), layout="nhwc")
    assert y.shape == (0, 4, 6, 3) and y.dtype == torch.float32


def test_rejected_inputs_raise_value_error():
    ok = _pixels((2, 4, 4, 3))
    m, s = MEAN[:3], STD[:3]

    def op(*a, **kw):
        return ops.image_u8_resize_to_float(*a, antialias=True, **kw)

    with pytest.raises(ValueError):
        op(ok.float(), (4, 4), m, s)
    with pytest.raises(ValueError):
        op(ok[0], (4, 4), m, s)
    with pytest.raises(ValueError):
        op(ok[..., :2], (4, 4), m[:2], s[:2])                 # strided
    with pytest.raises(ValueError):
        op(_pixels((1, 4, 4, 5)), (4, 4), (0.5,) * 5, (0.5,) * 5)
    with pytest.raises(ValueError):
        op(ok, (4, 4), m[:2], s[:2])
    with pytest.raises(ValueError):
        op(ok, (0, 4), m, s)
    with pytest.raises(ValueError):
        op(ok, (4, 16385), m, s)
    with pytest.raises(ValueError):
        op(ok, 4, m, s)
    with pytest.raises(ValueError):
        op(ok, (8, 8), m, s, crop=(0, 4, 8, 5))
    with pytest.raises(ValueError):
        op(ok, (8, 8), m, s, crop=(0, 0, 0, 4))
    with pytest.raises(ValueError):
        op(ok, (4, 4), m, s, out_dtype=torch.float64)
    with pytest.raises(ValueError):
        op(ok, (4, 4), m, s, layout="chwn")
    with pytest.raises(ValueError):
        op(torch.empty((1, 0, 4, 3), dtype=torch.uint8), (4, 4), m, s)


# ---------------------------------------------------------------------------
# plumbing: ImagePreprocess, the ResNet-50 servable, model.json
# ---------------------------------------------------------------------------

def test_image_preprocess_antialias_needs_resize_or_crop():
    with pytest.raises(ValueError, match="antialias"):
        ImagePreprocess(MEAN[:3], STD[:3], antialias=True)
    assert ImagePreprocess(MEAN[:3], STD[:3]).antialias is False
    assert ImagePreprocess(MEAN[:3], STD[:3], resize=8,
                           antialias=True).antialias is True
    assert ImagePreprocess(MEAN[:3], STD[:3], center_crop=4,
                           antialias=True).antialias is True


def test_image_preprocess_antialias_equals_direct_op():
    x = _pixels((2, 40, 60, 3), seed=7)
    pre = ImagePreprocess(MEAN[:3], STD[:3], out_dtype=torch.bfloat16,
                          resize=12, center_crop=(8, 10), antialias=True)
    direct = _op(x, (12, 18), (2, 4, 8, 10), out_dtype=torch.bfloat16)
    assert torch.equal(pre(x), direct)
    assert torch.equal(pre(x.numpy()), direct)
    off = ImagePreprocess(MEAN[:3], STD[:3], out_dtype=torch.bfloat16,
                          resize=12, center_crop=(8, 10))
    assert torch.equal(off(x), ops.image_u8_resize_to_float(
        x, (12, 18), MEAN[:3], STD[:3], crop=(2, 4, 8, 10),
        out_dtype=torch.bfloat16))
    assert not torch.equal(off(x), direct)


def test_resnet50_antialias_needs_resize_mode():
    for mode in ("float_nchw", "uint8_nhwc"):
        with pytest.raises(ValueError, match="antialias"):
            resnet50_servable(input_format=mode, antialias=True)
    with pytest.raises(ValueError, match="antialias"):
        resnet50_servable(antialias=True)


def test_resnet50_antialias_mode():
    s = resnet50_servable(input_format="uint8_nhwc_resize", antialias=True)
    pre = s.preprocess["images"]
    assert pre.antialias is True
    assert pre.resize == 256 and pre.center_crop == (224, 224)
    assert s.signature["inputs"]["images"] == (4, [-1, -1, -1, 3])
    plain = resnet50_servable(input_format="uint8_nhwc_resize")
    assert plain.preprocess["images"].antialias is False


def test_loader_passes_antialias(tmp_path):
    vdir = tmp_path / "m" / "1"
    vdir.mkdir(parents=True)
    (vdir / "model.json").write_text(json.dumps(
        {"family": "resnet50", "input_format": "uint8_nhwc_resize",
         "antialias": True}))
    s = default_loader("m", str(vdir))
    pre = s.preprocess["images"]
    assert pre.antialias is True
    assert pre.resize == 256 and pre.center_crop == (224, 224)
    x = _pixels((1, 300, 400, 3), seed=8)
    assert torch.equal(pre(x), ops.image_u8_resize_to_float(
        x, (256, 341), pre.mean, pre.std, crop=(16, 58, 224, 224),
        antialias=True))
    (vdir / "model.json").write_text(json.dumps(
        {"family": "resnet50", "antialias": True}))
    with pytest.raises(ValueError, match="antialias"):
        default_loader("m", str(vdir))
