"""Fused bilinear resize + crop image ingest on CPU:
ops.image_u8_resize_to_float, ImagePreprocess(resize=, center_crop=), the
ResNet-50 ``uint8_nhwc_resize`` mode and its model.json key.

The reference is the pinned fp32 expression, written out here in numpy
float32 arithmetic (every operation rounds once) with constants rounded
through numpy.float32; it does not call the op's CPU path. Comparisons are
exact (torch.equal) except against F.interpolate, which differs by
rounding."""
import json

import grpc
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from min_tfs_client_amd import ops
from min_tfs_client_amd.client import TensorServingClient
from min_tfs_client_amd.models import resnet50_servable
from min_tfs_client_amd.preprocess import (IMAGENET_MEAN, IMAGENET_STD,
                                           ImagePreprocess)
from min_tfs_client_amd.repository import default_loader
from min_tfs_client_amd.server import ModelServer, Servable

MEAN = (0.485, 0.456, 0.406, 0.5)
STD = (0.229, 0.224, 0.225, 0.25)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16,
          "f16": torch.float16}
f32 = np.float32


def _taps(n_out, offset, n_in, n_resized):
    ratio = f32(n_in / n_resized)                # Python double, rounded once
    o = np.arange(offset, offset + n_out).astype(f32)
    s = np.maximum(((o + f32(0.5)) * ratio) - f32(0.5), f32(0))
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, s - i0.astype(f32)


def reference(x, size, crop=None, out_dtype=torch.float32, layout="nchw",
              mean=None, std=None, pixel_scale=1.0 / 255.0):
    x = x.cpu().numpy()
    _, Hin, Win, C = x.shape
    mean = MEAN[:C] if mean is None else mean
    std = STD[:C] if std is None else std
    Hr, Wr = size
    top, left, Hc, Wc = (0, 0, Hr, Wr) if crop is None else crop
    y0, y1, wy = _taps(Hc, top, Hin, Hr)
    x0, x1, wx = _taps(Wc, left, Win, Wr)
    p = x.astype(f32)
    wx = wx.reshape(1, 1, Wc, 1)
    wy = wy.reshape(1, Hc, 1, 1)
    r0, r1 = p[:, y0], p[:, y1]
    t = r0[:, :, x0] + wx * (r0[:, :, x1] - r0[:, :, x0])
    b = r1[:, :, x0] + wx * (r1[:, :, x1] - r1[:, :, x0])
    v = t + wy * (b - t)
    scale = np.array([f32(pixel_scale / s) for s in std], dtype=f32)
    bias = np.array([f32(-m / s) for m, s in zip(mean, std)], dtype=f32)
    y = (v * scale.reshape(1, 1, 1, C)) + bias.reshape(1, 1, 1, C)
    assert y.dtype == f32
    y = torch.from_numpy(y)
    if layout == "nchw":
        y = y.permute(0, 3, 1, 2)
    return y.to(out_dtype).contiguous()


def _pixels(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)


def _op(x, size, crop=None, **kw):
    C = x.shape[3]
    return ops.image_u8_resize_to_float(x, size, MEAN[:C], STD[:C],
                                        crop=crop, **kw)


# (input shape, size, crop)
CASES = [
    ((2, 8, 8, 3), (8, 8), None),
    ((2, 17, 31, 3), (8, 8), None),
    ((2, 7, 9, 3), (20, 33), None),
    ((1, 1, 5, 3), (4, 4), None),
    ((1, 5, 1, 3), (4, 12), None),
    ((2, 64, 64, 3), (3, 3), None),
    ((2, 37, 53, 3), (32, 46), (4, 11, 24, 24)),
    ((2, 16, 16, 1), (12, 20), None),
    ((2, 16, 16, 2), (12, 20), None),
    ((2, 16, 16, 4), (12, 20), (1, 2, 9, 17)),
]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape,size,crop", CASES, ids=str)
def test_cpu_op_matches_reference(shape, size, crop, dtype, layout):
    x = _pixels(shape)
    y = _op(x, size, crop, out_dtype=DTYPES[dtype], layout=layout)
    ref = reference(x, size, crop, DTYPES[dtype], layout)
    assert y.dtype == DTYPES[dtype] and y.is_contiguous()
    assert y.shape == ref.shape
    assert torch.equal(y, ref)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", [(2, 8, 8, 3), (3, 7, 9, 3), (2, 5, 6, 4),
                                   (1, 16, 16, 3)], ids=str)
def test_identity_size_equals_image_u8_to_float(shape, dtype, layout):
    if shape == (1, 16, 16, 3):                   # all 256 byte values
        x = (torch.arange(768) % 256).to(torch.uint8).view(shape)
    else:
        x = _pixels(shape, seed=1)
    C = shape[3]
    y = _op(x, shape[1:3], out_dtype=DTYPES[dtype], layout=layout)
    same = ops.image_u8_to_float(x, MEAN[:C], STD[:C],
                                 out_dtype=DTYPES[dtype], layout=layout)
    assert torch.equal(y, same)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_crop_equals_slice_of_uncropped(dtype):
    x = _pixels((2, 37, 53, 3), seed=2)
    full = _op(x, (32, 46), out_dtype=DTYPES[dtype])
    part = _op(x, (32, 46), (4, 11, 24, 24), out_dtype=DTYPES[dtype])
    assert torch.equal(part, full[:, :, 4:28, 11:35])
    full = _op(x, (32, 46), out_dtype=DTYPES[dtype], layout="nhwc")
    part = _op(x, (32, 46), (4, 11, 24, 24), out_dtype=DTYPES[dtype],
               layout="nhwc")
    assert torch.equal(part, full[:, 4:28, 11:35, :])


@pytest.mark.parametrize("shape,size", [
    ((2, 17, 31, 3), (8, 8)), ((2, 7, 9, 3), (20, 33)),
    ((1, 1, 5, 3), (4, 4)), ((1, 5, 1, 3), (4, 12)),
    ((2, 64, 64, 3), (3, 3)), ((2, 37, 53, 3), (32, 46)),
    ((1, 64, 48, 3), (24, 40)), ((1, 33, 64, 2), (64, 63)),
], ids=str)
def test_close_to_f_interpolate(shape, size):
    """Rounding differences only: coordinates are below 64, so a coordinate
    ulp is at most 2^-18 and moves a value by about 1e-3 levels; 2^-6 levels
    catches a wrong formula (align_corners, a missing half pixel), which is
    off by whole levels."""
    x = _pixels(shape, seed=3)
    C = shape[3]
    y = ops.image_u8_resize_to_float(x, size, (0.0,) * C, (1.0,) * C,
                                     pixel_scale=1.0)
    ref = F.interpolate(x.permute(0, 3, 1, 2).float(), size=size,
                        mode="bilinear", align_corners=False,
                        antialias=False)
    diff = float((y - ref).abs().max())
    print(f"{shape} -> {size}: max |diff| = {diff:.3e} levels")
    assert diff <= 2.0 ** -6


def test_empty_batch():
    x = torch.empty((0, 8, 8, 3), dtype=torch.uint8)
    y = _op(x, (4, 6), out_dtype=torch.bfloat16)
    assert y.shape == (0, 3, 4, 6) and y.dtype == torch.bfloat16
    y = _op(x, (4, 6), (1, 1, 2, 3), out_dtype=torch.float16, layout="nhwc")
    assert y.shape == (0, 2, 3, 3) and y.dtype == torch.float16


def test_rejected_inputs_raise_value_error():
    ok = _pixels((2, 4, 4, 3))
    m, s = MEAN[:3], STD[:3]
    op = ops.image_u8_resize_to_float
    with pytest.raises(ValueError):          # C > 4
        op(_pixels((1, 4, 4, 5)), (4, 4), (0.5,) * 5, (0.5,) * 5)
    with pytest.raises(ValueError):          # not uint8
        op(ok.float(), (4, 4), m, s)
    with pytest.raises(ValueError):          # signed bytes are not pixels
        op(ok.to(torch.int8), (4, 4), m, s)
    with pytest.raises(ValueError):          # rank 3
        op(ok[0], (4, 4), m, s)
    with pytest.raises(ValueError):          # rank 5
        op(ok[None], (4, 4), m, s)
    with pytest.raises(ValueError):          # non-contiguous
        op(_pixels((2, 3, 4, 4)).permute(0, 2, 3, 1), (4, 4), m, s)
    with pytest.raises(ValueError):          # len(mean) != C
        op(ok, (4, 4), MEAN[:2], s)
    with pytest.raises(ValueError):          # len(std) != C
        op(ok, (4, 4), m, STD[:4])
    with pytest.raises(ValueError):          # Hin == 0
        op(torch.empty((1, 0, 4, 3), dtype=torch.uint8), (4, 4), m, s)
    with pytest.raises(ValueError):          # Win == 0
        op(torch.empty((1, 4, 0, 3), dtype=torch.uint8), (4, 4), m, s)
    with pytest.raises(ValueError):          # Win > 16384
        op(torch.zeros((1, 1, 16385, 3), dtype=torch.uint8), (4, 4), m, s)
    with pytest.raises(ValueError):          # Hin > 16384
        op(torch.zeros((1, 16385, 1, 3), dtype=torch.uint8), (4, 4), m, s)
    for size in [(0, 4), (4, 0), (16385, 4), (4, 16385), (-1, 4), (4,), 4]:
        with pytest.raises(ValueError):
            op(ok, size, m, s)
    for crop in [(-1, 0, 2, 2), (0, -1, 2, 2), (3, 0, 6, 2), (0, 3, 2, 6),
                 (0, 0, 9, 2), (0, 0, 2, 9), (0, 0, 0, 2), (0, 0, 2, 0),
                 (0, 0, -2, 2), (0, 0, 2)]:
        with pytest.raises(ValueError):
            op(ok, (8, 8), m, s, crop=crop)
    with pytest.raises(ValueError):
        op(ok, (4, 4), m, s, layout="chwn")
    with pytest.raises(ValueError):
        op(ok, (4, 4), m, s, out_dtype=torch.float64)
    # the largest legal sides and a crop touching the far corner are fine
    y = op(torch.zeros((1, 1, 16384, 1), dtype=torch.uint8), (2, 16384),
           (0.0,), (1.0,), crop=(1, 16380, 1, 4))
    assert y.shape == (1, 1, 1, 4)


# ---------------------------------------------------------------------------
# ImagePreprocess
# ---------------------------------------------------------------------------

def _pre(**kw):
    return ImagePreprocess(MEAN[:3], STD[:3], **kw)


@pytest.mark.parametrize("hw,expected", [
    ((300, 200), (384, 256)),      # portrait: 256 * 300 // 200
    ((200, 300), (256, 384)),      # landscape
    ((256, 341), (256, 341)),
    ((341, 256), (341, 256)),
    ((100, 333), (256, 852)),      # 256 * 333 // 100 = 852 (852.48 floored)
    ((77, 77), (256, 256)),        # square
])
def test_shorter_side_arithmetic(hw, expected):
    assert _pre(resize=256).resized_size(*hw) == expected


def test_shorter_side_resize_and_center_crop_match_reference():
    pre = _pre(resize=12, center_crop=(8, 10), out_dtype=torch.bfloat16)
    for shape, size in [((2, 30, 20, 3), (18, 12)),     # portrait
                        ((2, 20, 30, 3), (12, 18)),     # landscape
                        ((1, 9, 9, 3), (12, 12))]:      # square
        x = _pixels(shape, seed=4)
        crop = ((size[0] - 8) // 2, (size[1] - 10) // 2, 8, 10)
        y = pre(x.numpy())
        assert y.shape == (shape[0], 3, 8, 10)
        assert torch.equal(y, reference(x, size, crop, torch.bfloat16))


def test_exact_resize_and_int_crop():
    x = _pixels((2, 17, 31, 3), seed=5)
    y = _pre(resize=(10, 12), center_crop=7, layout="nhwc")(x)
    assert torch.equal(
        y, reference(x, (10, 12), (1, 2, 7, 7), layout="nhwc"))
    y = _pre(resize=(10, 12))(x)                   # no crop: whole image
    assert torch.equal(y, reference(x, (10, 12)))


def test_center_crop_without_resize_crops_input_size():
    x = _pixels((2, 9, 12, 3), seed=6)
    y = _pre(center_crop=(4, 6))(x)
    plain = ops.image_u8_to_float(x, MEAN[:3], STD[:3])
    assert torch.equal(y, plain[:, :, 2:6, 3:9])


def test_crop_larger_than_resized_image_raises():
    pre = _pre(resize=8, center_crop=(8, 12))
    assert pre(_pixels((1, 10, 15, 3))).shape == (1, 3, 8, 12)
    with pytest.raises(ValueError, match="larger than the resized image"):
        pre(_pixels((1, 10, 14, 3)))              # resized to 8 x 11
    with pytest.raises(ValueError):
        _pre(center_crop=5)(_pixels((1, 4, 8, 3)))


def test_bad_constructor_arguments_raise():
    for kw in [{"resize": 0}, {"resize": -3}, {"resize": (4,)},
               {"resize": (4, 0)}, {"resize": 2.5}, {"resize": "256"},
               {"resize": (4, 5, 6)}, {"center_crop": 0},
               {"center_crop": (0, 4)}, {"center_crop": (4, 4, 4)},
               {"center_crop": 1.5}, {"resize": True}]:
        with pytest.raises(ValueError):
            _pre(**kw)


def test_defaults_leave_image_preprocess_unchanged(monkeypatch):
    pre = _pre(out_dtype=torch.float16)
    assert pre.resize is None and pre.center_crop is None

    def boom(*a, **k):
        raise AssertionError("the resize op must not run by default")

    monkeypatch.setattr(ops, "image_u8_resize_to_float", boom)
    x = _pixels((2, 6, 7, 3), seed=7)
    y = pre(x.numpy())
    assert torch.equal(y, ops.image_u8_to_float(
        x, MEAN[:3], STD[:3], out_dtype=torch.float16))
    with pytest.raises(ValueError):
        pre(x.float())


# ---------------------------------------------------------------------------
# ResNet-50 resize mode (the 224x224 model itself is not run on CPU)
# ---------------------------------------------------------------------------

class _Capture(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.seen = None

    def forward(self, x):
        self.seen = x
        return torch.zeros(x.shape[0], 1000, dtype=x.dtype)


def test_resnet50_resize_mode():
    s = resnet50_servable(input_format="uint8_nhwc_resize")
    assert s.signature["inputs"]["images"] == (4, [-1, -1, -1, 3])
    assert s.signature["outputs"]["logits"] == (1, [-1, 1000])
    cap = _Capture()
    s.module = cap
    for shape, size in [((2, 160, 200, 3), (256, 320)),
                        ((1, 300, 256, 3), (300, 256))]:
        x = _pixels(shape, seed=8)
        out = s({"images": x.numpy()})
        assert out["logits"].shape == (shape[0], 1000)
        assert out["logits"].dtype == torch.float32
        crop = ((size[0] - 224) // 2, (size[1] - 224) // 2, 224, 224)
        assert torch.equal(cap.seen, reference(
            x, size, crop, mean=IMAGENET_MEAN, std=IMAGENET_STD))
    with pytest.raises(ValueError, match="resized height"):
        # 1000 x 10 -> 25600 x 256: past the 16384 limit of the op
        s({"images": _pixels((1, 1000, 10, 3)).numpy()})


def test_resnet50_unknown_mode_lists_all_three():
    with pytest.raises(ValueError) as ei:
        resnet50_servable(input_format="uint8_nchw")
    for mode in ("float_nchw", "uint8_nhwc", "uint8_nhwc_resize"):
        assert repr(mode) in str(ei.value)


def test_loader_passes_resize_input_format(tmp_path):
    vdir = tmp_path / "m" / "1"
    vdir.mkdir(parents=True)
    (vdir / "model.json").write_text(json.dumps(
        {"family": "resnet50", "input_format": "uint8_nhwc_resize"}))
    s = default_loader("m", str(vdir))
    assert s.signature["inputs"] == {"images": (4, [-1, -1, -1, 3])}
    pre = s.preprocess["images"]
    assert pre.resize == 256 and pre.center_crop == (224, 224)


# ---------------------------------------------------------------------------
# end to end over a unix socket, python server
# ---------------------------------------------------------------------------

def test_crop_too_large_is_invalid_argument(sock_dir):
    addr = f"unix://{sock_dir}/resize.sock"
    pre = _pre(resize=8, center_crop=(8, 12))
    servable = Servable(lambda inputs: {"images": inputs["images"]},
                        preprocess={"images": pre})
    with ModelServer(address=addr, transport="grpcio") as srv:
        srv.manager.load("pre", servable, version=1)
        with TensorServingClient("unix", f"//{sock_dir}/resize.sock",
                                 backend="grpcio") as client:
            x = _pixels((1, 10, 15, 3))
            resp = client.predict_request("pre", {"images": x.numpy()},
                                          timeout=20)
            assert list(resp.outputs["images"].tensor_shape.dim)[3].size == 12
            with pytest.raises(grpc.RpcError) as ei:
                client.predict_request(
                    "pre", {"images": _pixels((1, 10, 14, 3)).numpy()},
                    timeout=20)
            assert ei.value.code() == grpc.StatusCode.INVALID_ARGUMENT
