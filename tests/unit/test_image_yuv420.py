"""YUV 4:2:0 (NV12 / I420) image ingest on the CPU: the pinned integer
conversion (``ops.yuv420_to_rgb_u8``), the fused op's contract against the
two-step expression, validation, ``Yuv420ImagePreprocess``, the ResNet-50
``nv12_resize`` / ``i420_resize`` modes and the ``model.json`` key."""
import json

import numpy as np
import pytest
import torch

from min_tfs_client_amd import ops
from min_tfs_client_amd.models import resnet50_servable
from min_tfs_client_amd.preprocess import (IMAGENET_MEAN, IMAGENET_STD,
                                           ImagePreprocess,
                                           Yuv420ImagePreprocess)
from min_tfs_client_amd.repository import default_loader

MEAN, STD = IMAGENET_MEAN, IMAGENET_STD
CHROMAS = ["nv12", "i420"]
MATRICES = ["bt601", "bt709", "bt601_full"]

# (matrix, (Y,U,V), (R,G,B))
PINNED = [
    ("bt601", (16, 128, 128), (0, 0, 0)),
    ("bt601", (235, 128, 128), (255, 255, 255)),
    ("bt601", (81, 90, 240), (255, 0, 0)),
    ("bt601", (145, 54, 34), (0, 255, 1)),
    ("bt601", (255, 255, 255), (255, 125, 255)),
    ("bt601", (0, 0, 0), (0, 135, 0)),
    ("bt709", (81, 90, 240), (255, 24, 0)),
    ("bt709", (145, 54, 34), (0, 216, 0)),
    ("bt709", (255, 255, 255), (255, 183, 255)),
    ("bt709", (0, 0, 0), (0, 77, 0)),
    ("bt601_full", (16, 128, 128), (16, 16, 16)),
    ("bt601_full", (81, 90, 240), (238, 14, 14)),
    ("bt601_full", (145, 54, 34), (13, 238, 14)),
    ("bt601_full", (255, 255, 255), (255, 121, 255)),
    ("bt601_full", (0, 0, 0), (0, 136, 0)),
]


def pack(y, u, v, chroma):
    """Planes ``[N,H,W]``, ``[N,H/2,W/2]`` x2 (uint8 numpy) -> the frame
    batch ``[N,H*3/2,W]`` as a torch tensor."""
    n, h, w = y.shape
    if chroma == "nv12":
        c = np.stack([u, v], axis=-1).reshape(n, -1)
    else:
        c = np.concatenate([u.reshape(n, -1), v.reshape(n, -1)], axis=1)
    flat = np.concatenate([y.reshape(n, -1), c], axis=1).astype(np.uint8)
    return torch.from_numpy(flat.reshape(n, h * 3 // 2, w))


def planes(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, h, w), dtype=np.uint8),
            rng.integers(0, 256, (n, h // 2, w // 2), dtype=np.uint8),
            rng.integers(0, 256, (n, h // 2, w // 2), dtype=np.uint8))


def frames(n, h, w, chroma, seed=0):
    return pack(*planes(n, h, w, seed), chroma)


# ---------------------------------------------------------------------------
# the conversion
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("matrix,yuv,rgb", PINNED, ids=str)
def test_pinned_triples(matrix, yuv, rgb, chroma):
    y = np.full((1, 2, 2), yuv[0], dtype=np.uint8)
    u = np.full((1, 1, 1), yuv[1], dtype=np.uint8)
    v = np.full((1, 1, 1), yuv[2], dtype=np.uint8)
    out = ops.yuv420_to_rgb_u8(pack(y, u, v, chroma), chroma, matrix)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (1, 2, 2, 3)
    assert out.reshape(4, 3).tolist() == [list(rgb)] * 4


@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("matrix", MATRICES)
def test_gray_chroma_gives_gray_for_every_luma(matrix, chroma):
    y = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    c = np.full((1, 8, 8), 128, dtype=np.uint8)
    out = ops.yuv420_to_rgb_u8(pack(y, c, c, chroma), chroma, matrix)
    assert torch.equal(out[..., 0], out[..., 1])
    assert torch.equal(out[..., 1], out[..., 2])
    # monotonic in Y and reaching both clamps' side of the range
    gray = out[0, :, :, 0].reshape(-1).to(torch.int32)
    assert bool((gray[1:] >= gray[:-1]).all())
    assert int(gray[0]) == 0 and int(gray[-1]) == 255


@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("n,h,w", [(2, 4, 4), (2, 6, 10), (1, 2, 2),
                                   (3, 10, 6)], ids=str)
def test_i420_and_nv12_of_the_same_planes_agree(n, h, w, matrix):
    # (6,10), (10,6): H/2 odd (and W/2 odd), so the I420 chroma planes end in
    # the middle of a W-byte row
    y, u, v = planes(n, h, w, seed=3)
    a = ops.yuv420_to_rgb_u8(pack(y, u, v, "nv12"), "nv12", matrix)
    b = ops.yuv420_to_rgb_u8(pack(y, u, v, "i420"), "i420", matrix)
    assert torch.equal(a, b)


def _convert_numpy(y, u, v, matrix):
    yoff, yc, rv, gu, gv, bu = {
        "bt601": (16, 298, 409, -100, -208, 516),
        "bt709": (16, 298, 459, -55, -136, 541),
        "bt601_full": (0, 256, 359, -88, -183, 454)}[matrix]
    c = y.astype(np.int32) - yoff
    d = np.repeat(np.repeat(u.astype(np.int32) - 128, 2, axis=1), 2, axis=2)
    e = np.repeat(np.repeat(v.astype(np.int32) - 128, 2, axis=1), 2, axis=2)
    rgb = np.stack([yc * c + rv * e, yc * c + gu * d + gv * e,
                    yc * c + bu * d], axis=-1)
    return np.clip((rgb + 128) >> 8, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("matrix", MATRICES)
def test_conversion_matches_numpy_int32(matrix, chroma):
    y, u, v = planes(2, 6, 10, seed=4)
    out = ops.yuv420_to_rgb_u8(pack(y, u, v, chroma), chroma, matrix)
    assert np.array_equal(out.numpy(), _convert_numpy(y, u, v, matrix))


@pytest.mark.parametrize("chroma", CHROMAS)
def test_chroma_sample_of_a_pixel_is_y_half_x_half(chroma):
    y = np.full((1, 4, 4), 128, dtype=np.uint8)
    u = np.array([[[30, 90], [150, 210]]], dtype=np.uint8)
    v = np.array([[[200, 140], [80, 20]]], dtype=np.uint8)
    out = ops.yuv420_to_rgb_u8(pack(y, u, v, chroma), chroma)
    seen = set()
    for yy in range(4):
        for xx in range(4):
            one = pack(np.full((1, 2, 2), 128, dtype=np.uint8),
                       u[:, yy >> 1:(yy >> 1) + 1, xx >> 1:(xx >> 1) + 1],
                       v[:, yy >> 1:(yy >> 1) + 1, xx >> 1:(xx >> 1) + 1],
                       chroma)
            want = ops.yuv420_to_rgb_u8(one, chroma)[0, 0, 0]
            assert torch.equal(out[0, yy, xx], want)
            seen.add(tuple(want.tolist()))
    assert len(seen) == 4


# ---------------------------------------------------------------------------
# the fused op on the CPU path
# ---------------------------------------------------------------------------

RESIZE_CASES = [
    ((2, 8, 12), None, None),                        # identity (size=None)
    ((2, 8, 12), (8, 12), None),                     # identity
    ((2, 6, 10), (15, 23), None),                    # upscale
    ((2, 18, 26), (7, 9), None),                     # downscale
    ((2, 18, 26), (14, 20), (3, 5, 8, 11)),          # odd top and left
]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16,
                                   torch.float16], ids=str)
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("shape,size,crop", RESIZE_CASES, ids=str)
def test_fused_equals_two_step(shape, size, crop, chroma, dtype, layout):
    x = frames(*shape, chroma, seed=5)
    y = ops.image_yuv420_resize_to_float(
        x, size, MEAN, STD, crop=crop, out_dtype=dtype, layout=layout,
        chroma=chroma, matrix="bt709")
    rgb = ops.yuv420_to_rgb_u8(x, chroma, "bt709")
    want = ops.image_u8_resize_to_float(
        rgb, size or shape[1:], MEAN, STD, crop=crop, out_dtype=dtype,
        layout=layout)
    assert y.dtype == dtype and y.is_contiguous()
    assert torch.equal(y, want)


def test_identity_size_equals_image_u8_to_float():
    x = frames(2, 8, 12, "i420", seed=6)
    y = ops.image_yuv420_resize_to_float(x, None, MEAN, STD, chroma="i420")
    want = ops.image_u8_to_float(ops.yuv420_to_rgb_u8(x, "i420"), MEAN, STD)
    assert torch.equal(y, want)


@pytest.mark.parametrize("layout,shape", [("nchw", (0, 3, 5, 7)),
                                          ("nhwc", (0, 5, 7, 3))])
def test_empty_batch(layout, shape):
    x = torch.empty((0, 12, 8), dtype=torch.uint8)
    y = ops.image_yuv420_resize_to_float(x, (5, 7), MEAN, STD,
                                         out_dtype=torch.bfloat16,
                                         layout=layout)
    assert tuple(y.shape) == shape and y.dtype == torch.bfloat16
    assert tuple(ops.yuv420_to_rgb_u8(x).shape) == (0, 8, 8, 3)


def test_validation_errors():
    op = ops.image_yuv420_resize_to_float
    ok = torch.zeros((1, 6, 4), dtype=torch.uint8)
    op(ok, (4, 4), MEAN, STD)
    # 3 and 9 rows are frames of H = 2 and H = 6 (H/2 odd): valid
    op(torch.zeros((1, 3, 4), dtype=torch.uint8), (4, 4), MEAN, STD)
    op(torch.zeros((1, 9, 4), dtype=torch.uint8), (4, 4), MEAN, STD)
    for x in [
            ok.float(),                                           # dtype
            ok[0],                                                # rank 2
            ok[None],                                             # rank 4
            torch.zeros((1, 6, 8), dtype=torch.uint8)[:, :, :4],  # strided
            ok.numpy()]:                                          # no tensor
        with pytest.raises(ValueError):
            op(x, (4, 4), MEAN, STD)
    # rows not a multiple of 3: an odd H (10 rows would be H = 6.67, 7 or 8
    # rows are no whole frame either) is caught here, H = rows*2/3 is even
    # for every multiple of 3
    for rows in (4, 5, 7, 8, 10):
        with pytest.raises(ValueError, match="multiple of 3"):
            op(torch.zeros((1, rows, 4), dtype=torch.uint8), (4, 4), MEAN,
               STD)
    for w in (5, 7):
        with pytest.raises(ValueError, match="even"):
            op(torch.zeros((1, 6, w), dtype=torch.uint8), (4, 4), MEAN, STD)
    with pytest.raises(ValueError):                          # W too large
        op(torch.zeros((1, 3, 16386), dtype=torch.uint8), (4, 4), MEAN, STD)
    with pytest.raises(ValueError):                          # H too large
        op(torch.zeros((1, 24579, 2), dtype=torch.uint8), (4, 4), MEAN, STD)
    with pytest.raises(ValueError):                          # empty frame
        op(torch.zeros((1, 0, 4), dtype=torch.uint8), (4, 4), MEAN, STD)
    with pytest.raises(ValueError):
        op(torch.zeros((1, 6, 0), dtype=torch.uint8), (4, 4), MEAN, STD)
    for size in [(0, 4), (4, 16385), (4,), "ab", 4]:
        with pytest.raises(ValueError):
            op(ok, size, MEAN, STD)
    for crop in [(0, 4, 8, 5), (0, 0, 0, 4), (-1, 0, 4, 4), (0, 0, 9, 4),
                 (0, 0, 4)]:
        with pytest.raises(ValueError):
            op(ok, (8, 8), MEAN, STD, crop=crop)
    with pytest.raises(ValueError, match="chroma"):
        op(ok, (4, 4), MEAN, STD, chroma="nv21")
    with pytest.raises(ValueError, match="matrix"):
        op(ok, (4, 4), MEAN, STD, matrix="bt2020")
    with pytest.raises(ValueError, match="layout"):
        op(ok, (4, 4), MEAN, STD, layout="chwn")
    with pytest.raises(ValueError, match="out_dtype"):
        op(ok, (4, 4), MEAN, STD, out_dtype=torch.float64)
    with pytest.raises(ValueError):
        op(ok, (4, 4), MEAN[:2], STD[:2])
    with pytest.raises(ValueError):
        op(ok, (4, 4), MEAN + (0.5,), STD + (0.5,))
    with pytest.raises(ValueError):
        op(ok, (4, 4), MEAN, (0.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="chroma"):
        ops.yuv420_to_rgb_u8(ok, "yv12")
    with pytest.raises(ValueError, match="matrix"):
        ops.yuv420_to_rgb_u8(ok, "nv12", "rec709")
    with pytest.raises(ValueError):
        ops.yuv420_to_rgb_u8(ok.float())


# ---------------------------------------------------------------------------
# Yuv420ImagePreprocess
# ---------------------------------------------------------------------------

def test_preprocess_size_and_crop_rules_are_image_preprocess_rules():
    for kw in [dict(resize=8, center_crop=6), dict(resize=(9, 7)),
               dict(center_crop=(4, 6)), dict()]:
        pre = Yuv420ImagePreprocess(MEAN, STD, **kw)
        rgb = ImagePreprocess(MEAN, STD, **kw)
        for h, w in [(12, 20), (20, 12), (10, 10)]:
            size = pre.resized_size(h, w)
            assert size == rgb.resized_size(h, w)
            assert pre.crop_window(*size) == rgb.crop_window(*size)


@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("as_numpy", [False, True], ids=["torch", "numpy"])
def test_preprocess_equals_image_preprocess_on_converted_frames(chroma,
                                                                as_numpy):
    x = frames(2, 12, 20, chroma, seed=7)
    kw = dict(out_dtype=torch.bfloat16, resize=8, center_crop=6)
    pre = Yuv420ImagePreprocess(MEAN, STD, chroma=chroma, matrix="bt601_full",
                                **kw)
    y = pre(x.numpy() if as_numpy else x)
    want = ImagePreprocess(MEAN, STD, **kw)(
        ops.yuv420_to_rgb_u8(x, chroma, "bt601_full"))
    assert tuple(y.shape) == (2, 3, 6, 6) and y.dtype == torch.bfloat16
    assert torch.equal(y, want)


def test_preprocess_without_resize_normalizes_at_frame_size():
    x = frames(1, 4, 6, "nv12", seed=8)
    y = Yuv420ImagePreprocess(MEAN, STD, layout="nhwc")(x)
    assert torch.equal(y, ops.image_u8_to_float(
        ops.yuv420_to_rgb_u8(x), MEAN, STD, layout="nhwc"))


def test_preprocess_rejections():
    with pytest.raises(ValueError, match="chroma"):
        Yuv420ImagePreprocess(MEAN, STD, chroma="nv21")
    with pytest.raises(ValueError, match="matrix"):
        Yuv420ImagePreprocess(MEAN, STD, matrix="bt2020")
    with pytest.raises(ValueError, match="layout"):
        Yuv420ImagePreprocess(MEAN, STD, layout="hwc")
    with pytest.raises(ValueError):
        Yuv420ImagePreprocess(MEAN, (0.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        Yuv420ImagePreprocess(MEAN + (0.5,), STD + (0.5,))
    with pytest.raises(ValueError):
        Yuv420ImagePreprocess(MEAN, STD, resize=0)
    pre = Yuv420ImagePreprocess(MEAN, STD, resize=8, center_crop=6)
    for bad in [np.zeros((2, 12, 20, 3), np.uint8),      # RGB, rank 4
                np.zeros((12, 20), np.uint8),            # one frame, rank 2
                np.zeros((1, 13, 20), np.uint8),         # rows % 3
                np.zeros((1, 12, 21), np.uint8),         # odd W
                np.zeros((1, 0, 20), np.uint8),
                np.zeros((1, 12, 20), np.float32),
                np.array([[["a"]]])]:
        with pytest.raises(ValueError):
            pre(bad)
    with pytest.raises(ValueError, match="center_crop"):
        Yuv420ImagePreprocess(MEAN, STD, center_crop=9)(
            np.zeros((1, 12, 20), np.uint8))             # frame is 8 x 20


# ---------------------------------------------------------------------------
# resnet50_servable modes and the model.json key
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def resnet_i420():
    return resnet50_servable(input_format="i420_resize", yuv_matrix="bt709")


def test_resnet_yuv_signature_and_preprocess(resnet_i420):
    s = resnet_i420
    assert s.signature["inputs"] == {"images": (4, [-1, -1, -1])}
    assert s.signature["outputs"] == {"logits": (1, [-1, 1000])}
    pre = s.preprocess["images"]
    assert isinstance(pre, Yuv420ImagePreprocess)
    assert (pre.chroma, pre.matrix) == ("i420", "bt709")
    assert pre.resize == 256 and pre.center_crop == (224, 224)
    assert (pre.mean, pre.std) == (IMAGENET_MEAN, IMAGENET_STD)


def test_resnet_yuv_forward_equals_rgb_mode_on_converted_frames(resnet_i420):
    x = frames(1, 240, 320, "i420", seed=9)
    rgb = ops.yuv420_to_rgb_u8(x, "i420", "bt709")
    pre = resnet_i420.preprocess["images"](x)
    want = ImagePreprocess(IMAGENET_MEAN, IMAGENET_STD, resize=256,
                           center_crop=224)(rgb)
    assert tuple(pre.shape) == (1, 3, 224, 224)
    assert torch.equal(pre, want)
    out = resnet_i420({"images": x.numpy()})
    assert tuple(out["logits"].shape) == (1, 1000)
    assert bool(torch.isfinite(torch.as_tensor(out["logits"])).all())


def test_resnet_yuv_rejections():
    for mode in ("nv12_resize", "i420_resize"):
        with pytest.raises(ValueError, match="antialias"):
            resnet50_servable(input_format=mode, antialias=True)
        with pytest.raises(ValueError, match="matrix"):
            resnet50_servable(input_format=mode, yuv_matrix="bt2020")
    for mode in ("float_nchw", "uint8_nhwc", "uint8_nhwc_resize",
                 "uint8_ragged", "uint8_ragged_antialias"):
        with pytest.raises(ValueError, match="yuv_matrix"):
            resnet50_servable(input_format=mode, yuv_matrix="bt709")
    with pytest.raises(ValueError, match="input_format"):
        resnet50_servable(input_format="nv21_resize")


def _version_dir(tmp_path, cfg):
    vdir = tmp_path / "m" / "1"
    vdir.mkdir(parents=True)
    (vdir / "model.json").write_text(json.dumps(cfg))
    return str(vdir)


def test_loader_passes_yuv_matrix(tmp_path):
    s = default_loader("m", _version_dir(
        tmp_path, {"family": "resnet50", "input_format": "nv12_resize",
                   "yuv_matrix": "bt601_full"}))
    pre = s.preprocess["images"]
    assert isinstance(pre, Yuv420ImagePreprocess)
    assert (pre.chroma, pre.matrix) == ("nv12", "bt601_full")
    assert s.signature["inputs"] == {"images": (4, [-1, -1, -1])}


def test_loader_rejects_yuv_matrix_without_a_yuv_mode(tmp_path):
    with pytest.raises(ValueError, match="yuv_matrix"):
        default_loader("m", _version_dir(
            tmp_path, {"family": "resnet50", "yuv_matrix": "bt709"}))
