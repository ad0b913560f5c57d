"""Antialiased resize of YUV 4:2:0 (NV12 / I420) frames on the CPU: the fused
op's ``antialias=True`` contract against the two-step expression
(``ops.yuv420_to_rgb_u8`` then ``ops.image_u8_resize_to_float(...,
antialias=True)``), ``Yuv420ImagePreprocess(antialias=True)``, the ResNet-50
``nv12_resize_antialias`` / ``i420_resize_antialias`` modes and the
``model.json`` key."""
import json

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
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
AA_MODES = {"nv12_resize_antialias": "nv12", "i420_resize_antialias": "i420"}


def frames(n, h, w, seed=0):
    # any bytes are a valid frame in either chroma layout
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h * 3 // 2, w), dtype=torch.uint8,
                         generator=g)


@pytest.mark.parametrize("crop", [None, (3, 5, 9, 12)], ids=str)
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("chroma", CHROMAS)
def test_op_equals_two_step_expression(chroma, matrix, crop):
    x = frames(2, 38, 54, seed=1)
    rgb = ops.yuv420_to_rgb_u8(x, chroma, matrix)
    for out_dtype in DTYPES:
        for layout in ("nchw", "nhwc"):
            got = ops.image_yuv420_resize_to_float(
                x, (16, 20), MEAN, STD, crop, out_dtype, layout, 1.0 / 255.0,
                chroma=chroma, matrix=matrix, antialias=True)
            want = ops.image_u8_resize_to_float(
                rgb, (16, 20), MEAN, STD, crop, out_dtype, layout,
                1.0 / 255.0, antialias=True)
            assert got.dtype == out_dtype
            assert torch.equal(got, want)
    # and the filter really is the antialiased one
    bilinear = ops.image_yuv420_resize_to_float(
        x, (16, 20), MEAN, STD, crop, chroma=chroma, matrix=matrix)
    aa = ops.image_yuv420_resize_to_float(
        x, (16, 20), MEAN, STD, crop, chroma=chroma, matrix=matrix,
        antialias=True)
    assert not torch.equal(aa, bilinear)


@pytest.mark.parametrize("chroma", CHROMAS)
def test_identity_size_equals_plain_normalize(chroma):
    x = frames(2, 8, 16, seed=2)
    rgb = ops.yuv420_to_rgb_u8(x, chroma, "bt709")
    for out_dtype in DTYPES:
        got = ops.image_yuv420_resize_to_float(
            x, None, MEAN, STD, out_dtype=out_dtype, chroma=chroma,
            matrix="bt709", antialias=True)
        want = ops.image_u8_to_float(rgb, MEAN, STD, out_dtype=out_dtype)
        assert torch.equal(got, want)


def test_antialias_is_keyword_only_and_empty_batch():
    x = frames(1, 8, 16)
    with pytest.raises(TypeError):
        ops.image_yuv420_resize_to_float(
            x, (4, 8), MEAN, STD, None, None, "nchw", 1.0 / 255.0, 0, "nv12",
            "bt601", True)
    y = ops.image_yuv420_resize_to_float(x[:0], (4, 8), MEAN, STD,
                                         antialias=True)
    assert tuple(y.shape) == (0, 3, 4, 8)
    with pytest.raises(ValueError):
        ops.image_yuv420_resize_to_float(x, (8, 8), MEAN, STD,
                                         crop=(0, 4, 8, 5), antialias=True)


@pytest.mark.parametrize("chroma", CHROMAS)
def test_preprocess_equals_rgb_preprocess_on_converted_frames(chroma):
    x = frames(2, 40, 64, seed=3)
    pre = Yuv420ImagePreprocess(MEAN, STD, out_dtype=torch.bfloat16,
                                resize=16, center_crop=12, chroma=chroma,
                                matrix="bt601_full", antialias=True)
    assert pre.antialias is True
    assert Yuv420ImagePreprocess(MEAN, STD).antialias is False
    want = ImagePreprocess(MEAN, STD, out_dtype=torch.bfloat16, resize=16,
                           center_crop=12, antialias=True)(
        ops.yuv420_to_rgb_u8(x, chroma, "bt601_full"))
    got = pre(x.numpy())
    assert tuple(got.shape) == (2, 3, 12, 12)
    assert torch.equal(got, want)


def test_preprocess_antialias_needs_resize_or_crop():
    with pytest.raises(ValueError, match="antialias"):
        Yuv420ImagePreprocess(MEAN, STD, antialias=True)
    Yuv420ImagePreprocess(MEAN, STD, center_crop=4, antialias=True)
    Yuv420ImagePreprocess(MEAN, STD, resize=8, antialias=True)


# ---------------------------------------------------------------------------
# resnet50_servable modes and the model.json key
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(AA_MODES))
def test_resnet_yuv_antialias_modes_answer(mode):
    s = resnet50_servable(input_format=mode, yuv_matrix="bt709")
    assert s.signature["inputs"] == {"images": (4, [-1, -1, -1])}
    pre = s.preprocess["images"]
    assert isinstance(pre, Yuv420ImagePreprocess)
    assert (pre.chroma, pre.matrix) == (AA_MODES[mode], "bt709")
    assert pre.antialias is True
    assert pre.resize == 256 and pre.center_crop == (224, 224)
    x = frames(1, 240, 320, seed=4)
    want = ImagePreprocess(MEAN, STD, resize=256, center_crop=224,
                           antialias=True)(
        ops.yuv420_to_rgb_u8(x, AA_MODES[mode], "bt709"))
    assert torch.equal(pre(x), want)
    out = s({"images": x.numpy()})
    assert tuple(out["logits"].shape) == (1, 1000)
    assert bool(torch.isfinite(torch.as_tensor(out["logits"])).all())


def test_resnet_rejections():
    for mode in AA_MODES:
        with pytest.raises(ValueError, match="antialias"):
            resnet50_servable(input_format=mode, antialias=True)
        with pytest.raises(ValueError, match="matrix"):
            resnet50_servable(input_format=mode, yuv_matrix="bt2020")
    # the bilinear modes point at their antialiased counterparts
    for chroma in CHROMAS:
        with pytest.raises(ValueError,
                           match=f"{chroma}_resize_antialias"):
            resnet50_servable(input_format=f"{chroma}_resize",
                              antialias=True)
    for mode in ("float_nchw", "uint8_nhwc", "uint8_nhwc_resize",
                 "uint8_ragged", "uint8_ragged_antialias"):
        with pytest.raises(ValueError, match="yuv_matrix"):
            resnet50_servable(input_format=mode, yuv_matrix="bt709")


def test_loader_accepts_the_antialiased_yuv_mode(tmp_path):
    vdir = tmp_path / "m" / "1"
    vdir.mkdir(parents=True)
    (vdir / "model.json").write_text(json.dumps(
        {"family": "resnet50", "input_format": "i420_resize_antialias",
         "yuv_matrix": "bt709"}))
    s = default_loader("m", str(vdir))
    pre = s.preprocess["images"]
    assert isinstance(pre, Yuv420ImagePreprocess)
    assert (pre.chroma, pre.matrix, pre.antialias) == ("i420", "bt709", True)
