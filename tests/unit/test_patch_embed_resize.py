"""Resize + crop patch embedding, CPU side: the eager path against fp64
within the bound of tests/gpu/test_gpu_patch_embed_resize.py, the identity
size, ``N == 0``, the ValueError cases and the ``model.json`` plumbing."""
import json

import pytest
import torch

from min_tfs_client_amd import ops
from min_tfs_client_amd.preprocess import IMAGENET_MEAN, IMAGENET_STD
from min_tfs_client_amd.repository import default_loader

# (Hin, Win), size, crop
CASES = {
    "crop": ((37, 53), (40, 56), (4, 5, 32, 48)),
    "upscale": ((9, 7), (32, 32), None),
    "downscale": ((106, 159), (32, 48), None),
}


def case(hw=(37, 53), size=(40, 56), crop=(4, 5, 32, 48), N=2, P=16, D=32):
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 256, (N, *hw, 3), dtype=torch.uint8, generator=g)
    wk, bias_f = ops.patch_embed_fold(
        torch.randn((D, 3, P, P), generator=g), torch.randn(D, generator=g),
        IMAGENET_MEAN, IMAGENET_STD)
    return dict(images=x, size=size, wk=wk, bias_f=bias_f, patch=P, crop=crop)


def error_over_bound(out, images, size, wk, bias_f, patch, crop):
    v = ops.image_u8_resize_to_float(
        images, size, (0.0,) * 3, (1.0,) * 3, crop=crop, layout="nhwc",
        pixel_scale=1.0).double()
    N, H, W, _ = v.shape
    K = 3 * patch * patch
    a = v.view(N, H // patch, patch, W // patch, patch, 3).permute(
        0, 1, 3, 2, 4, 5).reshape(N, -1, K)
    ref = a @ wk.double().t() + bias_f.double()
    vw = a @ wk.double().abs().t()
    bound = (2 * K + 2) * 2.0 ** -23 * (1 + 2.0 ** -7) * (
        vw + bias_f.double().abs()) + 2.0 ** -16 * vw
    return ((out.double() - ref).abs() / bound).max().item()


@pytest.mark.parametrize("name", sorted(CASES))
def test_cpu_path_within_bound_of_fp64(name):
    c = case(*CASES[name])
    out = ops.image_u8_resize_patch_embed(**c)
    assert error_over_bound(out, **c) <= 1.0


def test_identity_size_equals_patch_embed():
    c = case((32, 48), (32, 48), None)
    pos, cls = torch.randn(7, 32), torch.randn(32)
    out = ops.image_u8_resize_patch_embed(
        **c, pos_embed=pos, cls_token=cls, out_dtype=torch.bfloat16)
    assert torch.equal(out, ops.image_u8_patch_embed(
        c["images"], c["wk"], c["bias_f"], 16, pos, cls, torch.bfloat16))


def test_empty_batch():
    c = case(N=0)
    out = ops.image_u8_resize_patch_embed(**c, cls_token=torch.zeros(32))
    assert out.shape == (0, 7, 32) and out.dtype == torch.float32


def _bad_calls():
    good = case()
    wk14, b14 = ops.patch_embed_fold(torch.randn(32, 3, 14, 14), None,
                                     IMAGENET_MEAN, IMAGENET_STD)
    return {
        "patch_14": dict(good, wk=wk14, bias_f=b14, patch=14,
                         crop=(0, 0, 28, 42)),
        "crop_not_multiple": dict(good, crop=(0, 0, 32, 40)),
        "crop_outside": dict(good, crop=(9, 5, 32, 48)),
        "size_zero": dict(good, size=(0, 56)),
        "size_too_large": dict(good, size=(40, 16385)),
        "wk_shape": dict(good, wk=good["wk"][:, :736].contiguous()),
        "pos_shape": dict(good, pos_embed=torch.zeros(7, 32)),
        "cls_shape": dict(good, cls_token=torch.zeros(16)),
    }


@pytest.mark.parametrize("name", sorted(_bad_calls()))
def test_invalid_arguments_raise_value_error(name):
    with pytest.raises(ValueError):
        ops.image_u8_resize_patch_embed(**_bad_calls()[name])


def test_model_json_reaches_the_vit_servable(tmp_path):
    (tmp_path / "model.json").write_text(json.dumps(
        {"family": "vit_b16", "input_format": "uint8_nhwc_resize"}))
    s = default_loader("vit", str(tmp_path))
    assert s.signature["inputs"] == {"images": (4, [-1, -1, -1, 3])}
    pre = s.preprocess["images"]
    assert (pre.resize, pre.center_crop) == (256, (224, 224))
