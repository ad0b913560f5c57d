"""Ragged patch embedding, CPU side: the op equals the per-image loop over
the dense op's eager path, one ValueError per validation rule, the per-image
windows of the hook and the servable's signature."""
import numpy as np
import pytest
import torch

from min_tfs_client_amd import ops
from min_tfs_client_amd.models import VitConfig, vit_b16_servable
from min_tfs_client_amd.preprocess import (IMAGENET_MEAN, IMAGENET_STD,
                                           RaggedImagePreprocess,
                                           RaggedResizePatchEmbedPreprocess)

SHAPES = [(37, 53), (9, 7), (106, 80)]
SIZES = [(40, 56), (32, 48), (53, 50)]
ORIGINS = [(4, 5), (0, 0), (21, 1)]


def case(D=32, P=16):
    g = torch.Generator().manual_seed(1)
    n = sum(h * w * 3 for h, w in SHAPES)
    wk, bias_f = ops.patch_embed_fold(
        torch.randn((D, 3, P, P), generator=g), torch.randn(D, generator=g),
        IMAGENET_MEAN, IMAGENET_STD)
    return dict(data=torch.randint(0, 256, (n,), dtype=torch.uint8,
                                   generator=g),
                shapes=SHAPES, sizes=SIZES, out_size=(32, 48), wk=wk,
                bias_f=bias_f, patch=P, origins=ORIGINS)


def test_cpu_op_equals_per_image_loop_and_empty_batch():
    c = case()
    pos, cls = torch.randn(7, 32), torch.randn(32)
    out = ops.image_u8_ragged_resize_patch_embed(
        **c, pos_embed=pos, cls_token=cls, out_dtype=torch.bfloat16)
    assert out.shape == (3, 7, 32)
    off = 0
    for i, (h, w) in enumerate(SHAPES):
        x = c["data"][off:off + h * w * 3].view(1, h, w, 3)
        off += h * w * 3
        assert torch.equal(out[i], ops.image_u8_resize_patch_embed(
            x, SIZES[i], c["wk"], c["bias_f"], 16, (*ORIGINS[i], 32, 48),
            pos, cls, torch.bfloat16)[0])
    empty = ops.image_u8_ragged_resize_patch_embed(
        **dict(c, data=c["data"][:0], shapes=[], sizes=(40, 56),
               origins=None), cls_token=cls)
    assert empty.shape == (0, 7, 32) and empty.dtype == torch.float32


def _bad_calls():
    good = case()
    wk14, b14 = ops.patch_embed_fold(torch.randn(32, 3, 14, 14), None,
                                     IMAGENET_MEAN, IMAGENET_STD)
    return {
        "patch_14": (dict(good, wk=wk14, bias_f=b14, patch=14,
                          out_size=(28, 42)), "patch"),
        "data_dtype": (dict(good, data=good["data"].float()), "uint8"),
        "data_rank": (dict(good, data=good["data"].view(1, -1)), "flat"),
        "shapes_rank": (dict(good, shapes=[37, 53]), "shapes"),
        "sizes_shape": (dict(good, sizes=SIZES[:2]), "sizes"),
        "origins_shape": (dict(good, origins=[(0, 0)] * 2), "origins"),
        "side_zero": (dict(good, sizes=[(40, 56), (0, 48), (53, 50)]),
                      "image 1"),
        "byte_count": (dict(good, shapes=[(37, 53), (9, 8), (106, 80)]),
                       r"bytes \(3 images"),
        "crop_outside": (dict(good, origins=[(4, 5), (0, 0), (22, 1)]),
                         "image 2"),
        "out_size_not_multiple": (dict(good, out_size=(32, 40)), "multiples"),
        "wk_shape": (dict(good, wk=good["wk"][:, :736].contiguous()), "wk"),
        "pos_shape": (dict(good, pos_embed=torch.zeros(7, 32)), "pos_embed"),
        "out_dtype": (dict(good, out_dtype=torch.float64), "out_dtype"),
    }


@pytest.mark.parametrize("name", sorted(_bad_calls()))
def test_invalid_arguments_raise_value_error(name):
    kwargs, word = _bad_calls()[name]
    with pytest.raises(ValueError, match=word):
        ops.image_u8_ragged_resize_patch_embed(**kwargs)


def test_hook_windows_are_those_of_ragged_image_preprocess():
    g = torch.Generator().manual_seed(2)
    w, b = torch.randn((32, 3, 16, 16), generator=g), torch.randn(32)
    pre = RaggedResizePatchEmbedPreprocess(
        w, b, IMAGENET_MEAN, IMAGENET_STD, resize=36, center_crop=32)
    shapes = [(50, 75), (90, 40), (36, 36)]
    data = torch.randint(0, 256, (sum(h * w * 3 for h, w in shapes),),
                         dtype=torch.uint8, generator=g)
    wk, bias_f = ops.patch_embed_fold(w, b, IMAGENET_MEAN, IMAGENET_STD)
    # the blends of the float hook under the same rule, split and embedded
    v = RaggedImagePreprocess((0.0,) * 3, (1.0,) * 3, layout="nhwc",
                              pixel_scale=1.0, resize=36,
                              center_crop=32)(data, shapes)
    hi = v.bfloat16().float()
    assert torch.equal(
        pre(data.numpy(), np.array(shapes, np.int32)),
        ops._patch_embed_eager(hi + (v - hi).bfloat16().float(), wk, bias_f,
                               16, None, None, torch.float32))
    crop_only = RaggedResizePatchEmbedPreprocess(
        w, b, IMAGENET_MEAN, IMAGENET_STD, center_crop=32)
    with pytest.raises(ValueError, match=r"image 1 \(20x90\)"):
        crop_only(torch.zeros((50 * 75 + 20 * 90) * 3, dtype=torch.uint8),
                  [(50, 75), (20, 90)])
    with pytest.raises(ValueError, match="one output size"):
        RaggedResizePatchEmbedPreprocess(w, b, IMAGENET_MEAN, IMAGENET_STD,
                                         resize=36)


def test_servable_signature_and_yuv_matrix_rejected():
    cfg = VitConfig(image_size=32, patch=16, hidden=32, layers=1, heads=2,
                    mlp=64, num_classes=10)
    s = vit_b16_servable(config=cfg, input_format="uint8_ragged")
    assert s.signature["inputs"] == {"images": (4, [-1]),
                                     "image_shapes": (3, [-1, 2])}
    pre = s.preprocess[("images", "image_shapes")]
    assert isinstance(pre, RaggedResizePatchEmbedPreprocess)
    assert (pre.resize, pre.center_crop) == (36, (32, 32))
    with pytest.raises(ValueError, match="yuv_matrix"):
        vit_b16_servable(config=cfg, input_format="uint8_ragged",
                         yuv_matrix="bt709")
