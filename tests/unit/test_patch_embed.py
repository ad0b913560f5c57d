"""Fused ViT patch embedding, CPU side: the host fold against its fp64
definition, the eager CPU path on integer data (bit-exact), the fold algebra
end to end against ``VisionTransformer.embed`` on normalized input, the
ValueError cases, and the ViT servable / ``model.json`` plumbing.

Integer data: ``wk`` entries in [-4, 4] and integer bias / pos / cls keep
every partial sum an integer below 2**24, so fp32 arithmetic is exact in any
order and the int64 reference must be met bit for bit.

Fold algebra bound, per element, against the fp32 model on normalized input
(``a`` the bytes, ``w'`` the folded weights before rounding)::

    2**-9 * sum|a||w'| + (K + 2) * 2**-23 * sum|a||w'|

the bf16 unit roundoff on every folded weight, plus fp32 summation on both
sides."""
import json

import numpy as np
import pytest
import torch

from min_tfs_client_amd import ops
from min_tfs_client_amd.models import VitConfig, vit_b16, vit_b16_servable
from min_tfs_client_amd.preprocess import (IMAGENET_MEAN, IMAGENET_STD,
                                           PatchEmbedPreprocess)
from min_tfs_client_amd.repository import default_loader

TINY = dict(image_size=32, patch=16, hidden=32, layers=1, heads=2, mlp=64,
            num_classes=10)


def int_case(N, H, W, P, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    K, T = 3 * P * P, (H // P) * (W // P) + 1
    x = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=g)
    wk = torch.zeros((D, (K + 31) // 32 * 32), dtype=torch.bfloat16)
    wk[:, :K] = torch.randint(-4, 5, (D, K), generator=g).to(torch.bfloat16)
    bias, pos, cls = (torch.randint(-64, 65, s, generator=g).float()
                      for s in ((D,), (T, D), (D,)))
    return x, wk, bias, pos, cls


def int_reference(x, wk, bias, P, pos=None, cls=None):
    N, H, W, _ = x.shape
    K, D = 3 * P * P, wk.shape[0]
    a = x.view(N, H // P, P, W // P, P, 3).permute(0, 1, 3, 2, 4, 5).reshape(
        N, -1, K).long()
    y = a @ wk[:, :K].long().t() + bias.long()
    if cls is not None:
        y = torch.cat((cls.long().expand(N, 1, D), y), dim=1)
    return y if pos is None else y + pos.long()[-y.shape[1]:]


def test_fold_matches_fp64_definition():
    g = torch.Generator().manual_seed(1)
    w = torch.randn((48, 3, 14, 14), generator=g)
    b = torch.randn(48, generator=g)
    wk, bias_f = ops.patch_embed_fold(w, b, IMAGENET_MEAN, IMAGENET_STD)
    scale, bias_c = ops.normalization_constants(IMAGENET_MEAN, IMAGENET_STD)
    w64 = w.double().numpy()
    prod = (w64 * np.array(scale).reshape(1, 3, 1, 1)).transpose(
        0, 2, 3, 1).reshape(48, 588)
    mant, exp = np.frexp(prod)              # bf16: 8 bits, ties to even
    want = np.ldexp(np.rint(mant * 256.0), exp - 8)
    assert wk.dtype == torch.bfloat16 and tuple(wk.shape) == (48, 608)
    assert np.array_equal(wk[:, :588].double().numpy(), want)
    assert not wk[:, 588:].any()
    ref = b.double().numpy() + (
        w64 * np.array(bias_c).reshape(1, 3, 1, 1)).sum((1, 2, 3))
    assert bias_f.dtype == torch.float32
    assert np.all(np.abs(bias_f.double().numpy() - ref)
                  <= np.spacing(np.abs(ref).astype(np.float32)))


@pytest.mark.parametrize("P,H,W", [(16, 32, 48), (14, 28, 42), (32, 64, 32)])
@pytest.mark.parametrize("extras", [True, False])
def test_cpu_path_integer_data_bit_exact(P, H, W, extras):
    x, wk, bias, pos, cls = int_case(3, H, W, P, 16)
    if not extras:
        pos = cls = None
    out = ops.image_u8_patch_embed(x, wk, bias, P, pos, cls)
    assert out.dtype == torch.float32
    assert torch.equal(out, int_reference(x, wk, bias, P, pos, cls).float())
    assert ops.image_u8_patch_embed(x[:0], wk, bias, P, pos, cls).shape == \
        (0, out.shape[1], 16)


def test_preprocess_tokens_match_model_embed():
    torch.manual_seed(0)
    model = vit_b16(VitConfig(**TINY)).eval()
    pre = PatchEmbedPreprocess(
        model.patch_embed.weight, model.patch_embed.bias, IMAGENET_MEAN,
        IMAGENET_STD, pos_embed=model.pos_embed, cls_token=model.cls_token)
    x = torch.randint(0, 256, (2, 32, 32, 3), dtype=torch.uint8)
    tokens = pre(x.numpy())
    with torch.no_grad():
        want = model.embed(ops.image_u8_to_float(x, IMAGENET_MEAN,
                                                 IMAGENET_STD))
    scale, _ = ops.normalization_constants(IMAGENET_MEAN, IMAGENET_STD)
    K = 3 * 16 * 16
    w = model.patch_embed.weight.detach().double().abs() * \
        torch.tensor(scale, dtype=torch.float64).view(1, 3, 1, 1)
    a = x.view(2, 2, 16, 2, 16, 3).permute(0, 1, 3, 2, 4, 5).reshape(
        2, 4, K).double()
    mass = a @ w.permute(0, 2, 3, 1).reshape(-1, K).t()
    bound = (2.0 ** -9 + (K + 2) * 2.0 ** -23) * mass
    assert torch.equal(tokens[:, 0], want[:, 0])
    assert ((tokens[:, 1:] - want[:, 1:]).double().abs() <= bound).all()


def _bad_calls():
    x, wk, bias, pos, cls = int_case(1, 32, 32, 16, 16)
    good = dict(images=x, wk=wk, bias_f=bias, patch=16, pos_embed=pos,
                cls_token=cls)
    return {
        "dtype": dict(good, images=x.float()),
        "rank": dict(good, images=x[0]),
        "channels": dict(good, images=x[..., :2].contiguous()),
        "height": dict(good, images=x[:, :24].contiguous()),
        "width": dict(good, images=x[:, :, :24].contiguous()),
        "wk_dtype": dict(good, wk=wk.float()),
        "wk_shape": dict(good, wk=wk[:, :736].contiguous()),
        "width_not_16": dict(good, wk=wk[:8], bias_f=bias[:8],
                             pos_embed=None, cls_token=None),
        "bias_shape": dict(good, bias_f=bias[:8]),
        "pos_shape": dict(good, pos_embed=pos[1:]),
        "pos_without_cls": dict(good, cls_token=None),
        "cls_shape": dict(good, cls_token=cls[:8]),
        "non_contiguous": dict(good, images=x.transpose(1, 2)),
        "patch": dict(good, patch=8),
        "out_dtype": dict(good, out_dtype=torch.float64),
    }


@pytest.mark.parametrize("case", sorted(_bad_calls()))
def test_invalid_arguments_raise_value_error(case):
    with pytest.raises(ValueError):
        ops.image_u8_patch_embed(**_bad_calls()[case])


def test_servable_follows_load_state_dict_and_rejects_unknown_modes():
    s = vit_b16_servable(input_format="uint8_nhwc", config=VitConfig(**TINY))
    x = torch.randint(0, 256, (2, 32, 32, 3), dtype=torch.uint8)

    def direct():
        m = s.module
        wk, bias_f = ops.patch_embed_fold(
            m.patch_embed.weight, m.patch_embed.bias, IMAGENET_MEAN,
            IMAGENET_STD)
        tokens = ops.image_u8_patch_embed(
            x, wk, bias_f, 16, m.pos_embed.detach()[0].contiguous(),
            m.cls_token.detach().reshape(-1))
        with torch.no_grad():
            return m.forward_tokens(tokens)

    first = s({"images": x.numpy()})["logits"]
    assert torch.equal(first, direct())
    torch.manual_seed(7)
    s.module.load_state_dict(vit_b16(VitConfig(**TINY)).state_dict())
    second = s({"images": x.numpy()})["logits"]
    assert torch.equal(second, direct())        # a stale fold would fail here
    assert not torch.equal(first, second)
    with pytest.raises(ValueError):
        vit_b16_servable(input_format="uint8_nchw")
    with pytest.raises(ValueError):
        vit_b16_servable(output_format="probabilities")


def test_model_json_vit_family_answers(tmp_path):
    (tmp_path / "model.json").write_text(json.dumps(
        {"family": "vit_b16", "input_format": "uint8_nhwc",
         "output_format": "topk", "top_k": 3}))
    s = default_loader("vit", str(tmp_path))
    assert s.signature["inputs"] == {"images": (4, [-1, 224, 224, 3])}
    x = np.random.default_rng(0).integers(0, 256, (1, 224, 224, 3), np.uint8)
    out = s({"images": x})
    assert tuple(out["scores"].shape) == (1, 3)
    assert tuple(out["classes"].shape) == (1, 3)
