"""Fused uint8 patch-embedding MFMA kernel on the GPU.

Bit-exact cases: random uint8 pixels, ``wk`` with integer entries in
[-4, 4] (exact in bf16) and integer bias / pos / cls. Every partial sum is an
integer below 3072*255*4 + small < 2**24, so fp32 accumulation is exact in
any order and under any rounding mode; the reference is an int64 matmul over
the unfolded bytes, converted with ``.to(out_dtype)``, compared with
``torch.equal``. (The one case at the tile-rule threshold needs 3e9
multiply-adds and runs the same reference in float64, still exact.)

Shapes are the smallest that reach each path of the kernel header: one
patch; a tile spanning three images; P = 14 (K = 588, 2-byte loads, a K tail
whose weight columns are set non-zero here, so only a zero-filled A tail
gives the right integer, inside a buffer of 255s); P = 32 (K = 3072); one
token past kPeSmallM = 32 / kPeLargeM = 128 with D one 16-step past
kPeSmallN = 32 / kPeLargeN = 128; and ceil(M/128) * ceil(D/128) = 272 >= 256
large tiles, the rule's threshold (which tile the rule picked is not
observable: the case shows that the rule and the forced large tile are both
right there). ``ops._image_u8_patch_embed(..., tile)`` forces a tile (1 small,
2 large; 0 is the rule).

Folded real weights against fp64, fp32 output, per element::

    |out - ref| <= (K + 2) * 2**-23 * (sum_k |a_k||wk_k| + |bias_f|)

bf16 products are exact in fp32, each of at most K + 1 additions errs by at
most one ulp of a partial sum under any faithful rounding, and the last unit
covers the output conversion. Largest observed ratio to this bound on an
MI355X: see docs/test_matrix.md."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from min_tfs_client_amd import ops  # noqa: E402
from min_tfs_client_amd.models import (VitConfig, vit_b16,  # noqa: E402
                                       vit_b16_servable)
from min_tfs_client_amd.preprocess import (IMAGENET_MEAN,  # noqa: E402
                                           IMAGENET_STD)

DEV = "cuda:0"
# (P, N, H, W, D)
CASES = {
    "one_patch": (16, 1, 16, 16, 16),
    "three_images": (16, 3, 32, 48, 48),
    "p14": (14, 2, 28, 42, 32),
    "p32": (32, 1, 64, 32, 16),
    "past_small_tile": (16, 33, 16, 16, 48),
    "past_large_tile": (16, 129, 16, 16, 144),
}


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.require_native()


def int_case(P, N, H, W, D, seed=0):
    """Device operands; the images are a view into a buffer of 255s and the
    K-tail columns of wk are 3, not 0."""
    g = torch.Generator().manual_seed(seed)
    K, T = 3 * P * P, (H // P) * (W // P) + 1
    n = N * H * W * 3
    buf = torch.full((n + 4096,), 255, dtype=torch.uint8)
    buf[:n] = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
    wk = torch.full((D, (K + 31) // 32 * 32), 3, dtype=torch.bfloat16)
    wk[:, :K] = torch.randint(-4, 5, (D, K), generator=g).to(torch.bfloat16)
    bias, pos, cls = (torch.randint(-64, 65, s, generator=g).float().to(DEV)
                      for s in ((D,), (T, D), (D,)))
    return buf.to(DEV)[:n].view(N, H, W, 3), wk.to(DEV), bias, pos, cls


def int_reference(x, wk, bias, P, pos=None, cls=None, dtype=torch.int64):
    N, H, W, _ = x.shape
    K, D = 3 * P * P, wk.shape[0]
    a = x.cpu().view(N, H // P, P, W // P, P, 3).permute(
        0, 1, 3, 2, 4, 5).reshape(N, -1, K).to(dtype)
    y = a @ wk.cpu()[:, :K].to(dtype).t() + bias.cpu().to(dtype)
    if cls is not None:
        y = torch.cat((cls.cpu().to(dtype).expand(N, 1, D), y), dim=1)
    return y if pos is None else y + pos.cpu().to(dtype)[-y.shape[1]:]


@pytest.mark.parametrize("tile", [0, 1, 2])
@pytest.mark.parametrize("case", sorted(CASES))
def test_integer_data_bit_exact(case, tile):
    P = CASES[case][0]
    x, wk, bias, pos, cls = int_case(*CASES[case])
    out = ops._image_u8_patch_embed(x, wk, bias, P, pos, cls, None, tile)
    assert out.dtype == torch.float32 and out.is_cuda
    want = int_reference(x, wk, bias, P, pos, cls).float()
    assert torch.equal(out.cpu(), want)
    again = ops._image_u8_patch_embed(x, wk, bias, P, pos, cls, None, tile)
    assert torch.equal(out, again)                       # deterministic


@pytest.mark.parametrize("with_pos,with_cls", [(False, False), (True, False),
                                               (False, True)])
def test_optional_class_token_and_position(with_pos, with_cls):
    P = 16
    x, wk, bias, pos, cls = int_case(*CASES["three_images"])
    cls = cls if with_cls else None
    pos = (pos if with_cls else pos[1:].contiguous()) if with_pos else None
    out = ops.image_u8_patch_embed(x, wk, bias, P, pos, cls)
    want = int_reference(x, wk, bias, P, pos, cls).float()
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16,
                                   torch.float16])
def test_output_dtypes_round_once(dtype):
    P = 16
    x, wk, bias, pos, cls = int_case(*CASES["three_images"])
    out = ops.image_u8_patch_embed(x, wk, bias, P, pos, cls, out_dtype=dtype)
    assert out.dtype == dtype
    want = int_reference(x, wk, bias, P, pos, cls).to(dtype)
    assert torch.equal(out.cpu(), want)


def test_correct_at_the_rule_threshold():
    # 16 x 17 = 272 large tiles: the rule and the forced large tile
    P, shape = 16, (16, 16 * 128 - 127, 16, 16, 16 * 128 + 16)
    x, wk, bias, pos, cls = int_case(*shape)
    want = int_reference(x, wk, bias, P, pos, cls, torch.float64).float()
    for tile in (0, 2):
        out = ops._image_u8_patch_embed(x, wk, bias, P, pos, cls, None,
                                        tile)
        assert torch.equal(out.cpu(), want)


def test_folded_real_weights_within_fp32_bound(capsys):
    P, D, K = 16, 64, 768
    g = torch.Generator().manual_seed(3)
    w = torch.randn((D, 3, P, P), generator=g)
    b = torch.randn(D, generator=g)
    x = torch.randint(0, 256, (2, 32, 32, 3), dtype=torch.uint8, generator=g)
    wk, bias_f = ops.patch_embed_fold(w, b, IMAGENET_MEAN, IMAGENET_STD)
    out = ops.image_u8_patch_embed(x.to(DEV), wk.to(DEV), bias_f.to(DEV), P)
    a = x.view(2, 2, P, 2, P, 3).permute(0, 1, 3, 2, 4, 5).reshape(
        2, 4, K).double()
    ref = a @ wk.double().t() + bias_f.double()
    mass = a @ wk.double().abs().t() + bias_f.double().abs()
    ratio = ((out.cpu().double() - ref).abs()
             / ((K + 2) * 2.0 ** -23 * mass)).max().item()
    with capsys.disabled():
        print(f"\npatch_embed fp64 check: largest error / bound = {ratio:.4f}")
    assert ratio <= 1.0


def test_servable_runs_kernel_and_follows_load_state_dict():
    cfg = dict(image_size=32, patch=16, hidden=32, layers=1, heads=2, mlp=64,
               num_classes=10)
    s = vit_b16_servable(DEV, torch.bfloat16, input_format="uint8_nhwc",
                         config=VitConfig(**cfg))
    x = torch.randint(0, 256, (2, 32, 32, 3), dtype=torch.uint8)

    def direct():
        m = s.module
        wk, bias_f = ops.patch_embed_fold(
            m.patch_embed.weight, m.patch_embed.bias, IMAGENET_MEAN,
            IMAGENET_STD)
        tokens = ops.image_u8_patch_embed(
            x.to(DEV), wk, bias_f, 16,
            m.pos_embed.detach().float()[0].contiguous(),
            m.cls_token.detach().float().reshape(-1),
            out_dtype=torch.bfloat16)
        with torch.no_grad():
            return m.forward_tokens(tokens).float()

    first = s({"images": x.numpy()})["logits"]
    assert first.is_cuda and torch.equal(first, direct())
    torch.manual_seed(7)
    s.module.load_state_dict(vit_b16(VitConfig(**cfg)).state_dict())
    second = s({"images": x.numpy()})["logits"]
    assert torch.equal(second, direct())        # a stale fold would fail here
    assert not torch.equal(first, second)
