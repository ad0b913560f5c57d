"""Resampling (resize + crop) loader of the patch-embedding MFMA kernel on
the GPU. ``tile`` 0 is the kernel's rule, 1 the small tile, 2 the large one
(64 x 128 for this loader).

Bit-exact cases. Identity size: the taps weigh 0, ``lo`` is 0 and the result
is that of ``ops._image_u8_patch_embed``. Exact 2:1 downscale: every tap
weight is 0.5, so the blend ``v`` is a multiple of 1/4 below 256 (checked in
the test); with ``wk`` integers in [-4, 4] and integer bias / pos / cls every
partial sum is a multiple of 1/4 below 3072*257*4 < 2**22, so fp32
accumulation is exact in any order and the reference is a float64 matmul over
the blends of the CPU resize op.

Folded real weights against fp64, ``v`` from the CPU resize op, ``mass =
sum |v||wk| + |bias_f|``: ``|out - ref| <= (2K + 2) * 2**-23 * (1 + 2**-7) *
mass + 2**-16 * sum |v||wk|``: 2K + 1 additions of exact bf16 products, each
within one ulp of a partial sum bounded by ``(1 + 2**-7) * mass``, one ulp for
the conversion, and the split error ``|v - (hi + lo)| <= 2**-16 |v|``.
Largest observed ratio on an MI355X: see docs/test_matrix.md."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from min_tfs_client_amd import ops  # noqa: E402
from min_tfs_client_amd.models import (VitConfig, vit_b16,  # noqa: E402
                                       vit_b16_servable)
from min_tfs_client_amd.preprocess import (IMAGENET_MEAN,  # noqa: E402
                                           IMAGENET_STD)

DEV = "cuda:0"
TILES = [0, 1, 2]
# exact 2:1 downscale: (P, N, resized (Hr, Wr), D, crop)
HALF = {
    "one_patch": (16, 1, (16, 16), 16, None),
    "three_images": (16, 3, (32, 48), 48, None),
    "p32": (32, 1, (64, 32), 16, None),
    "past_small_tile": (16, 33, (16, 16), 48, None),
    "past_large_tile": (16, 65, (16, 16), 144, None),
    "odd_crop": (16, 2, (40, 56), 48, (3, 5, 32, 48)),
}
# fp64 bound: (Hin, Win), size, crop; the last one is smaller than a gather
BOUND = {
    "crop": ((37, 53), (40, 56), (4, 5, 32, 48)),
    "upscale": ((9, 7), (32, 32), None),
    "downscale": ((106, 159), (32, 48), None),
    "one_pixel": ((1, 1), (16, 16), None),
}


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.require_native()


def make_case(P, N, hw, D, tokens, integer, seed=0):
    """Device operands; the images are a view into a buffer of 255s."""
    g = torch.Generator().manual_seed(seed)
    n, K = N * hw[0] * hw[1] * 3, 3 * P * P
    buf = torch.full((n + 4096,), 255, dtype=torch.uint8)
    buf[:n] = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
    shapes = ((D, K), (D,), (tokens + 1, D), (D,))
    if integer:
        wk, bias, pos, cls = (
            torch.randint(-m, m + 1, s, generator=g).float()
            for m, s in zip((4, 64, 64, 64), shapes))
    else:
        wk, bias, pos, cls = (torch.randn(s, generator=g) for s in shapes)
    return (buf.to(DEV)[:n].view(N, *hw, 3), wk.to(torch.bfloat16).to(DEV),
            bias.to(DEV), pos.to(DEV), cls.to(DEV))


def blends(x, size, crop, P):
    """fp64 ``[N, tokens, K]`` blends of the CPU resize op."""
    v = ops.image_u8_resize_to_float(
        x.cpu(), size, (0.0,) * 3, (1.0,) * 3, crop=crop, layout="nhwc",
        pixel_scale=1.0).double()
    N, H, W, _ = v.shape
    return v.view(N, H // P, P, W // P, P, 3).permute(
        0, 1, 3, 2, 4, 5).reshape(N, -1, 3 * P * P)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("P,N,H,W,D,dtypes", [
    (16, 3, 32, 48, 48, (None, torch.bfloat16, torch.float16)),
    (32, 1, 64, 32, 16, (None,))])
def test_identity_size_bit_identical_to_rgb_kernel(P, N, H, W, D, dtypes,
                                                   tile):
    x, wk, bias, pos, cls = make_case(P, N, (H, W), D, (H // P) * (W // P),
                                      False)
    for dtype in dtypes:
        out = ops._image_u8_resize_patch_embed(
            x, (H, W), wk, bias, P, None, pos, cls, dtype, tile)
        assert torch.equal(out, ops._image_u8_patch_embed(
            x, wk, bias, P, pos, cls, dtype, tile))


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", sorted(HALF))
def test_exact_half_downscale_bit_exact(case, tile):
    P, N, (Hr, Wr), D, crop = HALF[case]
    Hc, Wc = (Hr, Wr) if crop is None else crop[2:]
    x, wk, bias, pos, cls = make_case(
        P, N, (2 * Hr, 2 * Wr), D, (Hc // P) * (Wc // P), True)

    def run():
        return ops._image_u8_resize_patch_embed(
            x, (Hr, Wr), wk, bias, P, crop, pos, cls, None, tile)

    a = blends(x, (Hr, Wr), crop, P)
    assert torch.equal(a * 4, (a * 4).round()) and a.max() < 256
    assert not torch.equal(a, a.bfloat16().double())     # lo is in play
    want = a @ wk.cpu().double().t() + bias.cpu().double()
    want = torch.cat((cls.cpu().double().expand(N, 1, D), want), dim=1)
    out = run()
    assert torch.equal(out.cpu(), (want + pos.cpu().double()).float())
    assert torch.equal(out, run())                       # deterministic


@pytest.mark.parametrize("tile", TILES)
def test_crop_equals_sliced_source_and_token_rows(tile):
    P, D = 16, 48
    x, wk, bias, _, _ = make_case(P, 2, (96, 128), D, 0, False, seed=2)

    def run(images, size, crop):
        return ops._image_u8_resize_patch_embed(
            images, size, wk, bias, P, crop, None, None, None, tile)

    # 2:1, even offsets: the window's taps are the sliced source's
    sliced = x[:, 8:72, 20:116].contiguous()
    assert torch.equal(run(x, (48, 64), (4, 10, 32, 48)),
                       run(sliced, (32, 48), None))
    # any ratio, patch offsets: token rows (hp, wp) in [1,3) x [1,4) of 4 x 5
    full = run(x, (64, 80), None).view(2, 4, 5, D)
    out = run(x, (64, 80), (16, 16, 32, 48))
    assert torch.equal(out, full[:, 1:3, 1:4].reshape(2, 6, D))


@pytest.mark.parametrize("tile", [1, 2])
@pytest.mark.parametrize("case", sorted(BOUND))
def test_folded_real_weights_within_fp64_bound(case, tile, capsys):
    hw, size, crop = BOUND[case]
    P, D, K = 16, 64, 768
    g = torch.Generator().manual_seed(3)
    wk, bias_f = ops.patch_embed_fold(
        torch.randn((D, 3, P, P), generator=g), torch.randn(D, generator=g),
        IMAGENET_MEAN, IMAGENET_STD)
    x = make_case(P, 2 if hw[0] > 1 else 1, hw, D, 0, False)[0]
    out = ops._image_u8_resize_patch_embed(
        x, size, wk.to(DEV), bias_f.to(DEV), P, crop, None, None, None, tile)
    a = blends(x, size, crop, P)
    ref = a @ wk.double().t() + bias_f.double()
    vw = a @ wk.double().abs().t()
    bound = (2 * K + 2) * 2.0 ** -23 * (1 + 2.0 ** -7) * (
        vw + bias_f.double().abs()) + 2.0 ** -16 * vw
    ratio = ((out.cpu().double() - ref).abs() / bound).max().item()
    with capsys.disabled():
        print(f"\nresize patch_embed {case} tile {tile}: largest error / "
              f"bound = {ratio:.4f}")
    assert ratio <= 1.0


def test_servable_runs_kernel_on_any_size_and_follows_load_state_dict():
    cfg = dict(image_size=32, patch=16, hidden=32, layers=1, heads=2, mlp=64,
               num_classes=10)
    s = vit_b16_servable(DEV, torch.bfloat16, config=VitConfig(**cfg),
                         input_format="uint8_nhwc_resize")
    g = torch.Generator().manual_seed(0)
    xs = [torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
          for shape in ((2, 50, 75, 3), (1, 90, 40, 3))]

    def direct(x):
        m, (H, W) = s.module, x.shape[1:3]
        size = (36, 36 * W // H) if H <= W else (36 * H // W, 36)
        wk, bias_f = ops.patch_embed_fold(
            m.patch_embed.weight, m.patch_embed.bias, IMAGENET_MEAN,
            IMAGENET_STD)
        tokens = ops.image_u8_resize_patch_embed(
            x.to(DEV), size, wk, bias_f, 16,
            ((size[0] - 32) // 2, (size[1] - 32) // 2, 32, 32),
            m.pos_embed.detach().float()[0].contiguous(),
            m.cls_token.detach().float().reshape(-1),
            out_dtype=torch.bfloat16)
        with torch.no_grad():
            return m.forward_tokens(tokens).float()

    first = [s({"images": x.numpy()})["logits"] for x in xs]
    assert all(f.is_cuda and torch.equal(f, direct(x))
               for f, x in zip(first, xs))
    torch.manual_seed(7)
    s.module.load_state_dict(vit_b16(VitConfig(**cfg)).state_dict())
    second = s({"images": xs[0].numpy()})["logits"]
    assert torch.equal(second, direct(xs[0]))   # a stale fold would fail here
    assert not torch.equal(first[0], second)
