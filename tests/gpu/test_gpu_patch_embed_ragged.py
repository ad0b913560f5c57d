"""Ragged batches into the resampling loader of the patch-embedding MFMA
kernel on the GPU (``tile``: 0 the rule, 1 small, 2 large). The contract is
bit identity, per image, with the dense resampling op on that image alone at
the same tile. One mixed-size case is held against fp64 with the bound derived
in tests/gpu/test_gpu_patch_embed_resize.py, ``v`` from the CPU ragged resize
op. Largest observed ratio on an MI355X: see docs/test_matrix.md."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from min_tfs_client_amd import ops  # noqa: E402
from min_tfs_client_amd.models import (VitConfig,  # noqa: E402
                                       vit_b16_servable)
from min_tfs_client_amd.preprocess import (IMAGENET_MEAN,  # noqa: E402
                                           IMAGENET_STD, pack_ragged_images)
from min_tfs_client_amd.server import ModelServer  # noqa: E402
from min_tfs_client_amd.turbo import TurboPredictClient  # noqa: E402

DEV = "cuda:0"
TILES = [0, 1, 2]
F32, BF16, F16 = None, torch.bfloat16, torch.float16
# one-patch images: (H, W), resized size, origin of the 16 x 16 window
CYCLE = [((16, 16), (16, 16), (0, 0)), ((23, 9), (18, 20), (1, 3)),
         ((5, 31), (31, 16), (15, 0)), ((40, 17), (24, 24), (7, 5)),
         ((1, 1), (16, 17), (0, 1))]


def cycle(n):
    return tuple([CYCLE[i % 5][k] for i in range(n)] for k in range(3))


# P, D, window, shapes, sizes, origins, output dtypes
CASES = {
    "three_sizes": (16, 48, (32, 48), [(37, 53), (9, 7), (106, 159)],
                    [(40, 56), (32, 48), (32, 48)], [(4, 5), (0, 0), (0, 0)],
                    (F32, BF16, F16)),
    "p32": (32, 16, (64, 32), [(70, 50), (33, 90)], [(64, 32), (80, 40)],
            [(0, 0), (7, 3)], (F32,)),
    "past_small_tile": (16, 48, (16, 16), *cycle(33), (F32,)),
    "past_large_tile": (16, 144, (16, 16), *cycle(65), (F32,)),
    "odd_origins": (16, 48, (32, 48), [(30, 77), (61, 45)],
                    [(41, 57), (45, 63)], [(3, 5), (13, 11)], (F32,)),
    "last_is_one_pixel": (16, 16, (16, 16), [(20, 30), (1, 1)],
                          [(16, 16), (16, 16)], [(0, 0), (0, 0)], (F32,)),
    "one_pixel_alone": (16, 16, (16, 16), [(1, 1)], [(16, 16)], [(0, 0)],
                        (F32,)),
}


def operands(P, D, tokens, shapes, seed=0, fold=False):
    """Device operands; the packed images are a view into a buffer of 255s."""
    g = torch.Generator().manual_seed(seed)
    n = sum(h * w * 3 for h, w in shapes)
    buf = torch.full((n + 4096,), 255, dtype=torch.uint8)
    buf[:n] = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
    if fold:
        wk, bias = ops.patch_embed_fold(
            torch.randn((D, 3, P, P), generator=g),
            torch.randn(D, generator=g), IMAGENET_MEAN, IMAGENET_STD)
    else:
        wk = torch.randn((D, 3 * P * P), generator=g).to(torch.bfloat16)
        bias = torch.randn(D, generator=g)
    pos = torch.randn((tokens + 1, D), generator=g)
    cls = torch.randn(D, generator=g)
    return (buf.to(DEV)[:n], wk.to(DEV), bias.to(DEV), pos.to(DEV),
            cls.to(DEV))


def per_image(data, shapes, sizes, origins, window, *rest):
    """The dense resampling op on every image alone."""
    outs, off = [], 0
    wk, bias, P, pos, cls, dtype, tile = rest
    for (h, w), size, origin in zip(shapes, sizes, origins):
        outs.append(ops._image_u8_resize_patch_embed(
            data[off:off + h * w * 3].view(1, h, w, 3), size, wk, bias, P,
            (*origin, *window), pos, cls, dtype, tile))
        off += h * w * 3
    return torch.cat(outs)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_every_image_bit_identical_to_dense_resampling_op(case, tile):
    P, D, window, shapes, sizes, origins, dtypes = CASES[case]
    tokens = (window[0] // P) * (window[1] // P)
    data, wk, bias, pos, cls = operands(P, D, tokens, shapes)
    for dtype in dtypes:
        def run():
            return ops._image_u8_ragged_resize_patch_embed(
                data, shapes, sizes, window, wk, bias, P, origins, pos, cls,
                dtype, tile)
        stream = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):       # table copy and launch
            out = run()
        stream.synchronize()
        assert out.shape == (len(shapes), tokens + 1, D)
        assert torch.equal(out, per_image(
            data, shapes, sizes, origins, window, wk, bias, P, pos, cls,
            dtype, tile))
        assert torch.equal(out, run())        # deterministic


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("hw,size,crop", [
    ((37, 53), (40, 56), (4, 5, 32, 48)), ((32, 48), (32, 48), None)])
def test_uniform_sizes_equal_the_dense_kernels(hw, size, crop, tile):
    N, P, D = 5, 16, 48
    data, wk, bias, pos, cls = operands(P, D, 6, [hw] * N, seed=1)
    x = data.view(N, *hw, 3)
    origin = (0, 0) if crop is None else crop[:2]
    out = ops._image_u8_ragged_resize_patch_embed(
        data, [hw] * N, size, (32, 48), wk, bias, P, origin, pos, cls, BF16,
        tile)
    assert torch.equal(out, ops._image_u8_resize_patch_embed(
        x, size, wk, bias, P, crop, pos, cls, BF16, tile))
    if crop is None:                          # identity size: the RGB kernel
        assert torch.equal(out, ops._image_u8_patch_embed(
            x, wk, bias, P, pos, cls, BF16, tile))
    empty = ops._image_u8_ragged_resize_patch_embed(
        data[:0], [], size, (32, 48), wk, bias, P, None, pos, cls, BF16, tile)
    torch.cuda.synchronize()
    assert empty.is_cuda and empty.shape == (0, 7, D) and empty.dtype == BF16


@pytest.mark.parametrize("tile", [1, 2])
def test_mixed_sizes_within_fp64_bound(tile, capsys):
    P, D, window, shapes, sizes, origins, _ = CASES["three_sizes"]
    K = 3 * P * P
    data, wk, bias_f, _, _ = operands(P, D, 6, shapes, seed=3, fold=True)
    out = ops._image_u8_ragged_resize_patch_embed(
        data, shapes, sizes, window, wk, bias_f, P, origins, None, None,
        None, tile)
    v = ops.image_u8_ragged_resize_to_float(
        data.cpu(), shapes, sizes, window, (0.0,) * 3, (1.0,) * 3,
        origins=origins, layout="nhwc", pixel_scale=1.0).double()
    a = v.view(len(shapes), window[0] // P, P, window[1] // P, P, 3).permute(
        0, 1, 3, 2, 4, 5).reshape(len(shapes), -1, K)
    w, b = wk.cpu().double(), bias_f.cpu().double()
    ref, vw = a @ w.t() + b, a @ w.abs().t()
    bound = (2 * K + 2) * 2.0 ** -23 * (1 + 2.0 ** -7) * (
        vw + b.abs()) + 2.0 ** -16 * vw
    ratio = ((out.cpu().double() - ref).abs() / bound).max().item()
    with capsys.disabled():
        print(f"\nragged patch_embed three_sizes tile {tile}: largest error "
              f"/ bound = {ratio:.4f}")
    assert ratio <= 1.0


def test_servable_end_to_end_behind_the_raw_server(tmp_path):
    cfg = VitConfig(image_size=32, patch=16, hidden=32, layers=1, heads=2,
                    mlp=64, num_classes=10)
    s = vit_b16_servable(DEV, BF16, config=cfg, input_format="uint8_ragged")
    g = torch.Generator().manual_seed(0)
    shapes = [(50, 75), (90, 40), (36, 36)]
    data, image_shapes = pack_ragged_images(
        [torch.randint(0, 256, (*hw, 3), dtype=torch.uint8,
                       generator=g).numpy() for hw in shapes])
    # shorter side to 36, centre crop 32
    sizes, origins = [(36, 54), (81, 36), (36, 36)], [(2, 11), (24, 2), (2, 2)]
    pre = s.preprocess[("images", "image_shapes")]
    tokens = pre(data, image_shapes)
    wk, bias_f, pos, cls = pre.folded()
    assert tokens.is_cuda and torch.equal(tokens, per_image(
        torch.from_numpy(data).to(DEV), shapes, sizes, origins, (32, 32),
        wk, bias_f, 16, pos, cls, BF16, 0))
    with ModelServer(address=f"unix://{tmp_path}/vit.sock", raw_predict=True,
                     device=DEV) as srv:
        srv.manager.load("vit", s, version=1)
        with TurboPredictClient(srv.address) as client:
            out = client.predict(
                "vit", {"images": torch.from_numpy(data),
                        "image_shapes": torch.from_numpy(image_shapes)},
                output_device=DEV)
    with torch.no_grad():
        want = s.module.forward_tokens(tokens).float()
    assert torch.equal(out["logits"], want)
