"""YUV 4:2:0 (NV12 / I420) loader of the patch-embedding MFMA kernel on the
GPU.

Frames are uniform random bytes (mostly out of gamut: both clamp directions
occur), placed as a view in front of a buffer of 255s so a stale or over-read
byte changes the integer. Integer cases: ``wk`` in [-4, 4] and integer bias /
pos / cls as in test_gpu_patch_embed.py, so fp32 accumulation is exact in any
order; the reference is ``ops.yuv420_to_rgb_u8`` on the CPU followed by an
int64 matmul, compared with ``torch.equal``.

With real folded weights the contract is bit-identity with the RGB kernel on
the converted frames; the fp64 bound of test_gpu_patch_embed.py,

    |out - ref| <= (K + 2) * 2**-23 * (sum_k |a_k||wk_k| + |bias_f|),

is asserted next to it, so a failed identity can be told from a wrong
result."""
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
    "p32": (32, 1, 64, 32, 16),
    "past_small_tile": (16, 33, 16, 16, 48),
    "past_large_tile": (16, 129, 16, 16, 144),
}
CHROMAS = ["nv12", "i420"]


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.require_native()


def frames_on_device(N, H, W, g):
    n = N * H * W * 3 // 2
    buf = torch.full((n + 4096,), 255, dtype=torch.uint8)
    buf[:n] = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
    return buf.to(DEV)[:n].view(N, H * 3 // 2, W)


def int_case(P, N, H, W, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    K, T = 3 * P * P, (H // P) * (W // P) + 1
    frames = frames_on_device(N, H, W, g)
    wk = torch.randint(-4, 5, (D, K), generator=g).to(torch.bfloat16).to(DEV)
    bias, pos, cls = (torch.randint(-64, 65, s, generator=g).float().to(DEV)
                      for s in ((D,), (T, D), (D,)))
    return frames, wk, bias, pos, cls


def int_reference(frames, chroma, matrix, wk, bias, P, pos, cls):
    x = ops.yuv420_to_rgb_u8(frames.cpu(), chroma, matrix)
    N, H, W, _ = x.shape
    K, D = 3 * P * P, wk.shape[0]
    a = x.view(N, H // P, P, W // P, P, 3).permute(
        0, 1, 3, 2, 4, 5).reshape(N, -1, K).long()
    y = a @ wk.cpu().long().t() + bias.cpu().long()
    y = torch.cat((cls.cpu().long().expand(N, 1, D), y), dim=1)
    return y + pos.cpu().long()


@pytest.mark.parametrize("tile", [0, 1, 2])
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_integer_data_bit_exact(case, chroma, tile):
    P = CASES[case][0]
    frames, wk, bias, pos, cls = int_case(*CASES[case])

    def run():
        return ops._image_yuv420_patch_embed(
            frames, wk, bias, P, pos, cls, None, tile, chroma=chroma)

    out = run()
    assert out.dtype == torch.float32 and out.is_cuda
    want = int_reference(frames, chroma, "bt601", wk, bias, P, pos, cls)
    assert torch.equal(out.cpu(), want.float())
    assert torch.equal(out, run())                       # deterministic


@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("matrix,dtype", [
    ("bt601", torch.float32), ("bt709", torch.float32),
    ("bt601_full", torch.float32), ("bt709", torch.bfloat16),
    ("bt601_full", torch.float16)])
def test_matrices_and_output_dtypes(matrix, dtype, chroma):
    P = 16
    frames, wk, bias, pos, cls = int_case(*CASES["three_images"])
    out = ops.image_yuv420_patch_embed(
        frames, wk, bias, P, pos, cls, out_dtype=dtype, chroma=chroma,
        matrix=matrix)
    assert out.dtype == dtype
    want = int_reference(frames, chroma, matrix, wk, bias, P, pos, cls)
    assert torch.equal(out.cpu(), want.to(dtype))


@pytest.mark.parametrize("tile", [1, 2])
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("case", ["three_images", "p32"])
def test_real_weights_bit_identical_to_rgb_kernel(case, chroma, tile):
    P, N, H, W, D = CASES[case]
    K = 3 * P * P
    g = torch.Generator().manual_seed(3)
    w = torch.randn((D, 3, P, P), generator=g)
    b = torch.randn(D, generator=g)
    frames = frames_on_device(N, H, W, g)
    wk, bias_f = (t.to(DEV) for t in ops.patch_embed_fold(
        w, b, IMAGENET_MEAN, IMAGENET_STD))
    rgb = ops.yuv420_to_rgb_u8(frames, chroma, "bt601")
    out = ops._image_yuv420_patch_embed(
        frames, wk, bias_f, P, None, None, None, tile, chroma=chroma)
    two_step = ops._image_u8_patch_embed(
        rgb, wk, bias_f, P, None, None, None, tile)
    a = rgb.cpu().view(N, H // P, P, W // P, P, 3).permute(
        0, 1, 3, 2, 4, 5).reshape(N, -1, K).double()
    wk64, bias64 = wk.cpu().double(), bias_f.cpu().double()
    ref = a @ wk64.t() + bias64
    mass = a @ wk64.abs().t() + bias64.abs()
    ratio = ((out.cpu().double() - ref).abs()
             / ((K + 2) * 2.0 ** -23 * mass)).max().item()
    print(f"yuv420 patch_embed fp64 check: error / bound = {ratio:.4f}")
    assert ratio <= 1.0
    assert torch.equal(out, two_step)


def test_servable_equals_rgb_servable_and_follows_load_state_dict():
    cfg = dict(image_size=32, patch=16, hidden=32, layers=1, heads=2, mlp=64,
               num_classes=10)
    frames = torch.randint(0, 256, (2, 48, 32), dtype=torch.uint8)
    rgb = ops.yuv420_to_rgb_u8(frames, "nv12", "bt601")
    yuv, u8 = (vit_b16_servable(DEV, torch.bfloat16, seed=5, input_format=f,
                                config=VitConfig(**cfg))
               for f in ("nv12", "uint8_nhwc"))
    first = yuv({"images": frames.numpy()})["logits"]
    assert first.is_cuda
    assert torch.equal(first, u8({"images": rgb.numpy()})["logits"])
    torch.manual_seed(7)
    state = vit_b16(VitConfig(**cfg)).state_dict()
    yuv.module.load_state_dict(state)
    u8.module.load_state_dict(state)
    second = yuv({"images": frames.numpy()})["logits"]
    # a stale fold would fail here
    assert torch.equal(second, u8({"images": rgb.numpy()})["logits"])
    assert not torch.equal(first, second)
