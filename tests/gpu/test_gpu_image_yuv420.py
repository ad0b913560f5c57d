"""YUV 4:2:0 (NV12 / I420) source side of the fused resize ingest on the GPU:
the yuv420_resize_normalize kernel against a reference written here (the
int32 conversion in numpy, then the pinned fp32 bilinear expression in numpy
float32), exact equality; then end to end through the raw server and the
ResNet-50 ``nv12_resize`` / ``i420_resize`` modes.

Paths of the kernel and the smallest shape here that reaches each (shapes are
frames (N,H,W), stored as uint8 [N,H*3/2,W], -> size / crop):

* tile geometry, chosen from the output width Wc as in the RGB kernel: 8 lane
  runs x 32 rows for Wc <= 64 (most shapes), 16 x 16 for Wc <= 128
  ((1,10,40) -> (20,100)), 32 x 8 above ((1,6,90) -> (10,200)); two column
  tiles with a ragged last one ((1,4,150) -> (5,290)); a ragged last row tile
  (most shapes) and two row tiles ((3,64,48) -> (40,24)).
* taps from LDS, converted while the workgroup fills it in chunks of 16
  pixels (48 LDS bytes) from the even column at or below the tile's first
  source column, or gathered and converted per tap when the tile's spans
  exceed the 32 KiB LDS budget. With 32 x 8 tiles there are 16 spans, so a
  span holds at most floor(2048 / 48) = 42 chunks = 672 pixels, one of which
  is kept for the even start: (1,4,670) -> (4,256) is the widest frame that
  still fits, (1,4,672) -> (4,256) the first that does not, (1,8,1024) ->
  (4,256) a 4x downscale well past it. ``_variant=1`` forces the direct path
  on small shapes too.
* LDS fill: unaligned 16 B luma and 16 B (NV12) or 2 x 8 B (I420) chroma
  loads, except a chunk whose loads would pass the end of the tensor, which
  is read bytewise: every frame of (1,2,2) (6 bytes in all, one chroma
  sample) and the last chroma rows of any tensor. Rows that are no multiple
  of 16 B (W = 18), I420 chroma rows of odd length (W/2 = 9, 3) and chroma
  planes that end in the middle of a W-byte row (H/2 = 3, 5) move every
  chunk's luma and chroma to unrelated alignments, as does a view that
  starts 1 byte into its storage. An odd first source column (crop with an
  odd left, upscales) starts the span one pixel early, on its chroma pair.
* stores: 16 B vectors, or scalar for a run that crosses the row end
  (Wc = 33, 3) and for a destination or NCHW plane stride that is not 16 B
  aligned ((2,8,10) -> (20,33): plane of 660 elements).
* one shape with more work items than the 2048-workgroup grid cap, so the
  grid-stride loop runs a second iteration."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from min_tfs_client_amd import ops  # noqa: E402
from min_tfs_client_amd.models import resnet50_servable  # noqa: E402
from min_tfs_client_amd.preprocess import (  # noqa: E402
    Yuv420ImagePreprocess)
from min_tfs_client_amd.server import ModelServer, Servable  # noqa: E402
from min_tfs_client_amd.turbo import TurboPredictClient  # noqa: E402

DEV = "cuda:0"
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16,
          "f16": torch.float16}
CHROMAS = ["nv12", "i420"]
# C offset, then the coefficients of C, (D, E) for R, G, B
MATRICES = {
    "bt601": (16, 298, (0, 409), (-100, -208), (516, 0)),
    "bt709": (16, 298, (0, 459), (-55, -136), (541, 0)),
    "bt601_full": (0, 256, (0, 359), (-88, -183), (454, 0)),
}
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.require_native()


def reference_rgb(x, chroma, matrix):
    """uint8 numpy [N,H*3/2,W] -> uint8 numpy [N,H,W,3], int32 arithmetic."""
    n, rows, w = x.shape
    h = rows * 2 // 3
    flat = x.reshape(n, -1).astype(np.int32)
    y = flat[:, :h * w].reshape(n, h, w)
    q = (h // 2) * (w // 2)
    if chroma == "nv12":
        uv = flat[:, h * w:].reshape(n, h // 2, w // 2, 2)
        u, v = uv[..., 0], uv[..., 1]
    else:
        u = flat[:, h * w:h * w + q].reshape(n, h // 2, w // 2)
        v = flat[:, h * w + q:].reshape(n, h // 2, w // 2)
    yy, xx = np.arange(h) >> 1, np.arange(w) >> 1
    d = u[:, yy][:, :, xx] - 128
    e = v[:, yy][:, :, xx] - 128
    yoff, yc, r, g, b = MATRICES[matrix]
    c = y - yoff
    out = np.empty((n, h, w, 3), dtype=np.uint8)
    for i, (kd, ke) in enumerate((r, g, b)):
        s = yc * c + kd * d + ke * e + 128
        assert s.dtype == np.int32
        out[..., i] = np.clip(np.floor_divide(s, 256), 0, 255)
    return out


def _taps(n_out, offset, n_in, n_resized):
    ratio = f32(n_in / n_resized)                # Python double, rounded once
    o = np.arange(offset, offset + n_out).astype(f32)
    s = np.maximum(((o + f32(0.5)) * ratio) - f32(0.5), f32(0))
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, s - i0.astype(f32)


def reference_nhwc_f32(x, size, crop, chroma, matrix):
    """The pinned expression on CPU, numpy float32 (one rounding per
    operation) on the converted bytes: fp32 NHWC torch tensor."""
    p = reference_rgb(x.cpu().numpy(), chroma, matrix).astype(f32)
    _, Hin, Win, C = p.shape
    Hr, Wr = (Hin, Win) if size is None else size
    top, left, Hc, Wc = (0, 0, Hr, Wr) if crop is None else crop
    y0, y1, wy = _taps(Hc, top, Hin, Hr)
    x0, x1, wx = _taps(Wc, left, Win, Wr)
    wx = wx.reshape(1, 1, Wc, 1)
    wy = wy.reshape(1, Hc, 1, 1)
    r0, r1 = p[:, y0], p[:, y1]
    t = r0[:, :, x0] + wx * (r0[:, :, x1] - r0[:, :, x0])
    b = r1[:, :, x0] + wx * (r1[:, :, x1] - r1[:, :, x0])
    v = t + wy * (b - t)
    scale = np.array([f32((1.0 / 255.0) / s) for s in STD], dtype=f32)
    bias = np.array([f32(-m / s) for m, s in zip(MEAN, STD)], dtype=f32)
    y = (v * scale.reshape(1, 1, 1, C)) + bias.reshape(1, 1, 1, C)
    assert y.dtype == f32
    return torch.from_numpy(y)


def _as(ref_nhwc_f32, out_dtype, layout):
    y = ref_nhwc_f32
    if layout == "nchw":
        y = y.permute(0, 3, 1, 2)
    return y.to(out_dtype).contiguous()


def _frames(n, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h * 3 // 2, w), dtype=torch.uint8,
                         generator=g)


def _run(x_dev, size, crop, out_dtype, layout, chroma, matrix="bt601",
         variant=0):
    return ops.image_yuv420_resize_to_float(
        x_dev, size, MEAN, STD, crop=crop, out_dtype=out_dtype,
        layout=layout, _variant=variant, chroma=chroma, matrix=matrix)


def _check(x_cpu, x_dev, size, crop, out_dtype, layout, chroma,
           matrix="bt601", variant=0, ref=None):
    y = _run(x_dev, size, crop, out_dtype, layout, chroma, matrix, variant)
    if ref is None:
        ref = reference_nhwc_f32(x_cpu, size, crop, chroma, matrix)
    ref = _as(ref, out_dtype, layout)
    assert y.is_cuda and y.dtype == out_dtype and y.is_contiguous()
    assert tuple(y.shape) == tuple(ref.shape)
    assert torch.equal(y.cpu(), ref)
    return y


CASES = [
    ((1, 2, 2), None, None),                # one chroma sample, bytewise fill
    ((1, 2, 2), (5, 7), None),
    ((2, 8, 16), (8, 16), None),            # identity, whole vectors
    ((2, 6, 18), None, None),               # rows of 18 B; W/2, H/2 odd
    ((2, 6, 18), (4, 7), None),
    ((3, 10, 6), (13, 11), None),           # W/2 = 3, H/2 = 5
    ((2, 18, 30), (8, 8), None),            # non-integer downscale
    ((2, 8, 10), (20, 33), None),           # upscale, ragged, odd planes
    ((3, 64, 48), (24, 40), None),          # several vectors per row
    ((3, 64, 48), (40, 24), None),          # two row tiles
    ((2, 64, 64), (3, 3), None),            # downscale above 8x
    ((2, 38, 54), (32, 46), (3, 11, 24, 24)),   # odd crop offsets
    ((1, 10, 40), (20, 100), None),         # 16-run tile
    ((1, 6, 90), (10, 200), None),          # 32-run tile
    ((1, 4, 150), (5, 290), None),          # two column tiles
    ((1, 4, 670), (4, 256), None),          # widest span that fits LDS
    ((1, 4, 672), (4, 256), None),          # first span past the budget
    ((1, 8, 1024), (4, 256), None),         # 4x downscale: direct gather
]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("shape,size,crop", CASES, ids=str)
def test_kernel_matches_reference(shape, size, crop, chroma, dtype, layout):
    x = _frames(*shape)
    _check(x, x.to(DEV), size, crop, DTYPES[dtype], layout, chroma)


DIRECT_CASES = [
    ((1, 2, 2), (5, 7), None),
    ((2, 6, 18), (4, 7), None),
    ((3, 10, 6), (13, 11), None),
    ((2, 38, 54), (32, 46), (3, 11, 24, 24)),
    ((2, 8, 10), (20, 33), None),
]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("shape,size,crop", DIRECT_CASES, ids=str)
def test_forced_direct_path_matches_reference(shape, size, crop, chroma,
                                              dtype, layout):
    x = _frames(*shape, seed=1)
    _check(x, x.to(DEV), size, crop, DTYPES[dtype], layout, chroma,
           variant=1)


@pytest.mark.parametrize("variant", [0, 1], ids=["lds", "direct"])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("matrix", list(MATRICES))
def test_matrices_and_clamps(matrix, chroma, layout, variant):
    # random bytes are valid frames and reach both clamps in every channel;
    # one frame of all 0 and one of all 255 pin the extremes
    x = _frames(3, 12, 22, seed=2)
    x[1] = 0
    x[2] = 255
    rgb = reference_rgb(x.numpy(), chroma, matrix)
    assert rgb.min() == 0 and rgb.max() == 255
    for size in (None, (9, 17)):
        _check(x, x.to(DEV), size, None, torch.float32, layout, chroma,
               matrix, variant)


@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_equals_rgb_kernel_on_converted_frames_on_device(dtype, chroma):
    x = _frames(2, 38, 54, seed=3).to(DEV)
    y = _run(x, (32, 46), (3, 11, 24, 24), DTYPES[dtype], "nchw", chroma,
             "bt709")
    rgb = ops.yuv420_to_rgb_u8(x, chroma, "bt709")
    assert rgb.is_cuda
    assert torch.equal(rgb.cpu(), torch.from_numpy(
        reference_rgb(x.cpu().numpy(), chroma, "bt709")))
    same = ops.image_u8_resize_to_float(rgb, (32, 46), MEAN, STD,
                                        crop=(3, 11, 24, 24),
                                        out_dtype=DTYPES[dtype])
    assert torch.equal(y, same)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("size", [None, (12, 20)], ids=str)
def test_one_byte_storage_offset(size, chroma, dtype, layout):
    n = 2 * 24 * 18
    flat = torch.randint(0, 256, (n + 16,), dtype=torch.uint8,
                         generator=torch.Generator().manual_seed(4)).to(DEV)
    x_dev = flat[1:1 + n].view(2, 24, 18)
    assert x_dev.is_contiguous() and x_dev.data_ptr() % 16 == 1
    _check(x_dev.cpu(), x_dev, size, None, DTYPES[dtype], layout, chroma)


@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("n", [0, 1, 3])
def test_batch_sizes(n, chroma):
    x = _frames(n, 8, 12, seed=5)
    y = _run(x.to(DEV), (5, 7), None, torch.bfloat16, "nchw", chroma)
    torch.cuda.synchronize()
    assert y.is_cuda and tuple(y.shape) == (n, 3, 5, 7)
    assert y.dtype == torch.bfloat16
    if n:
        ref = reference_nhwc_f32(x, (5, 7), None, chroma, "bt601")
        assert torch.equal(y.cpu(), _as(ref, torch.bfloat16, "nchw"))
    empty = _run(x.to(DEV)[:0], (5, 7), None, torch.float32, "nhwc", chroma)
    assert tuple(empty.shape) == (0, 5, 7, 3)


@pytest.fixture(scope="module")
def large():
    # Wc = 170 -> 32-run x 8-row tiles, one per 8 rows: 132 * 16 = 2112
    # work items, more than the 2048 workgroups of the capped grid.
    # Input 4.3 MB, fp32 output 34 MB.
    x = _frames(132, 128, 170, seed=6)
    return x, x.to(DEV), {c: reference_nhwc_f32(x, None, None, c, "bt601")
                          for c in CHROMAS}


@pytest.mark.parametrize("dtype,layout,chroma", [("bf16", "nchw", "nv12"),
                                                 ("f32", "nhwc", "i420")])
def test_grid_stride_second_iteration(large, dtype, layout, chroma):
    x, x_dev, refs = large
    _check(x, x_dev, None, None, DTYPES[dtype], layout, chroma,
           ref=refs[chroma])


def test_launch_uses_current_stream():
    x = _frames(4, 18, 30, seed=7)
    x_dev = x.to(DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        y = _run(x_dev, (12, 20), None, torch.float32, "nchw", "nv12")
    stream.synchronize()
    ref = reference_nhwc_f32(x, (12, 20), None, "nv12", "bt601")
    assert torch.equal(y.cpu(), _as(ref, torch.float32, "nchw"))


def test_device_tensor_errors_are_value_errors():
    op = ops.image_yuv420_resize_to_float
    ok = torch.zeros((1, 6, 4), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        op(torch.zeros((1, 6, 8), dtype=torch.uint8, device=DEV)[:, :, :4],
           (4, 4), MEAN, STD)                                # strided
    with pytest.raises(ValueError):
        op(ok.float(), (4, 4), MEAN, STD)
    with pytest.raises(ValueError):
        op(torch.zeros((1, 7, 4), dtype=torch.uint8, device=DEV), (4, 4),
           MEAN, STD)
    with pytest.raises(ValueError):
        op(torch.zeros((1, 6, 5), dtype=torch.uint8, device=DEV), (4, 4),
           MEAN, STD)
    with pytest.raises(ValueError):
        op(ok, (0, 4), MEAN, STD)
    with pytest.raises(ValueError):
        op(ok, (4, 16385), MEAN, STD)
    with pytest.raises(ValueError):
        op(ok, (8, 8), MEAN, STD, crop=(0, 4, 8, 5))
    with pytest.raises(ValueError):
        op(ok, (4, 4), MEAN, STD, chroma="nv21")
    with pytest.raises(ValueError):
        op(ok, (4, 4), MEAN, STD, matrix="bt2020")
    with pytest.raises(ValueError):
        op(ok, (4, 4), MEAN, STD, out_dtype=torch.float64)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# end to end through the raw server
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def resnets():
    return {mode: resnet50_servable(DEV, torch.bfloat16, seed=0,
                                    input_format=mode)
            for mode in ("nv12_resize", "i420_resize", "uint8_nhwc_resize")}


@pytest.fixture(scope="module")
def server(tmp_path_factory, resnets):
    sock = f"unix://{tmp_path_factory.mktemp('s')}/yuv.sock"
    with ModelServer(address=sock, raw_predict=True, device=DEV) as srv:
        pre = Yuv420ImagePreprocess(MEAN, STD, out_dtype=torch.bfloat16,
                                    layout="nchw", device=DEV,
                                    resize=(24, 40), center_crop=(16, 32),
                                    chroma="i420", matrix="bt709")
        srv.manager.load(
            "pre",
            Servable(lambda inputs: {"images": inputs["images"]},
                     preprocess={"images": pre}),
            version=1)
        for mode, servable in resnets.items():
            srv.manager.load(mode, servable, version=1)
        yield srv


def test_predict_yuv_preprocess_end_to_end(server):
    x = _frames(4, 64, 48, seed=8)
    with TurboPredictClient(server.address) as client:
        out = client.predict("pre", {"images": x.to(DEV)},
                             output_device=DEV)
    y = out["images"]
    assert y.is_cuda and y.dtype == torch.bfloat16
    assert tuple(y.shape) == (4, 3, 16, 32)
    ref = reference_nhwc_f32(x, (24, 40), (4, 4, 16, 32), "i420", "bt709")
    assert torch.equal(y.cpu(), _as(ref, torch.bfloat16, "nchw"))


@pytest.fixture
def deterministic_convolutions():
    # By default two forwards of one ResNet-50 on the same input differ in
    # the last bits on this stack, in every dtype (the convolution backend
    # picks non-reproducible algorithms), so no two modes could be compared
    # bit for bit. With deterministic algorithms requested, repeated forwards
    # and two servables of the same seed agree exactly.
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.mark.parametrize("chroma", CHROMAS)
def test_resnet50_yuv_modes_equal_rgb_mode_on_converted_frames(
        server, deterministic_convolutions, chroma):
    x = _frames(2, 160, 200, seed=9)
    rgb = torch.from_numpy(reference_rgb(x.numpy(), chroma, "bt601"))
    with TurboPredictClient(server.address) as client:
        got = client.predict(f"{chroma}_resize", {"images": x.to(DEV)},
                             output_device=DEV)["logits"]
        want = client.predict("uint8_nhwc_resize", {"images": rgb.to(DEV)},
                              output_device=DEV)["logits"]
    assert tuple(got.shape) == (2, 1000) and got.dtype == torch.float32
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
