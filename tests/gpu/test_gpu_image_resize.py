"""Fused bilinear resize + crop image ingest on the GPU: the
u8_nhwc_resize_normalize kernel against the pinned fp32 expression computed
on CPU in numpy float32 (exact equality), then end to end through the raw
server and the ResNet-50 ``uint8_nhwc_resize`` mode.

Paths of the kernel and the smallest shape here that reaches each
(shapes are (N,Hin,Win,C) -> size / crop):

* tile geometry, chosen from the output width Wc: 8 lane runs x 32 rows for
  Wc <= 64 (most shapes), 16 x 16 for Wc <= 128 ((1,9,40,3) -> (20,100)),
  32 x 8 above ((1,6,90,3) -> (10,200)); more than one column tile for
  Wc > 256 ((1,3,150,3) -> (5,290), also a ragged last tile); a ragged last
  row tile whenever Hc is not a multiple of the tile rows (most shapes) and
  more than one row tile ((3,64,48,3) -> (40,24): 40 rows in tiles of 32).
* taps from LDS (every shape unless noted) or gathered directly when the
  tile's source spans exceed the 32 KiB LDS budget: (1,4,677,3) -> (4,256)
  is the widest source that still fits (2 x 8 spans of 2048 B),
  (1,4,678,3) -> (4,256) the first that does not, (1,8,1024,3) -> (4,256)
  a 4x downscale well past it.
* LDS fill: aligned 16 B loads, except a chunk that is not wholly inside
  the tensor, which is read bytewise: the first chunk of a source view that
  starts 1 byte off 16 B alignment, and the last chunk of any tensor whose
  end is not 16 B-aligned.
* stores: 16 B vectors, or scalar for a run that crosses the row end
  (Wc = 33, 3, 12) and for a destination or NCHW plane stride that is not
  16 B-aligned ((2,7,9,3) -> (20,33): plane of 660 elements).
* one large shape with more work items than the 2048-workgroup grid cap,
  so the grid-stride loop runs a second iteration."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from min_tfs_client_amd import ops  # noqa: E402
from min_tfs_client_amd.models import resnet50_servable  # noqa: E402
from min_tfs_client_amd.preprocess import (IMAGENET_MEAN,  # noqa: E402
                                           IMAGENET_STD, ImagePreprocess)
from min_tfs_client_amd.server import ModelServer, Servable  # noqa: E402
from min_tfs_client_amd.turbo import TurboPredictClient  # noqa: E402

DEV = "cuda:0"
MEAN = (0.485, 0.456, 0.406, 0.5)
STD = (0.229, 0.224, 0.225, 0.25)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16,
          "f16": torch.float16}
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.require_native()


def _taps(n_out, offset, n_in, n_resized):
    ratio = f32(n_in / n_resized)                # Python double, rounded once
    o = np.arange(offset, offset + n_out).astype(f32)
    s = np.maximum(((o + f32(0.5)) * ratio) - f32(0.5), f32(0))
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, s - i0.astype(f32)


def reference_nhwc_f32(x, size, crop=None, mean=None, std=None):
    """The pinned expression on CPU, numpy float32 (one rounding per
    operation), constants rounded through numpy.float32: fp32 NHWC."""
    x = x.cpu().numpy()
    _, Hin, Win, C = x.shape
    mean = MEAN[:C] if mean is None else mean
    std = STD[:C] if std is None else std
    Hr, Wr = size
    top, left, Hc, Wc = (0, 0, Hr, Wr) if crop is None else crop
    y0, y1, wy = _taps(Hc, top, Hin, Hr)
    x0, x1, wx = _taps(Wc, left, Win, Wr)
    p = x.astype(f32)
    wx = wx.reshape(1, 1, Wc, 1)
    wy = wy.reshape(1, Hc, 1, 1)
    r0, r1 = p[:, y0], p[:, y1]
    t = r0[:, :, x0] + wx * (r0[:, :, x1] - r0[:, :, x0])
    b = r1[:, :, x0] + wx * (r1[:, :, x1] - r1[:, :, x0])
    v = t + wy * (b - t)
    scale = np.array([f32((1.0 / 255.0) / s) for s in std], dtype=f32)
    bias = np.array([f32(-m / s) for m, s in zip(mean, std)], dtype=f32)
    y = (v * scale.reshape(1, 1, 1, C)) + bias.reshape(1, 1, 1, C)
    assert y.dtype == f32
    return torch.from_numpy(y)


def _as(ref_nhwc_f32, out_dtype, layout):
    y = ref_nhwc_f32
    if layout == "nchw":
        y = y.permute(0, 3, 1, 2)
    return y.to(out_dtype).contiguous()


def reference(x, size, crop=None, out_dtype=torch.float32, layout="nchw",
              **kw):
    return _as(reference_nhwc_f32(x, size, crop, **kw), out_dtype, layout)


def _pixels(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)


def _run(x_dev, size, crop, out_dtype, layout):
    C = x_dev.shape[3]
    return ops.image_u8_resize_to_float(x_dev, size, MEAN[:C], STD[:C],
                                        crop=crop, out_dtype=out_dtype,
                                        layout=layout)


def _check(x_cpu, x_dev, size, crop, out_dtype, layout):
    y = _run(x_dev, size, crop, out_dtype, layout)
    ref = reference(x_cpu, size, crop, out_dtype, layout)
    assert y.is_cuda and y.dtype == out_dtype and y.is_contiguous()
    assert tuple(y.shape) == tuple(ref.shape)
    assert torch.equal(y.cpu(), ref)
    return y


CASES = [
    ((2, 8, 8, 3), (8, 8), None),           # identity, whole vectors
    ((2, 17, 31, 3), (8, 8), None),         # non-integer downscale
    ((2, 7, 9, 3), (20, 33), None),         # upscale, ragged, odd planes
    ((1, 1, 5, 3), (4, 4), None),           # one source row, short run
    ((1, 5, 1, 3), (4, 12), None),          # one source column
    ((3, 64, 48, 3), (24, 40), None),       # several vectors per row
    ((3, 64, 48, 3), (40, 24), None),       # two row tiles
    ((2, 64, 64, 3), (3, 3), None),         # downscale above 8x
    ((2, 37, 53, 3), (32, 46), (4, 11, 24, 24)),   # odd crop offsets
    ((2, 16, 16, 1), (12, 20), None),
    ((2, 16, 16, 2), (12, 20), None),
    ((2, 16, 16, 4), (12, 20), None),
    ((1, 9, 40, 3), (20, 100), None),       # 16-run tile
    ((1, 6, 90, 3), (10, 200), None),       # 32-run tile
    ((1, 3, 150, 3), (5, 290), None),       # two column tiles
    ((1, 4, 677, 3), (4, 256), None),       # widest span that fits LDS
    ((1, 4, 678, 3), (4, 256), None),       # first span past the budget
    ((1, 8, 1024, 3), (4, 256), None),      # 4x downscale: direct gather
]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape,size,crop", CASES, ids=str)
def test_kernel_matches_reference(shape, size, crop, dtype, layout):
    x = _pixels(shape)
    _check(x, x.to(DEV), size, crop, DTYPES[dtype], layout)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_identity_size_equals_image_u8_to_float_on_device(dtype, layout):
    x = _pixels((2, 8, 8, 3), seed=1).to(DEV)
    y = _run(x, (8, 8), None, DTYPES[dtype], layout)
    same = ops.image_u8_to_float(x, MEAN[:3], STD[:3],
                                 out_dtype=DTYPES[dtype], layout=layout)
    assert torch.equal(y, same)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_crop_equals_slice_of_uncropped_on_device(dtype, layout):
    x = _pixels((2, 37, 53, 3), seed=2).to(DEV)
    full = _run(x, (32, 46), None, DTYPES[dtype], layout)
    part = _run(x, (32, 46), (4, 11, 24, 24), DTYPES[dtype], layout)
    if layout == "nchw":
        assert torch.equal(part, full[:, :, 4:28, 11:35])
    else:
        assert torch.equal(part, full[:, 4:28, 11:35, :])


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("size", [(16, 16), (12, 20)], ids=str)
def test_one_byte_storage_offset(size, dtype, layout):
    n = 2 * 16 * 16 * 3
    flat = _pixels((n + 16,), seed=1).to(DEV)
    x_dev = flat[1:1 + n].view(2, 16, 16, 3)
    assert x_dev.is_contiguous() and x_dev.data_ptr() % 16 == 1
    _check(x_dev.cpu(), x_dev, size, None, DTYPES[dtype], layout)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("size", [(16, 16), (8, 8)], ids=str)
def test_all_byte_values(size, dtype, layout):
    x = (torch.arange(768) % 256).to(torch.uint8).view(1, 16, 16, 3)
    y = _check(x, x.to(DEV), size, None, DTYPES[dtype], layout)
    if size == (16, 16):
        assert torch.equal(y, ops.image_u8_to_float(
            x.to(DEV), MEAN[:3], STD[:3], out_dtype=DTYPES[dtype],
            layout=layout))


@pytest.mark.parametrize("layout,shape", [("nchw", (0, 3, 5, 7)),
                                          ("nhwc", (0, 5, 7, 3))])
def test_empty_batch_does_not_launch(layout, shape):
    x = torch.empty((0, 8, 8, 3), dtype=torch.uint8, device=DEV)
    y = _run(x, (5, 7), None, torch.bfloat16, layout)
    torch.cuda.synchronize()
    assert y.is_cuda and tuple(y.shape) == shape
    assert y.dtype == torch.bfloat16


@pytest.fixture(scope="module")
def large():
    # Wc = 170 -> 32-run x 8-row tiles, one per 8 rows: 132 * 16 = 2112
    # work items, more than the 2048 workgroups of the capped grid.
    # Input 8.6 MB, fp32 output 34 MB.
    x = _pixels((132, 128, 170, 3), seed=3)
    return x, x.to(DEV), reference_nhwc_f32(x, (128, 170))


@pytest.mark.parametrize("dtype,layout", [("bf16", "nchw"),
                                          ("f32", "nhwc")])
def test_grid_stride_second_iteration(large, dtype, layout):
    x, x_dev, ref = large
    y = _run(x_dev, (128, 170), None, DTYPES[dtype], layout)
    assert torch.equal(y.cpu(), _as(ref, DTYPES[dtype], layout))


def test_launch_uses_current_stream():
    x = _pixels((4, 17, 31, 3), seed=4)
    x_dev = x.to(DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        y = _run(x_dev, (12, 20), None, torch.float32, "nchw")
    stream.synchronize()
    assert torch.equal(y.cpu(), reference(x, (12, 20)))


def test_device_tensor_errors_are_value_errors():
    op = ops.image_u8_resize_to_float
    x = torch.zeros((1, 4, 4, 5), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        op(x, (4, 4), (0.5,) * 5, (0.5,) * 5)
    with pytest.raises(ValueError):
        op(x[..., :3], (4, 4), MEAN[:3], STD[:3])            # strided
    ok = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        op(ok.float(), (4, 4), MEAN[:3], STD[:3])
    with pytest.raises(ValueError):
        op(ok, (0, 4), MEAN[:3], STD[:3])
    with pytest.raises(ValueError):
        op(ok, (4, 16385), MEAN[:3], STD[:3])
    with pytest.raises(ValueError):
        op(ok, (8, 8), MEAN[:3], STD[:3], crop=(0, 4, 8, 5))
    with pytest.raises(ValueError):
        op(ok, (8, 8), MEAN[:3], STD[:3], crop=(0, 0, 0, 4))
    with pytest.raises(ValueError):
        op(torch.empty((1, 0, 4, 3), dtype=torch.uint8, device=DEV),
           (4, 4), MEAN[:3], STD[:3])
    with pytest.raises(ValueError):
        op(ok, (4, 4), MEAN[:3], STD[:3], out_dtype=torch.float64)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# end to end through the raw server (mirrors test_gpu_image_preprocess.py)
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def resnet_resize():
    return resnet50_servable(DEV, torch.bfloat16,
                             input_format="uint8_nhwc_resize")


@pytest.fixture(scope="module")
def server(tmp_path_factory, resnet_resize):
    sock = f"unix://{tmp_path_factory.mktemp('s')}/resize.sock"
    with ModelServer(address=sock, raw_predict=True, device=DEV) as srv:
        pre = ImagePreprocess(MEAN[:3], STD[:3], out_dtype=torch.bfloat16,
                              layout="nchw", device=DEV, resize=(24, 40),
                              center_crop=(16, 32))
        srv.manager.load(
            "pre",
            Servable(lambda inputs: {"images": inputs["images"]},
                     preprocess={"images": pre}),
            version=1)
        srv.manager.load("resnet50_resize", resnet_resize, version=1)
        yield srv


def test_predict_resize_device_tensor_end_to_end(server):
    x = _pixels((4, 64, 48, 3), seed=5)
    with TurboPredictClient(server.address) as client:
        out = client.predict("pre", {"images": x.to(DEV)},
                             output_device=DEV)
    y = out["images"]
    assert y.is_cuda and y.dtype == torch.bfloat16
    assert tuple(y.shape) == (4, 3, 16, 32)
    assert torch.equal(
        y.cpu(), reference(x, (24, 40), (4, 4, 16, 32), torch.bfloat16))


def test_resnet50_resize_mode_end_to_end(server):
    with TurboPredictClient(server.address) as client:
        for shape in [(2, 160, 200, 3), (1, 300, 256, 3)]:
            x = _pixels(shape, seed=6)
            out = client.predict("resnet50_resize", {"images": x.to(DEV)},
                                 output_device=DEV)
            logits = out["logits"]
            assert tuple(logits.shape) == (shape[0], 1000)
            assert logits.dtype == torch.float32
            assert bool(torch.isfinite(logits).all())


def test_resnet50_resize_mode_preprocess_is_center_crop(resnet_resize):
    # 256 x 256 is already the resized size: only the 224 centre crop is left
    x = _pixels((2, 256, 256, 3), seed=7).to(DEV)
    y = resnet_resize.preprocess["images"](x)
    same = ops.image_u8_to_float(
        x[:, 16:240, 16:240, :].contiguous(), IMAGENET_MEAN, IMAGENET_STD,
        out_dtype=torch.bfloat16)
    assert tuple(y.shape) == (2, 3, 224, 224)
    assert torch.equal(y, same)
