"""Antialiased resize + crop image ingest on the GPU: the
u8_resize_aa_h_kernel / u8_resize_aa_v_kernel pair against the CPU path of
``ops.image_u8_resize_to_float(antialias=True)`` (exact equality; the CPU
path is pinned to the tap-by-tap recipe in
tests/unit/test_image_resize_antialias.py), then end to end through the raw
server and the ResNet-50 ``uint8_nhwc_resize`` mode with ``antialias=True``.

Paths of the two kernels and the smallest shape here that reaches each
(shapes are (N,Hin,Win,C) -> size / crop):

* (2,37,53,3) -> (16,20): downscale on both axes with non-integer ratios;
  Wc = 20 leaves a ragged last lane run (4 of 8 columns: scalar workspace
  loads with clamped columns, scalar stores); bf16/f16 NCHW rows of 40 B
  put every odd row's runs off 16 B alignment (scalar stores).
* (2,48,64,3) -> (24,32), crop (4,8,16,16): whole runs, 16 B vector loads
  from the workspace and 16 B vector stores; crop offsets on both axes, so
  the workspace starts at a source row > 0 and holds fewer rows than Hin.
* (1,20,30,1) -> (40,45): upscale, support 1, at most 2 non-zero taps;
  workspace rows of 45 floats are not 16 B-aligned (scalar loads).
* (1,40,30,2) -> (10,60): down on one axis, up on the other.
* (1,33,47,4) -> (5,3): many taps per output; Wc < 8, a single short run.
* (1,9,9,3) -> (1,1): a single output pixel.
* (1,3,4096,1) -> (3,2): a horizontal tap loop of about 4096 iterations.
* (1,64,64,3) -> (64,64): identity, weights exactly (1, 0); also compared
  with the device ``image_u8_to_float``.
* (5,37,53,3) with a workspace cap sized for 2 images: the chunked loop
  (chunks of 2, 2 and 1 images through one workspace).
* grid cap: both grids are min(ceil(lanes/256), 2048) workgroups of 256,
  so one pass covers 524288 lanes. (131073,8,16,1) -> (4,8) has 131073 * 8
  source rows * 8 columns = 8.4 M horizontal lanes (16 passes) and
  131073 * 4 rows * 1 run = 524292 vertical lanes: 4 more than one pass, so
  the last image's rows come from the second grid-stride iteration. Input
  and fp32 output are 16.8 MB each."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from min_tfs_client_amd import ops  # noqa: E402
from min_tfs_client_amd.models import resnet50_servable  # noqa: E402
from min_tfs_client_amd.preprocess import (IMAGENET_MEAN,  # noqa: E402
                                           IMAGENET_STD)
from min_tfs_client_amd.server import ModelServer  # noqa: E402
from min_tfs_client_amd.turbo import TurboPredictClient  # noqa: E402

DEV = "cuda:0"
MEAN = (0.485, 0.456, 0.406, 0.5)
STD = (0.229, 0.224, 0.225, 0.25)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16,
          "f16": torch.float16}


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.require_native()


def _pixels(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)


def _run(x, size, crop, out_dtype, layout, **kw):
    C = x.shape[3]
    return ops.image_u8_resize_to_float(x, size, MEAN[:C], STD[:C],
                                        crop=crop, out_dtype=out_dtype,
                                        layout=layout, antialias=True, **kw)


def _check(x_cpu, x_dev, size, crop, out_dtype, layout, **kw):
    assert x_dev.is_cuda and not x_cpu.is_cuda
    y = _run(x_dev, size, crop, out_dtype, layout, **kw)
    ref = _run(x_cpu, size, crop, out_dtype, layout)
    assert y.is_cuda and y.dtype == out_dtype and y.is_contiguous()
    assert tuple(y.shape) == tuple(ref.shape)
    assert torch.equal(y.cpu(), ref)
    return y


CASES = [
    ((2, 37, 53, 3), (16, 20), None),           # down on both axes, ragged
    ((2, 48, 64, 3), (24, 32), (4, 8, 16, 16)),  # vector path, crop offsets
    ((1, 20, 30, 1), (40, 45), None),           # upscale, support 1
    ((1, 40, 30, 2), (10, 60), None),           # down on one axis, up on other
    ((1, 33, 47, 4), (5, 3), None),             # many taps, Wc < 8
    ((1, 9, 9, 3), (1, 1), None),               # single output pixel
    ((1, 3, 4096, 1), (3, 2), None),            # ~4096-iteration tap loop
    ((1, 64, 64, 3), (64, 64), None),           # identity
]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape,size,crop", CASES, ids=str)
def test_kernels_match_cpu_path(shape, size, crop, dtype, layout):
    x = _pixels(shape)
    y = _check(x, x.to(DEV), size, crop, DTYPES[dtype], layout)
    if size == shape[1:3]:
        C = shape[3]
        assert torch.equal(y, ops.image_u8_to_float(
            x.to(DEV), MEAN[:C], STD[:C], out_dtype=DTYPES[dtype],
            layout=layout))


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_chunked_workspace_loop(dtype, layout):
    x = _pixels((5, 37, 53, 3), seed=1)
    # workspace bytes of one image: an uncropped window needs all 37 source
    # rows, x Wc x C floats
    per_image = 37 * 20 * 3 * 4
    x_dev = x.to(DEV)
    y = _check(x, x_dev, (16, 20), None, DTYPES[dtype], layout,
               _ws_cap_bytes=2 * per_image + per_image // 2)
    assert torch.equal(y, _run(x_dev, (16, 20), None, DTYPES[dtype], layout))
    # a cap below one image still runs, one image per chunk
    assert torch.equal(y, _run(x_dev, (16, 20), None, DTYPES[dtype], layout,
                               _ws_cap_bytes=1))


@pytest.fixture(scope="module")
def large():
    x = _pixels((131073, 8, 16, 1), seed=2)
    ref = ops.image_u8_resize_to_float(x, (4, 8), MEAN[:1], STD[:1],
                                       layout="nhwc", antialias=True)
    return x.to(DEV), ref


@pytest.mark.parametrize("dtype,layout", [("bf16", "nchw"),
                                          ("f32", "nhwc")])
def test_grid_stride_second_iteration(large, dtype, layout):
    x_dev, ref = large
    y = _run(x_dev, (4, 8), None, DTYPES[dtype], layout)
    if layout == "nchw":
        ref = ref.permute(0, 3, 1, 2)
    assert torch.equal(y.cpu(), ref.to(DTYPES[dtype]).contiguous())


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("size", [(16, 16), (7, 8)], ids=str)
def test_one_byte_storage_offset(size, dtype, layout):
    n = 2 * 16 * 16 * 3
    flat = _pixels((n + 16,), seed=3).to(DEV)
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


def test_launch_uses_current_stream():
    x = _pixels((4, 17, 31, 3), seed=4)
    x_dev = x.to(DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        y = _run(x_dev, (12, 20), None, torch.float32, "nchw")
    stream.synchronize()
    assert torch.equal(y.cpu(), _run(x, (12, 20), None, torch.float32,
                                     "nchw"))


def test_two_runs_are_bit_equal():
    x_dev = _pixels((3, 37, 53, 3), seed=5).to(DEV)
    a = _run(x_dev, (16, 20), (1, 2, 13, 17), torch.float32, "nchw")
    b = _run(x_dev, (16, 20), (1, 2, 13, 17), torch.float32, "nchw")
    assert torch.equal(a, b)


def test_device_tensor_errors_are_value_errors():
    def op(*a, **kw):
        return ops.image_u8_resize_to_float(*a, antialias=True, **kw)

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
# end to end: ResNet-50 uint8_nhwc_resize mode with antialias=True
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def resnet_aa():
    return resnet50_servable(DEV, torch.bfloat16,
                             input_format="uint8_nhwc_resize", antialias=True)


@pytest.fixture
def deterministic_convolutions():
    """Comparing logits bit for bit needs a model that repeats itself. With
    the default solver choice ResNet-50's layer2..4 convolutions do not: two
    forwards of one input differ (measured: up to 2.4e-4 in bf16, 1.3e-8 in
    f32, five of five repeats); with ``cudnn.deterministic`` five of five
    repeats were bit-equal. The flag is process-wide, so it also covers the
    server's worker thread."""
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


def test_resnet50_antialias_predict_end_to_end(tmp_path, resnet_aa,
                                               deterministic_convolutions):
    x = _pixels((2, 300, 400, 3), seed=6)
    sock = f"unix://{tmp_path}/aa.sock"
    with ModelServer(address=sock, raw_predict=True, device=DEV) as srv:
        srv.manager.load("resnet50_aa", resnet_aa, version=1)
        with TurboPredictClient(srv.address) as client:
            out = client.predict("resnet50_aa", {"images": x.to(DEV)},
                                 output_device=DEV)
    logits = out["logits"]
    assert tuple(logits.shape) == (2, 1000)
    assert logits.dtype == torch.float32
    # 300x400 -> short side 256 -> (256, 341), centre crop 224
    pre = ops.image_u8_resize_to_float(
        x, (256, 341), IMAGENET_MEAN, IMAGENET_STD, crop=(16, 58, 224, 224),
        out_dtype=torch.bfloat16, antialias=True)
    with torch.no_grad():
        expected = resnet_aa.module(pre.to(DEV)).float()
    assert torch.equal(logits, expected)


def test_antialias_flag_switches_kernels(resnet_aa):
    """A one-pixel checkerboard at 300x400 -> (256,341): the 2-tap bilinear
    samples single squares, the antialiased filter averages them."""
    ij = torch.arange(300).view(300, 1) + torch.arange(400).view(1, 400)
    board = ((ij % 2) * 255).to(torch.uint8)
    x = board.view(1, 300, 400, 1).expand(2, 300, 400, 3).contiguous()
    plain = resnet50_servable(DEV, torch.bfloat16,
                              input_format="uint8_nhwc_resize")
    y_aa = resnet_aa.preprocess["images"](x.to(DEV))
    y_plain = plain.preprocess["images"](x.to(DEV))
    assert tuple(y_aa.shape) == tuple(y_plain.shape) == (2, 3, 224, 224)
    assert not torch.equal(y_aa, y_plain)
    assert torch.equal(y_aa.cpu(), ops.image_u8_resize_to_float(
        x, (256, 341), IMAGENET_MEAN, IMAGENET_STD, crop=(16, 58, 224, 224),
        out_dtype=torch.bfloat16, antialias=True))
    assert torch.equal(y_plain.cpu(), ops.image_u8_resize_to_float(
        x, (256, 341), IMAGENET_MEAN, IMAGENET_STD, crop=(16, 58, 224, 224),
        out_dtype=torch.bfloat16))
