"""Fused uint8 image ingest on the GPU: the u8_nhwc_normalize kernel against
the eager torch expression computed on CPU (exact equality), then end to end
through the raw server and the ResNet-50 uint8 input mode.

Each shape is the smallest that reaches a distinct path of the kernel:
all-vector interior, images made of whole chunks only, ragged tail with
misaligned image bases and planes, HW below one chunk, every channel count,
a source that is 1 byte off alignment, and one large shape that forces a
second grid-stride iteration."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from min_tfs_client_amd import ops  # noqa: E402
from min_tfs_client_amd.models import resnet50_servable  # noqa: E402
from min_tfs_client_amd.preprocess import ImagePreprocess  # noqa: E402
from min_tfs_client_amd.server import ModelServer, Servable  # noqa: E402
from min_tfs_client_amd.turbo import TurboPredictClient  # noqa: E402

DEV = "cuda:0"
MEAN = (0.485, 0.456, 0.406, 0.5)
STD = (0.229, 0.224, 0.225, 0.25)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16,
          "f16": torch.float16}


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.require_native()


def reference(x, out_dtype=torch.float32, layout="nchw"):
    """Eager chain on CPU, constants rounded through numpy.float32."""
    x = x.cpu()
    C = x.shape[3]
    scale = torch.from_numpy(np.array(
        [np.float32((1.0 / 255.0) / s) for s in STD[:C]], dtype=np.float32))
    bias = torch.from_numpy(np.array(
        [np.float32(-m / s) for m, s in zip(MEAN[:C], STD[:C])],
        dtype=np.float32))
    y = (x.permute(0, 3, 1, 2).float() * scale.view(1, C, 1, 1)
         + bias.view(1, C, 1, 1)).to(out_dtype)
    if layout == "nhwc":
        y = y.permute(0, 2, 3, 1)
    return y.contiguous()


def _pixels(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)


def _run(x_dev, out_dtype, layout):
    C = x_dev.shape[3]
    return ops.image_u8_to_float(x_dev, MEAN[:C], STD[:C],
                                 out_dtype=out_dtype, layout=layout)


def _check(x_cpu, x_dev, out_dtype, layout):
    y = _run(x_dev, out_dtype, layout)
    ref = reference(x_cpu, out_dtype, layout)
    assert y.is_cuda and y.dtype == out_dtype and y.is_contiguous()
    assert tuple(y.shape) == tuple(ref.shape)
    assert torch.equal(y.cpu(), ref)


SMALL_SHAPES = [
    (2, 8, 8, 3),      # HW=64: all fast path
    (5, 4, 4, 3),      # HW=16: whole chunks only, at most two per image
    (4, 17, 31, 3),    # HW=527: ragged tail, misaligned bases and planes
    (3, 7, 9, 3),      # HW=63
    (1, 1, 5, 3),      # HW below one chunk
    (2, 16, 16, 1),
    (2, 16, 16, 2),
    (2, 16, 16, 4),
]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=str)
def test_kernel_matches_reference(shape, dtype, layout):
    x = _pixels(shape)
    _check(x, x.to(DEV), DTYPES[dtype], layout)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_one_byte_storage_offset_takes_scalar_path(dtype, layout):
    n = 2 * 16 * 16 * 3
    flat = _pixels((n + 16,), seed=1).to(DEV)
    x_dev = flat[1:1 + n].view(2, 16, 16, 3)
    assert x_dev.is_contiguous() and x_dev.data_ptr() % 16 == 1
    _check(x_dev.cpu(), x_dev, DTYPES[dtype], layout)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_all_byte_values(dtype, layout):
    x = (torch.arange(768) % 256).to(torch.uint8).view(1, 16, 16, 3)
    _check(x, x.to(DEV), DTYPES[dtype], layout)


@pytest.mark.parametrize("layout,shape", [("nchw", (0, 3, 8, 8)),
                                          ("nhwc", (0, 8, 8, 3))])
def test_empty_batch_does_not_launch(layout, shape):
    x = torch.empty((0, 8, 8, 3), dtype=torch.uint8, device=DEV)
    y = _run(x, torch.bfloat16, layout)
    torch.cuda.synchronize()
    assert y.is_cuda and tuple(y.shape) == shape
    assert y.dtype == torch.bfloat16


@pytest.fixture(scope="module")
def large_pixels():
    # at 16 px/lane or fewer: N*ceil(HW/16) = 602112 chunks, more than the
    # 2048 blocks x 256 lanes of the capped grid
    x = _pixels((48, 448, 448, 3), seed=2)
    return x, x.to(DEV)


@pytest.mark.parametrize("dtype,layout", [("bf16", "nchw"),
                                          ("f32", "nhwc")])
def test_grid_stride_second_iteration(large_pixels, dtype, layout):
    x, x_dev = large_pixels
    _check(x, x_dev, DTYPES[dtype], layout)


def test_launch_uses_current_stream():
    x = _pixels((4, 17, 31, 3), seed=3)
    x_dev = x.to(DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        y = _run(x_dev, torch.float32, "nchw")
    stream.synchronize()
    assert torch.equal(y.cpu(), reference(x))


def test_device_tensor_errors_are_value_errors():
    x = torch.zeros((1, 4, 4, 5), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ops.image_u8_to_float(x, (0.5,) * 5, (0.5,) * 5)
    with pytest.raises(ValueError):
        ops.image_u8_to_float(x[..., :3], MEAN[:3], STD[:3])  # strided


# ---------------------------------------------------------------------------
# end to end through the raw server (mirrors test_gpu_serving.py)
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def server(tmp_path_factory):
    sock = f"unix://{tmp_path_factory.mktemp('s')}/pre.sock"
    with ModelServer(address=sock, raw_predict=True, device=DEV) as srv:
        pre = ImagePreprocess(MEAN[:3], STD[:3], out_dtype=torch.bfloat16,
                              layout="nchw", device=DEV)
        srv.manager.load(
            "pre",
            Servable(lambda inputs: {"images": inputs["images"]},
                     preprocess={"images": pre}),
            version=1)
        srv.manager.load(
            "resnet50_u8",
            resnet50_servable(DEV, torch.bfloat16,
                              input_format="uint8_nhwc"),
            version=1)
        yield srv


def test_predict_uint8_device_tensor_end_to_end(server):
    x = _pixels((8, 64, 64, 3), seed=4)
    with TurboPredictClient(server.address) as client:
        out = client.predict("pre", {"images": x.to(DEV)},
                             output_device=DEV)
    y = out["images"]
    assert y.is_cuda and y.dtype == torch.bfloat16
    assert tuple(y.shape) == (8, 3, 64, 64)
    assert torch.equal(y.cpu(), reference(x, torch.bfloat16))


def test_resnet50_uint8_mode_end_to_end(server):
    x = _pixels((2, 224, 224, 3), seed=5)
    with TurboPredictClient(server.address) as client:
        out = client.predict("resnet50_u8", {"images": x.to(DEV)},
                             output_device=DEV)
    logits = out["logits"]
    assert tuple(logits.shape) == (2, 1000)
    assert logits.dtype == torch.float32
    assert bool(torch.isfinite(logits).all())
