"""uint8 image ingest on CPU: ops.image_u8_to_float, the Servable
``preprocess=`` hook, ImagePreprocess and the ResNet-50 uint8 input mode.

The reference everywhere is the eager torch expression, computed from the
input on CPU with scale/bias built here through numpy.float32 (not through
ops.normalization_constants). Comparisons are exact (torch.equal)."""
import grpc
import numpy as np
import pytest
import torch

from min_tfs_client_amd import ops
from min_tfs_client_amd.batching import BatchingServable
from min_tfs_client_amd.client import TensorServingClient
from min_tfs_client_amd.models import resnet50_servable
from min_tfs_client_amd.preprocess import ImagePreprocess
from min_tfs_client_amd.server import ModelServer, Servable
from min_tfs_client_amd.tensors import tensor_proto_to_ndarray

MEAN = (0.485, 0.456, 0.406, 0.5)
STD = (0.229, 0.224, 0.225, 0.25)
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _consts(C, pixel_scale=1.0 / 255.0):
    scale = torch.from_numpy(np.array(
        [np.float32(pixel_scale / s) for s in STD[:C]], dtype=np.float32))
    bias = torch.from_numpy(np.array(
        [np.float32(-m / s) for m, s in zip(MEAN[:C], STD[:C])],
        dtype=np.float32))
    return scale, bias


def reference(x, out_dtype=torch.float32, layout="nchw"):
    x = x.cpu()
    C = x.shape[3]
    scale, bias = _consts(C)
    y = (x.permute(0, 3, 1, 2).float() * scale.view(1, C, 1, 1)
         + bias.view(1, C, 1, 1)).to(out_dtype)
    if layout == "nhwc":
        y = y.permute(0, 2, 3, 1)
    return y.contiguous()


def _pixels(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)


SHAPES = [(2, 8, 8, 3), (3, 7, 9, 3), (2, 4, 4, 1), (2, 4, 4, 2),
          (2, 4, 4, 4)]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_cpu_op_matches_reference(shape, out_dtype, layout):
    x = _pixels(shape)
    C = shape[3]
    y = ops.image_u8_to_float(x, MEAN[:C], STD[:C], out_dtype=out_dtype,
                              layout=layout)
    ref = reference(x, out_dtype, layout)
    assert y.dtype == out_dtype and y.shape == ref.shape
    assert y.is_contiguous()
    assert torch.equal(y, ref)


@pytest.mark.parametrize("layout,shape", [("nchw", (0, 3, 8, 8)),
                                          ("nhwc", (0, 8, 8, 3))])
def test_cpu_op_empty_batch(layout, shape):
    x = torch.empty((0, 8, 8, 3), dtype=torch.uint8)
    y = ops.image_u8_to_float(x, MEAN[:3], STD[:3],
                              out_dtype=torch.bfloat16, layout=layout)
    assert y.shape == shape and y.dtype == torch.bfloat16


def test_all_byte_values_are_unsigned():
    x = (torch.arange(768) % 256).to(torch.uint8).view(1, 16, 16, 3)
    y = ops.image_u8_to_float(x, MEAN[:3], STD[:3])
    assert torch.equal(y, reference(x))
    # 200 is 200.0, not -56: every byte >= 128 lands above byte 127
    xc = x.permute(0, 3, 1, 2)
    at127 = reference(torch.full((1, 1, 1, 3), 127, dtype=torch.uint8))
    for c in range(3):
        assert bool((y[:, c][xc[:, c] >= 128] > at127[0, c, 0, 0]).all())
    assert y.max() > 2.0  # 255 -> (1-0.406)/0.225 = 2.64 on channel 2


def test_normalization_constants_are_float32_rounded():
    scale, bias = ops.normalization_constants(MEAN[:3], STD[:3])
    rs, rb = _consts(3)
    assert isinstance(scale, list) and isinstance(bias, list)
    assert all(isinstance(v, float) for v in scale + bias)
    assert scale == [float(v) for v in rs.numpy()]
    assert bias == [float(v) for v in rb.numpy()]
    scale, _ = ops.normalization_constants((0.5,), (0.5,), pixel_scale=1.0)
    assert scale == [2.0]


def test_rejected_inputs_raise_value_error():
    ok = _pixels((2, 4, 4, 3))
    m, s = MEAN[:3], STD[:3]
    with pytest.raises(ValueError):          # C > 4
        ops.image_u8_to_float(_pixels((1, 4, 4, 5)), (0.5,) * 5, (0.5,) * 5)
    with pytest.raises(ValueError):          # not uint8
        ops.image_u8_to_float(ok.float(), m, s)
    with pytest.raises(ValueError):          # signed bytes are not pixels
        ops.image_u8_to_float(ok.to(torch.int8), m, s)
    with pytest.raises(ValueError):          # rank 3
        ops.image_u8_to_float(ok[0], m, s)
    with pytest.raises(ValueError):          # rank 5
        ops.image_u8_to_float(ok[None], m, s)
    with pytest.raises(ValueError):          # non-contiguous
        ops.image_u8_to_float(_pixels((2, 3, 4, 4)).permute(0, 2, 3, 1),
                              m, s)
    with pytest.raises(ValueError):          # len(mean) != C
        ops.image_u8_to_float(ok, MEAN[:2], s)
    with pytest.raises(ValueError):          # len(std) != C
        ops.image_u8_to_float(ok, m, STD[:4])
    with pytest.raises(ValueError):          # std == 0
        ops.image_u8_to_float(ok, m, (0.229, 0.0, 0.225))
    with pytest.raises(ValueError):
        ops.image_u8_to_float(ok, m, s, layout="chwn")
    with pytest.raises(ValueError):
        ops.normalization_constants((0.5,), (0.0,))


# ---------------------------------------------------------------------------
# Servable hook
# ---------------------------------------------------------------------------

def _capture_servable(**kw):
    seen = {}

    def fn(inputs):
        seen.update(inputs)
        return {"images": inputs["images"]}

    pre = ImagePreprocess(MEAN[:3], STD[:3], **kw)
    return Servable(fn, preprocess={"images": pre}), seen


def test_servable_preprocess_hook():
    s, seen = _capture_servable()
    x = _pixels((2, 8, 8, 3))
    other = np.arange(4, dtype=np.int32)
    inputs = {"images": x.numpy(), "ids": other}
    out = s(inputs)
    assert torch.equal(seen["images"], reference(x))
    assert seen["ids"] is other                  # untouched alias
    assert inputs["images"].dtype == np.uint8    # caller's dict not mutated
    assert inputs["images"].shape == (2, 8, 8, 3)
    assert torch.equal(out["images"], reference(x))
    # torch input, other dtype/layout
    s2, seen2 = _capture_servable(out_dtype=torch.bfloat16, layout="nhwc")
    s2({"images": x})
    assert torch.equal(seen2["images"],
                       reference(x, torch.bfloat16, "nhwc"))


def test_servable_without_preprocess_is_unchanged():
    calls = []

    def fn(inputs):
        calls.append(inputs)
        return inputs

    s = Servable(fn)
    inputs = {"x": np.ones(3, np.float32)}
    assert s(inputs) is inputs
    assert calls[0] is inputs                    # no copy, same object
    assert s.preprocess == {}


def test_servable_preprocess_missing_alias_passes_through():
    s, seen = _capture_servable()
    s.fn = lambda inputs: dict(inputs)
    out = s({"ids": np.zeros(2, np.int32)})
    assert list(out) == ["ids"]


def test_batching_servable_preprocesses_once():
    count = []
    pre = ImagePreprocess(MEAN[:3], STD[:3])

    def counting(x):
        count.append(tuple(x.shape))
        return pre(x)

    inner = Servable(lambda inputs: {"images": inputs["images"]},
                     preprocess={"images": counting})
    b = BatchingServable(inner, max_batch_size=8, batch_timeout_s=0.01)
    try:
        assert b.preprocess == {}
        x = _pixels((2, 8, 8, 3))
        out = b({"images": x.numpy()})
        assert torch.equal(torch.as_tensor(out["images"]), reference(x))
        assert count == [(2, 8, 8, 3)]
    finally:
        b.close()


# ---------------------------------------------------------------------------
# ResNet-50 uint8 mode (the 224x224 model itself is not run on CPU)
# ---------------------------------------------------------------------------

class _Capture(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.seen = None

    def forward(self, x):
        self.seen = x
        return torch.zeros(x.shape[0], 1000, dtype=x.dtype)


def test_resnet50_uint8_mode():
    s = resnet50_servable(input_format="uint8_nhwc")
    assert s.signature["inputs"]["images"] == (4, [-1, 224, 224, 3])
    assert s.signature["outputs"]["logits"] == (1, [-1, 1000])
    cap = _Capture()
    s.module = cap
    x = _pixels((2, 16, 16, 3))
    out = s({"images": x.numpy()})
    assert torch.equal(cap.seen, reference(x))
    assert out["logits"].shape == (2, 1000)
    assert out["logits"].dtype == torch.float32


def test_resnet50_uint8_mode_bf16_hands_model_bf16():
    s = resnet50_servable(dtype=torch.bfloat16, input_format="uint8_nhwc")
    cap = _Capture()
    s.module = cap
    x = _pixels((1, 8, 8, 3))
    s({"images": x})
    assert torch.equal(cap.seen, reference(x, torch.bfloat16))


def test_resnet50_default_mode_unchanged():
    s = resnet50_servable()
    assert s.signature["inputs"]["images"] == (1, [-1, 3, 224, 224])
    assert s.preprocess == {}
    cap = _Capture()
    s.module = cap
    x = torch.randn(1, 3, 8, 8)
    s({"images": x.numpy()})
    assert torch.equal(cap.seen, x)
    with pytest.raises(ValueError):
        resnet50_servable(input_format="uint8_nchw")


# ---------------------------------------------------------------------------
# end to end over a unix socket, python server
# ---------------------------------------------------------------------------

@pytest.fixture
def preprocess_server(sock_dir):
    addr = f"unix://{sock_dir}/pre.sock"
    with ModelServer(address=addr, transport="grpcio") as srv:
        servable, _ = _capture_servable()
        srv.manager.load("pre", servable, version=1)
        with TensorServingClient("unix", f"//{sock_dir}/pre.sock",
                                 backend="grpcio") as client:
            yield client


def test_predict_uint8_over_unix_socket(preprocess_server):
    x = _pixels((2, 8, 8, 3))
    resp = preprocess_server.predict_request("pre", {"images": x.numpy()},
                                             timeout=20)
    got = tensor_proto_to_ndarray(resp.outputs["images"])
    assert got.dtype == np.float32 and got.shape == (2, 3, 8, 8)
    assert torch.equal(torch.from_numpy(np.array(got)), reference(x))


def test_predict_float_to_uint8_servable_is_invalid_argument(
        preprocess_server):
    x = np.zeros((2, 8, 8, 3), np.float32)
    with pytest.raises(grpc.RpcError) as ei:
        preprocess_server.predict_request("pre", {"images": x}, timeout=20)
    assert ei.value.code() == grpc.StatusCode.INVALID_ARGUMENT
