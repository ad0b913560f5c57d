"""Ragged uint8 image batches on CPU: ``ops.image_u8_ragged_resize_to_float``
against the per-image loop of the dense op it is defined by (bit for bit),
its argument errors, ``pack_ragged_images``, ``RaggedImagePreprocess``, the
tuple-of-aliases ``Servable`` preprocess key, the ResNet-50 ``uint8_ragged``
mode with its model.json key, and one Predict through an in-process server.
"""
import json

import grpc
import numpy as np
import pytest
import torch

from min_tfs_client_amd import ops
from min_tfs_client_amd.client import TensorServingClient
from min_tfs_client_amd.models import resnet50_servable
from min_tfs_client_amd.preprocess import (IMAGENET_MEAN, IMAGENET_STD,
                                           ImagePreprocess,
                                           RaggedImagePreprocess,
                                           pack_ragged_images)
from min_tfs_client_amd.repository import default_loader
from min_tfs_client_amd.server import ModelServer, Servable
from min_tfs_client_amd.tensors import tensor_proto_to_ndarray

MEAN = (0.485, 0.456, 0.406, 0.5)
STD = (0.229, 0.224, 0.225, 0.25)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16,
          "f16": torch.float16}
SHAPES = [(7, 9), (17, 31), (8, 8), (1, 5), (5, 1), (64, 48)]


def _images(shapes, C=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, C), dtype=torch.uint8, generator=g)
            for h, w in shapes]


def _pack(images):
    return torch.cat([im.reshape(-1) for im in images])


def _pairs(value, n):
    arr = np.asarray(value)
    return np.broadcast_to(arr, (n, 2)) if arr.ndim == 1 else arr


def dense_loop(images, sizes, out_size, origins=None, out_dtype=torch.float32,
               layout="nchw", mean=None, std=None):
    """The definition of the ragged op: the dense op on each image alone."""
    n = len(images)
    C = images[0].shape[2] if n else 3
    mean = MEAN[:C] if mean is None else mean
    std = STD[:C] if std is None else std
    sizes = _pairs(sizes, n)
    origins = _pairs((0, 0) if origins is None else origins, n)
    outs = [ops.image_u8_resize_to_float(
        im.unsqueeze(0), tuple(int(v) for v in sizes[i]), mean, std,
        crop=(int(origins[i][0]), int(origins[i][1])) + tuple(out_size),
        out_dtype=out_dtype, layout=layout) for i, im in enumerate(images)]
    return torch.cat(outs)


def _op(images, sizes, out_size, C=3, **kw):
    return ops.image_u8_ragged_resize_to_float(
        _pack(images), [im.shape[:2] for im in images], sizes, out_size,
        MEAN[:C], STD[:C], **kw)


# ---------------------------------------------------------------------------
# the op
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_cpu_op_equals_dense_loop(dtype, layout):
    images = _images(SHAPES)
    y = _op(images, (24, 40), (16, 32), origins=(4, 4),
            out_dtype=DTYPES[dtype], layout=layout)
    ref = dense_loop(images, (24, 40), (16, 32), (4, 4), DTYPES[dtype],
                     layout)
    assert y.dtype == DTYPES[dtype] and y.is_contiguous()
    assert tuple(y.shape) == ((6, 3, 16, 32) if layout == "nchw"
                              else (6, 16, 32, 3))
    assert torch.equal(y, ref)


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_cpu_op_channels(C):
    images = _images(SHAPES, C=C, seed=1)
    y = _op(images, (24, 40), (16, 32), C=C, origins=(4, 4))
    assert torch.equal(y, dense_loop(images, (24, 40), (16, 32), (4, 4)))


def test_cpu_op_per_image_sizes_and_origins():
    images = _images(SHAPES, seed=2)
    sizes = [(12, 21), (20, 33), (11, 13), (9, 40), (31, 10), (15, 15)]
    origins = [(1, 3), (5, 11), (0, 0), (0, 27), (22, 1), (3, 2)]
    for kind in (list, np.array, torch.tensor):
        y = _op(images, kind(sizes), (9, 9), origins=kind(origins),
                out_dtype=torch.bfloat16)
        assert torch.equal(y, dense_loop(images, sizes, (9, 9), origins,
                                         torch.bfloat16))


def test_shapes_container_kinds():
    images = _images(SHAPES[:3], seed=3)
    data = _pack(images)
    ref = dense_loop(images, (8, 8), (8, 8))
    shapes = [im.shape[:2] for im in images]
    for s in (shapes, np.array(shapes, dtype=np.int32),
              torch.tensor(shapes, dtype=torch.int32),
              torch.tensor(shapes, dtype=torch.int64)):
        y = ops.image_u8_ragged_resize_to_float(
            data, s, (8, 8), (8, 8), MEAN[:3], STD[:3])
        assert torch.equal(y, ref)


@pytest.mark.parametrize("layout,shape", [("nchw", (0, 3, 5, 7)),
                                          ("nhwc", (0, 5, 7, 3))])
def test_empty_batch(layout, shape):
    empty = torch.empty((0,), dtype=torch.uint8)
    for shapes in ([], np.zeros((0, 2), dtype=np.int32)):
        y = ops.image_u8_ragged_resize_to_float(
            empty, shapes, (9, 9), (5, 7), MEAN[:3], STD[:3],
            out_dtype=torch.bfloat16, layout=layout)
        assert tuple(y.shape) == shape and y.dtype == torch.bfloat16


def test_rejected_inputs_raise_value_error():
    op = ops.image_u8_ragged_resize_to_float
    images = _images([(4, 5), (6, 3)])
    data = _pack(images)
    shapes = [(4, 5), (6, 3)]
    m, s = MEAN[:3], STD[:3]
    ok = dict(sizes=(8, 8), out_size=(8, 8), mean=m, std=s)
    assert tuple(op(data, shapes, **ok).shape) == (2, 3, 8, 8)

    # data: dtype, rank, contiguity, type
    with pytest.raises(ValueError, match="uint8"):
        op(data.float(), shapes, **ok)
    with pytest.raises(ValueError, match="rank"):
        op(data.view(2, -1), shapes, **ok)
    with pytest.raises(ValueError, match="contiguous"):
        op(torch.cat([data, data])[::2], shapes, **ok)
    with pytest.raises(ValueError, match="torch tensor"):
        op(data.numpy(), shapes, **ok)
    # shapes: integer [N,2]
    for bad in ([(4, 5, 3), (6, 3, 3)], [4, 5], np.array(shapes, dtype=float),
                [[(4, 5)], [(6, 3)]]):
        with pytest.raises(ValueError, match="shapes"):
            op(data, bad, **ok)
    # mean / std / channels
    with pytest.raises(ValueError, match="std"):
        op(data, shapes, (8, 8), (8, 8), m, STD[:2])
    with pytest.raises(ValueError, match="channels"):
        op(data, shapes, (8, 8), (8, 8), (0.5,) * 5, (0.5,) * 5)
    with pytest.raises(ValueError, match="channels"):
        op(data, shapes, (8, 8), (8, 8), (), ())
    # sides of an image, named by index
    with pytest.raises(ValueError, match="image 1.*input sides"):
        op(data, [(4, 5), (0, 3)], **ok)
    with pytest.raises(ValueError, match="image 1.*input sides"):
        op(data, [(4, 5), (16385, 3)], **ok)
    with pytest.raises(ValueError, match="image 0.*input sides"):
        op(data, [(-4, 5), (6, 3)], **ok)
    with pytest.raises(ValueError, match="image 1.*resized sides"):
        op(data, shapes, [(8, 8), (8, 16385)], (8, 8), m, s)
    with pytest.raises(ValueError, match="image 0.*resized sides"):
        op(data, shapes, [(0, 8), (8, 8)], (8, 8), m, s)
    # the byte count: one byte more, one byte fewer, a wrong shape
    with pytest.raises(ValueError, match="bytes"):
        op(torch.cat([data, data[:1]]), shapes, **ok)
    with pytest.raises(ValueError, match="bytes"):
        op(data[:-1], shapes, **ok)
    with pytest.raises(ValueError, match="bytes"):
        op(data, [(4, 5), (6, 4)], **ok)
    with pytest.raises(ValueError, match="bytes"):
        op(data, shapes, (8, 8), (8, 8), MEAN[:4], STD[:4])
    with pytest.raises(ValueError, match="bytes"):
        op(data, [], **ok)
    # sizes / origins / out_size of the wrong shape
    for bad in ((8,), (8, 8, 8), [(8, 8)] * 3, 8, (8.0, 8.0), None):
        with pytest.raises(ValueError, match="sizes"):
            op(data, shapes, bad, (8, 8), m, s)
    for bad in ((0,), [(0, 0)] * 3, (0.0, 0.0)):
        with pytest.raises(ValueError, match="origins"):
            op(data, shapes, (8, 8), (8, 8), m, s, origins=bad)
    for bad in (8, (8,), (8, 8, 8), (0, 8), (8, 16385)):
        with pytest.raises(ValueError, match="out_size"):
            op(data, shapes, (8, 8), bad, m, s)
    # crop window not inside an image's resized size, named by index
    with pytest.raises(ValueError, match="image 1.*crop window"):
        op(data, shapes, [(8, 8), (8, 7)], (8, 8), m, s)
    with pytest.raises(ValueError, match="image 0.*crop window"):
        op(data, shapes, (8, 8), (8, 8), m, s, origins=[(1, 0), (0, 0)])
    with pytest.raises(ValueError, match="image 1.*crop window"):
        op(data, shapes, (8, 8), (4, 4), m, s, origins=[(0, 0), (0, -1)])
    # layout / out_dtype
    with pytest.raises(ValueError, match="layout"):
        op(data, shapes, layout="chw", **ok)
    with pytest.raises(ValueError, match="out_dtype"):
        op(data, shapes, out_dtype=torch.float64, **ok)


# ---------------------------------------------------------------------------
# pack_ragged_images
# ---------------------------------------------------------------------------

def test_pack_ragged_images_round_trips():
    images = [im.numpy() for im in _images(SHAPES, seed=4)]
    data, shapes = pack_ragged_images(images)
    assert data.dtype == np.uint8 and data.ndim == 1
    assert shapes.dtype == np.int32 and shapes.shape == (6, 2)
    off = 0
    for im, (h, w) in zip(images, shapes):
        assert (h, w) == im.shape[:2]
        assert np.array_equal(data[off:off + h * w * 3].reshape(h, w, 3), im)
        off += h * w * 3
    assert off == data.size
    data, shapes = pack_ragged_images([])
    assert data.shape == (0,) and shapes.shape == (0, 2)


def test_pack_ragged_images_rejects_bad_images():
    a = np.zeros((4, 5, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="image 1.*channels"):
        pack_ragged_images([a, np.zeros((4, 5, 4), dtype=np.uint8)])
    with pytest.raises(ValueError, match="image 1"):
        pack_ragged_images([a, np.zeros((4, 5), dtype=np.uint8)])
    with pytest.raises(ValueError, match="image 0"):
        pack_ragged_images([a.astype(np.float32)])


# ---------------------------------------------------------------------------
# RaggedImagePreprocess
# ---------------------------------------------------------------------------

def _pre(**kw):
    return RaggedImagePreprocess(MEAN[:3], STD[:3], **kw)


def test_preprocess_construction_rules():
    assert _pre(resize=(12, 20)).out_size == (12, 20)
    assert _pre(resize=(12, 20), center_crop=8).out_size == (8, 8)
    assert _pre(resize=16, center_crop=(8, 12)).out_size == (8, 12)
    assert _pre(center_crop=4).out_size == (4, 4)
    for kw in ({}, {"resize": 16}):
        with pytest.raises(ValueError, match="one output size"):
            _pre(**kw)
    with pytest.raises(ValueError, match="antialias"):
        _pre(resize=16, center_crop=8, antialias=True)
    with pytest.raises(ValueError):
        _pre(resize=(12, 20), layout="chw")
    with pytest.raises(ValueError):
        _pre(resize=(0, 20))
    with pytest.raises(ValueError):
        RaggedImagePreprocess(MEAN[:3], STD[:2], resize=(12, 20))


@pytest.mark.parametrize("kw", [
    dict(resize=16, center_crop=(12, 14)),
    dict(resize=(12, 20)),
    dict(resize=(12, 20), center_crop=(8, 16)),
], ids=str)
def test_preprocess_equals_dense_preprocess_per_image(kw):
    # the short-side rule and the centring are ImagePreprocess's, per image
    shapes = [(20, 31), (31, 20), (16, 16), (40, 17), (16, 100)]
    images = _images(shapes, seed=5)
    data, image_shapes = pack_ragged_images([im.numpy() for im in images])
    y = _pre(out_dtype=torch.bfloat16, **kw)(data, image_shapes)
    dense = ImagePreprocess(MEAN[:3], STD[:3], out_dtype=torch.bfloat16, **kw)
    ref = torch.cat([dense(im.unsqueeze(0)) for im in images])
    assert torch.equal(y, ref)
    # tensors work as well as arrays
    y2 = _pre(out_dtype=torch.bfloat16, **kw)(
        torch.from_numpy(data), torch.from_numpy(image_shapes))
    assert torch.equal(y2, ref)


def test_preprocess_center_crop_alone_crops_input_size():
    images = _images([(9, 12), (6, 5), (5, 20)], seed=6)
    data, image_shapes = pack_ragged_images([im.numpy() for im in images])
    y = _pre(center_crop=(5, 4), layout="nhwc")(data, image_shapes)
    ref = torch.cat([ops.image_u8_to_float(
        im[(h - 5) // 2:(h - 5) // 2 + 5,
           (w - 4) // 2:(w - 4) // 2 + 4].contiguous().unsqueeze(0),
        MEAN[:3], STD[:3], layout="nhwc")
        for im, (h, w) in zip(images, image_shapes)])
    assert torch.equal(y, ref)


def test_preprocess_crop_too_large_names_the_image():
    pre = _pre(resize=8, center_crop=(8, 12))
    images = _images([(10, 15), (10, 14)])
    data, image_shapes = pack_ragged_images([im.numpy() for im in images])
    with pytest.raises(ValueError, match="image 1"):
        pre(data, image_shapes)                  # 10x14 -> 8x11 < 8x12
    with pytest.raises(ValueError, match="image_shapes"):
        pre(data, image_shapes.reshape(-1))
    with pytest.raises(ValueError, match="image 0"):
        pre(data, np.array([[0, 15], [10, 14]]))
    with pytest.raises(ValueError, match="uint8"):
        pre(data.astype(np.float32), image_shapes[:1])


# ---------------------------------------------------------------------------
# Servable: a tuple of aliases as a preprocess key
# ---------------------------------------------------------------------------

def test_servable_tuple_key():
    calls = []

    def both(a, b):
        calls.append((a, b))
        return a + b

    seen = {}

    def fn(inputs):
        seen.update(inputs)
        return {"y": inputs["a"]}

    s = Servable(fn, preprocess={("a", "b"): both, "c": lambda v: v * 10})
    request = {"b": 2, "a": 1, "c": 3, "d": 4}
    out = s(request)
    assert calls == [(1, 2)]                     # key order, not dict order
    assert out == {"y": 3}
    assert seen == {"a": 3, "c": 30, "d": 4}     # "b" dropped, "d" untouched
    assert request == {"b": 2, "a": 1, "c": 3, "d": 4}   # never mutated

    for partial in ({"a": 1}, {"b": 2, "c": 3}):
        with pytest.raises(ValueError, match="go together"):
            s(dict(partial))
    assert len(calls) == 1
    # none of the tuple's aliases: the hook does not run, strings still do
    seen.clear()
    s.fn = lambda inputs: dict(inputs)
    assert s({"c": 1, "d": 2}) == {"c": 10, "d": 2}
    assert len(calls) == 1


def test_servable_string_keys_unchanged():
    s = Servable(lambda inputs: dict(inputs),
                 preprocess={"a": lambda v: v + 1})
    request = {"a": 1, "b": 2}
    assert s(request) == {"a": 2, "b": 2}
    assert request == {"a": 1, "b": 2}
    assert s({"b": 5}) == {"b": 5}


# ---------------------------------------------------------------------------
# ResNet-50 mode, loader
# ---------------------------------------------------------------------------

class _Capture(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.seen = None

    def forward(self, x):
        self.seen = x
        return torch.zeros(x.shape[0], 1000, dtype=x.dtype)


@pytest.fixture(scope="module")
def ragged_resnet():
    return resnet50_servable(input_format="uint8_ragged")


def test_resnet50_ragged_mode(ragged_resnet):
    s = ragged_resnet
    assert s.signature["inputs"] == {"images": (4, [-1]),
                                     "image_shapes": (3, [-1, 2])}
    assert s.signature["outputs"]["logits"] == (1, [-1, 1000])
    pre = s.preprocess[("images", "image_shapes")]
    assert isinstance(pre, RaggedImagePreprocess)
    assert pre.resize == 256 and pre.out_size == (224, 224)
    model, cap = s.module, _Capture()
    s.module = cap
    try:
        images = _images([(160, 200), (300, 256), (256, 341)], seed=8)
        data, shapes = pack_ragged_images([im.numpy() for im in images])
        out = s({"images": data, "image_shapes": shapes})
        assert out["logits"].shape == (3, 1000)
        dense = ImagePreprocess(IMAGENET_MEAN, IMAGENET_STD, resize=256,
                                center_crop=224)
        assert torch.equal(cap.seen, torch.cat(
            [dense(im.unsqueeze(0)) for im in images]))
        with pytest.raises(ValueError, match="go together"):
            s({"images": data})
    finally:
        s.module = model


def test_resnet50_ragged_mode_rejects_antialias():
    with pytest.raises(ValueError, match="antialias"):
        resnet50_servable(input_format="uint8_ragged", antialias=True)


def test_resnet50_unknown_mode_lists_ragged():
    with pytest.raises(ValueError) as ei:
        resnet50_servable(input_format="uint8_nchw")
    for mode in ("float_nchw", "uint8_nhwc", "uint8_nhwc_resize",
                 "uint8_ragged"):
        assert repr(mode) in str(ei.value)


def test_loader_passes_ragged_input_format(tmp_path):
    vdir = tmp_path / "m" / "1"
    vdir.mkdir(parents=True)
    (vdir / "model.json").write_text(json.dumps(
        {"family": "resnet50", "input_format": "uint8_ragged"}))
    s = default_loader("m", str(vdir))
    assert set(s.signature["inputs"]) == {"images", "image_shapes"}
    assert isinstance(s.preprocess[("images", "image_shapes")],
                      RaggedImagePreprocess)


# ---------------------------------------------------------------------------
# end to end over a unix socket, python server
# ---------------------------------------------------------------------------

def test_ragged_predict_end_to_end(sock_dir, ragged_resnet):
    addr = f"unix://{sock_dir}/ragged.sock"
    images = _images([(40, 64), (72, 48)], seed=9)
    data, shapes = pack_ragged_images([im.numpy() for im in images])
    with ModelServer(address=addr, transport="grpcio") as srv:
        srv.manager.load("resnet50_ragged", ragged_resnet, version=1)
        with TensorServingClient("unix", f"//{sock_dir}/ragged.sock",
                                 backend="grpcio") as client:
            resp = client.predict_request(
                "resnet50_ragged", {"images": data, "image_shapes": shapes},
                timeout=60)
            logits = tensor_proto_to_ndarray(resp.outputs["logits"])
            assert logits.shape == (2, 1000) and logits.dtype == np.float32
            assert np.isfinite(logits).all()
            wrong = shapes.copy()
            wrong[1, 1] += 1                     # does not match the bytes
            with pytest.raises(grpc.RpcError) as ei:
                client.predict_request(
                    "resnet50_ragged",
                    {"images": data, "image_shapes": wrong}, timeout=60)
            assert ei.value.code() == grpc.StatusCode.INVALID_ARGUMENT
