"""Antialiased ragged uint8 image batches on the GPU: the
u8_ragged_resize_aa_h / _v kernels (N images of N sizes, two launches per
chunk) against the dense antialiased op run on CPU for each image alone
(exact equality), then end to end through the raw server and the ResNet-50
``uint8_ragged_antialias`` mode.

Paths of the two kernels and the smallest batch here that reaches each (a
batch is a list of (Hin,Win) -> resized size / crop window, C = 3 unless
noted):

* per-image table and the binary search over ws_row0: AA,
  [(7,9),(50,70),(8,8),(1,5),(5,1),(64,48),(33,200)] -> (12,20), crop
  (2,3,8,16), mixes up- and downscales (support 1 and up to 10 taps), one
  source row and one source column; its first image has 189 bytes, so every
  later image starts off 16 B alignment, and the images own 7, 38, 6, 1, 5,
  48 and 25 workspace rows. Run with C in 1..4.
* vertical kernel, 16 B vector loads of the workspace: out (8,16) with C = 3
  or 1, 2, 4 has Wc*C % 4 == 0 and whole runs.
* vertical kernel, scalar loads with the clamped column, and scalar stores:
  the same images -> (20,33), no crop: Wc*C = 99, the last run of a row is
  ragged and the NCHW plane has 660 elements.
* chunked loop: the AA batch needs 1344, 7296, 1152, 192, 960, 9216 and 4800
  workspace bytes per image; a 9000-byte cap gives chunks of 2, 3, 1 and 1
  images (the 9216-byte image exceeds the cap on its own), a 1-byte cap one
  image per chunk. ws_row0 restarts in every chunk.
* grid-stride loop of both kernels: 2100 images cycling through four shapes
  -> (16,128): 3,360,000 horizontal lanes and 537,600 vertical lanes against
  the 524,288 lanes of the capped grid; the first image differs from the
  last, so a wrong table index shows.
* byte loads of the source at any alignment: a view that starts 1 byte off
  16 B alignment, and a buffer end that is not 16 B-aligned with the last
  pixel of the last image tapped."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from min_tfs_client_amd import ops  # noqa: E402
from min_tfs_client_amd.models import resnet50_servable  # noqa: E402
from min_tfs_client_amd.preprocess import (  # noqa: E402
    AntialiasedRaggedImagePreprocess, pack_ragged_images)
from min_tfs_client_amd.server import ModelServer, Servable  # noqa: E402
from min_tfs_client_amd.turbo import TurboPredictClient  # noqa: E402

DEV = "cuda:0"
MEAN = (0.485, 0.456, 0.406, 0.5)
STD = (0.229, 0.224, 0.225, 0.25)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16,
          "f16": torch.float16}

AA = [(7, 9), (50, 70), (8, 8), (1, 5), (5, 1), (64, 48), (33, 200)]
# name -> (input shapes, resized size, (top, left), output size)
BATCHES = {
    "mixed": (AA, (12, 20), (2, 3), (8, 16)),
    "scalar_paths": (AA, (20, 33), (0, 0), (20, 33)),
}


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.require_native()


def _images(shapes, C=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, C), dtype=torch.uint8, generator=g)
            for h, w in shapes]


def _pack(images):
    return torch.cat([im.reshape(-1) for im in images])


def _pairs(value, n):
    arr = np.asarray(value)
    return np.broadcast_to(arr, (n, 2)) if arr.ndim == 1 else arr


def oracle_nhwc_f32(images, sizes, origins, out_size):
    """The dense antialiased op on CPU, one image at a time: fp32 NHWC."""
    n = len(images)
    C = images[0].shape[2]
    sizes, origins = _pairs(sizes, n), _pairs(origins, n)
    return torch.cat([ops.image_u8_resize_to_float(
        im.unsqueeze(0), tuple(int(v) for v in sizes[i]), MEAN[:C], STD[:C],
        crop=(int(origins[i][0]), int(origins[i][1])) + tuple(out_size),
        layout="nhwc", antialias=True) for i, im in enumerate(images)])


def _as(ref_nhwc_f32, out_dtype, layout):
    # the op rounds the same fp32 value once, whatever the layout
    y = ref_nhwc_f32
    if layout == "nchw":
        y = y.permute(0, 3, 1, 2)
    return y.to(out_dtype).contiguous()


_ORACLES = {}


def _batch(name, C=3):
    """(images, flat device buffer, fp32 NHWC oracle), computed once."""
    if (name, C) not in _ORACLES:
        shapes, size, origin, out_size = BATCHES[name]
        images = _images(shapes, C=C)
        _ORACLES[(name, C)] = (
            images, _pack(images).to(DEV),
            oracle_nhwc_f32(images, size, origin, out_size))
    return _ORACLES[(name, C)]


def _run(data_dev, shapes, sizes, out_size, origins, out_dtype, layout, C=3,
         **kw):
    return ops.image_u8_ragged_resize_to_float(
        data_dev, shapes, sizes, out_size, MEAN[:C], STD[:C],
        origins=origins, out_dtype=out_dtype, layout=layout, antialias=True,
        **kw)


def _check_batch(name, dtype, layout, C=3, **kw):
    shapes, size, origin, out_size = BATCHES[name]
    images, data_dev, ref = _batch(name, C)
    y = _run(data_dev, shapes, size, out_size, origin, DTYPES[dtype], layout,
             C, **kw)
    expected = _as(ref, DTYPES[dtype], layout)
    assert y.is_cuda and y.dtype == DTYPES[dtype] and y.is_contiguous()
    assert tuple(y.shape) == tuple(expected.shape)
    assert torch.equal(y.cpu(), expected)


def test_oracle_layout_and_dtype_shortcut_is_the_dense_op():
    # _as() derives every dtype / layout from the fp32 NHWC oracle; check it
    # against the dense CPU op called with that dtype and layout
    images, _, ref = _batch("mixed")
    for dtype in DTYPES.values():
        direct = torch.cat([ops.image_u8_resize_to_float(
            im.unsqueeze(0), (12, 20), MEAN[:3], STD[:3],
            crop=(2, 3, 8, 16), out_dtype=dtype, antialias=True)
            for im in images])
        assert torch.equal(_as(ref, dtype, "nchw"), direct)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_kernels_equal_dense_loop(C, dtype, layout):
    _check_batch("mixed", dtype, layout, C)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_scalar_workspace_loads_and_scalar_stores(dtype, layout):
    _check_batch("scalar_paths", dtype, layout)


def test_flag_reaches_the_filter():
    shapes, size, origin, out_size = BATCHES["mixed"]
    _, data_dev, ref = _batch("mixed")
    bilinear = ops.image_u8_ragged_resize_to_float(
        data_dev, shapes, size, out_size, MEAN[:3], STD[:3], origins=origin,
        layout="nhwc")
    assert not torch.equal(bilinear.cpu(), ref)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_per_image_sizes_and_origins(layout):
    images = _images(AA, seed=2)
    sizes = [(12, 21), (20, 33), (11, 13), (9, 40), (31, 10), (15, 15),
             (10, 25)]
    origins = [(1, 3), (5, 11), (0, 0), (0, 27), (22, 1), (3, 2), (1, 16)]
    ref = oracle_nhwc_f32(images, sizes, origins, (9, 9))
    y = _run(_pack(images).to(DEV), AA, np.array(sizes), (9, 9),
             torch.tensor(origins), torch.bfloat16, layout)
    assert torch.equal(y.cpu(), _as(ref, torch.bfloat16, layout))


def _table(shapes, sizes, origins, C):
    """The host table of the ragged ops, int32 [N,8]."""
    shp = np.asarray(shapes, dtype=np.int64)
    n = len(shp)
    siz, org = _pairs(sizes, n), _pairs(origins, n)
    offsets = np.zeros(n, dtype=np.int64)
    np.cumsum((shp[:, 0] * shp[:, 1] * C)[:-1], out=offsets[1:])
    t = np.zeros((n, 8), dtype=np.int32)
    t[:, 0:2] = offsets.astype("<i8").view("<i4").reshape(n, 2)
    t[:, 2:4] = shp
    t[:, 4:6] = org
    t[:, 6:8] = (shp / siz).astype(np.float32).view(np.int32)
    return torch.from_numpy(t), int((shp[:, 0] * shp[:, 1] * C).sum())


@pytest.mark.parametrize("cap,chunks", [(9000, [2, 3, 1, 1]),
                                        (1, [1] * 7)])
@pytest.mark.parametrize("dtype,layout", [("bf16", "nchw"), ("f32", "nhwc")])
def test_chunked_loop_equals_one_chunk(cap, chunks, dtype, layout):
    shapes, size, origin, out_size = BATCHES["mixed"]
    table, nbytes = _table(shapes, size, origin, 3)
    entries, plan = ops.require_native().u8_ragged_resize_aa_plan(
        table, nbytes, 3, 8, 16, cap)
    assert (entries[:, 15] * 16 * 3 * 4).tolist() == [
        1344, 7296, 1152, 192, 960, 9216, 4800]
    assert plan[:, 1].tolist() == chunks
    _check_batch("mixed", dtype, layout, _ws_cap_bytes=cap)
    uncapped = _run(_batch("mixed")[1], shapes, size, out_size, origin,
                    DTYPES[dtype], layout)
    capped = _run(_batch("mixed")[1], shapes, size, out_size, origin,
                  DTYPES[dtype], layout, _ws_cap_bytes=cap)
    assert torch.equal(capped, uncapped)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_single_image_equals_dense_device_op(dtype, layout):
    x = _images([(37, 53)], seed=3)[0].to(DEV)
    y = _run(x.reshape(-1), [(37, 53)], (16, 23), (12, 16), (2, 5),
             DTYPES[dtype], layout)
    dense = ops.image_u8_resize_to_float(
        x.unsqueeze(0), (16, 23), MEAN[:3], STD[:3], crop=(2, 5, 12, 16),
        out_dtype=DTYPES[dtype], layout=layout, antialias=True)
    assert torch.equal(y, dense)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_one_byte_storage_offset_and_unaligned_end(dtype, layout):
    images = _images(AA, seed=4)
    packed = _pack(images)
    n = packed.numel()
    assert n % 16 != 0 and (n + 1) % 16 != 0
    flat = torch.cat([torch.zeros(1, dtype=torch.uint8), packed]).to(DEV)
    view = flat[1:1 + n]
    assert view.is_contiguous() and view.data_ptr() % 16 == 1
    # no crop: the last row and column of the last image are tapped, so the
    # last byte of the buffer is read
    ref = oracle_nhwc_f32(images, (12, 20), (0, 0), (12, 20))
    y = _run(view, AA, (12, 20), (12, 20), None, DTYPES[dtype], layout)
    assert torch.equal(y.cpu(), _as(ref, DTYPES[dtype], layout))


@pytest.fixture(scope="module")
def many():
    cycle = [(6, 7), (3, 5), (40, 2), (1, 4)]
    shapes = [cycle[i % 4] for i in range(2100)]
    assert shapes[0] != shapes[-1]
    images = _images(shapes, seed=5)
    # the dense op treats the images of a batch independently: one CPU call
    # per distinct shape (525 images each) instead of 2100 calls
    ref = torch.empty((2100, 16, 128, 3), dtype=torch.float32)
    for k in range(4):
        ref[k::4] = ops.image_u8_resize_to_float(
            torch.stack(images[k::4]), (16, 128), MEAN[:3], STD[:3],
            layout="nhwc", antialias=True)
    return shapes, _pack(images).to(DEV), ref


@pytest.mark.parametrize("dtype,layout", [("bf16", "nchw"),
                                          ("f32", "nhwc")])
def test_grid_stride_second_iteration(many, dtype, layout):
    shapes, data_dev, ref = many
    y = _run(data_dev, shapes, (16, 128), (16, 128), None, DTYPES[dtype],
             layout)
    assert tuple(y.shape)[0] == 2100
    assert torch.equal(y.cpu(), _as(ref, DTYPES[dtype], layout))


def test_launches_and_table_copy_use_current_stream():
    shapes, size, origin, out_size = BATCHES["mixed"]
    _, data_dev, ref = _batch("mixed")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        y = _run(data_dev, shapes, size, out_size, origin, torch.float32,
                 "nchw")
    stream.synchronize()
    assert torch.equal(y.cpu(), _as(ref, torch.float32, "nchw"))


@pytest.mark.parametrize("layout,shape", [("nchw", (0, 3, 5, 7)),
                                          ("nhwc", (0, 5, 7, 3))])
def test_empty_batch_does_not_launch(layout, shape):
    data = torch.empty((0,), dtype=torch.uint8, device=DEV)
    y = _run(data, [], (9, 9), (5, 7), None, torch.bfloat16, layout)
    torch.cuda.synchronize()
    assert y.is_cuda and tuple(y.shape) == shape
    assert y.dtype == torch.bfloat16


def test_image_shapes_as_device_tensor():
    shapes, size, origin, out_size = BATCHES["mixed"]
    _, data_dev, ref = _batch("mixed")
    shapes_dev = torch.tensor(shapes, dtype=torch.int32, device=DEV)
    y = _run(data_dev, shapes_dev, size, out_size, origin, torch.bfloat16,
             "nchw")
    assert torch.equal(y.cpu(), _as(ref, torch.bfloat16, "nchw"))


def test_device_tensor_errors_are_value_errors():
    def op(*a, **kw):
        return ops.image_u8_ragged_resize_to_float(*a, antialias=True, **kw)

    m, s = MEAN[:3], STD[:3]
    shapes = [(4, 5), (6, 3)]
    data = torch.zeros((114,), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        op(data.float(), shapes, (8, 8), (8, 8), m, s)
    with pytest.raises(ValueError):
        op(data.view(2, 57), shapes, (8, 8), (8, 8), m, s)
    with pytest.raises(ValueError):
        op(torch.zeros((228,), dtype=torch.uint8, device=DEV)[::2], shapes,
           (8, 8), (8, 8), m, s)                                 # strided
    with pytest.raises(ValueError):
        op(data, shapes, (8, 8), (8, 8), (0.5,) * 5, (0.5,) * 5)
    with pytest.raises(ValueError):
        op(data, shapes, (8, 8), (8, 8), m, STD[:2])
    with pytest.raises(ValueError, match="image 1"):
        op(data, [(4, 5), (0, 3)], (8, 8), (8, 8), m, s)
    with pytest.raises(ValueError, match="image 1"):
        op(data, shapes, [(8, 8), (8, 16385)], (8, 8), m, s)
    # the byte count, one byte either way: raised before any launch
    with pytest.raises(ValueError, match="bytes"):
        op(data[:-1], shapes, (8, 8), (8, 8), m, s)
    with pytest.raises(ValueError, match="bytes"):
        op(torch.zeros((115,), dtype=torch.uint8, device=DEV), shapes,
           (8, 8), (8, 8), m, s)
    with pytest.raises(ValueError, match="image 1"):
        op(data, shapes, [(8, 8), (8, 7)], (8, 8), m, s)
    with pytest.raises(ValueError):
        op(data, shapes, (8, 8), (8, 8), m, s, layout="chw")
    with pytest.raises(ValueError):
        op(data, shapes, (8, 8), (8, 8), m, s, out_dtype=torch.float64)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# end to end through the raw server (mirrors test_gpu_image_ragged.py)
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def server(tmp_path_factory):
    sock = f"unix://{tmp_path_factory.mktemp('s')}/ragged_aa.sock"
    with ModelServer(address=sock, raw_predict=True, device=DEV) as srv:
        pre = AntialiasedRaggedImagePreprocess(
            MEAN[:3], STD[:3], out_dtype=torch.bfloat16, layout="nchw",
            device=DEV, resize=(12, 20), center_crop=(8, 16))
        srv.manager.load(
            "pre",
            Servable(lambda inputs: {"images": inputs["images"]},
                     preprocess={("images", "image_shapes"): pre}),
            version=1)
        srv.manager.load(
            "resnet50_ragged_aa",
            resnet50_servable(DEV, torch.bfloat16,
                              input_format="uint8_ragged_antialias"),
            version=1)
        yield srv


def test_predict_ragged_antialias_end_to_end(server):
    images = _batch("mixed")[0]
    # the centre crop of (12,20) to (8,16) starts at (2,2)
    ref = oracle_nhwc_f32(images, (12, 20), (2, 2), (8, 16))
    data, shapes = pack_ragged_images([im.numpy() for im in images])
    with TurboPredictClient(server.address) as client:
        out = client.predict(
            "pre", {"images": torch.from_numpy(data).to(DEV),
                    "image_shapes": torch.from_numpy(shapes)},
            output_device=DEV)
    y = out["images"]
    assert y.is_cuda and y.dtype == torch.bfloat16
    assert tuple(y.shape) == (7, 3, 8, 16)
    assert torch.equal(y.cpu(), _as(ref, torch.bfloat16, "nchw"))


def test_resnet50_ragged_antialias_mode_end_to_end(server):
    images = _images([(160, 200), (300, 256), (256, 341)], seed=6)
    data, shapes = pack_ragged_images([im.numpy() for im in images])
    with TurboPredictClient(server.address) as client:
        out = client.predict(
            "resnet50_ragged_aa", {"images": torch.from_numpy(data),
                                   "image_shapes": torch.from_numpy(shapes)},
            output_device=DEV)
    logits = out["logits"]
    assert tuple(logits.shape) == (3, 1000)
    assert logits.dtype == torch.float32
    assert bool(torch.isfinite(logits).all())
