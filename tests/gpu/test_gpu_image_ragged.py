"""Ragged uint8 image batches on the GPU: the u8_ragged_resize_normalize
kernel (N images of N sizes, one launch) against the dense op run on CPU for
each image alone (exact equality), then end to end through the raw server
and the ResNet-50 ``uint8_ragged`` mode.

Paths of the kernel and the smallest batch here that reaches each (a batch
is a list of (Hin,Win) -> resized size / crop window, C = 3 unless noted):

* per-image table: MIXED, [(7,9),(17,31),(8,8),(1,5),(5,1),(64,48)] ->
  (24,40), crop (4,4,16,32), mixes up- and downscales, one source row and one
  source column; its first image has 189 bytes, so every later image starts
  off 16 B alignment. Run with C in 1..4.
* taps from LDS or gathered directly, chosen per work item from the item's
  own span: SPANS, [(4,677),(4,678),(8,1024),(4,100)] -> (4,256), has the
  widest span that fits the 32 KiB budget (2 x 8 spans of 2048 B), the first
  that does not, a 4x downscale far past it and a small LDS item behind
  them, all in one launch.
* tile geometry, chosen from the output width Wc and shared by the batch:
  8 lane runs x 32 rows for Wc <= 64 (most batches), 16 x 16 for out
  (20,100), 32 x 8 for out (10,200); two column tiles with a ragged last one
  for out (5,290); two row tiles for out (40,24).
* stores: 16 B vectors, or scalar for a run that crosses the row end and an
  NCHW plane that is not 16 B-aligned: out (20,33), plane of 660 elements.
* LDS fill: aligned 16 B loads tested against the bounds of the whole flat
  buffer, except a chunk that is not wholly inside it, which is read
  bytewise: the first chunk of a view that starts 1 byte off 16 B alignment
  and the last chunk of the last image when the buffer end is not 16
  B-aligned (MIXED resized without a crop reads the last pixel of the last
  image).
* grid-stride loop: 2100 tiny images, one tile each, more work items than
  the 2048 workgroups of the capped grid; sizes cycle through four shapes so
  the first image differs from the last and a wrong table index shows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from min_tfs_client_amd import ops  # noqa: E402
from min_tfs_client_amd.models import resnet50_servable  # noqa: E402
from min_tfs_client_amd.preprocess import (IMAGENET_MEAN,  # noqa: E402
                                           IMAGENET_STD,
                                           RaggedImagePreprocess,
                                           pack_ragged_images)
from min_tfs_client_amd.server import ModelServer, Servable  # noqa: E402
from min_tfs_client_amd.turbo import TurboPredictClient  # noqa: E402

DEV = "cuda:0"
MEAN = (0.485, 0.456, 0.406, 0.5)
STD = (0.229, 0.224, 0.225, 0.25)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16,
          "f16": torch.float16}

MIXED = [(7, 9), (17, 31), (8, 8), (1, 5), (5, 1), (64, 48)]
SPANS = [(4, 677), (4, 678), (8, 1024), (4, 100)]
WIDE = [(9, 40), (6, 90), (3, 150), (7, 9)]
# name -> (input shapes, resized size, (top, left), output size)
BATCHES = {
    "mixed": (MIXED, (24, 40), (4, 4), (16, 32)),
    "lds_and_direct": (SPANS, (4, 256), (0, 0), (4, 256)),
    "tile16": (WIDE, (20, 100), (0, 0), (20, 100)),
    "tile32": (WIDE, (10, 200), (0, 0), (10, 200)),
    "two_column_tiles": (WIDE, (5, 290), (0, 0), (5, 290)),
    "two_row_tiles": (MIXED, (40, 24), (0, 0), (40, 24)),
    "scalar_stores": (MIXED, (20, 33), (0, 0), (20, 33)),
}
ALL_DTYPES = ("mixed", "lds_and_direct", "tile16")


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
    """The dense op on CPU, one image at a time: fp32 NHWC."""
    n = len(images)
    C = images[0].shape[2]
    sizes, origins = _pairs(sizes, n), _pairs(origins, n)
    return torch.cat([ops.image_u8_resize_to_float(
        im.unsqueeze(0), tuple(int(v) for v in sizes[i]), MEAN[:C], STD[:C],
        crop=(int(origins[i][0]), int(origins[i][1])) + tuple(out_size),
        layout="nhwc") for i, im in enumerate(images)])


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


def _run(data_dev, shapes, sizes, out_size, origins, out_dtype, layout, C=3):
    return ops.image_u8_ragged_resize_to_float(
        data_dev, shapes, sizes, out_size, MEAN[:C], STD[:C],
        origins=origins, out_dtype=out_dtype, layout=layout)


def _check_batch(name, dtype, layout, C=3):
    shapes, size, origin, out_size = BATCHES[name]
    images, data_dev, ref = _batch(name, C)
    y = _run(data_dev, shapes, size, out_size, origin, DTYPES[dtype], layout,
             C)
    expected = _as(ref, DTYPES[dtype], layout)
    assert y.is_cuda and y.dtype == DTYPES[dtype] and y.is_contiguous()
    assert tuple(y.shape) == tuple(expected.shape)
    assert torch.equal(y.cpu(), expected)


def test_oracle_layout_and_dtype_shortcut_is_the_dense_op():
    # _as() derives every dtype / layout from the fp32 NHWC oracle; check it
    # against the dense CPU op called with that dtype and layout
    images = _images(MIXED)
    ref = oracle_nhwc_f32(images, (24, 40), (4, 4), (16, 32))
    for dtype in DTYPES.values():
        direct = torch.cat([ops.image_u8_resize_to_float(
            im.unsqueeze(0), (24, 40), MEAN[:3], STD[:3],
            crop=(4, 4, 16, 32), out_dtype=dtype) for im in images])
        assert torch.equal(_as(ref, dtype, "nchw"), direct)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", ALL_DTYPES)
def test_kernel_equals_dense_loop(name, dtype, layout):
    _check_batch(name, dtype, layout)


@pytest.mark.parametrize("dtype,layout", [("bf16", "nchw"), ("f32", "nhwc")])
@pytest.mark.parametrize("name",
                         [n for n in BATCHES if n not in ALL_DTYPES])
def test_kernel_tile_geometries_and_stores(name, dtype, layout):
    _check_batch(name, dtype, layout)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("C", [1, 2, 4])
def test_kernel_channels(C, layout):
    _check_batch("mixed", "bf16", layout, C)
    _check_batch("mixed", "f32", layout, C)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_per_image_sizes_and_origins(layout):
    images = _images(MIXED, seed=2)
    sizes = [(12, 21), (20, 33), (11, 13), (9, 40), (31, 10), (15, 15)]
    origins = [(1, 3), (5, 11), (0, 0), (0, 27), (22, 1), (3, 2)]
    ref = oracle_nhwc_f32(images, sizes, origins, (9, 9))
    y = _run(_pack(images).to(DEV), MIXED, np.array(sizes), (9, 9),
             torch.tensor(origins), torch.bfloat16, layout)
    assert torch.equal(y.cpu(), _as(ref, torch.bfloat16, layout))


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_single_image_equals_dense_device_op(dtype, layout):
    x = _images([(37, 53)], seed=3)[0].to(DEV)
    y = _run(x.reshape(-1), [(37, 53)], (32, 46), (24, 24), (4, 11),
             DTYPES[dtype], layout)
    dense = ops.image_u8_resize_to_float(
        x.unsqueeze(0), (32, 46), MEAN[:3], STD[:3], crop=(4, 11, 24, 24),
        out_dtype=DTYPES[dtype], layout=layout)
    assert torch.equal(y, dense)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_one_byte_storage_offset_and_unaligned_end(dtype, layout):
    images = _images(MIXED, seed=4)
    packed = _pack(images)
    n = packed.numel()
    assert n % 16 != 0 and (n + 1) % 16 != 0
    flat = torch.cat([torch.zeros(1, dtype=torch.uint8), packed]).to(DEV)
    view = flat[1:1 + n]
    assert view.is_contiguous() and view.data_ptr() % 16 == 1
    # no crop: the last row and column of the last image are tapped, so the
    # last chunk of the buffer is read
    ref = oracle_nhwc_f32(images, (24, 40), (0, 0), (24, 40))
    y = _run(view, MIXED, (24, 40), (24, 40), None, DTYPES[dtype], layout)
    assert torch.equal(y.cpu(), _as(ref, DTYPES[dtype], layout))


@pytest.fixture(scope="module")
def many():
    cycle = [(6, 7), (3, 5), (5, 2), (1, 4)]
    shapes = [cycle[i % 4] for i in range(2100)]
    assert shapes[0] != shapes[-1]
    images = _images(shapes, seed=5)
    # the dense op treats the images of a batch independently: one CPU call
    # per distinct shape instead of 2100 calls
    ref = torch.empty((2100, 4, 8, 3), dtype=torch.float32)
    for k in range(4):
        ref[k::4] = ops.image_u8_resize_to_float(
            torch.stack(images[k::4]), (4, 8), MEAN[:3], STD[:3],
            layout="nhwc")
    return shapes, _pack(images).to(DEV), ref


@pytest.mark.parametrize("dtype,layout", [("bf16", "nchw"),
                                          ("f32", "nhwc")])
def test_grid_stride_second_iteration(many, dtype, layout):
    shapes, data_dev, ref = many
    y = _run(data_dev, shapes, (4, 8), (4, 8), None, DTYPES[dtype], layout)
    assert tuple(y.shape)[0] == 2100
    assert torch.equal(y.cpu(), _as(ref, DTYPES[dtype], layout))


def test_launch_and_table_copy_use_current_stream():
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


def test_device_tensor_errors_are_value_errors():
    op = ops.image_u8_ragged_resize_to_float
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
    with pytest.raises(ValueError):
        op(data, [4, 5, 6, 3], (8, 8), (8, 8), m, s)
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
    with pytest.raises(ValueError):
        op(data, shapes, [(8, 8)] * 3, (8, 8), m, s)
    with pytest.raises(ValueError):
        op(data, shapes, (8, 8), (8, 8), m, s, origins=(0,))
    with pytest.raises(ValueError, match="image 1"):
        op(data, shapes, [(8, 8), (8, 7)], (8, 8), m, s)
    with pytest.raises(ValueError):
        op(data, shapes, (8, 8), (8, 8), m, s, layout="chw")
    with pytest.raises(ValueError):
        op(data, shapes, (8, 8), (8, 8), m, s, out_dtype=torch.float64)
    torch.cuda.synchronize()


def test_image_shapes_as_device_tensor():
    shapes, size, origin, out_size = BATCHES["mixed"]
    _, data_dev, ref = _batch("mixed")
    shapes_dev = torch.tensor(shapes, dtype=torch.int32, device=DEV)
    y = _run(data_dev, shapes_dev, size, out_size, origin, torch.bfloat16,
             "nchw")
    assert torch.equal(y.cpu(), _as(ref, torch.bfloat16, "nchw"))


# ---------------------------------------------------------------------------
# end to end through the raw server (mirrors test_gpu_image_resize.py)
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def resnet_ragged():
    return resnet50_servable(DEV, torch.bfloat16, input_format="uint8_ragged")


@pytest.fixture(scope="module")
def server(tmp_path_factory, resnet_ragged):
    sock = f"unix://{tmp_path_factory.mktemp('s')}/ragged.sock"
    with ModelServer(address=sock, raw_predict=True, device=DEV) as srv:
        pre = RaggedImagePreprocess(
            MEAN[:3], STD[:3], out_dtype=torch.bfloat16, layout="nchw",
            device=DEV, resize=(24, 40), center_crop=(16, 32))
        srv.manager.load(
            "pre",
            Servable(lambda inputs: {"images": inputs["images"]},
                     preprocess={("images", "image_shapes"): pre}),
            version=1)
        srv.manager.load("resnet50_ragged", resnet_ragged, version=1)
        yield srv


def test_predict_ragged_end_to_end(server):
    _, _, ref = _batch("mixed")        # (24,40), centre crop = (4,4,16,32)
    data, shapes = pack_ragged_images(
        [im.numpy() for im in _batch("mixed")[0]])
    with TurboPredictClient(server.address) as client:
        out = client.predict(
            "pre", {"images": torch.from_numpy(data).to(DEV),
                    "image_shapes": torch.from_numpy(shapes)},
            output_device=DEV)
    y = out["images"]
    assert y.is_cuda and y.dtype == torch.bfloat16
    assert tuple(y.shape) == (6, 3, 16, 32)
    assert torch.equal(y.cpu(), _as(ref, torch.bfloat16, "nchw"))


def test_resnet50_ragged_mode_end_to_end(server):
    images = _images([(160, 200), (300, 256), (256, 341)], seed=6)
    data, shapes = pack_ragged_images([im.numpy() for im in images])
    with TurboPredictClient(server.address) as client:
        out = client.predict(
            "resnet50_ragged", {"images": torch.from_numpy(data),
                                "image_shapes": torch.from_numpy(shapes)},
            output_device=DEV)
    logits = out["logits"]
    assert tuple(logits.shape) == (3, 1000)
    assert logits.dtype == torch.float32
    assert bool(torch.isfinite(logits).all())


def test_resnet50_ragged_mode_preprocess_is_center_crop(resnet_ragged):
    # 256 x 256 is already the resized size: only the 224 centre crop is left
    g = torch.Generator().manual_seed(7)
    x = torch.randint(0, 256, (3, 256, 256, 3), dtype=torch.uint8,
                      generator=g).to(DEV)
    pre = resnet_ragged.preprocess[("images", "image_shapes")]
    y = pre(x.reshape(-1), [(256, 256)] * 3)
    same = ops.image_u8_to_float(
        x[:, 16:240, 16:240, :].contiguous(), IMAGENET_MEAN, IMAGENET_STD,
        out_dtype=torch.bfloat16)
    assert tuple(y.shape) == (3, 3, 224, 224)
    assert torch.equal(y, same)
