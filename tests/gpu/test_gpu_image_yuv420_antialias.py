"""Antialiased resize of YUV 4:2:0 (NV12 / I420) frames on the GPU: the
yuv420_resize_aa_h_kernel + u8_resize_aa_v_kernel pair against a reference
assembled here, exact equality everywhere. The reference converts with an
int32 numpy expression written in this file and feeds the bytes to the CPU
path of ``ops.image_u8_resize_to_float(..., antialias=True)``, which
tests/unit/test_image_resize_antialias.py pins tap by tap. Then end to end
through the raw server and the ResNet-50 ``nv12_resize_antialias`` /
``i420_resize_antialias`` modes.

Paths of the horizontal kernel and the smallest shape here that reaches each
(shapes are frames (N,H,W), stored as uint8 [N,H*3/2,W], -> size / crop):

* tile geometry from the output width Wc, the widest tile of 8..64 columns
  that pads Wc by at most 1/8, else 8 columns: 8 columns x 32 source rows
  for Wc = 20, 24 and everything below 8 (most shapes), 16 x 16 for Wc = 16
  ((2,48,64) cropped) and 45 ((1,20,30) -> (40,45)), 32 x 8 for Wc = 32
  ((2,12,70) -> (6,32)), 64 x 4 for Wc = 60 ((1,40,30) -> (10,60)) and 128;
  a ragged last column tile (Wc = 20: 8 + 8 + 4), a ragged last row tile and
  two row tiles (Rs = 38 on 32-row tiles).
* taps from LDS (variant 0): the workgroup converts the tile's column span
  of each of its source rows once, in 16-pixel chunks from the even column at
  or below the first tap, so an odd first tap ((2,38,54) -> (32,46) crop
  (3,11,24,24)) starts one pixel early. The budget is 16 KiB: with 8 x 32
  tiles a row holds floor(512 / 48) = 10 chunks = 160 pixels, one of which is
  kept for the even start, and for (1,2,W) -> (2,2) the host's span estimate
  is W: (1,2,158) is the widest frame whose span still fits, (1,2,160) the
  first that does not; (1,2,4096) and (1,2,16384) are far past it and take
  the direct path whatever the variant.
* taps converted one by one from global memory with byte loads (variant 1
  forces this everywhere): every case runs in both variants.
* LDS fill: unaligned 16 B luma and 16 B (NV12) or 2 x 8 B (I420) chroma
  loads, except a chunk whose loads would pass the end of the tensor, which
  is read bytewise: all of (1,2,2) (6 bytes) and the last rows of any
  tensor; W = 18 and 6 give I420 chroma rows of odd length and planes that
  end in mid-row; a view that starts 1 byte into its storage moves
  everything to odd addresses.
* work items are (frame, row tile, column tile), at most 2048 workgroups:
  (33,128,256) -> (64,128) has Rs = 128, 64 x 4 tiles, 33 * 32 * 2 = 2112
  items, so the grid-stride loop runs a second iteration (1.6 MB of input).
* workspace chunks: 5 frames through a workspace of 2 frames, and of 1."""
import functools

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
LAYOUTS = ["nchw", "nhwc"]
CHROMAS = ["nv12", "i420"]
VARIANTS = {"lds": 0, "direct": 1}
# C offset, then the coefficients of C, (D, E) for R, G, B
MATRICES = {
    "bt601": (16, 298, (0, 409), (-100, -208), (516, 0)),
    "bt709": (16, 298, (0, 459), (-55, -136), (541, 0)),
    "bt601_full": (0, 256, (0, 359), (-88, -183), (454, 0)),
}


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


def reference_nhwc_f32(x, size, crop, chroma, matrix):
    """fp32 NHWC: numpy conversion, then the pinned CPU antialiased op."""
    rgb = torch.from_numpy(reference_rgb(x.cpu().numpy(), chroma, matrix))
    assert not rgb.is_cuda
    if size is None:
        size = tuple(rgb.shape[1:3])
    return ops.image_u8_resize_to_float(
        rgb, size, MEAN, STD, crop=crop, out_dtype=torch.float32,
        layout="nhwc", antialias=True)


def _as(ref_nhwc_f32, out_dtype, layout):
    y = ref_nhwc_f32
    if layout == "nchw":
        y = y.permute(0, 3, 1, 2)
    return y.to(out_dtype).contiguous()


@functools.lru_cache(maxsize=None)
def _frames(n, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h * 3 // 2, w), dtype=torch.uint8,
                         generator=g)


@functools.lru_cache(maxsize=None)
def _cached_ref(shape, seed, size, crop, chroma, matrix):
    # computed once per case and shared; never modified (_as copies)
    return reference_nhwc_f32(_frames(*shape, seed=seed), size, crop, chroma,
                              matrix)


def _run(x_dev, size, crop, out_dtype, layout, chroma, matrix="bt601",
         variant=0, ws_cap=None):
    return ops.image_yuv420_resize_to_float(
        x_dev, size, MEAN, STD, crop=crop, out_dtype=out_dtype,
        layout=layout, _variant=variant, chroma=chroma, matrix=matrix,
        antialias=True, _ws_cap_bytes=ws_cap)


def _check(y, ref_nhwc_f32, out_dtype, layout):
    ref = _as(ref_nhwc_f32, out_dtype, layout)
    assert y.is_cuda and y.dtype == out_dtype and y.is_contiguous()
    assert tuple(y.shape) == tuple(ref.shape)
    assert torch.equal(y.cpu(), ref)


def _check_all(x_dev, ref, size, crop, chroma, matrix="bt601", variant=0,
               combos=None):
    for dtype, layout in combos or [(d, la) for d in DTYPES
                                    for la in LAYOUTS]:
        y = _run(x_dev, size, crop, DTYPES[dtype], layout, chroma, matrix,
                 variant)
        _check(y, ref, DTYPES[dtype], layout)


CASES = [
    ((2, 38, 54), (16, 20), None),          # non-integer ratios, ragged run
    ((2, 48, 64), (24, 32), (4, 8, 16, 16)),    # workspace from a row > 0
    ((2, 38, 54), (32, 46), (3, 11, 24, 24)),   # odd offsets, odd first tap
    ((1, 20, 30), (40, 45), None),          # upscale, support 1
    ((1, 40, 30), (10, 60), None),          # down on one axis, up on the other
    ((2, 12, 70), (6, 32), None),           # 32-column tiles
    ((1, 34, 48), (5, 3), None),            # many taps, Wc < 8
    ((1, 10, 10), (1, 1), None),            # one output pixel
    ((1, 2, 2), None, None),                # 6 bytes: no wide load fits
    ((1, 2, 2), (5, 7), None),
    ((2, 6, 18), (4, 7), None),             # I420 chroma rows of 9 bytes
    ((3, 10, 6), (7, 5), None),             # W/2 = 3, H/2 = 5
    ((1, 2, 158), (2, 2), None),            # widest span inside the budget
    ((1, 2, 160), (2, 2), None),            # first span past it
    ((1, 2, 4096), (2, 2), None),           # about 4096 taps per column
    ((1, 2, 16384), (2, 2), None),          # 49 KB: direct fallback
]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("shape,size,crop", CASES, ids=str)
def test_kernel_matches_reference(shape, size, crop, chroma, variant):
    x = _frames(*shape)
    ref = _cached_ref(shape, 0, size, crop, chroma, "bt601")
    _check_all(x.to(DEV), ref, size, crop, chroma,
               variant=VARIANTS[variant])


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("chroma", CHROMAS)
def test_identity_equals_plain_normalize_on_device(chroma, variant):
    x = _frames(2, 8, 16, seed=1).to(DEV)
    rgb = ops.yuv420_to_rgb_u8(x, chroma, "bt601")
    for dtype in DTYPES.values():
        for layout in LAYOUTS:
            y = _run(x, None, None, dtype, layout, chroma,
                     variant=VARIANTS[variant])
            want = ops.image_u8_to_float(rgb, MEAN, STD, out_dtype=dtype,
                                         layout=layout)
            assert torch.equal(y, want)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_equals_rgb_antialiased_kernel_on_converted_frames_on_device(
        dtype, chroma, variant):
    x = _frames(2, 38, 54, seed=3).to(DEV)
    y = _run(x, (16, 20), (2, 3, 12, 16), DTYPES[dtype], "nchw", chroma,
             "bt709", VARIANTS[variant])
    rgb = ops.yuv420_to_rgb_u8(x, chroma, "bt709")
    assert rgb.is_cuda
    assert torch.equal(rgb.cpu(), torch.from_numpy(
        reference_rgb(x.cpu().numpy(), chroma, "bt709")))
    same = ops.image_u8_resize_to_float(
        rgb, (16, 20), MEAN, STD, crop=(2, 3, 12, 16),
        out_dtype=DTYPES[dtype], antialias=True)
    assert torch.equal(y, same)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("matrix", list(MATRICES))
def test_matrices_and_clamps(matrix, chroma, variant):
    # random bytes are valid frames and reach both clamps in every channel;
    # one frame of all 0 and one of all 255 pin the extremes
    x = _frames(3, 12, 22, seed=2).clone()
    x[1] = 0
    x[2] = 255
    rgb = reference_rgb(x.numpy(), chroma, matrix)
    assert rgb.min() == 0 and rgb.max() == 255
    for size in (None, (5, 9)):
        ref = reference_nhwc_f32(x, size, None, chroma, matrix)
        _check_all(x.to(DEV), ref, size, None, chroma, matrix,
                   VARIANTS[variant], combos=[("f32", "nchw"),
                                              ("bf16", "nhwc")])


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("size", [None, (7, 8)], ids=str)
def test_one_byte_storage_offset(size, chroma, variant):
    n = 2 * 24 * 18
    flat = torch.randint(0, 256, (n + 16,), dtype=torch.uint8,
                         generator=torch.Generator().manual_seed(4)).to(DEV)
    x_dev = flat[1:1 + n].view(2, 24, 18)
    assert x_dev.is_contiguous() and x_dev.data_ptr() % 16 == 1
    ref = reference_nhwc_f32(x_dev.cpu(), size, None, chroma, "bt601")
    _check_all(x_dev, ref, size, None, chroma, variant=VARIANTS[variant])


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("chroma", CHROMAS)
def test_chunked_workspace_equals_unchunked(chroma, variant):
    shape, size = (5, 38, 54), (16, 20)
    x_dev = _frames(*shape).to(DEV)
    ref = _cached_ref(shape, 0, size, None, chroma, "bt601")
    v = VARIANTS[variant]
    whole = _run(x_dev, size, None, torch.float32, "nchw", chroma, variant=v)
    _check(whole, ref, torch.float32, "nchw")
    per_image = 38 * 20 * 3 * 4          # Rs = Hin = 38 source rows
    for cap in (per_image * 5 // 2, 1):  # chunks of 2 + 2 + 1, then of 1
        y = _run(x_dev, size, None, torch.float32, "nchw", chroma, variant=v,
                 ws_cap=cap)
        assert torch.equal(y, whole)


@pytest.fixture(scope="module")
def large():
    shape, size = (33, 128, 256), (64, 128)
    x = _frames(*shape, seed=6)
    return x.to(DEV), size, {c: reference_nhwc_f32(x, size, None, c, "bt601")
                             for c in CHROMAS}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("dtype,layout,chroma", [("bf16", "nchw", "nv12"),
                                                 ("f32", "nhwc", "i420")])
def test_grid_stride_second_iteration(large, dtype, layout, chroma, variant):
    x_dev, size, refs = large
    y = _run(x_dev, size, None, DTYPES[dtype], layout, chroma,
             variant=VARIANTS[variant])
    _check(y, refs[chroma], DTYPES[dtype], layout)


@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("n", [0, 1, 3])
def test_batch_sizes(n, chroma):
    x = _frames(n, 8, 12, seed=5)
    for v in VARIANTS.values():
        y = _run(x.to(DEV), (5, 7), None, torch.bfloat16, "nchw", chroma,
                 variant=v)
        torch.cuda.synchronize()
        assert y.is_cuda and tuple(y.shape) == (n, 3, 5, 7)
        assert y.dtype == torch.bfloat16
        if n:
            ref = reference_nhwc_f32(x, (5, 7), None, chroma, "bt601")
            _check(y, ref, torch.bfloat16, "nchw")
    empty = _run(x.to(DEV)[:0], (5, 7), None, torch.float32, "nhwc", chroma)
    assert tuple(empty.shape) == (0, 5, 7, 3)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_launch_uses_current_stream(variant):
    x = _frames(4, 18, 30, seed=7)
    x_dev = x.to(DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        y = _run(x_dev, (7, 11), None, torch.float32, "nchw", "nv12",
                 variant=VARIANTS[variant])
    stream.synchronize()
    ref = reference_nhwc_f32(x, (7, 11), None, "nv12", "bt601")
    _check(y, ref, torch.float32, "nchw")


def test_device_tensor_errors_are_value_errors():
    def op(*args, **kwargs):
        return ops.image_yuv420_resize_to_float(*args, antialias=True,
                                                **kwargs)
    ok = torch.zeros((1, 6, 4), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        op(torch.zeros((1, 6, 8), dtype=torch.uint8, device=DEV)[:, :, :4],
           (4, 4), MEAN, STD)                                # strided
    with pytest.raises(ValueError):
        op(ok.float(), (4, 4), MEAN, STD)
    with pytest.raises(ValueError):
        op(torch.zeros((1, 7, 4), dtype=torch.uint8, device=DEV), (4, 4),
           MEAN, STD)                                        # rows % 3
    with pytest.raises(ValueError):
        op(torch.zeros((1, 6, 5), dtype=torch.uint8, device=DEV), (4, 4),
           MEAN, STD)                                        # odd W
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
    modes = {mode: resnet50_servable(DEV, torch.bfloat16, seed=0,
                                     input_format=mode)
             for mode in ("nv12_resize_antialias", "i420_resize_antialias")}
    modes["rgb_antialias"] = resnet50_servable(
        DEV, torch.bfloat16, seed=0, input_format="uint8_nhwc_resize",
        antialias=True)
    return modes


@pytest.fixture(scope="module")
def server(tmp_path_factory, resnets):
    sock = f"unix://{tmp_path_factory.mktemp('s')}/yuvaa.sock"
    with ModelServer(address=sock, raw_predict=True, device=DEV) as srv:
        pre = Yuv420ImagePreprocess(MEAN, STD, out_dtype=torch.bfloat16,
                                    layout="nchw", device=DEV,
                                    resize=(24, 40), center_crop=(16, 32),
                                    chroma="i420", matrix="bt709",
                                    antialias=True)
        srv.manager.load(
            "pre",
            Servable(lambda inputs: {"images": inputs["images"]},
                     preprocess={"images": pre}),
            version=1)
        for mode, servable in resnets.items():
            srv.manager.load(mode, servable, version=1)
        yield srv


def test_predict_yuv_antialias_preprocess_end_to_end(server):
    x = _frames(4, 64, 48, seed=8)
    with TurboPredictClient(server.address) as client:
        out = client.predict("pre", {"images": x.to(DEV)},
                             output_device=DEV)
    y = out["images"]
    assert tuple(y.shape) == (4, 3, 16, 32)
    ref = reference_nhwc_f32(x, (24, 40), (4, 4, 16, 32), "i420", "bt709")
    _check(y, ref, torch.bfloat16, "nchw")


@pytest.fixture
def deterministic_convolutions():
    # as in test_gpu_image_yuv420.py: without deterministic algorithms two
    # forwards of one ResNet-50 differ in the last bits on this stack
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.mark.parametrize("chroma", CHROMAS)
def test_resnet50_yuv_antialias_modes_equal_rgb_mode_on_converted_frames(
        server, deterministic_convolutions, chroma):
    x = _frames(2, 160, 200, seed=9)
    rgb = torch.from_numpy(reference_rgb(x.numpy(), chroma, "bt601"))
    with TurboPredictClient(server.address) as client:
        got = client.predict(f"{chroma}_resize_antialias",
                             {"images": x.to(DEV)},
                             output_device=DEV)["logits"]
        want = client.predict("rgb_antialias", {"images": rgb.to(DEV)},
                              output_device=DEV)["logits"]
    assert tuple(got.shape) == (2, 1000) and got.dtype == torch.float32
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
