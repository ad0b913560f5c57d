"""ResNet-50 (v1.5) in plain PyTorch — the BASELINE config-2 model family.

Written from scratch (no torchvision in this environment); standard
bottleneck architecture, random-init weights, NCHW fp32/bf16 inference.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..preprocess import (IMAGENET_MEAN, IMAGENET_STD,
                          AntialiasedRaggedImagePreprocess, ImagePreprocess,
                          RaggedImagePreprocess, Yuv420ImagePreprocess)

_RAGGED_MODES = {"uint8_ragged": RaggedImagePreprocess,
                 "uint8_ragged_antialias": AntialiasedRaggedImagePreprocess}
# mode -> (chroma layout, antialiased filter)
_YUV_MODES = {"nv12_resize": ("nv12", False), "i420_resize": ("i420", False),
              "nv12_resize_antialias": ("nv12", True),
              "i420_resize_antialias": ("i420", True)}


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, in_ch: int, width: int, stride: int = 1):
        super().__init__()
        out_ch = width * self.expansion
        self.conv1 = nn.Conv2d(in_ch, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1,
                               bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, out_ch, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(out_ch)
        self.relu = nn.ReLU(inplace=True)
        if stride != 1 or in_ch != out_ch:
            self.downsample = nn.Sequential(
                nn.Conv2d(in_ch, out_ch, 1, stride=stride, bias=False),
                nn.BatchNorm2d(out_ch))
        else:
            self.downsample = None

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class ResNet(nn.Module):
    def __init__(self, layers, num_classes: int = 1000):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.in_ch = 64
        self.layer1 = self._make_layer(64, layers[0], 1)
        self.layer2 = self._make_layer(128, layers[1], 2)
        self.layer3 = self._make_layer(256, layers[2], 2)
        self.layer4 = self._make_layer(512, layers[3], 2)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(512 * Bottleneck.expansion, num_classes)

    def _make_layer(self, width, blocks, stride):
        layers = [Bottleneck(self.in_ch, width, stride)]
        self.in_ch = width * Bottleneck.expansion
        for _ in range(blocks - 1):
            layers.append(Bottleneck(self.in_ch, width))
        return nn.Sequential(*layers)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = self.avgpool(x).flatten(1)
        return self.fc(x)


def resnet50(num_classes: int = 1000) -> ResNet:
    return ResNet([3, 4, 6, 3], num_classes)


def resnet50_servable(device: str = "cpu", dtype=torch.float32,
                      seed: int = 0, input_format: str = "float_nchw",
                      antialias: bool = False, output_format: str = "logits",
                      top_k: int = 5, yuv_matrix: str = "bt601"):
    """ResNet-50 Servable: input alias "images", output "logits" (N,1000).

    ``input_format="float_nchw"`` (default): "images" is DT_FLOAT
    (N,3,224,224), already normalized by the client.
    ``input_format="uint8_nhwc"``: "images" is DT_UINT8 (N,224,224,3) raw
    pixels — a quarter of the wire and H2D bytes; the server applies the
    ImageNet normalization and NHWC->NCHW in one fused kernel
    (``preprocess.ImagePreprocess``) before the model.
    ``input_format="uint8_nhwc_resize"``: "images" is DT_UINT8 (N,H,W,3) raw
    pixels of any size; the same kernel pass also resizes the shorter side
    to 256 (bilinear, aspect ratio kept) and takes the 224x224 centre crop
    (``ImagePreprocess(resize=256, center_crop=224)``). All images of one
    request share one size. ``antialias=True`` (this mode only) resizes with
    the antialiased filter that PIL / torchvision ``Resize`` apply when they
    shrink a photo, so large inputs match what ImageNet models were trained
    on.
    ``input_format="uint8_ragged"``: one request carries N photos of N
    different sizes. "images" is DT_UINT8 [total_bytes], the HWC pixels of
    the images back to back with no padding, and "image_shapes" is DT_INT32
    (N,2), row i being (H_i, W_i) (``preprocess.pack_ragged_images`` builds
    both). One kernel launch resizes each image's shorter side to 256, takes
    its 224x224 centre crop and normalizes
    (``RaggedImagePreprocess(resize=256, center_crop=224)``); every image
    gets exactly what the ``uint8_nhwc_resize`` mode gives it alone. The
    filter is bilinear; ``antialias=True`` is rejected in this mode, whose
    antialiased counterpart has a name of its own:
    ``input_format="uint8_ragged_antialias"``: the same two inputs, resized
    with the antialiased filter in two kernel launches
    (``AntialiasedRaggedImagePreprocess(resize=256, center_crop=224)``);
    every image gets exactly what ``uint8_nhwc_resize`` with
    ``antialias=True`` gives it alone. The mode name carries the filter, so
    ``antialias=True`` on top of it is rejected like in every mode but
    ``uint8_nhwc_resize``.
    ``input_format="nv12_resize"`` / ``"i420_resize"``: "images" is DT_UINT8
    (N,H*3/2,W), YUV 4:2:0 frames of any even size as a video or JPEG decoder
    emits them (NV12: interleaved chroma, I420: planar), 1.5 bytes per pixel,
    half the request bytes of ``uint8_nhwc_resize``. One kernel launch
    converts to RGB with the integer matrix ``yuv_matrix`` ("bt601", the
    default, "bt709" or "bt601_full"), resizes the shorter side to 256, takes
    the 224x224 centre crop and normalizes
    (``Yuv420ImagePreprocess(resize=256, center_crop=224)``): exactly what
    ``uint8_nhwc_resize`` gives for the converted RGB frames
    (``ops.yuv420_to_rgb_u8``). The filter is bilinear; ``antialias=True`` is
    rejected, because the antialiased counterparts have names of their own:
    ``input_format="nv12_resize_antialias"`` / ``"i420_resize_antialias"``:
    the same input, resized with the antialiased filter in two kernel
    launches, the first of which converts
    (``Yuv420ImagePreprocess(resize=256, center_crop=224, antialias=True)``):
    exactly what ``uint8_nhwc_resize`` with ``antialias=True`` gives for the
    converted RGB frames. ``yuv_matrix`` is accepted; the mode name carries
    the filter, so ``antialias=True`` on top of it is rejected. A non-default
    ``yuv_matrix`` is rejected in every mode but these four.

    ``output_format="logits"`` (default): the only output is "logits",
    DT_FLOAT (N,1000).
    ``output_format="topk"``: the outputs are "scores", DT_FLOAT (N,top_k),
    and "classes", DT_INT32 (N,top_k) — the ``top_k`` (1..64, default 5) most
    probable classes of each image in rank order with their softmax
    probabilities, 40 bytes per image at 5 instead of 4000. The head runs on the
    server in one fused kernel (``postprocess.TopKClassification``,
    ``ops.softmax_topk``) straight from the model's own dtype; the full
    logits never leave the device."""
    from ..postprocess import TopKClassification
    from ..server import Servable

    if input_format not in ("float_nchw", "uint8_nhwc", "uint8_nhwc_resize",
                            "uint8_ragged", "uint8_ragged_antialias",
                            *_YUV_MODES):
        raise ValueError(
            f"input_format must be 'float_nchw', 'uint8_nhwc', "
            f"'uint8_nhwc_resize', 'uint8_ragged', "
            f"'uint8_ragged_antialias', 'nv12_resize', 'i420_resize', "
            f"'nv12_resize_antialias' or 'i420_resize_antialias', got "
            f"{input_format!r}")
    if yuv_matrix != "bt601" and input_format not in _YUV_MODES:
        raise ValueError(
            "yuv_matrix needs a YUV input_format ('nv12_resize', "
            "'i420_resize' or their '_antialias' counterparts), got "
            f"{input_format!r}")
    if antialias and input_format == "uint8_ragged":
        raise ValueError(
            "antialias=True is not supported with input_format="
            "'uint8_ragged': antialiased ragged batches are "
            "input_format='uint8_ragged_antialias'")
    if antialias and input_format in _YUV_MODES:
        raise ValueError(
            "antialias=True is not supported with input_format="
            f"{input_format!r}: antialiased YUV frames are input_format="
            f"'{_YUV_MODES[input_format][0]}_resize_antialias'")
    if antialias and input_format != "uint8_nhwc_resize":
        raise ValueError(
            "antialias=True needs input_format='uint8_nhwc_resize', got "
            f"{input_format!r}")
    if output_format not in ("logits", "topk"):
        raise ValueError(
            f"output_format must be 'logits' or 'topk', got "
            f"{output_format!r}")
    topk = output_format == "topk"
    # top_k is validated in every mode: a typo must not wait for "topk"
    postprocess = TopKClassification(top_k)

    torch.manual_seed(seed)
    model = resnet50().to(device=device, dtype=dtype).eval()

    @torch.no_grad()
    def fn(inputs):
        x = inputs["images"]
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(x)
        # a no-op (same tensor) when preprocessing already produced
        # device/dtype
        x = x.to(device=device, dtype=dtype)
        logits = s.module(x)
        # the top-k head reads the model's own dtype
        return {"logits": logits if topk else logits.float()}

    if input_format == "uint8_nhwc":
        images_sig = (4, [-1, 224, 224, 3])                 # DT_UINT8
        preprocess = {"images": ImagePreprocess(
            IMAGENET_MEAN, IMAGENET_STD, out_dtype=dtype, layout="nchw",
            device=device)}
    elif input_format == "uint8_nhwc_resize":
        images_sig = (4, [-1, -1, -1, 3])                   # DT_UINT8
        preprocess = {"images": ImagePreprocess(
            IMAGENET_MEAN, IMAGENET_STD, out_dtype=dtype, layout="nchw",
            device=device, resize=256, center_crop=224,
            antialias=bool(antialias))}
    elif input_format in _YUV_MODES:
        images_sig = (4, [-1, -1, -1])                      # DT_UINT8
        preprocess = {"images": Yuv420ImagePreprocess(
            IMAGENET_MEAN, IMAGENET_STD, out_dtype=dtype, layout="nchw",
            device=device, resize=256, center_crop=224,
            chroma=_YUV_MODES[input_format][0], matrix=yuv_matrix,
            antialias=_YUV_MODES[input_format][1])}
    elif input_format in _RAGGED_MODES:
        images_sig = (4, [-1])                              # DT_UINT8
        preprocess = {("images", "image_shapes"): _RAGGED_MODES[input_format](
            IMAGENET_MEAN, IMAGENET_STD, out_dtype=dtype, layout="nchw",
            device=device, resize=256, center_crop=224)}
    else:
        images_sig = (1, [-1, 3, 224, 224])                 # DT_FLOAT
        preprocess = None
    sig_inputs = {"images": images_sig}
    if input_format in _RAGGED_MODES:
        sig_inputs["image_shapes"] = (3, [-1, 2])           # DT_INT32
    if topk:
        outputs = {"scores": (1, [-1, postprocess.k]),      # DT_FLOAT
                   "classes": (3, [-1, postprocess.k])}     # DT_INT32
    else:
        outputs = {"logits": (1, [-1, 1000])}
    s = Servable(
        fn,
        signature={
            "method_name": "tensorflow/serving/predict",
            "inputs": sig_inputs,
            "outputs": outputs,
        },
        preprocess=preprocess,
        postprocess=postprocess if topk else None)
    s.module = model
    return s
