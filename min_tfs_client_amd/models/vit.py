"""Vision Transformer (ViT-B/16 by default) in plain PyTorch.

Self-contained implementation (no checkpoint download; random init):
pre-LayerNorm encoder blocks, a class token, learned position embeddings and
a linear head on the class token. The embedding (``embed``) and the encoder
(``forward_tokens``) are separate methods, so a server can replace the
embedding by the fused uint8 patch-embedding kernel
(``preprocess.PatchEmbedPreprocess``).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..preprocess import (IMAGENET_MEAN, IMAGENET_STD, PatchEmbedPreprocess,
                          RaggedResizePatchEmbedPreprocess,
                          ResizePatchEmbedPreprocess,
                          Yuv420PatchEmbedPreprocess)


class VitConfig:
    image_size = 224
    patch = 16
    hidden = 768
    layers = 12
    heads = 12
    mlp = 3072
    num_classes = 1000
    eps = 1e-6

    def __init__(self, **overrides):
        for key, value in overrides.items():
            if not hasattr(type(self), key):
                raise ValueError(f"unknown VitConfig field {key!r}")
            setattr(self, key, value)


class VitBlock(nn.Module):
    def __init__(self, cfg: VitConfig):
        super().__init__()
        h = cfg.hidden
        self.ln1 = nn.LayerNorm(h, eps=cfg.eps)
        self.qkv = nn.Linear(h, 3 * h)
        self.attn_out = nn.Linear(h, h)
        self.ln2 = nn.LayerNorm(h, eps=cfg.eps)
        self.ff1 = nn.Linear(h, cfg.mlp)
        self.ff2 = nn.Linear(cfg.mlp, h)
        self.heads = cfg.heads
        self.head_dim = h // cfg.heads

    def forward(self, x):
        B, T, H = x.shape
        qkv = self.qkv(self.ln1(x)).view(B, T, 3, self.heads, self.head_dim)
        q, k, v = (t.transpose(1, 2) for t in qkv.unbind(2))
        attn = F.scaled_dot_product_attention(q, k, v)
        x = x + self.attn_out(attn.transpose(1, 2).reshape(B, T, H))
        return x + self.ff2(F.gelu(self.ff1(self.ln2(x))))


class VisionTransformer(nn.Module):
    def __init__(self, cfg: VitConfig = None):
        super().__init__()
        cfg = VitConfig() if cfg is None else cfg
        if cfg.image_size % cfg.patch or cfg.hidden % cfg.heads:
            raise ValueError(
                "image_size must be a multiple of patch and hidden of heads")
        self.cfg = cfg
        tokens = (cfg.image_size // cfg.patch) ** 2 + 1
        self.patch_embed = nn.Conv2d(3, cfg.hidden, cfg.patch,
                                     stride=cfg.patch)
        self.cls_token = nn.Parameter(torch.randn(1, 1, cfg.hidden) * 0.02)
        self.pos_embed = nn.Parameter(
            torch.randn(1, tokens, cfg.hidden) * 0.02)
        self.blocks = nn.ModuleList(
            [VitBlock(cfg) for _ in range(cfg.layers)])
        self.ln = nn.LayerNorm(cfg.hidden, eps=cfg.eps)
        self.head = nn.Linear(cfg.hidden, cfg.num_classes)

    def embed(self, x):
        """Normalized ``[N,3,H,W]`` -> tokens ``[N,T,D]``."""
        x = self.patch_embed(x).flatten(2).transpose(1, 2)
        x = torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1)
        return x + self.pos_embed

    def forward_tokens(self, tokens):
        """Tokens ``[N,T,D]`` -> logits ``[N,num_classes]``."""
        x = tokens
        for blk in self.blocks:
            x = blk(x)
        return self.head(self.ln(x)[:, 0])

    def forward(self, x):
        return self.forward_tokens(self.embed(x))


def vit_b16(config: VitConfig = None) -> VisionTransformer:
    return VisionTransformer(config)


def vit_b16_servable(device: str = "cpu", dtype=torch.float32, seed: int = 0,
                     input_format: str = "float_nchw",
                     output_format: str = "logits", top_k: int = 5,
                     config: VitConfig = None, yuv_matrix: str = "bt601"):
    """ViT-B/16 Servable: input alias "images", output "logits"
    (N,num_classes).

    ``input_format="float_nchw"`` (default): "images" is DT_FLOAT
    (N,3,224,224), already normalized by the client; the model embeds it
    itself (``VisionTransformer.forward``).
    ``input_format="uint8_nhwc"``: "images" is DT_UINT8 (N,224,224,3) raw
    pixels. The server turns them into the encoder's input tokens in one
    fused kernel (``preprocess.PatchEmbedPreprocess``,
    ``ops.image_u8_patch_embed``): ImageNet normalization, the 16x16 patch
    projection, the class token and the position embeddings, built from the
    module's own parameters and refolded whenever they change
    (``load_state_dict`` after construction included); the model runs
    ``forward_tokens``. In this mode the patch projection uses bf16 weights
    with fp32 accumulation whatever ``dtype`` is; the pixel operand is exact.
    ``input_format="nv12"`` / ``"i420"``: "images" is DT_UINT8
    (N,224*3/2,224), YUV 4:2:0 frames as a video or JPEG decoder emits them
    (layout: ``ops.yuv420_to_rgb_u8``), half the request bytes of
    ``uint8_nhwc``. The same kernel converts them to RGB with the integer
    matrix ``yuv_matrix`` ("bt601", the default, "bt709" or "bt601_full")
    while it fills its tile (``preprocess.Yuv420PatchEmbedPreprocess``,
    ``ops.image_yuv420_patch_embed``): the logits are exactly those of
    ``uint8_nhwc`` on the converted frames. The patch must be 16 or 32. A
    non-default ``yuv_matrix`` is rejected in every other mode.
    ``input_format="uint8_nhwc_resize"``: "images" is DT_UINT8 (N,H,W,3) raw
    pixels of any size (every image of one request has the same size;
    requests may differ), as ``resnet50_servable`` takes them: the shorter
    side is resized to ``image_size * 8 // 7`` (256 for 224, bilinear, no
    antialiasing), then a centre crop of ``image_size``, both inside the same
    kernel while it fills its tile (``preprocess.ResizePatchEmbedPreprocess``,
    ``ops.image_u8_resize_patch_embed``); the model runs ``forward_tokens``.
    The resized pixel is an fp32 blend and reaches the matrix cores as two
    bf16 pieces, within 2^-16 of its value. The patch must be 16 or 32.
    On an MI355X the one launch measured faster than resize-then-embed at
    every batch and source size tried (profiles/README.md); images that
    already are ``image_size`` square are served faster by ``uint8_nhwc``
    (the resampling loader costs 1.6-2.0x there).
    ``input_format="uint8_ragged"``: one request carries N photos of N
    different sizes, as ``resnet50_servable`` takes them in the mode of the
    same name. "images" is DT_UINT8 [total_bytes], the HWC pixels of the
    images back to back with no padding, and "image_shapes" is DT_INT32
    (N,2), row i being (H_i, W_i) (``preprocess.pack_ragged_images`` builds
    both). Per image the shorter side is resized to ``image_size * 8 // 7``,
    then a centre crop of ``image_size``, bilinear, in ONE launch of the same
    kernel, whose resampling loader reads the source geometry per tile row
    (``preprocess.RaggedResizePatchEmbedPreprocess``,
    ``ops.image_u8_ragged_resize_patch_embed``); every image gets exactly the
    tokens ``uint8_nhwc_resize`` gives it alone. The patch must be 16 or 32.
    Measured on an MI355X (ViT-B/16, bf16, photos of 256..512 x 341..683):
    the op took 47 us for 8 photos and 105 us for 32, against 142 and 561 us
    for one dense launch per photo plus ``torch.cat`` and 110-120 and 147 us
    for ``ops.image_u8_ragged_resize_to_float`` plus ``embed``. For a single
    photo it is slower than the dense mode (34 against 18 us: the per-image
    table is built on the host). On batches of one size the launch costs
    0.99-1.03 of the dense one, inside the spread of the measurement, but the
    table still costs 6-18 us per call: keep ``uint8_nhwc_resize`` for
    same-size requests (profiles/README.md; Predict latency not measured).

    ``output_format="logits"`` / ``"topk"`` and ``top_k``: as for
    ``resnet50_servable`` (``postprocess.TopKClassification``).
    ``config`` replaces the ViT-B/16 ``VitConfig`` (image size, patch, width,
    depth), e.g. a one-layer model in tests."""
    from ..postprocess import TopKClassification
    from ..server import Servable

    if input_format not in ("float_nchw", "uint8_nhwc", "uint8_nhwc_resize",
                            "uint8_ragged", "nv12", "i420"):
        raise ValueError(
            f"input_format must be 'float_nchw', 'uint8_nhwc', "
            f"'uint8_nhwc_resize', 'uint8_ragged', 'nv12' or 'i420', got "
            f"{input_format!r}")
    yuv = input_format in ("nv12", "i420")
    if yuv_matrix != "bt601" and not yuv:
        raise ValueError(
            "yuv_matrix needs a YUV input_format ('nv12' or 'i420'), got "
            f"{input_format!r}")
    if output_format not in ("logits", "topk"):
        raise ValueError(
            f"output_format must be 'logits' or 'topk', got "
            f"{output_format!r}")
    topk = output_format == "topk"
    # top_k is validated in every mode: a typo must not wait for "topk"
    postprocess = TopKClassification(top_k)
    cfg = VitConfig() if config is None else config
    resize = input_format == "uint8_nhwc_resize"
    ragged = input_format == "uint8_ragged"
    # tokens from the kernel
    u8 = input_format == "uint8_nhwc" or resize or ragged or yuv

    torch.manual_seed(seed)
    model = vit_b16(cfg).to(device=device, dtype=dtype).eval()

    @torch.no_grad()
    def fn(inputs):
        x = inputs["images"]
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(x)
        # a no-op (same tensor) when preprocessing already produced
        # device/dtype
        x = x.to(device=device, dtype=dtype)
        logits = s.module.forward_tokens(x) if u8 else s.module(x)
        # the top-k head reads the model's own dtype
        return {"logits": logits if topk else logits.float()}

    size = cfg.image_size
    if yuv:
        images_sig = (4, [-1, size * 3 // 2, size])         # DT_UINT8
        preprocess = {"images": Yuv420PatchEmbedPreprocess(
            model.patch_embed.weight, model.patch_embed.bias, IMAGENET_MEAN,
            IMAGENET_STD, pos_embed=model.pos_embed,
            cls_token=model.cls_token, out_dtype=dtype, device=device,
            chroma=input_format, matrix=yuv_matrix)}
    elif resize:
        images_sig = (4, [-1, -1, -1, 3])                   # DT_UINT8
        preprocess = {"images": ResizePatchEmbedPreprocess(
            model.patch_embed.weight, model.patch_embed.bias, IMAGENET_MEAN,
            IMAGENET_STD, pos_embed=model.pos_embed,
            cls_token=model.cls_token, out_dtype=dtype, device=device,
            resize=size * 8 // 7, center_crop=size)}
    elif ragged:
        images_sig = (4, [-1])                              # DT_UINT8
        preprocess = {("images", "image_shapes"):
                      RaggedResizePatchEmbedPreprocess(
            model.patch_embed.weight, model.patch_embed.bias, IMAGENET_MEAN,
            IMAGENET_STD, pos_embed=model.pos_embed,
            cls_token=model.cls_token, out_dtype=dtype, device=device,
            resize=size * 8 // 7, center_crop=size)}
    elif u8:
        images_sig = (4, [-1, size, size, 3])               # DT_UINT8
        preprocess = {"images": PatchEmbedPreprocess(
            model.patch_embed.weight, model.patch_embed.bias, IMAGENET_MEAN,
            IMAGENET_STD, pos_embed=model.pos_embed,
            cls_token=model.cls_token, out_dtype=dtype, device=device)}
    else:
        images_sig = (1, [-1, 3, size, size])               # DT_FLOAT
        preprocess = None
    sig_inputs = {"images": images_sig}
    if ragged:
        sig_inputs["image_shapes"] = (3, [-1, 2])           # DT_INT32
    if topk:
        outputs = {"scores": (1, [-1, postprocess.k]),      # DT_FLOAT
                   "classes": (3, [-1, postprocess.k])}     # DT_INT32
    else:
        outputs = {"logits": (1, [-1, cfg.num_classes])}
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
