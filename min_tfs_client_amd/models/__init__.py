"""Model families servable by the loopback PredictionService.

The reference serves TF SavedModels out of process; this framework serves
PyTorch-ROCm modules in process (random-init synthetic weights — no network
for checkpoints). Families match the BASELINE configs: ResNet-50 (config 2)
and BERT-base (config 3), plus the identity fixture model, and ViT-B/16,
whose uint8 mode starts at the fused patch-embedding kernel.
"""
from .resnet import resnet50, resnet50_servable  # noqa: F401
from .bert import bert_base, bert_servable  # noqa: F401
from .vit import (VisionTransformer, VitConfig, vit_b16,  # noqa: F401
                  vit_b16_servable)
