"""Declarative server-side output postprocessing for ``Servable``.

A ``Servable`` takes ``postprocess=callable``: the callable gets the whole
``{alias: tensor}`` result of the model function and returns the dict that
becomes the response. It is the output-side counterpart of
``preprocess.py``: the reduction a client would do on the full result runs
next to the model, and only the reduced tensors cross D2H and the wire.
``TopKClassification`` is the classifier case: ``[B,C]`` logits become the
``k`` most probable classes and their softmax scores in one fused kernel
(``ops.softmax_topk``).
"""
from __future__ import annotations

import warnings

import numpy as np

try:
    import torch
except ImportError:  # pragma: no cover
    torch = None

from . import ops


class TopKClassification:
    """Replaces the ``logits`` output (``[B,C]``, f32 / bf16 / f16) by
    ``scores`` (fp32 ``[B,k]``) and ``classes`` (int32 ``[B,k]``), the ``k``
    most probable classes in rank order; every other output passes through
    and the model function's dict is not mutated.

    Accepts a torch tensor on any device (the kernel runs where the logits
    live, in the model's own dtype) or a numpy array. A result without the
    ``logits`` alias, logits of the wrong rank or dtype, or fewer than ``k``
    classes raise ``ValueError`` (servers answer INVALID_ARGUMENT).
    Semantics: see ``ops.softmax_topk``."""

    def __init__(self, k: int, logits: str = "logits",
                 scores: str = "scores", classes: str = "classes"):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) \
                or not 1 <= k <= ops.SOFTMAX_TOPK_MAX_K:
            raise ValueError(
                f"k must be an int in 1..{ops.SOFTMAX_TOPK_MAX_K}, got {k!r}")
        if scores == classes:
            raise ValueError(
                f"scores and classes need two aliases, got {scores!r} twice")
        self.k = int(k)
        self.logits = logits
        self.scores = scores
        self.classes = classes

    def __call__(self, outputs):
        if self.logits not in outputs:
            raise ValueError(
                f"expected a {self.logits!r} output to take the top "
                f"{self.k} of; the model returned {sorted(outputs)}")
        x = outputs[self.logits]
        if not isinstance(x, torch.Tensor):
            with warnings.catch_warnings():
                # a read-only array is only read here
                warnings.simplefilter("ignore", UserWarning)
                x = torch.as_tensor(np.asarray(x))
        out = {a: v for a, v in outputs.items() if a != self.logits}
        out[self.scores], out[self.classes] = ops.softmax_topk(
            x.contiguous(), self.k)
        return out
