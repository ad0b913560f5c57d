"""BERT-base encoder in plain PyTorch — the BASELINE config-3 model family
(multi-input: input_ids + attention_mask int32, batch 128 x seq 512).

Self-contained implementation (no checkpoint download; random init).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn


class BertConfig:
    vocab_size = 30522
    hidden = 768
    layers = 12
    heads = 12
    intermediate = 3072
    max_pos = 512
    type_vocab = 2
    eps = 1e-12


class BertLayer(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        h = cfg.hidden
        self.qkv = nn.Linear(h, 3 * h)
        self.attn_out = nn.Linear(h, h)
        self.ln1 = nn.LayerNorm(h, eps=cfg.eps)
        self.ff1 = nn.Linear(h, cfg.intermediate)
        self.ff2 = nn.Linear(cfg.intermediate, h)
        self.ln2 = nn.LayerNorm(h, eps=cfg.eps)
        self.heads = cfg.heads
        self.head_dim = h // cfg.heads

    def forward(self, x, attn_mask, lengths=None, tiles=None, keys=None):
        """``lengths`` (int32 (B) on x's device): every mask is the prefix
        given by its length, and attention runs in the fused length-masked
        kernel on the projection as stored, with no transposed views, no
        mask and no copy of the result (``attn_mask`` is not read). Query
        rows at and past a length are zeros there.

        ``tiles`` (``ops.attention_tiles`` on x's device): ``x`` is packed,
        (T,H) with the sequences back to back, and the projection goes to
        the packed form of the same kernel; every other layer of the block
        is row-wise and runs on the T rows as it is.

        ``keys`` (``ops.attention_keys`` of the request's (B,S) mask, on x's
        device): an arbitrary key mask in the keys form of the same kernel.
        Every query row is computed, as the additive mask would have it."""
        if lengths is not None or tiles is not None or keys is not None:
            from .. import ops
            attn = ops.masked_self_attention(self.qkv(x), lengths, self.heads,
                                             tiles=tiles, keys=keys)
            x = self.ln1(x + self.attn_out(attn))
            return self.ln2(
                x + self.ff2(torch.nn.functional.gelu(self.ff1(x))))
        B, S, H = x.shape
        qkv = self.qkv(x).view(B, S, 3, self.heads, self.head_dim)
        q, k, v = qkv.unbind(2)  # each B,S,heads,hd
        q = q.transpose(1, 2)
        k = k.transpose(1, 2)
        v = v.transpose(1, 2)
        # scaled_dot_product_attention uses the fused path on ROCm
        attn = torch.nn.functional.scaled_dot_product_attention(
            q, k, v, attn_mask=attn_mask)
        attn = attn.transpose(1, 2).reshape(B, S, H)
        x = self.ln1(x + self.attn_out(attn))
        x = self.ln2(x + self.ff2(torch.nn.functional.gelu(self.ff1(x))))
        return x


class BertEncoder(nn.Module):
    def __init__(self, cfg: BertConfig = BertConfig()):
        super().__init__()
        self.cfg = cfg
        self.tok = nn.Embedding(cfg.vocab_size, cfg.hidden)
        self.pos = nn.Embedding(cfg.max_pos, cfg.hidden)
        self.typ = nn.Embedding(cfg.type_vocab, cfg.hidden)
        self.ln = nn.LayerNorm(cfg.hidden, eps=cfg.eps)
        self.blocks = nn.ModuleList(
            [BertLayer(cfg) for _ in range(cfg.layers)])
        self.pooler = nn.Linear(cfg.hidden, cfg.hidden)

    def embed(self, input_ids, token_type_ids=None):
        """ids (B,S) -> the encoder's input (B,S,H): token + position + type
        embeddings, LayerNorm. ``token_type_ids`` None: all zero."""
        B, S = input_ids.shape
        if S > self.cfg.max_pos:
            raise ValueError(
                f"sequence length {S} exceeds max_position_embeddings "
                f"{self.cfg.max_pos}")
        pos_ids = torch.arange(S, device=input_ids.device)
        x = self.tok(input_ids.long()) + self.pos(pos_ids)
        # the types are built after the two gathers, as forward always did
        x = x + self.typ(torch.zeros_like(input_ids.long())
                         if token_type_ids is None else token_type_ids.long())
        return self.ln(x)

    @staticmethod
    def additive_mask(attention_mask, dtype):
        """(B,S) keep mask -> additive (B,1,1,S): 0 where attend, finfo.min
        where padded; None stays None."""
        if attention_mask is None:
            return None
        m = attention_mask[:, None, None, :].to(dtype)
        return (1.0 - m) * torch.finfo(dtype).min

    def forward_embedded(self, x, mask, lengths=None, tiles=None,
                         first_rows=None, keys=None):
        """The encoder blocks and the pooler on an embedded input. With
        ``lengths`` every block runs the fused length-masked attention (see
        ``BertLayer.forward``); all blocks share the one tensor. With
        ``tiles`` the input is packed (T,H) and stays packed through every
        block; ``first_rows`` (int64 (B)) is the first row of each sequence,
        which the pooler reads. With ``keys`` every block runs the keys
        form on the one (index, count) pair."""
        for blk in self.blocks:
            x = blk(x, mask, lengths, tiles, keys)
        first = x[:, 0] if tiles is None else x.index_select(0, first_rows)
        pooled = torch.tanh(self.pooler(first))
        return x, pooled

    def forward(self, input_ids, attention_mask=None):
        x = self.embed(input_ids)
        return self.forward_embedded(
            x, self.additive_mask(attention_mask, x.dtype))


def bert_base() -> BertEncoder:
    return BertEncoder()


def bert_servable(device: str = "cpu", dtype=torch.float32, seed: int = 0,
                  output_format: str = "hidden",
                  normalize_embedding: bool = True,
                  input_format: str = "ids", config: BertConfig = None,
                  attention: str = "sdpa"):
    """BERT-base Servable: inputs "input_ids"/"attention_mask" int32.

    ``input_format="ids"`` (default): the encoder input is built by the
    module's eager ``embed`` and ``additive_mask`` (about a dozen launches).
    ``input_format="ids_fused"``: the same two inputs plus an optional
    "token_type_ids" (DT_INT32 (B,S), for sentence pairs; absent: all zero).
    Ids, types and mask go through ONE launch of the fused embedding kernel
    (``ops.bert_embed``) on the module's own parameters, read at call time
    (``load_state_dict`` needs no refold), then ``forward_embedded``.
    ``input_format="ids_ragged"``: "input_ids" is DT_INT32 (total), the ids
    of B sequences back to back with no padding, and "sequence_lengths" is
    DT_INT32 (B) (``preprocess.pack_ragged_tokens`` builds both); an optional
    flat "token_type_ids" as well. There is no "attention_mask": the same
    launch (``ops.bert_embed_ragged``) pads to S = the longest sequence with
    id 0 and derives the mask from the lengths, and the outputs have that S.
    It equals ``"ids_fused"`` on the padded request bit for bit.

    Numeric contract of the two fused modes: the three embedding rows are
    summed in fp32 from the values as stored, LayerNorm is two-pass fp32
    (biased variance, IEEE ``1/sqrt(var + eps)``) and the result is rounded
    once, to the model's dtype; the additive mask is +0.0 where a position is
    kept and ``finfo(dtype).min`` where it is not. In fp32 that differs from
    ``"ids"`` by a few units in the last place, in bf16/f16 ``"ids"`` rounds
    after every eager step and the fused modes are the closer to exact. They
    are deterministic. An id outside the vocabulary, a type outside the type
    vocabulary, a sequence longer than ``max_pos`` or lengths that do not sum
    to the ids are INVALID_ARGUMENT naming the row; on the device a bad id
    never indexes a table. That check costs one 4-byte synchronizing D2H
    read per request (profiles/README.md has the measured cost).

    ``config``: a ``BertConfig`` to build instead of BERT-base (tests serve a
    one-layer model).

    ``attention="sdpa"`` (default): every block runs
    ``scaled_dot_product_attention`` over the full S x S square with the
    additive mask. ``attention="fused"``: every block runs
    ``ops.masked_self_attention``, the length-masked MFMA kernel, on the qkv
    projection as stored; key and query tiles that are wholly padding are
    never touched. It needs ``input_format="ids_ragged"`` (the only mode with
    lengths: a general mask is not a prefix) and a bfloat16 or float16
    ``dtype`` with 64-wide heads; anything else is a ``ValueError`` here. The
    request's "sequence_lengths", already validated on the host by the
    embedding, goes to the device once per request (pinned int32,
    non-blocking copy) and all blocks share it. Kept positions and
    "pooled_output" follow the default mode within bf16 / f16 noise;
    "last_hidden_state" at PADDED positions is finite and deterministic but
    differs from the default mode, because attention rows there are zeros
    instead of an average over the kept keys. "sentence_embedding" pools
    kept positions only and follows the default mode.

    ``attention="packed"``: the same constraints as ``"fused"``, and the
    batch stays packed from the ids to the last block: the embedding kernel
    writes (total,H) (``ops.bert_embed_ragged(packed=True)``), every block
    runs its GEMMs, LayerNorms and GELU on those ``total`` rows instead of
    ``B * S`` and its attention in the packed form of the kernel. Per
    request the lengths are read once on the host, which builds the
    embedding's table, the tile table (``ops.attention_tiles``) and two
    index vectors (the first row of each sequence, and ``b * S + s`` of each
    packed row), all shipped from pinned memory without a synchronization.
    After the last block the rows are scattered into zeros once
    (``index_copy_``): "last_hidden_state" has S = the longest length and
    is exactly +0.0 at padded positions; kept positions, "pooled_output"
    and "sentence_embedding" follow the default mode as ``"fused"`` does.

    ``attention="masked"``: the same kernel for the DENSE request, "ids" or
    "ids_fused" with any "attention_mask": prefixes, left padding, holes.
    One launch per request (``ops.attention_keys``) turns the mask into the
    ascending list of kept key positions of every sequence, and every block
    runs the keys form of ``ops.masked_self_attention`` on that one pair: it
    loads K and V rows through the list, so key tiles cost what the kept keys
    cost and masked K and V rows are never read. Every query row is
    computed, so "last_hidden_state" follows the default mode within
    bf16 / f16 noise at ALL positions, padded ones included, and so do
    "pooled_output" and "sentence_embedding"; a sequence with nothing kept
    gets the default mode's uniform average. It needs a bfloat16 or float16
    ``dtype`` with 64-wide heads; ``input_format="ids_ragged"`` has no mask
    and is a ``ValueError`` naming ``"fused"`` / ``"packed"``. A request
    without "attention_mask" runs the length form with full lengths. The
    additive mask is not built on this path.

    ``output_format="hidden"`` (default): outputs "last_hidden_state"
    (B,S,768) + "pooled_output" (B,768), both DT_FLOAT.
    ``output_format="sentence_embedding"``: the only output is
    "sentence_embedding", DT_FLOAT (B,768) — the mean of the hidden state
    over the positions ``attention_mask`` keeps (all positions when the mask
    is absent), L2-normalized when ``normalize_embedding``. It is S x fewer
    response bytes, pooled on the server by one fused kernel
    (``ops.masked_mean_pool``) straight from the model's own dtype; a pooled
    row is deterministic and ignores masked positions."""
    from .. import ops
    from ..server import Servable

    if output_format not in ("hidden", "sentence_embedding"):
        raise ValueError(
            f"output_format must be 'hidden' or 'sentence_embedding', got "
            f"{output_format!r}")
    if input_format not in ("ids", "ids_fused", "ids_ragged"):
        raise ValueError(
            f"input_format must be 'ids', 'ids_fused' or 'ids_ragged', got "
            f"{input_format!r}")
    if attention not in ("sdpa", "fused", "packed", "masked"):
        raise ValueError(
            f"attention must be 'sdpa' or 'fused' or 'packed' or 'masked', "
            f"got {attention!r}")
    cfg = BertConfig() if config is None else config
    fused_attention = attention == "fused"
    packed_attention = attention == "packed"
    masked_attention = attention == "masked"
    if masked_attention and input_format == "ids_ragged":
        raise ValueError(
            "attention='masked' needs input_format='ids' or 'ids_fused' (a "
            "request with an attention_mask); 'ids_ragged' has lengths: use "
            "attention='fused' or 'packed'")
    if attention != "sdpa":
        if not masked_attention and input_format != "ids_ragged":
            raise ValueError(
                f"attention={attention!r} needs input_format='ids_ragged' "
                "(the only mode whose masks are prefixes given by lengths), "
                f"got {input_format!r}")
        if dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(
                f"attention={attention!r} needs dtype bfloat16 or float16, "
                f"got {dtype}")
        if cfg.hidden != cfg.heads * ops.ATTENTION_HEAD_DIM:
            raise ValueError(
                f"attention={attention!r} needs {ops.ATTENTION_HEAD_DIM}-wide "
                f"heads, got hidden {cfg.hidden} over {cfg.heads} heads")
    embed = output_format == "sentence_embedding"
    normalize_embedding = bool(normalize_embedding)
    fused = input_format == "ids_fused"
    ragged = input_format == "ids_ragged"

    torch.manual_seed(seed)
    model = BertEncoder(cfg).to(device=device, dtype=dtype).eval()

    def on_device(value):
        if value is None:
            return None
        if not isinstance(value, torch.Tensor):
            value = torch.as_tensor(value)
        return value.to(device=device)

    def device_lengths(lengths):
        """The request's lengths as int32 on the model's device: from a
        pinned buffer on the current stream, no synchronization."""
        if not isinstance(lengths, torch.Tensor):
            lengths = torch.as_tensor(np.asarray(lengths))
        if lengths.is_cuda or torch.device(device).type != "cuda":
            return lengths.to(device=device, dtype=torch.int32)
        host = torch.empty(lengths.shape, dtype=torch.int32, pin_memory=True)
        host.copy_(lengths)
        # the caching host allocator keeps the buffer until the copy is done
        return host.to(device, non_blocking=True)

    def fused_embed(inputs):
        """(encoder input, additive mask, pooling mask) from the fused
        kernel, on the module's parameters as they are at call time."""
        m = s.module
        ids = on_device(inputs["input_ids"])
        types = on_device(inputs.get("token_type_ids"))
        tables = (m.tok.weight, m.pos.weight, m.typ.weight, m.ln.weight,
                  m.ln.bias, m.ln.eps)
        out_dtype = m.tok.weight.dtype
        if ragged:
            # read on the host: keep a host tensor on the host
            x, add_mask = ops.bert_embed_ragged(
                ids, inputs["sequence_lengths"], *tables,
                token_type_ids=types, out_dtype=out_dtype)
            return x, add_mask, add_mask[:, 0, 0, :] == 0
        mask = on_device(inputs.get("attention_mask"))
        x, add_mask = ops.bert_embed(
            ids, *tables, attention_mask=mask, token_type_ids=types,
            out_dtype=out_dtype)
        return x, add_mask, mask

    def pinned_to_device(host):
        """A host tensor on the model's device: through a pinned buffer on
        the current stream, no synchronization."""
        if torch.device(device).type != "cuda":
            return host
        pinned = torch.empty(host.shape, dtype=host.dtype, pin_memory=True)
        pinned.copy_(host)
        # the caching host allocator keeps the buffer until the copy is done
        return pinned.to(device, non_blocking=True)

    def packed_forward(inputs):
        """(hidden (B,S,H) with +0.0 at padded positions, pooled, pooling
        mask) of a ragged request that stays packed through the encoder."""
        m = s.module
        lengths = inputs["sequence_lengths"]
        # validates the lengths against the ids and max_pos, on the host
        x = ops.bert_embed_ragged(
            on_device(inputs["input_ids"]), lengths, m.tok.weight,
            m.pos.weight, m.typ.weight, m.ln.weight, m.ln.bias, m.ln.eps,
            token_type_ids=on_device(inputs.get("token_type_ids")),
            out_dtype=m.tok.weight.dtype, packed=True)
        if isinstance(lengths, torch.Tensor):
            lengths = lengths.cpu().numpy()
        lens = np.asarray(lengths).astype(np.int64)
        B, S = len(lens), int(lens.max()) if len(lens) else 0
        offsets = np.cumsum(lens) - lens
        seq = np.repeat(np.arange(B), lens)
        # first row of each sequence, then b * S + s of each packed row
        index = pinned_to_device(torch.from_numpy(np.concatenate(
            (offsets, seq * S + (np.arange(len(seq)) - offsets[seq])))))
        tiles = ops.attention_tiles(lens, device)
        x, pooled = m.forward_embedded(x, None, tiles=tiles,
                                       first_rows=index[:B])
        hidden = x.new_zeros((B * S, x.shape[1])).index_copy_(
            0, index[B:], x).view(B, S, x.shape[1])
        mask = None
        if embed:
            mask = torch.arange(S, device=device)[None, :] < \
                pinned_to_device(torch.from_numpy(lens))[:, None]
        return hidden, pooled, mask

    def masked_forward(inputs):
        """(hidden, pooled, pooling mask) of a dense request whose blocks run
        the keys form of the attention kernel: the mask goes to the device
        once, one launch compacts it and all blocks share the pair. The
        additive mask is not built (the fused embedding still returns one,
        which is not passed on)."""
        m = s.module
        if fused:
            x, _, mask = fused_embed(inputs)
        else:
            mask = on_device(inputs.get("attention_mask"))
            x = m.embed(on_device(inputs["input_ids"]))
        if mask is None:
            # no mask: the length form with every sequence S long
            B, S = x.shape[:2]
            lengths = torch.full((B,), S, dtype=torch.int32, device=x.device)
            return m.forward_embedded(x, None, lengths) + (None,)
        keys = ops.attention_keys(mask)
        return m.forward_embedded(x, None, keys=keys) + (mask,)

    @torch.no_grad()
    def fn(inputs):
        if packed_attention:
            hidden, pooled, mask = packed_forward(inputs)
        elif masked_attention:
            hidden, pooled, mask = masked_forward(inputs)
        elif fused or ragged:
            x, add_mask, mask = fused_embed(inputs)
            lengths = device_lengths(inputs["sequence_lengths"]) \
                if fused_attention else None
            hidden, pooled = s.module.forward_embedded(x, add_mask, lengths)
        else:
            ids = on_device(inputs["input_ids"])
            mask = on_device(inputs.get("attention_mask"))
            hidden, pooled = s.module(ids, mask)
        if embed:
            return {"sentence_embedding": ops.masked_mean_pool(
                hidden.contiguous(), mask, normalize_embedding)}
        return {"last_hidden_state": hidden.float(),
                "pooled_output": pooled.float()}

    H = cfg.hidden
    if embed:
        outputs = {"sentence_embedding": (1, [-1, H])}
    else:
        outputs = {"last_hidden_state": (1, [-1, -1, H]),
                   "pooled_output": (1, [-1, H])}
    if ragged:
        sig_inputs = {"input_ids": (3, [-1]),              # DT_INT32
                      "sequence_lengths": (3, [-1]),
                      "token_type_ids": (3, [-1])}
    else:
        sig_inputs = {"input_ids": (3, [-1, -1]),          # DT_INT32
                      "attention_mask": (3, [-1, -1])}
        if fused:
            sig_inputs["token_type_ids"] = (3, [-1, -1])
    signature = {"method_name": "tensorflow/serving/predict",
                 "inputs": sig_inputs, "outputs": outputs}
    if fused or ragged:
        signature["optional_inputs"] = ["token_type_ids"]
    s = Servable(fn, signature=signature)
    s.module = model
    return s
