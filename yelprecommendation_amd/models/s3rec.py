"""S3Rec — drop-in for the scoring surface of reference models/s3rec.py:10-115,184-214.

Same constructor ``S3Rec(cfg, num_items, attributes_count)``, same sub-modules in the same construction order (so a
seeded build draws the reference's RNG stream), same ``_init_weights`` reach — Xavier on the two embeddings, on the
Linears directly inside the ``ffn1s`` / ``ffn2s`` lists and on the four ``*_weight`` Linears; the attention Linears
(one level deeper) and the LayerNorms keep PyTorch's defaults; ``positional_encoding`` is ``torch.rand`` — and the
same parameter names, so ``load_state_dict(torch.load('best_model.pt'), strict=True)`` takes a reference checkpoint.
Build on the CPU under the seed, then move to the GPU (as models/mf.py).

``finetune(X, pos_items, neg_items)`` and ``evaluate(X, pos_item, neg_items)`` return the reference's shapes and run
the fused encoder of csrc/s3rec.hip (one launch from the embedding gather to the last LayerNorm) plus one score
launch.  They are forward-only: in ``eval()`` mode under ``torch.no_grad()``.  Training (the backward pass and
dropout) is not built yet and raises NotImplementedError, as do ``pretrain`` / ``encode`` — the reference's own
``encode`` calls ``_self_attention_block`` without its two mask arguments (models/s3rec.py:117-118), so its
pre-training cannot run as published and there is nothing to be faithful to.

Supported: embed_size 16 / 32 / 64 / 128, max_seq_len 1 .. 64, 1 .. 4 heads, 1 .. 4 blocks; anything else raises
NotImplementedError at construction.
"""
import torch
import torch.nn as nn

from .. import engine
from .base_model import BaseModel


def check_supported(embed_size, max_seq_len, num_heads, num_blocks):
    if embed_size not in engine.SUPPORTED_WIDTHS:
        raise NotImplementedError(f"S3Rec: embed_size {embed_size} (the kernel takes {engine.SUPPORTED_WIDTHS})")
    if not 1 <= max_seq_len <= engine.S3REC_MAX_L:
        raise NotImplementedError(f"S3Rec: max_seq_len {max_seq_len}: 1 to {engine.S3REC_MAX_L} are supported")
    if not 1 <= num_heads <= engine.S3REC_MAX_HEADS:
        raise NotImplementedError(f"S3Rec: num_heads {num_heads}: 1 to {engine.S3REC_MAX_HEADS} are supported")
    if not 1 <= num_blocks <= engine.S3REC_MAX_BLOCKS:
        raise NotImplementedError(f"S3Rec: num_blocks {num_blocks}: 1 to {engine.S3REC_MAX_BLOCKS} are supported")


class MultiHeadAttention(nn.Module):
    """The parameters of reference models/s3rec.py:184-195 (full-width heads, no bias on q / k / v); the arithmetic
    is in the encoder kernel."""

    def __init__(self, embed_size, num_heads):
        super().__init__()
        self.embed_size = embed_size
        self.num_heads = num_heads
        self.q_weights = nn.ModuleList([nn.Linear(embed_size, embed_size, bias=False) for _ in range(num_heads)])
        self.k_weights = nn.ModuleList([nn.Linear(embed_size, embed_size, bias=False) for _ in range(num_heads)])
        self.v_weights = nn.ModuleList([nn.Linear(embed_size, embed_size, bias=False) for _ in range(num_heads)])
        self.output = nn.Linear(num_heads * embed_size, embed_size)


class S3Rec(BaseModel):

    def __init__(self, cfg, num_items, attributes_count):
        super().__init__()
        check_supported(int(cfg.embed_size), int(cfg.max_seq_len), int(cfg.num_heads), int(cfg.num_blocks))
        self.cfg = cfg
        E, nb = cfg.embed_size, cfg.num_blocks
        # reference models/s3rec.py:15-36, in its order (the RNG stream depends on it)
        self.item_embedding = nn.Embedding(num_items + 1, E, dtype=torch.float32)
        self.attribute_embedding = nn.Embedding(attributes_count, E, dtype=torch.float32)
        self.positional_encoding = nn.Parameter(torch.rand(cfg.max_seq_len, E))
        self.multihead_attns = nn.ModuleList([MultiHeadAttention(E, cfg.num_heads) for _ in range(nb)])
        self.layernorm1s = nn.ModuleList([nn.LayerNorm(E) for _ in range(nb)])
        self.ffn1s = nn.ModuleList([nn.Linear(E, E) for _ in range(nb)])
        self.ffn2s = nn.ModuleList([nn.Linear(E, E) for _ in range(nb)])
        self.layernorm2s = nn.ModuleList([nn.LayerNorm(E) for _ in range(nb)])
        self.dropout = nn.Dropout(cfg.dropout_ratio)
        self.aap_weight = nn.Linear(E, E, bias=False)
        self.mip_weight = nn.Linear(E, E, bias=False)
        self.map_weight = nn.Linear(E, E, bias=False)
        self.sp_weight = nn.Linear(E, E, bias=False)
        self._init_weights()
        self.num_items = num_items
        self._packed = None
        self._packed_key = None
        self._err_flag = None

    def _init_weights(self):
        # reference models/s3rec.py:40-51: direct children, and the Linears directly inside a ModuleList
        for child in self.children():
            if isinstance(child, nn.Embedding):
                nn.init.xavier_uniform_(child.weight)
            elif isinstance(child, nn.ModuleList):
                for sub_child in child.children():
                    if isinstance(sub_child, nn.Linear):
                        nn.init.xavier_uniform_(sub_child.weight)
            elif isinstance(child, nn.Linear):
                nn.init.xavier_uniform_(child.weight)

    # -- device buffers ------------------------------------------------------------------------------
    def _block_tensors(self):
        """The encoder's parameters in the order of the packed buffer (include/yelprec_engine.h)."""
        out = []
        for mha, ln1, f1, f2, ln2 in zip(self.multihead_attns, self.layernorm1s, self.ffn1s, self.ffn2s,
                                         self.layernorm2s):
            for heads in (mha.q_weights, mha.k_weights, mha.v_weights):
                out.extend(lin.weight for lin in heads)
            out.extend((mha.output.weight, mha.output.bias, ln1.weight, ln1.bias, f1.weight, f1.bias, f2.weight,
                        f2.bias, ln2.weight, ln2.bias))
        return out

    def _params(self):
        """The packed f32 buffer, built on the device and re-packed when a parameter was written (its ``_version``
        moved) or replaced (``.to()``, ``load_state_dict``)."""
        ts = self._block_tensors()
        key = tuple((t.data_ptr(), t._version) for t in ts)
        if self._packed is None or key != self._packed_key:
            self._packed = torch.cat([t.detach().reshape(-1) for t in ts]).contiguous()
            self._packed_key = key
        return self._packed

    def _flag(self):
        dev = self.item_embedding.weight.device
        if self._err_flag is None or self._err_flag.device != dev:
            self._err_flag = engine.new_error_flag(dev)
        return self._err_flag

    def check_indices(self):
        """Raise IndexError if a batch since the last check held an id outside [0, num_items] (one device sync)."""
        if self._err_flag is not None:
            engine.raise_on_flag(self._err_flag, "S3Rec")

    def _scoring_only(self, what):
        if self.training or torch.is_grad_enabled():
            raise NotImplementedError(
                f"S3Rec.{what}: training is not built yet (no backward pass, no dropout): call it in eval() mode "
                "under torch.no_grad()")

    def _encode(self, X, last_only):
        if X.dim() != 2 or X.shape[1] != self.cfg.max_seq_len:
            raise ValueError(f"S3Rec: X must be [batch, max_seq_len = {self.cfg.max_seq_len}], got {tuple(X.shape)}")
        return engine.s3rec_encode(self.item_embedding.weight.detach(), self.positional_encoding.detach(),
                                   self._params(), X.contiguous(), int(self.cfg.num_heads), int(self.cfg.num_blocks),
                                   last_only=last_only, err_flag=self._flag())

    # -- reference surface -----------------------------------------------------------------------------
    def finetune(self, X, pos_items, neg_items):
        # reference models/s3rec.py:89-100 -> two [batch * max_seq_len] score vectors, padded positions included
        self._scoring_only("finetune")
        h = self._encode(X, last_only=False)
        return engine.s3rec_seq_scores(self.item_embedding.weight.detach(), h, pos_items.contiguous(),
                                       neg_items.contiguous(), err_flag=self._flag())

    def evaluate(self, X, pos_item, neg_items):
        # reference models/s3rec.py:102-115 -> ([batch, 1], [batch, candidates]) from the last position
        self._scoring_only("evaluate")
        h_last = self._encode(X, last_only=True)
        return engine.s3rec_candidate_scores(self.item_embedding.weight.detach(), h_last, pos_item.contiguous(),
                                             neg_items.contiguous(), err_flag=self._flag())

    def encode(self, X):
        raise NotImplementedError("S3Rec.encode: pre-training is not built (the reference's encode() cannot run as "
                                  "published: models/s3rec.py:117-118)")

    def pretrain(self, *sequences):
        raise NotImplementedError("S3Rec.pretrain: pre-training is not built (the reference's encode() cannot run as "
                                  "published: models/s3rec.py:117-118)")
