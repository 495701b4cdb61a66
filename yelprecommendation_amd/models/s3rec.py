"""S3Rec — drop-in for the scoring surface of reference models/s3rec.py:10-115,184-214.

Same constructor ``S3Rec(cfg, num_items, attributes_count)``, same sub-modules in the same construction order (so a
seeded build draws the reference's RNG stream), same ``_init_weights`` reach — Xavier on the two embeddings, on the
Linears directly inside the ``ffn1s`` / ``ffn2s`` lists and on the four ``*_weight`` Linears; the attention Linears
(one level deeper) and the LayerNorms keep PyTorch's defaults; ``positional_encoding`` is ``torch.rand`` — and the
same parameter names, so ``load_state_dict(torch.load('best_model.pt'), strict=True)`` takes a reference checkpoint.
Build on the CPU under the seed, then move to the GPU (as models/mf.py).

``finetune(X, pos_items, neg_items)`` and ``evaluate(X, pos_item, neg_items)`` return the reference's shapes and run
the fused encoder of csrc/s3rec.hip (one launch from the embedding gather to the last LayerNorm) plus one score
launch.  ``evaluate`` is forward-only: ``eval()`` mode under ``torch.no_grad()``.

``finetune`` in ``train()`` mode with grad enabled trains: its two outputs carry an autograd node whose backward runs the HIP backward
pass (csrc/s3rec.hip) and gives ``item_embedding.weight``, ``positional_encoding`` and every attention / FFN /
LayerNorm tensor its gradient; ``attribute_embedding`` and the four ``*_weight`` take no part and keep ``grad =
None``, as after the reference's ``backward``.  With ``dropout_ratio > 0`` it applies the reference's two dropouts per block
(models/s3rec.py:62,68) with a mask drawn in the kernel from a fresh 64-bit seed per call — from a generator the
model owns, seeded from ``torch.initial_seed()``; ``finetune(..., dropout_seed=s)`` fixes it.  ``eval()`` mode is for
scoring: under ``torch.no_grad()`` it scores, with grad enabled it raises NotImplementedError (as it did before training
was built; ``train()`` mode with ``dropout_ratio = 0`` is training without dropout).

``pretrain`` / ``encode`` raise NotImplementedError — the reference's own ``encode`` calls
``_self_attention_block`` without its two mask arguments (models/s3rec.py:117-118), so its pre-training cannot run
as published and there is nothing to be faithful to.

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


class _FinetuneFn(torch.autograd.Function):
    """``finetune`` under grad: the stash-keeping encoder and the score launch forward; backward runs the score
    gradient, the backward kernel, the gradient products / column sums and the item gradient (csrc/s3rec.hip) and
    hands ``item_embedding.weight``, ``positional_encoding`` and every tensor of ``_block_tensors()`` its gradient."""

    @staticmethod
    def forward(ctx, model, X, pos_items, neg_items, seed, p, item_emb, pos_enc, *block_tensors):
        heads, blocks = int(model.cfg.num_heads), int(model.cfg.num_blocks)
        params = model._params()
        flag = model._flag()
        h, ws = engine.s3rec_encode_train(item_emb.detach(), pos_enc.detach(), params, X, heads, blocks, seed=seed, p=p,
                                          err_flag=flag)
        pos, neg = engine.s3rec_seq_scores(item_emb.detach(), h, pos_items, neg_items, err_flag=flag)
        ctx.save_for_backward(X, pos_items, neg_items, h, ws, params, item_emb)
        ctx.cfg = (heads, blocks, seed, p, flag, [t.shape for t in block_tensors])
        return pos, neg

    @staticmethod
    def backward(ctx, gpos, gneg):
        X, pos_items, neg_items, h, ws, params, item_emb = ctx.saved_tensors
        heads, blocks, seed, p, flag, shapes = ctx.cfg
        (B, L), E = X.shape, h.shape[-1]
        gpos, gneg = gpos.contiguous(), gneg.contiguous()
        dh = engine.s3rec_score_grad(item_emb.detach(), pos_items, neg_items, gpos, gneg, err_flag=flag)
        d_emb = engine.s3rec_backward(params, X, dh.view(B, L, E), ws, heads, blocks, seed=seed, p=p)
        packed = engine.s3rec_param_grads(ws, B, L, E, heads, blocks)
        d_pos = engine.colsum(d_emb.view(B, L * E)).view(L, E)
        d_item = torch.zeros_like(item_emb)
        engine.s3rec_item_grad(X, pos_items, neg_items, d_emb, h, gpos, gneg, d_item, err_flag=flag)
        grads, at = [], 0
        for shape in shapes:
            n = shape.numel()
            grads.append(packed[at:at + n].view(shape))
            at += n
        return (None, None, None, None, None, None, d_item, d_pos, *grads)


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
        self._dropout_gen = None

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
                f"S3Rec.{what}: training is not built for this entry point (it goes through finetune): call it in "
                "eval() mode under torch.no_grad()")

    def _dropout_seed(self):
        """A fresh 64-bit seed per training call from a generator the model owns, seeded from torch.initial_seed()
        (so utils.set_seed makes runs repeatable)."""
        if self._dropout_gen is None:
            self._dropout_gen = torch.Generator().manual_seed(torch.initial_seed())
        lo, hi = torch.randint(0, 2 ** 32, (2,), generator=self._dropout_gen, dtype=torch.int64).tolist()
        return (hi << 32) | lo

    def _encode(self, X, last_only):
        if X.dim() != 2 or X.shape[1] != self.cfg.max_seq_len:
            raise ValueError(f"S3Rec: X must be [batch, max_seq_len = {self.cfg.max_seq_len}], got {tuple(X.shape)}")
        return engine.s3rec_encode(self.item_embedding.weight.detach(), self.positional_encoding.detach(),
                                   self._params(), X.contiguous(), int(self.cfg.num_heads), int(self.cfg.num_blocks),
                                   last_only=last_only, err_flag=self._flag())

    # -- reference surface -----------------------------------------------------------------------------
    def finetune(self, X, pos_items, neg_items, *, dropout_seed=None):
        # reference models/s3rec.py:89-100 -> two [batch * max_seq_len] score vectors, padded positions included
        if torch.is_grad_enabled():
            if not self.item_embedding.weight.is_cuda:
                raise NotImplementedError("S3Rec.finetune: training is not built for CPU tensors (the kernels run on "
                                          "the GPU only): move the model and the batch to the device")
            if not self.training:
                # the scoring contract from before training existed, which its tests still hold: eval() scores only
                raise NotImplementedError("S3Rec.finetune: training is not built for eval() mode: call train() to "
                                          "train (dropout_ratio = 0 trains without dropout), or score under "
                                          "torch.no_grad()")
            if X.dim() != 2 or X.shape[1] != self.cfg.max_seq_len:
                raise ValueError(f"S3Rec: X must be [batch, max_seq_len = {self.cfg.max_seq_len}], got {tuple(X.shape)}")
            p = float(self.cfg.dropout_ratio)
            seed = 0
            if p > 0.0:
                seed = self._dropout_seed() if dropout_seed is None else int(dropout_seed)
            return _FinetuneFn.apply(self, X.contiguous(), pos_items.contiguous(), neg_items.contiguous(), seed, p,
                                     self.item_embedding.weight, self.positional_encoding, *self._block_tensors())
        if self.training:
            raise NotImplementedError("S3Rec.finetune: training is not built under torch.no_grad() (dropout without a "
                                      "backward pass): call eval() first, or enable grad")
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
