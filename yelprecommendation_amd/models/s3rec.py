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

Pre-training (models/s3rec.py:117-181).  The reference's own ``encode`` calls ``_self_attention_block`` without its
two mask arguments, so it cannot run as published; the repair is the obvious one: ``encode(X)`` is what ``finetune``
runs before its prediction layer (``padding_mask = X <= 0`` and the causal mask), every quirk of the encoder kept.
In ``train()`` mode under grad ``encode`` is an autograd node over the training encoder and the HIP backward; in
``eval()`` mode under ``torch.no_grad()`` it is the scoring encoder.  ``pretrain(item_masked, segment_masked,
pos_segments, neg_segments)`` returns the reference's four outputs dense (its ``map()`` uses ``aap_weight``, kept:
``map_weight`` takes no part and keeps ``grad = None``); the encoding of the segment-masked sequence, which the
reference computes and never consumes, is skipped.  ``pretrain_loss`` gives the four losses of
trainers/s3rec_trainer.py:137-158 through the catalogue-BCE kernel (csrc/s3rec_pretrain.hip): no [B, L, num_items +
1] array exists in its forward or backward.  On CPU tensors all three raise NotImplementedError.

Full-catalogue evaluation (new; the reference ranks the held-out item against 99 sampled negatives only).
``rank_catalogue(X, target, history, users)`` gives the exact 0-based place of one item per sequence among ALL items
(csrc/s3rec_rank.hip: no [B, num_items + 1] array), ``recommend(X, k, history, users)`` the top-k item ids through the
fused list sweep the other models evaluate with; both run the ``last_only`` encoder, in eval() mode under
``torch.no_grad()`` on CUDA tensors only.

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

    # -- full-catalogue evaluation (csrc/s3rec_rank.hip; the lists through engine.mf_recommend) ----------------
    def _catalogue_rows(self, what, X, history, users):
        """The checks of the two full-catalogue entry points and the CSR rows of the batch: (ptr, idx, rows) or
        (None, None, None) without a history."""
        self._scoring_only(what)
        if not self.item_embedding.weight.is_cuda or not X.is_cuda:
            raise NotImplementedError(f"S3Rec.{what}: full-catalogue evaluation is not built for CPU tensors (the "
                                      "kernels run on the GPU only): move the model and the batch to the device")
        if history is None:
            return None, None, None
        ptr, idx = history
        rows = torch.arange(X.shape[0], device=X.device) if users is None else users.to(X.device).long().contiguous()
        if rows.numel() != X.shape[0]:
            raise ValueError(f"S3Rec.{what}: users must hold one CSR row per sequence")
        return ptr, idx, rows

    def _catalogue_lists(self, h_last, k, ptr, idx, rows, target=None):
        """[B, k] int64 item ids 1..num_items, best first, -1 where a row has fewer than k free items: the rows' history
        lists gathered into a batch CSR in the 0-based space of ``item_embedding.weight[1:]`` (index preparation), then
        engine.mf_recommend.  ``target`` [B]: an entry equal to the row's target is dropped, as the rank sweep does."""
        B, dev = h_last.shape[0], h_last.device
        mptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        midx = torch.zeros(0, dtype=torch.int64, device=dev)
        K = 0 if ptr is None else ptr.numel() - 1
        if K > 0 and B > 0:
            ok = (rows >= 0) & (rows < K)
            self._flag().bitwise_or_((~ok).any().to(torch.int32) * engine.FLAG_BAD_USER)
            r = rows.clamp(0, K - 1)
            start = ptr[r]
            n = torch.where(ok, ptr[r + 1] - start, torch.zeros_like(start))
            row_of = torch.repeat_interleave(torch.arange(B, device=dev), n)
            first = torch.cumsum(n, 0) - n
            vals = idx[start[row_of] + torch.arange(row_of.numel(), device=dev) - first[row_of]]
            keep = (vals >= 1) & (vals <= self.num_items)
            if target is not None:
                keep &= vals != target[row_of]
            row_of, midx = row_of[keep], (vals[keep] - 1).contiguous()
            mptr[1:] = torch.cumsum(torch.bincount(row_of, minlength=B), 0)
        table = self.item_embedding.weight.detach()[1:]
        lists = engine.mf_recommend(h_last, table, torch.arange(B, device=dev), mptr, midx, int(k))
        free = self.num_items - (mptr[1:] - mptr[:-1])
        return torch.where(torch.arange(int(k), device=dev)[None, :] < free[:, None], lists + 1,
                           torch.full_like(lists, -1))

    def rank_catalogue(self, X, target, history=None, users=None):
        """int64 [B]: the 0-based place of item ``target[b]`` (1..num_items; 0: no target, -1) among ALL items by the
        score <h[b, L - 1], item_embedding.weight[r]>, score descending and id ascending among equal scores, the pad
        row never a candidate.  ``history`` = (ptr, idx), a CSR of ascending 1-based item ids per user
        (``S3RecSequences.history``): row ``users[b]`` (default b) is left out of the count, except the target itself.
        eval() mode under torch.no_grad(), CUDA tensors; ids go through the model's error flag."""
        ptr, idx, rows = self._catalogue_rows("rank_catalogue", X, history, users)
        h_last = self._encode(X, last_only=True)
        return engine.s3rec_catalogue_rank(h_last, self.item_embedding.weight.detach(), target.contiguous(), ptr, idx,
                                           rows, first_col=1, err_flag=self._flag())

    def recommend(self, X, k, history=None, users=None):
        """int64 [B, k]: the k best item ids (1..num_items) for each sequence, best first, the row's history left out
        and the pad never returned; rows with fewer than k free items are padded with -1.  Same modes as
        ``rank_catalogue``."""
        ptr, idx, rows = self._catalogue_rows("recommend", X, history, users)
        return self._catalogue_lists(self._encode(X, last_only=True), k, ptr, idx, rows)

    def rank_and_recommend(self, X, target, k, history=None, users=None):
        """(rank_catalogue, recommend) from one run of the encoder, the lists keeping the target as the rank does: a
        row's target is in its list exactly when its rank is below k (up to float near-ties between the sweeps)."""
        ptr, idx, rows = self._catalogue_rows("rank_and_recommend", X, history, users)
        h_last = self._encode(X, last_only=True)
        target = target.contiguous()
        rank = engine.s3rec_catalogue_rank(h_last, self.item_embedding.weight.detach(), target, ptr, idx, rows,
                                           first_col=1, err_flag=self._flag())
        return rank, self._catalogue_lists(h_last, k, ptr, idx, rows, target=target)

    # -- pre-training (reference models/s3rec.py:117-181) ----------------------------------------------------
    def _pretrain_on_device(self, what):
        if not self.item_embedding.weight.is_cuda:
            raise NotImplementedError(f"S3Rec.{what}: pre-training is not built for CPU tensors (the kernels run on "
                                      "the GPU only): move the model and the batch to the device")

    def encode(self, X, *, dropout_seed=None):
        """h [B, L, E]: what ``finetune`` runs before its prediction layer (the reference's one-line defect repaired
        with the masks finetune builds).  eval() under no_grad: the scoring encoder; train() under grad: an autograd
        node over the training encoder and the HIP backward."""
        self._pretrain_on_device("encode")
        if X.dim() != 2 or X.shape[1] != self.cfg.max_seq_len:
            raise ValueError(f"S3Rec: X must be [batch, max_seq_len = {self.cfg.max_seq_len}], got {tuple(X.shape)}")
        if torch.is_grad_enabled() and self.training:
            p = float(self.cfg.dropout_ratio)
            seed = 0
            if p > 0.0:
                seed = self._dropout_seed() if dropout_seed is None else int(dropout_seed)
            return _EncodeFn.apply(self, X.contiguous(), seed, p, self.item_embedding.weight, self.positional_encoding,
                                   *self._block_tensors())
        if torch.is_grad_enabled() or self.training:
            raise NotImplementedError("S3Rec.encode: pre-training runs in train() mode with grad enabled, scoring in "
                                      "eval() mode under torch.no_grad()")
        return self._encode(X, last_only=False)

    def pretrain(self, *sequences, dropout_seeds=None):
        """reference models/s3rec.py:120-135: (aap [B, L, A], mip [B, L, num_items + 1], map [B, L, A], (sp_pos [B],
        sp_neg [B])) DENSE, ``encode`` plus ordinary torch products: the reference's surface, the baseline of
        scripts/bench_s3rec_pretrain.py and the path ``pretrain_loss`` is checked against.  The encoding of the
        segment-masked sequence, which the reference computes and never consumes, is skipped."""
        self._pretrain_on_device("pretrain")
        if len(sequences) != 4:
            raise TypeError("S3Rec.pretrain(item_masked_sequences, subsequence_masked_sequences, pos_subsequences, "
                            "neg_subsequences)")
        item_masked, _segment_masked, pos_segments, neg_segments = sequences
        s = dropout_seeds or (None, None, None)
        h = self.encode(item_masked, dropout_seed=s[0])
        h_pos = self.encode(pos_segments, dropout_seed=s[1])
        h_neg = self.encode(neg_segments, dropout_seed=s[2])
        FW = self.aap_weight(h)
        aap = torch.matmul(FW, self.attribute_embedding.weight.T)
        mip = torch.matmul(self.mip_weight(h), self.item_embedding.weight.t())
        map_ = torch.matmul(FW, self.attribute_embedding.weight.T)       # the reference's map() uses aap_weight
        SW = self.sp_weight(h[:, -1, :])
        return aap, mip, map_, ((SW * h_pos[:, -1, :]).sum(-1), (SW * h_neg[:, -1, :]).sum(-1))

    def pretrain_loss(self, X, masks, item_masked, pos_segments, neg_segments, attr_ptr, attr_idx, *,
                      dropout_seeds=None):
        """(aap_loss, mip_loss, map_loss, sp_loss) of reference trainers/s3rec_trainer.py:137-158 without a
        [B, L, R] array: X [B, L] the unmasked sequences (the targets come from them), masks [B, L] bool,
        item_masked = masks * X, the two SP segments, and the device CSR item id -> categories (attr_ptr
        [num_items + 2], attr_idx; int64).  Each catalogue loss is one autograd node over yr_s3rec_catalogue_bce."""
        self._pretrain_on_device("pretrain_loss")
        s = dropout_seeds or (None, None, None)
        h = self.encode(item_masked, dropout_seed=s[0])
        h_pos = self.encode(pos_segments, dropout_seed=s[1])
        h_neg = self.encode(neg_segments, dropout_seed=s[2])
        B, L, E = h.shape
        on = masks.reshape(-1).to(torch.float32)
        off = 1.0 - on
        ones = torch.ones_like(on)
        key = X.reshape(-1).contiguous()
        flag = self._flag()
        FA = self.aap_weight(h).reshape(B * L, E)
        FM = self.mip_weight(h).reshape(B * L, E)
        A, I = self.attribute_embedding.weight, self.item_embedding.weight
        aap_loss = _CatalogueBCEFn.apply(FA, A, ones, on, key, attr_ptr, attr_idx, flag)
        mip_loss = _CatalogueBCEFn.apply(FM, I, off, off, key, None, None, flag)
        map_loss = _CatalogueBCEFn.apply(FA, A, off, off, key, attr_ptr, attr_idx, flag)
        SW = self.sp_weight(h[:, -1, :])
        sp_out = torch.cat([(SW * h_neg[:, -1, :]).sum(-1), (SW * h_pos[:, -1, :]).sum(-1)])
        sp_actual = torch.cat([torch.zeros(B, device=h.device), torch.ones(B, device=h.device)])
        sp_loss = nn.functional.binary_cross_entropy_with_logits(sp_out, sp_actual)
        return aap_loss, mip_loss, map_loss, sp_loss


class _EncodeFn(torch.autograd.Function):
    """``encode`` under grad: the stash-keeping encoder forward; backward runs the backward kernel, the gradient
    products / column sums and the item-lookup gradient of X alone, all in a fixed order without atomics."""

    @staticmethod
    def forward(ctx, model, X, seed, p, item_emb, pos_enc, *block_tensors):
        heads, blocks = int(model.cfg.num_heads), int(model.cfg.num_blocks)
        params = model._params()
        flag = model._flag()
        h, ws = engine.s3rec_encode_train(item_emb.detach(), pos_enc.detach(), params, X, heads, blocks, seed=seed, p=p,
                                          err_flag=flag)
        ctx.save_for_backward(X, ws, params, item_emb)
        ctx.cfg = (heads, blocks, seed, p, flag, [t.shape for t in block_tensors])
        return h

    @staticmethod
    def backward(ctx, gh):
        X, ws, params, item_emb = ctx.saved_tensors
        heads, blocks, seed, p, flag, shapes = ctx.cfg
        (B, L), E = X.shape, gh.shape[-1]
        d_emb = engine.s3rec_backward(params, X, gh.contiguous().view(B, L, E), ws, heads, blocks, seed=seed, p=p)
        packed = engine.s3rec_param_grads(ws, B, L, E, heads, blocks)
        d_pos = engine.colsum(d_emb.view(B, L * E)).view(L, E)
        d_item = torch.zeros_like(item_emb)
        engine.s3rec_item_grad_one(X, d_emb, d_item, err_flag=flag)
        grads, at = [], 0
        for shape in shapes:
            n = shape.numel()
            grads.append(packed[at:at + n].view(shape))
            at += n
        return (None, None, None, None, d_item, d_pos, *grads)


class _CatalogueBCEFn(torch.autograd.Function):
    """One catalogue loss (csrc/s3rec_pretrain.hip): the mean BCE with logits of zscale <F, T> against the listed
    targets.  The forward call takes the loss and both gradients (the sweep is the cost; the gradient of a scalar
    needs no second sweep); backward scales them by the arriving gradient."""

    @staticmethod
    def forward(ctx, F, T, zscale, yscale, key, tgt_ptr, tgt_idx, flag):
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        loss, _, dF, dT = engine.s3rec_catalogue_bce(F.detach().contiguous(), T.detach().contiguous(), zscale, yscale,
                                                     key, tgt_ptr, tgt_idx, want_dF=bool(need and ctx.needs_input_grad[0]),
                                                     want_dT=bool(need and ctx.needs_input_grad[1]), err_flag=flag)
        ctx.grads = (dF, dT)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        dF, dT = ctx.grads
        return (None if dF is None else dF * g, None if dT is None else dT * g, None, None, None, None, None, None)
