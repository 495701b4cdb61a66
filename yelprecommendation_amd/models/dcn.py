"""Deep & Cross Network — drop-in for reference models/dcn.py:7-62.

Same constructor ``DCN(cfg, num_users, num_items, attributes_count)``, same parameter names (``user_embedding.weight``,
``attributes_embeddings.0.weight``, ``deep.0.weight``, ``cross_weights.0``, ``cross_bias.0``, ``output_layer.weight``,
...: state_dict-compatible with the reference's ``best_model.pt``), same construction order and initialisation quirks
(``_init_weights`` reaches the two id embeddings and the output layer only; the attribute embeddings keep N(0, 1), the
deep Linears PyTorch's default, the cross weights and biases ``torch.rand``), so a seeded run starts from the
reference's tensors.  Build on the CPU under the seed, then move to the GPU (as models/mf.py).

Underneath, every op is a HIP kernel (csrc/dcn.hip): the input rows are gathered on the device from the item ->
attributes table, the deep tower is yr_gemm_f32 with a ReLU epilogue, and one head kernel runs the cross network in
closed form (x_l = alpha_l x0 + beta_l), the output layer, the sigmoid and BPRLoss with their backward.
``score_catalogue`` scores users against the whole catalogue without building the pair rows.

Supported: embed_size 16 / 32 / 64 / 128, one or two hidden layers of widths that are multiples of 32 up to 1024,
1 to 8 cross orders, two attributes (categories, statecity).  Anything else raises NotImplementedError here.
"""
import torch
import torch.nn as nn

from .. import engine
from .base_model import BaseModel


def check_supported(embed_size, hidden_dims, cross_orders, n_attributes=2):
    if embed_size not in engine.SUPPORTED_WIDTHS:
        raise NotImplementedError(f"DCN: embed_size {embed_size} (the kernels take {engine.SUPPORTED_WIDTHS})")
    if n_attributes != 2:
        raise NotImplementedError("DCN: exactly two item attributes (categories, statecity)")
    if not 1 <= len(hidden_dims) <= 2:
        raise NotImplementedError(f"DCN: hidden_dims {list(hidden_dims)}: one or two hidden layers are supported")
    for h in hidden_dims:
        if h % 32 or not 0 < h <= engine.DCN_MAX_H:
            raise NotImplementedError(f"DCN: hidden width {h}: multiples of 32 up to {engine.DCN_MAX_H} are supported")
    if not 1 <= cross_orders <= engine.DCN_MAX_L:
        raise NotImplementedError(f"DCN: cross_orders {cross_orders}: 1 to {engine.DCN_MAX_L} are supported")


class _DCNForward(torch.autograd.Function):
    """pred = model(user, item, categories, statecity) with the categories / statecity given per row."""

    @staticmethod
    def forward(ctx, model, user_id, item_id, cats, sc, *params):
        attrs = model._attrs(cats, sc)
        x0, hs = model._rows_forward(user_id, item_id, None, attrs, attr_per_row=True)
        pred = torch.empty(x0.shape[0], dtype=torch.float32, device=x0.device)
        model._head(x0, hs, bpr=False, pred=pred)
        ctx.model = model
        ctx.state = (user_id, item_id, attrs, x0, hs, pred)
        return pred.unsqueeze(1)

    @staticmethod
    def backward(ctx, gout):
        model = ctx.model
        if model.deterministic:
            raise NotImplementedError("DCN: deterministic=true covers the fused training step (bpr_loss_backward); the "
                                      "per-row attribute form of forward().backward() has no ordered scatter")
        user_id, item_id, attrs, x0, hs, pred = ctx.state
        params = model._param_list()
        grads = [torch.zeros_like(p) for p in params]
        model._rows_backward(user_id, item_id, None, attrs, True, x0, hs, dict(zip(params, grads)),
                             gpred=gout.reshape(-1).contiguous(), pred=pred)
        return (None, None, None, None, None) + tuple(grads)


class DCN(BaseModel):
    def __init__(self, cfg, num_users, num_items, attributes_count: list):
        super().__init__()
        check_supported(cfg.embed_size, list(cfg.hidden_dims), int(cfg.cross_orders), len(attributes_count))
        # reference models/dcn.py:9-21, in its order (the RNG stream depends on it)
        self.user_embedding = nn.Embedding(num_users, cfg.embed_size, dtype=torch.float32)
        self.item_embedding = nn.Embedding(num_items, cfg.embed_size, dtype=torch.float32)
        self.attributes_embeddings = nn.ModuleList([
            nn.Embedding(count + 1, cfg.embed_size, dtype=torch.float32) for count in attributes_count
        ])
        self.hidden_dims = [(2 + len(attributes_count)) * cfg.embed_size] + list(cfg.hidden_dims)
        self.cross_dims = [(2 + len(attributes_count)) * cfg.embed_size] * int(cfg.cross_orders)
        self.deep = nn.Sequential()
        for idx in range(len(self.hidden_dims) - 1):
            self.deep.append(nn.Linear(self.hidden_dims[idx], self.hidden_dims[idx + 1]))
            self.deep.append(nn.ReLU())
        self.cross_weights = nn.ParameterList([nn.Parameter(torch.rand(dim)) for dim in self.cross_dims])
        self.cross_bias = nn.ParameterList([nn.Parameter(torch.rand(dim)) for dim in self.cross_dims])
        self.output_layer = nn.Linear(self.hidden_dims[-1] + self.cross_dims[-1], 1)
        self.device = cfg.device
        self._init_weights()
        self.num_users, self.num_items = num_users, num_items
        self.embed_size = cfg.embed_size
        self.cat_ids = None
        self.sc_ids = None
        self._err_flag = None
        self._loss_partials = None
        # deterministic: the training step sums every gradient in a fixed order (csrc/dcn_owned.hip: no float atomics)
        self.deterministic = False
        self._attr_lists = None
        self._owned_ws = {}

    def _init_weights(self):
        # reference models/dcn.py:34-40: direct children only
        for child in self.children():
            if isinstance(child, nn.Embedding):
                nn.init.kaiming_normal_(child.weight)
            elif isinstance(child, nn.Linear):
                nn.init.kaiming_normal_(child.weight)
                nn.init.zeros_(child.bias)

    # -- device tables and buffers -------------------------------------------------------
    def set_item_attributes(self, cat_ids, sc_ids):
        """The item -> attributes table (DCNDataPipeline.cat_ids / sc_ids) the training and scoring kernels gather from."""
        dev = self.user_embedding.weight.device
        self.cat_ids = cat_ids.to(dev, torch.int32).contiguous()
        self.sc_ids = sc_ids.to(dev, torch.int32).contiguous()
        self._attr_lists = None

    def _lists(self):
        """The table inverted (category -> items, state-city -> items) for the ordered scatter: built on first use of
        the deterministic mode, once per table."""
        dev = self.user_embedding.weight.device
        if self._attr_lists is None or self._attr_lists.cat_ptr.device != dev:
            cats, sc, nc, ns = self._attrs()
            self._attr_lists = engine.DCNAttrLists(cats, sc, nc, ns, device=dev)
        return self._attr_lists

    def _owned_workspace(self, which, nbytes):
        """Cached uint8 scratch of the ordered kernels (contents irrelevant between calls), grown on demand."""
        dev = self.user_embedding.weight.device
        ws = self._owned_ws.get(which)
        if ws is None or ws.device != dev or ws.numel() < nbytes:
            ws = self._owned_ws[which] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        return ws

    def _linears(self):
        return [m for m in self.deep if isinstance(m, nn.Linear)]

    def _param_list(self):
        return list(self.parameters())

    def _flag(self):
        dev = self.user_embedding.weight.device
        if self._err_flag is None or self._err_flag.device != dev:
            self._err_flag = engine.new_error_flag(dev)
        return self._err_flag

    def _partials(self):
        dev = self.user_embedding.weight.device
        if self._loss_partials is None or self._loss_partials.device != dev:
            self._loss_partials = torch.zeros(engine.LOSS_PARTIALS, dtype=torch.float32, device=dev)
        return self._loss_partials

    def check_indices(self):
        if self._err_flag is not None:
            engine.raise_on_flag(self._err_flag, "DCN")

    def _attrs(self, cats=None, sc=None):
        C, S = self.attributes_embeddings[0].weight, self.attributes_embeddings[1].weight
        if cats is None:
            if self.cat_ids is None:
                raise RuntimeError("DCN: set_item_attributes() first (the item -> attributes table)")
            cats, sc = self.cat_ids, self.sc_ids
        else:
            cats = cats.to(torch.int32).reshape(cats.shape[0], -1).contiguous()
            sc = sc.to(torch.int32).reshape(-1).contiguous()
        return (cats, sc, C.shape[0], S.shape[0])

    def _cross_packed(self):
        """The cross weights / biases as [L, F] tensors whose rows ARE the parameters: the head kernel reads one
        contiguous block.  Re-packed whenever a parameter was replaced (.to(), load_state_dict(assign=True) ...)."""
        out = []
        for plist in (self.cross_weights, self.cross_bias):
            block = _as_block([p.data for p in plist])
            if block is None:
                block = torch.stack([p.data for p in plist])
                for l, p in enumerate(plist):
                    p.data = block[l]
            out.append(block)
        return tuple(out)

    def _cross_grads(self):
        """The same for the gradients: [L, F] blocks whose rows are the parameters' ``.grad`` (the values a gradient
        already holds are kept; a missing one starts at zero)."""
        out = []
        for plist in (self.cross_weights, self.cross_bias):
            block = _as_block([p.grad for p in plist])
            if block is None:
                block = torch.stack([p.grad if p.grad is not None else torch.zeros_like(p) for p in plist])
                for l, p in enumerate(plist):
                    p.grad = block[l]
            out.append(block)
        return tuple(out)

    # -- the pieces of a step ------------------------------------------------------------------
    def _rows_forward(self, user, item_a, item_b, attrs, attr_per_row=False):
        U, I = self.user_embedding.weight.detach(), self.item_embedding.weight.detach()
        C, S = self.attributes_embeddings[0].weight.detach(), self.attributes_embeddings[1].weight.detach()
        x0 = engine.dcn_assemble(U, I, C, S, attrs, user.contiguous(), item_a.contiguous(),
                                 None if item_b is None else item_b.contiguous(), attr_per_row=attr_per_row,
                                 err_flag=self._flag())
        hs = [x0]
        for lin in self._linears():
            hs.append(engine.gemm_f32(hs[-1], lin.weight.detach(), transB=True, bias=lin.bias.detach(),
                                      act=engine.ACT_RELU))
        return x0, hs

    def _head(self, x0, hs, bpr, inv_batch=0.0, pred=None, gpred=None, grads=None, loss_partials=None):
        cw, cb = self._cross_packed()
        Wo, bo = self.output_layer.weight.detach(), self.output_layer.bias.detach()
        ws = None
        if self.deterministic and grads is not None:
            units = x0.shape[0] // 2 if bpr else x0.shape[0]
            ws = self._owned_workspace("head", engine.dcn_owned_head_workspace_bytes(units, x0.shape[1], hs[-1].shape[1],
                                                                                     cw.shape[0]))
        engine.dcn_head(x0, hs[-1], cw, cb, Wo, bo, bpr, inv_batch=inv_batch, pred=pred, gpred=gpred, grads=grads,
                        loss_partials=loss_partials, deterministic=self.deterministic, workspace=ws)

    def _rows_backward(self, user, item_a, item_b, attrs, attr_per_row, x0, hs, grads, gpred=None, pred=None,
                       inv_batch=0.0, loss_partials=None):
        """Head (forward again + backward), deep tower backward and the scatter into the tables.  ``grads``: parameter
        -> the tensor its gradient is ADDED to (cross rows: the rows of two [L, F] blocks)."""
        cw_rows = [grads[p] for p in self.cross_weights]
        cb_rows = [grads[p] for p in self.cross_bias]
        # the kernel adds into [L, F] blocks: the gradients themselves when they are one, else staged copies
        cw_g, cb_g = _as_block(cw_rows), _as_block(cb_rows)
        staged = [(rows, torch.stack(rows)) for rows, blk in ((cw_rows, cw_g), (cb_rows, cb_g)) if blk is None]
        if cw_g is None:
            cw_g = staged[0][1]
        if cb_g is None:
            cb_g = staged[-1][1]
        dh = torch.empty_like(hs[-1])
        dx0 = torch.empty_like(x0)
        Wo, bo = self.output_layer.weight, self.output_layer.bias
        self._head(x0, hs, bpr=gpred is None, inv_batch=inv_batch, gpred=gpred,
                   grads=(dh, dx0, cw_g, cb_g, grads[Wo], grads[bo]), loss_partials=loss_partials)
        for rows, block in staged:
            for l, t in enumerate(rows):
                t.copy_(block[l])
        g = dh
        lins = self._linears()
        for li in range(len(lins) - 1, -1, -1):
            lin = lins[li]
            engine.gemm_f32(g, hs[li], transA=True, out=grads[lin.weight], accumulate=True)
            engine.colsum(g, out=grads[lin.bias], accumulate=True)
            if li > 0:
                g = engine.relu_bwd_(engine.gemm_f32(g, lin.weight.detach()), hs[li])
            else:
                engine.gemm_f32(g, lin.weight.detach(), out=dx0, accumulate=True)
        C, S = self.attributes_embeddings[0].weight, self.attributes_embeddings[1].weight
        lists = ws = None
        if self.deterministic:
            lists = self._lists()
            ws = self._owned_workspace("scatter", engine.dcn_owned_scatter_workspace_bytes(
                self.num_users, self.num_items, user.numel(), self.embed_size, lists))
        engine.dcn_assemble_bwd(dx0, attrs, user.contiguous(), item_a.contiguous(),
                                None if item_b is None else item_b.contiguous(), grads[self.user_embedding.weight],
                                grads[self.item_embedding.weight], grads[C], grads[S], self.num_users,
                                attr_per_row=attr_per_row, err_flag=self._flag(), deterministic=self.deterministic,
                                lists=lists, workspace=ws)

    # -- reference surface ---------------------------------------------------------------------
    def forward(self, user_id, item_id, *attributes):
        # reference models/dcn.py:42-57 -> [B, 1] sigmoid outputs
        cats, sc = attributes
        return _DCNForward.apply(self, user_id, item_id, cats, sc, *self._param_list())

    # -- fused training op ---------------------------------------------------------------------
    def bpr_loss_backward(self, user_id, pos_item, neg_item, loss_out=None, loss_accum=None, inv_batch=None,
                          backward=True):
        """model(u, p), model(u, n), BPRLoss and loss.backward() of reference dcn_trainer.py:102-116 for a batch:
        the pos and neg rows side by side through one gather, the deep tower GEMMs and one head kernel.  Gradients
        are ACCUMULATED into every parameter's dense ``.grad`` (allocated zero-filled on first use).  Returns the
        batch-mean loss as a 1-element device tensor; ``loss_accum`` (float64[1]) also receives it.
        ``self.deterministic``: the ordered head and the ordered scatter (every GEMM of the tower already runs with
        split_k = 1, one owner per output); an empty batch is then a step with a zero loss that adds nothing."""
        B = user_id.numel()
        scale = inv_batch if inv_batch is not None else (1.0 / B if B else 0.0)
        attrs = self._attrs()
        partials = self._partials()
        if self.deterministic and B == 0:
            if backward:
                self._cross_grads()
                for p in self.parameters():
                    if p.grad is None:
                        p.grad = torch.zeros_like(p)
            partials.zero_()
            return engine.loss_finalize(partials, 0.0, loss_out, loss_accum)
        x0, hs = self._rows_forward(user_id, pos_item, neg_item, attrs)
        if backward:
            self._cross_grads()
            for p in self.parameters():
                if p.grad is None:
                    p.grad = torch.zeros_like(p)
            grads = {p: p.grad for p in self.parameters()}
            self._rows_backward(user_id, pos_item, neg_item, attrs, False, x0, hs, grads, inv_batch=scale,
                                loss_partials=partials)
        else:
            self._head(x0, hs, bpr=True, loss_partials=partials)
        return engine.loss_finalize(partials, scale, loss_out, loss_accum)

    # -- evaluation ---------------------------------------------------------------------------------
    @torch.no_grad()
    def score_prep(self):
        """The per-evaluation operands of the fused scorer: the first layer split over the concatenation
        (Au = U W1[:, :D]^T, Bi = x_item W1[:, D:]^T + b1) and the cross / output dot products split the same way."""
        D = self.embed_size
        U, I = self.user_embedding.weight.detach(), self.item_embedding.weight.detach()
        C, S = self.attributes_embeddings[0].weight.detach(), self.attributes_embeddings[1].weight.detach()
        x_item = engine.dcn_assemble(None, I, C, S, self._attrs(), None, None, err_flag=self._flag())
        lins = self._linears()
        W1, b1 = lins[0].weight.detach(), lins[0].bias.detach()
        Au = engine.gemm_f32(U, W1[:, :D], transB=True)
        Bi = engine.gemm_f32(x_item, W1[:, D:], transB=True, bias=b1)
        cw, cb = self._cross_packed()
        H = self.hidden_dims[-1]
        Wc = torch.cat([cw, self.output_layer.weight.detach()[:, H:]], 0)
        Pu = engine.gemm_f32(U, Wc[:, :D], transB=True)
        Pi = engine.gemm_f32(x_item, Wc[:, D:], transB=True)
        return Au, Bi, Pu, Pi

    @torch.no_grad()
    def score_catalogue(self, users, out, prep=None):
        """out[r, i] = model(users[r], i) for every item i (the sigmoid outputs; reference dcn_trainer.py:145-160)."""
        Au, Bi, Pu, Pi = prep if prep is not None else self.score_prep()
        lins = self._linears()
        W2 = b2 = None
        if len(lins) == 2:
            W2, b2 = lins[1].weight.detach(), lins[1].bias.detach()
        cw, cb = self._cross_packed()
        return engine.dcn_score(Au, Bi, Pu, Pi, users.contiguous(), W2, b2, self.output_layer.weight.detach(),
                                self.output_layer.bias.detach(), cw, cb, out, err_flag=self._flag())


def _as_block(ts):
    """The [L, F] view whose rows are exactly the 1-D tensors ``ts`` — when they are consecutive, contiguous slices of
    ONE storage (so the view cannot reach past it) — else None."""
    if any(t is None for t in ts):
        return None
    t0 = ts[0]
    F = t0.numel()
    base = t0.untyped_storage().data_ptr()
    for l, t in enumerate(ts):
        if (t.dim() != 1 or t.numel() != F or t.stride(0) != 1 or t.untyped_storage().data_ptr() != base
                or t.storage_offset() != t0.storage_offset() + l * F):
            return None
    return t0.as_strided((len(ts), F), (F, 1))
