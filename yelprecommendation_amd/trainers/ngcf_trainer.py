"""NGCF trainer — drop-in for reference trainers/ngcf_trainer.py:22-182.

Same constructor ``NGCFTrainer(cfg, num_items, num_users, laplacian_matrix)`` and the same
``run / train / validate / evaluate`` contract.  ``evaluate`` scores
``np.random.randint(len(eval_data), size=100)`` eval rows — WITH replacement, drawn from the global
NumPy RNG exactly like the reference (ngcf_trainer.py:140) — but propagates the graph once per
call instead of once per sampled user.  With Adam / AdamW ``train`` runs every batch as ONE engine call
(ngcf_step.NGCFStep: the launches of the autograd route, issued from C; cfg.fused_step=False keeps the reference's
loop shape — bpr_forward, zero_grad, loss, backward, step — on the HIP autograd ops).  ``cfg.deterministic=true``: the
fused step without float atomics (NGCFStep(deterministic=True)): runs repeat bit for bit under one seed; where the
fused step is not available (SGD, fused_step=false) ``train`` raises NotImplementedError instead of running unordered.

Full-catalogue evaluation (new; the reference has only the 100-row sample): ``evaluate_full`` ranks the whole
catalogue for EVERY row of the eval frame — one propagation, then the fused sweep over the layer tables
(engine.ngcf_eval_topk: no score matrix, the layers not concatenated) and the metrics on the device, as MF, CDAE and
DCN evaluate.  ``cfg.full_eval=true`` makes ``evaluate`` delegate to it in both modes, so ``run`` selects its best
model on all users and draws nothing from NumPy's global RNG; false or absent, ``evaluate`` is the reference's sample,
including its one ``np.random.randint(len(eval_data), size=100)`` draw.
"""
import numpy as np
import torch

from .. import engine
from ..metric import ranking_metrics
from ..models.ngcf import NGCF, _iadd
from ..utils import logger
from .base_trainer import TripletTrainer
from .eval_set import EvalSets, _lists_to_csr, top_k_of_scores


class NGCFTrainer(TripletTrainer):
    def __init__(self, cfg, num_items: int, num_users: int, laplacian_matrix) -> None:
        super().__init__(cfg)
        if cfg.get("deterministic", False):
            from ..ngcf_step import DETERMINISTIC_NEEDS, deterministic_available
            if not deterministic_available(cfg):               # refused before a model is built, never run unordered
                raise NotImplementedError(DETERMINISTIC_NEEDS)
        logger.info(f'[DEVICE] device = {self.device}')
        self.num_items = num_items
        self.num_users = num_users
        self.model = NGCF(self.cfg, num_users, num_items).to(self.device)
        self.optimizer = self._optimizer(self.cfg.optimizer, self.model, self.cfg.lr, self.cfg.weight_decay)
        self.loss = self._loss()
        self.laplacian_matrix = laplacian_matrix
        self._eval_sets = EvalSets(self.device)

    def _fused_step(self):
        """The whole batch step as one engine call (ngcf_step.NGCFStep) for Adam / AdamW unless
        cfg.fused_step is False; None -> the launch-by-launch autograd route below (SGD, or on request)."""
        from .. import optim
        from ..ngcf_step import DETERMINISTIC_NEEDS, NGCFStep
        deterministic = bool(self.cfg.get("deterministic", False))
        if not isinstance(self.optimizer, optim.Adam) or not self.cfg.get("fused_step", True):
            if deterministic:
                raise NotImplementedError(DETERMINISTIC_NEEDS)     # the autograd route adds in arrival order
            return None
        graph = self.model.graph(self.laplacian_matrix)
        st = getattr(self, "_step", None)
        if st is None or st.deterministic != deterministic or not st.bound_to(self.model, self.optimizer, graph):
            st = self._step = NGCFStep(self.model, self.optimizer, graph, self.model._subset_fraction(),
                                       deterministic=deterministic)
        return st

    def train(self, train_dataloader) -> float:
        # reference ngcf_trainer.py:102-117
        self.model.train()
        step = self._fused_step()
        if step is not None:
            step.loss_accum.zero_()
            for data in train_dataloader:
                step.step(*self._batch(data))
            step.check()
            return step.epoch_loss()
        self._loss_accum.zero_()
        for data in train_dataloader:
            user_id, pos_item, neg_item = self._batch(data)
            pos_pred, neg_pred = self.model.bpr_forward(user_id, pos_item, neg_item, self.laplacian_matrix)
            self.optimizer.zero_grad()
            loss = self.loss(pos_pred, neg_pred)
            loss.backward()
            self.optimizer.step()
            self._accumulate(loss)
        self.model.check_indices()
        return float(self._loss_accum.item())

    def validate(self, valid_dataloader) -> float:
        # reference ngcf_trainer.py:119-132 (the reference keeps autograd on here; the values are the same)
        self.model.eval()
        self._loss_accum.zero_()
        with torch.no_grad():
            # the parameters do not change during validation, so the K propagation layers are the same for every
            # batch: computed once (the reference re-propagates the whole graph per batch, ngcf_trainer.py:124), then
            # every batch is one scoring launch on them — the same kernels on the same data, bit-identical values
            once = self.cfg.get("propagate_once", True)
            layers = self.model.propagate(self.laplacian_matrix) if once else None
            for data in valid_dataloader:
                user_id, pos_item, neg_item = self._batch(data)
                if once:
                    pos_pred, neg_pred = engine.ngcf_score(layers, self.num_users, user_id.contiguous(),
                                                           pos_item.contiguous(), neg_item.contiguous(),
                                                           err_flag=self.model._flag())
                else:
                    pos_pred, neg_pred = self.model.bpr_forward(user_id, pos_item, neg_item, self.laplacian_matrix)
                self._accumulate(self.loss(pos_pred, neg_pred))
        self.model.check_indices()
        return float(self._loss_accum.item())

    def recommend(self, users, mask_ptr, mask_idx, fused=False, hint_key=None):
        """Top-``top_n`` unmasked items for the given user ids ([n, top_n] int64 on the device):
        one propagation, then S = sum_k E_k[users] E_k[items]^T on the matrix cores, mask, top-k.
        ``fused``: the sweep over the layer tables instead (engine.ngcf_eval_topk: scores, mask and top-k in one
        kernel, no [n, num_items] matrix; top_n <= 16; the mask lists must be sorted ascending inside each row).
        ``hint_key``: fused evaluations under the same key hand their result to the next one as hint lists
        (BaseTrainer._with_hints; cfg.eval_hints=False turns it off)."""
        layers = self.model.propagate(self.laplacian_matrix)
        nu = self.num_users
        if fused:
            users = users.contiguous()
            return self._with_hints(hint_key, users.numel(), lambda hint: engine.ngcf_eval_topk(
                layers, nu, users, mask_ptr, mask_idx, self.cfg.top_n, hint=hint))
        scores = None
        for E in layers:
            s = engine.mf_scores_gemm(E[:nu], E[nu:], users)
            scores = s if scores is None else _iadd(scores, s)
        return engine.topk_masked(scores, mask_ptr, mask_idx, self.cfg.top_n)

    # rows per chunk of the dense route of evaluate_full: two score buffers of this many rows, 4,096 x num_items
    # floats in all (0.62 GB at Yelp2018 size)
    full_eval_chunk_users = 2048

    def _recommend_chunked(self, users, mask_ptr, mask_idx):
        """:meth:`recommend`'s dense route for any number of users: one propagation, then chunk after chunk of
        ``full_eval_chunk_users`` rows through the same two score buffers — never an [all users, items] array."""
        layers = self.model.propagate(self.laplacian_matrix)
        nu, n = self.num_users, users.numel()
        rows = max(1, min(int(self.full_eval_chunk_users), n))
        bufs = [torch.empty((rows, self.num_items), dtype=torch.float32, device=self.device) for _ in range(2)]
        out = torch.empty((n, self.cfg.top_n), dtype=torch.int64, device=self.device)
        mask_rows = torch.arange(n, dtype=torch.int64, device=self.device)
        flag = self.model._flag()
        for lo in range(0, n, rows):
            hi = min(lo + rows, n)
            chunk = users[lo:hi].contiguous()
            scores = engine.mf_scores_gemm(layers[0][:nu], layers[0][nu:], chunk, out=bufs[0], err_flag=flag)
            for E in layers[1:]:
                _iadd(scores, engine.mf_scores_gemm(E[:nu], E[nu:], chunk, out=bufs[1], err_flag=flag))
            engine.topk_masked(scores, mask_ptr, mask_idx, self.cfg.top_n, out=out[lo:hi], mask_rows=mask_rows[lo:hi])
        self.model.check_indices()
        return out

    def evaluate_full(self, eval_data, mode='valid') -> tuple:
        """(precision, recall, map, ndcg)@top_n over ALL rows of ``eval_data`` (a frame indexed by user id with list
        columns 'pos_items' and 'mask_items'), the whole catalogue ranked for each: the fused sweep over the layer
        tables up to top_n = 16, beyond it the dense route in chunks of users (:meth:`_recommend_chunked`).  The
        lists stay in ``last_full_topk`` ([rows, top_n] int64 on the device, in the frame's row order)."""
        self.model.eval()
        users, mask_ptr, mask_idx, pos_ptr, pos_idx = self._eval_sets.eval_set(eval_data, sort_masks=True)[2:7]
        if engine.ngcf_eval_supports(self.cfg.top_n):
            predicted = self.recommend(users, mask_ptr, mask_idx, fused=True, hint_key=id(eval_data))
        else:
            predicted = self._recommend_chunked(users, mask_ptr, mask_idx)
        self.last_full_topk = predicted
        p, r, m, n = engine.rank_metrics(predicted, pos_ptr, pos_idx)[:4].tolist()
        if mode == 'test':
            self._log_test(p, r, m, n)
        return (p, r, m, n)

    def evaluate_ranks(self, eval_data, ks=None, mode='valid'):
        """``{k: (precision, recall, map, ndcg, hr)}`` for every k of ``ks`` (default ``(cfg.top_n,)``; any k >= 1)
        plus ``mrr`` and ``auc`` over ALL rows of ``eval_data``: one propagation, then the rank of every held-out item
        against the whole masked catalogue in one sweep over the layer tables (engine.catalogue_ranks, the layered
        score of engine.ngcf_eval_topk), no top-k list and no score matrix.  Up to top_n = 16 the four metrics equal
        :meth:`evaluate_full`'s."""
        self.model.eval()
        with torch.no_grad():
            layers = self.model.propagate(self.laplacian_matrix)
        nu = self.num_users
        return self._evaluate_ranks([E[:nu] for E in layers], [E[nu:] for E in layers],
                                    self._eval_sets.eval_set(eval_data, sort_masks=True), ks, mode)

    def evaluate(self, eval_data, mode='valid') -> tuple:
        # reference ngcf_trainer.py:134-165
        if self.cfg.get("full_eval", False):
            if self.cfg.get("rank_eval", False):           # the same four figures at any top_n, by the rank sweep
                p, r, m, n = self.evaluate_ranks(eval_data, (self.cfg.top_n,))[int(self.cfg.top_n)][:4]
                if mode == 'test':
                    self._log_test(p, r, m, n)
                return (p, r, m, n)
            return self.evaluate_full(eval_data, mode)
        self.model.eval()
        positions = np.random.randint(eval_data.shape[0], size=100)            # :140, global NumPy RNG
        users = np.asarray(eval_data.index.values, dtype=np.int64)[positions]
        rows = eval_data.iloc[positions]
        actual = [list(x) for x in rows['pos_items']]
        mask_ptr, mask_idx = _lists_to_csr([list(x) for x in rows['mask_items']])
        dev = self.device
        predicted = self.recommend(torch.from_numpy(users).to(dev), torch.from_numpy(mask_ptr).to(dev),
                                   torch.from_numpy(mask_idx).to(dev)).cpu().numpy()
        p, r, m, n = ranking_metrics(actual, predicted.tolist(), self.cfg.top_n)
        if mode == 'test':
            self._log_test(p, r, m, n)
        return (p, r, m, n)

    def _generate_top_k_recommendation(self, pred, mask_items):
        return top_k_of_scores(pred, mask_items, self.cfg.top_n)
