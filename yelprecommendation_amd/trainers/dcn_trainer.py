"""DCN trainer — drop-in for reference trainers/dcn_trainer.py:22-181.

Same constructor ``DCNTrainer(cfg, num_items, num_users, item2attributes, attributes_count)`` and the same
``run / train / validate / evaluate`` contract: ``train`` and ``validate`` return the SUM of per-batch mean losses,
``evaluate(eval_data, mode)`` returns ``(precision, recall, map, ndcg)@top_n`` over the first 1,000 users in 'valid'
mode and all users in 'test' mode.

Differences underneath (results equal to float rounding):
* the attributes come from the device table ``cat_ids`` / ``sc_ids`` (DCNDataPipeline) instead of four per-item dict
  lookups per batch (dcn_trainer.py:106-109);
* a training step is DCN.bpr_loss_backward (gather, deep-tower GEMMs, one fused head kernel, scatter) and one Adam
  launch over all tensors (optimizer.step: yr_adam_dense_flat); the running loss stays on the device;
* ``evaluate`` scores all eval users against the whole catalogue with the fused scorer (yr_dcn_score) instead of one
  user at a time in chunks of ``batch_size`` items (dcn_trainer.py:145-165), then masks (``pred[mask] = 0``) and
  takes the top-n on the device.  Ties (the sigmoid saturates at 1.0f) are ordered by item id.
* ``cfg.deterministic=true``: the training step sums every gradient in a fixed order (DCN.deterministic: no float
  atomics), so a run repeats bit for bit under one seed — with any of the optimizers and either loader.
"""
import torch

from .. import engine
from ..models.dcn import DCN
from .base_trainer import TripletTrainer
from .eval_set import EvalSets


class DCNTrainer(TripletTrainer):
    EVAL_CHUNK = 4096                 # users per score buffer (4096 x 38,048 f32 = 623 MB)

    def __init__(self, cfg, num_items: int, num_users: int, item2attributes=None, attributes_count=None,
                 cat_ids=None, sc_ids=None) -> None:
        super().__init__(cfg)
        self.num_items = num_items
        self.num_users = num_users
        # built on the CPU under the seed (the reference's init order), then moved
        self.model = DCN(self.cfg, num_users, num_items, attributes_count).to(self.device)
        # cfg.deterministic=true: the ordered head and scatter (csrc/dcn_owned.hip); Adam, AdamW and SGD are element-wise
        self.model.deterministic = bool(self.cfg.get("deterministic", False))
        self.optimizer = self._optimizer(self.cfg.optimizer, self.model, self.cfg.lr, self.cfg.weight_decay)
        self.loss = self._loss()
        self.item2attributes = item2attributes
        if cat_ids is None:
            cat_ids, sc_ids = _tables_from_dict(item2attributes, num_items)
        self.model.set_item_attributes(cat_ids, sc_ids)
        self._eval_sets = EvalSets(self.device)

    def train(self, train_dataloader) -> float:
        # reference dcn_trainer.py:100-118
        self.model.train()
        self._loss_accum.zero_()
        for data in train_dataloader:
            user_id, pos_item, neg_item = self._batch(data)
            self.model.bpr_loss_backward(user_id, pos_item, neg_item, loss_accum=self._loss_accum)
            self.optimizer.step(zero_grad=True)
        self.model.check_indices()
        return float(self._loss_accum.item())

    def validate(self, valid_dataloader) -> float:
        # reference dcn_trainer.py:120-137: the sum of the batch-mean losses
        self.model.eval()
        self._loss_accum.zero_()
        for data in valid_dataloader:
            user_id, pos_item, neg_item = self._batch(data)
            self.model.bpr_loss_backward(user_id, pos_item, neg_item, loss_accum=self._loss_accum, backward=False)
        self.model.check_indices()
        return float(self._loss_accum.item())

    # -- evaluation ---------------------------------------------------------------------------------
    def _eval_arrays(self, eval_data, limit=None):
        return self._eval_sets.eval_set(eval_data, limit=limit)

    @torch.no_grad()
    def recommend(self, users, mask_ptr, mask_idx):
        """Top-``top_n`` item ids per user after ``pred[mask_items] = 0`` on the sigmoid outputs ([n, top_n] int64)."""
        n = users.numel()
        top = torch.empty((n, self.cfg.top_n), dtype=torch.int64, device=self.device)
        if n == 0:
            return top
        prep = self.model.score_prep()
        chunk = min(n, self.EVAL_CHUNK)
        scores = torch.empty((chunk, self.num_items), dtype=torch.float32, device=self.device)
        for a in range(0, n, chunk):
            b = min(n, a + chunk)
            self.model.score_catalogue(users[a:b], scores[:b - a], prep=prep)
            engine.topk_masked(scores[:b - a], mask_ptr[a:b + 1], mask_idx, self.cfg.top_n, mask_value=0.0,
                               out=top[a:b])
        self.model.check_indices()
        return top

    def evaluate(self, eval_data, mode='valid') -> tuple:
        # reference dcn_trainer.py:139-172
        self.model.eval()
        _, actual, users, mask_ptr, mask_idx, pos_ptr, pos_idx = self._eval_arrays(
            eval_data, 1000 if mode == 'valid' else None)
        predicted = self.recommend(users, mask_ptr, mask_idx)
        p, r, m, n = engine.rank_metrics(predicted, pos_ptr, pos_idx)[:4].tolist()
        if mode == 'test':
            self._log_test(p, r, m, n)
        return (p, r, m, n)


def _tables_from_dict(item2attributes, num_items):
    """cat_ids / sc_ids from the reference's item2attributes dict (padded, shifted lists)."""
    cats = [list(item2attributes[i]['categories']) for i in range(num_items)]
    sc = [int(item2attributes[i]['statecity']) for i in range(num_items)]
    return torch.tensor(cats, dtype=torch.int32), torch.tensor(sc, dtype=torch.int32)
