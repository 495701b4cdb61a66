"""S3Rec trainers — drop-ins for ``S3RecTrainer`` of reference trainers/s3rec_trainer.py:173-314 (fine-tuning, below)
and for ``S3RecPreTrainer`` of :21-171 (pre-training: see the class).

Same constructor ``S3RecTrainer(cfg, num_items, item2attributes, attributes_count)``; batches are dicts with the
reference's keys (``X``, ``pos_items``, ``neg_items``; ``pos_item`` for the test loader).

* ``train`` is s3rec_trainer.py:233-247: ``model.train()``, then per batch ``finetune``, ``zero_grad``, the BPR loss,
  ``backward`` and ``step`` of the optimizer ``BaseTrainer._optimizer`` built (:177).  Returns the SUM of the batch
  losses; the sum stays on the device until the end.
* ``run`` is :196-231: ``best_model.pt`` on every improvement of the validation loss, early stopping on
  ``patience``.
* ``validate`` returns the SUM over batches of ``BPRLoss(finetune(...))`` (s3rec_trainer.py:249-262); the sum stays
  on the device until the end.
* ``evaluate`` returns (precision, recall, MAP, NDCG)@top_n over ``[pos | sampled negatives]`` the way the reference
  computes them (s3rec_trainer.py:265-314): ``predicted`` is its odd array — the positive's id where the positive
  lands in the top-n, 0 elsewhere — fed to the same metric functions.  The positive's rank is the number of negatives
  scoring strictly higher (the reference's ``argsort`` leaves ties to the sort; its recorded runs have none).
* ``evaluate_full`` (new) ranks the held-out item against the WHOLE catalogue, the user's earlier items left out: the
  four metrics by the protocol and the code of ``MFTrainer.evaluate`` (comparable across the five models), and
  HR@k / NDCG@k / MRR from the exact ranks in ``last_full_eval``.  ``evaluate`` is unchanged.
"""
import os

import numpy as np
import torch

from .. import engine
from ..loss import BPRLoss
from ..metric import ranking_metrics
from ..models.s3rec import S3Rec
from ..utils import logger
from .base_trainer import BaseTrainer


def attribute_csr(item2attributes, num_items, attributes_count):
    """(ptr [num_items + 2], idx) int64 on the host: the categories of item id k (``item2attributes[k]['categories']``,
    the reference's dict: key 0 is the pad and has none, a missing key has none), ascending and duplicate-free inside
    an item.  An attribute id outside [0, attributes_count) raises ValueError."""
    lists = []
    for k in range(num_items + 1):
        entry = item2attributes.get(k) if item2attributes is not None else None
        cats = sorted(set(int(a) for a in (entry['categories'] if entry is not None else ())))
        if k == 0:
            cats = []                                      # aap_actual of the pad is all zero (decision 2)
        if cats and not 0 <= cats[0] <= cats[-1] < attributes_count:
            raise ValueError(f"S3RecPreTrainer: item {k} has an attribute id outside [0, {attributes_count}): {cats}")
        lists.append(cats)
    ptr = np.zeros(num_items + 2, dtype=np.int64)
    np.cumsum([len(c) for c in lists], out=ptr[1:])
    return ptr, np.fromiter((a for c in lists for a in c), dtype=np.int64, count=int(ptr[-1]))


class S3RecPreTrainer(BaseTrainer):
    """Drop-in for ``S3RecPreTrainer`` of reference trainers/s3rec_trainer.py:21-171.

    ``train(loader)`` is :118-167 per batch — ``item_level_masking``, ``segment_masking``, the four losses, their sum,
    ``backward``, ``step`` — and returns the SUM of the batch losses.  It reads only ``data['X']``: the reference's
    dense ``aap_actual`` / ``mip_actual`` ([B, L, num_items + 1] float64 built in Python loops) are replaced by X itself
    and an item -> categories CSR built once on the device, and the losses go through ``S3Rec.pretrain_loss`` (the
    catalogue-BCE kernel).  Works on the batches of ``DataLoader(S3RecDataset)`` and of ``S3RecBatchLoader``.

    ``segment_masking`` (:96-115): per row a segment length uniform in [2, L // 2 - 1] (``max_seq_len >= 6``) and a start
    uniform in [0, L - len - 1]; the segment is right-aligned into the positive sequence.  The reference's loop
    ``while neg_user_idx != i`` can only end at ``i``, so its negative segment comes from the SAME row at another,
    independently drawn start: that is the default, ``sp_negative="same_row"``.  ``sp_negative="other_row"`` draws a
    different row of the batch (B >= 2), the documented intent.  Both masking functions run vectorised on the device
    from a generator the trainer owns, seeded from ``cfg.seed``; nothing replays the reference's host RNG stream.

    ``pretrain(loader)`` is :59-89: ``best_pretrain_model.pt`` on every improvement of the TRAINING loss when
    ``best_metric == 'loss'``, early stopping on ``patience``.  On a non-cuda device ``train`` / ``pretrain`` raise
    NotImplementedError."""

    def __init__(self, cfg, num_items: int, item2attributes, attributes_count: int, sp_negative: str = "same_row") -> None:
        super().__init__(cfg)
        if sp_negative not in ("same_row", "other_row"):
            raise ValueError(f"S3RecPreTrainer: sp_negative {sp_negative!r} (same_row or other_row)")
        self.num_items, self.attributes_count = num_items, attributes_count
        self.item2attribute = item2attributes
        self.sp_negative = sp_negative
        ptr, idx = attribute_csr(item2attributes, num_items, attributes_count)       # validated on the host
        self.model = S3Rec(self.cfg, num_items, attributes_count).to(self.device)
        self.optimizer = self._optimizer(self.cfg.optimizer, self.model, self.cfg.lr)
        self.attr_ptr, self.attr_idx = torch.from_numpy(ptr).to(self.device), torch.from_numpy(idx).to(self.device)
        self._gen = None

    def _generator(self):
        if self._gen is None:
            self._gen = torch.Generator(device=self.device).manual_seed(int(self.cfg.get("seed", 0)))
        return self._gen

    def _is_surpass_best_metric(self, **metric) -> bool:
        return self.cfg.best_metric == 'loss' and metric['current'][0] < metric['best'][0]

    def _trainable(self, what):
        if self.device.type != "cuda":
            raise NotImplementedError(f"S3RecPreTrainer.{what}: pre-training is not built for the {self.device.type} "
                                      "device (the kernels run on the GPU only)")

    def item_level_masking(self, sequences):
        # reference s3rec_trainer.py:91-94: keeps the items where the mask is set
        masks = torch.rand(sequences.shape, device=sequences.device, generator=self._generator()) < self.cfg.mask_portion
        return masks, masks * sequences

    def segment_masking(self, sequences):
        # reference s3rec_trainer.py:96-115, every row at once
        B, L = sequences.shape
        if L < 6:
            raise ValueError(f"S3RecPreTrainer.segment_masking: max_seq_len {L} leaves no segment length in "
                             "[2, L // 2 - 1] (6 is the least)")
        dev, gen = sequences.device, self._generator()

        def randint(high):                                  # uniform in [0, high[b]) per row
            u = torch.rand(B, device=dev, generator=gen, dtype=torch.float64)
            return torch.minimum((u * high).long(), high - 1)

        seg_len = 2 + randint(torch.full((B,), L // 2 - 2, device=dev))
        start = randint(L - seg_len)
        neg_start = randint(L - seg_len)
        rows = torch.arange(B, device=dev)
        if self.sp_negative == "other_row":
            if B < 2:
                raise ValueError("S3RecPreTrainer: sp_negative='other_row' needs a batch of at least two rows")
            neg_rows = (rows + 1 + randint(torch.full((B,), B - 1, device=dev))) % B
        else:
            neg_rows = rows
        at = torch.arange(L, device=dev)[None, :]
        inside = (at >= start[:, None]) & (at < (start + seg_len)[:, None])
        tail = at >= (L - seg_len)[:, None]                 # the right-aligned places
        src = (at - (L - seg_len)[:, None]).clamp(min=0)    # offset inside the segment
        pos = torch.where(tail, torch.gather(sequences, 1, (start[:, None] + src).clamp(max=L - 1)), 0)
        neg = torch.where(tail, torch.gather(sequences[neg_rows], 1, (neg_start[:, None] + src).clamp(max=L - 1)), 0)
        return torch.where(inside, 0, sequences), pos, neg

    def train(self, train_dataloader) -> float:
        self._trainable("train")
        self.model.train()
        self._loss_accum.zero_()
        for data in train_dataloader:
            sequences = data['X'].to(self.device)
            masks, item_masked = self.item_level_masking(sequences)
            _segment_masked, pos_segments, neg_segments = self.segment_masking(sequences)
            losses = self.model.pretrain_loss(sequences, masks, item_masked, pos_segments, neg_segments, self.attr_ptr,
                                              self.attr_idx)
            self.optimizer.zero_grad()
            loss = losses[0] + losses[1] + losses[2] + losses[3]
            loss.backward()
            self.optimizer.step()
            self._accumulate(loss)
        self.model.check_indices()
        return float(self._loss_accum.item())

    def pretrain(self, train_dataset):
        self._trainable("pretrain")
        logger.info("[Pre-Trainer] run...")
        best_train_loss = 1e+6
        endurance = 0
        for epoch in range(self.cfg.pretrain_epochs):
            train_loss = self.train(train_dataset)
            logger.info(f"[Pre-Trainer] epoch: {epoch} > pretrain loss: {train_loss:.4f}")
            if self._is_surpass_best_metric(current=(train_loss,), best=(best_train_loss,)):
                logger.info("[Trainer] update best model...")
                best_train_loss = train_loss
                endurance = 0
                torch.save(self.model.state_dict(), f'{self.cfg.model_dir}/best_pretrain_model.pt')
            else:
                endurance += 1
                if endurance > self.cfg.patience:
                    logger.info("[Trainer] ealry stopping...")
                    break

    def load_best_model(self):
        logger.info("[Trainer] Load best model...")
        self.model.load_state_dict(torch.load(f'{self.cfg.model_dir}/best_pretrain_model.pt', map_location=self.device,
                                              weights_only=True))

    def validate(self, valid_dataloader):
        raise NotImplementedError("S3RecPreTrainer has no validation: the reference's pre-training watches its training loss")

    def evaluate(self, test_dataloader):
        raise NotImplementedError("S3RecPreTrainer has no evaluation: fine-tune with S3RecTrainer")


class S3RecTrainer(BaseTrainer):

    def __init__(self, cfg, num_items: int, item2attributes=None, attributes_count: int = 1) -> None:
        super().__init__(cfg)
        self.num_items = num_items
        self.item2attributes = item2attributes
        # built on the CPU under the seed (the reference's init order), then moved
        self.model = S3Rec(self.cfg, num_items, attributes_count).to(self.device)
        if self.cfg.get("optimizer") is not None:          # reference s3rec_trainer.py:177 (scoring-only configs have none)
            self.optimizer = self._optimizer(self.cfg.optimizer, self.model, self.cfg.lr)
        self.loss = self._loss()
        self._load_best_pretrain_model()

    def _loss(self):
        return BPRLoss()

    def _is_surpass_best_metric(self, **metric) -> bool:
        # reference s3rec_trainer.py:184-194: one-element tuples, the loss only
        return self.cfg.best_metric == 'loss' and metric['current'][0] < metric['best'][0]

    def _trainable(self, what):
        if self.device.type != "cuda":
            raise NotImplementedError(f"S3RecTrainer.{what}: training is not built for the {self.device.type} device "
                                      "(the kernels run on the GPU only)")
        if not hasattr(self, "optimizer"):
            raise ValueError(f"S3RecTrainer.{what}: the config names no optimizer")

    def run(self, train_dataloader, valid_dataloader):
        # reference s3rec_trainer.py:196-231.  Not BaseTrainer.run: validate() returns the loss alone here, where the
        # shared loop unpacks (valid_loss, precision, recall, map, ndcg).
        self._trainable("run")
        logger.info("[Trainer] run...")
        best_valid_loss = 1e+6
        endurance = 0
        for epoch in range(self.cfg.epochs):
            train_loss = self.train(train_dataloader)
            valid_loss = self.validate(valid_dataloader)
            logger.info(f"[Trainer] epoch: {epoch} > train loss: {train_loss:.4f} / valid loss: {valid_loss:.4f}")
            if self._is_surpass_best_metric(current=(valid_loss,), best=(best_valid_loss,)):
                logger.info("[Trainer] update best model...")
                best_valid_loss = valid_loss
                endurance = 0
                self._save_best()
            else:
                endurance += 1
                if endurance > self.cfg.patience:
                    logger.info("[Trainer] ealry stopping...")
                    break

    def train(self, train_dataloader) -> float:
        # reference s3rec_trainer.py:233-247
        self._trainable("train")
        self.model.train()
        self._loss_accum.zero_()
        dev = self.device
        for data in train_dataloader:
            X, pos_items, neg_items = data['X'].to(dev), data['pos_items'].to(dev), data['neg_items'].to(dev)
            pos_preds, neg_preds = self.model.finetune(X, pos_items, neg_items)
            self.optimizer.zero_grad()
            loss = self.loss(pos_preds, neg_preds)
            loss.backward()
            self.optimizer.step()
            self._accumulate(loss)
        self.model.check_indices()
        return float(self._loss_accum.item())

    @torch.no_grad()
    def validate(self, valid_dataloader) -> float:
        self.model.eval()
        self._loss_accum.zero_()
        dev = self.device
        for data in valid_dataloader:
            X, pos_items, neg_items = data['X'].to(dev), data['pos_items'].to(dev), data['neg_items'].to(dev)
            pos_preds, neg_preds = self.model.finetune(X, pos_items, neg_items)
            self._accumulate(self.loss(pos_preds, neg_preds))
        self.model.check_indices()
        return float(self._loss_accum.item())

    @torch.no_grad()
    def evaluate(self, test_dataloader) -> tuple:
        self.model.eval()
        dev = self.device
        k = self.cfg.top_n
        pos_ids, ranks = [], []
        for data in test_dataloader:
            X, pos_item, neg_items = data['X'].to(dev), data['pos_item'].to(dev), data['neg_items'].to(dev)
            pos_scores, neg_scores = self.model.evaluate(X, pos_item, neg_items)
            ranks.append((neg_scores > pos_scores).sum(dim=1))
            pos_ids.append(pos_item.reshape(-1))
        self.model.check_indices()
        pos_ids = torch.cat(pos_ids).cpu().numpy()
        ranks = torch.cat(ranks).cpu().numpy()
        # the reference's predicted array: float rows of zeros with the positive's id at its rank when inside the top-n
        predicted = np.zeros((len(pos_ids), k), dtype=np.float32)
        hit = ranks < k
        predicted[np.nonzero(hit)[0], ranks[hit]] = pos_ids[hit]
        actual = pos_ids.reshape(-1, 1).tolist()
        p, r, m, n = ranking_metrics(actual, predicted, k)
        self._log_test(p, r, m, n)
        return (p, r, m, n)

    @torch.no_grad()
    def evaluate_full(self, dataloader, history=None) -> tuple:
        """(precision, recall, MAP, NDCG)@top_n of the held-out item against the WHOLE catalogue — the protocol and
        the code of ``MFTrainer.evaluate`` (fused lists, then ``engine.rank_metrics``: reference metric.py with its
        quirks), so the figures stand next to the other models'.  The target is ``pos_item`` (test batches) or
        ``pos_items[:, -1]`` (valid batches), the exclude rows are ``user_id``'s of ``history`` = (ptr, idx)
        (``S3RecSequences.history(mode)``; None masks nothing but the pad).  Sets ``last_full_eval``: the exact ranks
        ρ of all rows (device, -1 without a target), ``n_users`` (rows with a target), ``n_skipped``, and from the ranks
        in float64, as means over the rows with a target, ``HR@k`` = [ρ < k], ``NDCG@k`` = [ρ < k] / log2(ρ + 2) for
        k in {1, 5, 10, top_n} and ``MRR`` = 1 / (ρ + 1)."""
        self.model.eval()
        dev = self.device
        k = int(self.cfg.top_n)
        ranks, lists, targets = [], [], []
        for data in dataloader:
            X = data['X'].to(dev)
            target = (data['pos_item'] if 'pos_item' in data else data['pos_items'][:, -1]).to(dev).reshape(-1).long()
            users = torch.as_tensor(data['user_id']).to(dev).reshape(-1).long()
            rank, topk = self.model.rank_and_recommend(X, target, k, history=history, users=users)
            ranks.append(rank)
            lists.append(topk)
            targets.append(target)
        if not ranks:
            raise ValueError("S3RecTrainer.evaluate_full: the loader gave no batch")
        ranks, lists, targets = torch.cat(ranks), torch.cat(lists), torch.cat(targets)
        has = ranks >= 0
        pos_ptr = torch.zeros(ranks.numel() + 1, dtype=torch.int64, device=dev)
        pos_ptr[1:] = torch.cumsum(has, 0)
        four = engine.rank_metrics(lists.contiguous(), pos_ptr, targets[has].contiguous())[:4]
        rho = ranks[has].to(torch.float64)
        ks = sorted({1, 5, 10, k})
        stats = [((rho < kk).to(torch.float64)).mean() for kk in ks]
        stats += [((rho < kk).to(torch.float64) / torch.log2(rho + 2.0)).mean() for kk in ks]
        stats += [(1.0 / (rho + 1.0)).mean(), has.sum().to(torch.float64)]
        self.model.check_indices()
        host = torch.cat([four, torch.stack(stats)]).tolist()       # the one read-back of the metrics
        p, r, m, n = host[:4]
        n_users = int(host[-1])
        out = {"ranks": ranks, "n_users": n_users, "n_skipped": int(ranks.numel()) - n_users, "MRR": host[-2]}
        for i, kk in enumerate(ks):
            out[f"HR@{kk}"] = host[4 + i]
            out[f"NDCG@{kk}"] = host[4 + len(ks) + i]
        self.last_full_eval = out
        self._log_test(p, r, m, n)
        logger.info("[Trainer] full catalogue > " + " / ".join(
            f"{name}: {out[name]:.4f}" for name in [f"HR@{kk}" for kk in ks] + [f"NDCG@{kk}" for kk in ks] + ["MRR"])
            + f" / users: {n_users} (skipped {out['n_skipped']})")
        return (p, r, m, n)

    def _load_best_pretrain_model(self):
        # reference s3rec_trainer.py:296-300
        path = f'{self.cfg.model_dir}/best_pretrain_model.pt'
        if self.cfg.get("load_pretrain", False) and os.path.exists(path):
            logger.info("[Trainer] Load best pretrain model...")
            self.model.load_state_dict(torch.load(path, map_location=self.device, weights_only=True))
