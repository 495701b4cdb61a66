"""S3Rec trainer — drop-in for ``S3RecTrainer`` of reference trainers/s3rec_trainer.py:173-314 (fine-tuning; the
pre-training trainer of :18-171 is not built).

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
"""
import os

import numpy as np
import torch

from ..loss import BPRLoss
from ..metric import ranking_metrics
from ..models.s3rec import S3Rec
from ..utils import logger
from .base_trainer import BaseTrainer


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

    def _load_best_pretrain_model(self):
        # reference s3rec_trainer.py:296-300
        path = f'{self.cfg.model_dir}/best_pretrain_model.pt'
        if self.cfg.get("load_pretrain", False) and os.path.exists(path):
            logger.info("[Trainer] Load best pretrain model...")
            self.model.load_state_dict(torch.load(path, map_location=self.device, weights_only=True))
