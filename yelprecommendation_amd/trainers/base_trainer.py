"""Trainer base — drop-in for reference trainers/base_trainer.py:14-157.

Same constructor, same helper names and semantics (`_device`, `_model`,
`_optimizer`, `_loss`, `run`, `_is_surpass_best_metric`, `load_best_model`); the
optimizers it hands out are the dense HIP-backed ones of :mod:`..optim`.
"""
import os
from abc import ABC, abstractmethod

import torch
from torch.nn import Module

from .. import engine, optim
from ..loss import BPRLoss
from ..utils import logger


# position of every selectable metric in the (valid_loss, precision, recall, map, ndcg) tuples and
# whether smaller is better (reference base_trainer.py:117-141)
_BEST_METRIC = {"loss": (0, True), "precision": (1, False), "recall": (2, False), "map": (3, False), "ndcg": (4, False)}
_OPTIMIZERS = {"adam": optim.Adam, "adamw": optim.AdamW, "sgd": optim.SGD}


class BaseTrainer(ABC):

    def __init__(self, cfg) -> None:
        self.cfg = cfg
        self.device: torch.device = self._device(cfg.device)
        os.makedirs(cfg.model_dir, exist_ok=True)
        self._loss_accum = torch.zeros(1, dtype=torch.float64, device=self.device)
        self._eval_hints = {}                              # eval set -> its last top-n lists (hints of the next evaluation)

    def _device(self, device_name: str) -> torch.device:
        """'cuda' is the ROCm device on MI355X.  'cpu' stays a legal name (the reference's default,
        base_trainer.py:20-25) but the HIP ops refuse CPU tensors, so such a run fails loudly at the
        first model call instead of silently falling back; any other name logs and yields cpu."""
        name = device_name.lower()
        if name not in ("cpu", "cuda"):
            logger.error(f"Not supported device: {device_name}")
            name = "cpu"
        return torch.device(name)

    def _model(self, model_name: str) -> Module:
        # reference base_trainer.py:27-32: only the placeholder name 'test' is known at this level
        if model_name.lower() != "test":
            logger.error(f"Not implemented model: {model_name}")
            raise NotImplementedError(f"Not implemented model: {model_name}")
        return type("TestModel", (Module,), {"forward": (lambda self, x: x)})()

    def _optimizer(self, optimizer_name: str, model: Module, learning_rate: float, weight_decay: float = 0):
        """adam / adamw / sgd over all parameters with torch's default betas / eps (reference
        base_trainer.py:34-43), as the dense HIP-backed optimizers of :mod:`..optim`."""
        make = _OPTIMIZERS.get(optimizer_name.lower())
        if make is None:
            logger.error(f"Optimizer Not Exists: {optimizer_name}")
            raise NotImplementedError(f"Optimizer Not Exists: {optimizer_name}")
        return make(model.parameters(), lr=learning_rate, weight_decay=weight_decay)

    def _loss(self, loss_name: str):
        # reference base_trainer.py:45-50
        if loss_name.lower() != "bce":
            logger.error(f"Loss Not Exists: {loss_name}")
            raise NotImplementedError(f"Loss Not Exists: {loss_name}")
        return torch.nn.BCELoss()

    def run(self, train_dataloader, valid_dataloader):
        # reference base_trainer.py:52-115 (validate() returns loss + the four metrics)
        logger.info("[Trainer] run...")
        best = (1e+6, .0, .0, .0, .0)
        endurance = 0
        for epoch in range(self.cfg.epochs):
            train_loss = self.train(train_dataloader)
            current = self.validate(valid_dataloader)
            self._log_epoch(epoch, train_loss, *current)
            if self._is_surpass_best_metric(current=current, best=best):
                logger.info("[Trainer] update best model...")
                best = tuple(current)
                endurance = 0
                self._save_best()
            else:
                endurance += 1
                if endurance > self.cfg.patience:
                    logger.info("[Trainer] ealry stopping...")
                    break

    def _save_best(self):
        torch.save(self.model.state_dict(), f'{self.cfg.model_dir}/best_model.pt')

    def _log_epoch(self, epoch, train_loss, valid_loss, p, r, m, n):
        logger.info(f"[Trainer] epoch: {epoch} > train loss: {train_loss:.4f} / valid loss: {valid_loss:.4f} / "
                    f"precision@K : {p:.4f} / Recall@K: {r:.4f} / MAP@K: {m:.4f} / NDCG@K: {n:.4f}")

    def _log_test(self, p, r, m, n):
        logger.info(f"[Trainer] Test > precision@{self.cfg.top_n} : {p:.4f} / Recall@{self.cfg.top_n}: {r:.4f} / "
                    f"MAP@{self.cfg.top_n}: {m:.4f} / NDCG@{self.cfg.top_n}: {n:.4f}")

    def _evaluate_ranks(self, layers_user, layers_item, eval_set, ks, mode):
        """The rank route of MF and NGCF (``evaluate_ranks``): engine.catalogue_ranks over an EvalSets tuple whose
        masks are sorted, then engine.metrics_from_ranks at every k of ``ks`` (default ``(cfg.top_n,)``)."""
        ks = tuple(int(k) for k in (ks if ks is not None else (self.cfg.top_n,)))
        users, mask_ptr, mask_idx, pos_ptr, pos_idx = eval_set[2:7]
        rank = engine.catalogue_ranks(layers_user, layers_item, users.contiguous(), pos_ptr, pos_idx, mask_ptr,
                                      mask_idx)
        res = engine.metrics_from_ranks(rank, pos_ptr, ks, num_items=layers_item[0].shape[0], mask_ptr=mask_ptr)
        if mode == 'test':
            for k in ks:
                p, r, m, n, h = res[k]
                logger.info(f"[Trainer] Test > precision@{k} : {p:.4f} / Recall@{k}: {r:.4f} / MAP@{k}: {m:.4f} / "
                            f"NDCG@{k}: {n:.4f} / HR@{k}: {h:.4f}")
            logger.info(f"[Trainer] Test > MRR : {res.mrr:.4f} / AUC : {res.auc:.4f}")
        return res

    def _accumulate(self, loss):
        # train_loss += loss.item() of the reference's loops without the per-step host sync
        p = getattr(self, "_partials", None)
        if p is None:
            p = self._partials = torch.zeros(engine.LOSS_PARTIALS, dtype=torch.float32, device=self.device)
        p[:1].copy_(loss.detach().reshape(1))
        engine.loss_finalize(p, 1.0, None, self._loss_accum)

    @staticmethod
    def metrics_from_sums(sums):
        """(precision, recall, map, ndcg) from [non-empty users, 4 sums, users] (engine.rank_metrics()[4:10])."""
        cnt, ps, rs, ms, ns, total = sums.tolist()                 # the one read-back
        return (ps / total, rs / cnt, ms / cnt, ns / cnt)

    def _with_hints(self, key, nrows, topk):
        """``topk(hint)`` — a fused evaluation of ``nrows`` rows — with the hint lists kept under ``key``:
        evaluations under the same key hand their result to the next one (the lists start from the smallest score
        among a user's previous top-n under the CURRENT model — a bound the result cannot depend on); ``key`` None or
        cfg.eval_hints=False turns that off."""
        hinted = key is not None and self.cfg.get("eval_hints", True)
        hint = self._eval_hints.get(key) if hinted else None
        if hint is not None and tuple(hint.shape) != (nrows, self.cfg.top_n):
            hint = None
        top = topk(hint)
        if hinted:
            self._eval_hints[key] = top
        return top

    def _hinted_topk(self, key, U, I, users, mask_ptr, mask_idx, **kw):
        """engine.mf_eval_topk under cfg.eval_precision ("bf16x3", the default: f32 scores from three-term bf16
        splits, or "f32"), with hint lists per ``key`` (:meth:`_with_hints`)."""
        return self._with_hints(key, users.numel(), lambda hint: engine.mf_eval_topk(
            U, I, users, mask_ptr, mask_idx, self.cfg.top_n, precision=self.cfg.get("eval_precision", "bf16x3"),
            hint=hint, **kw))

    def _is_surpass_best_metric(self, **metric) -> bool:
        """``current`` beats ``best`` on ``cfg.best_metric`` (both are (valid_loss, precision, recall,
        map, ndcg) tuples; an unknown metric name never improves — reference base_trainer.py:117-141)."""
        choice = _BEST_METRIC.get(self.cfg.best_metric)
        if choice is None:
            return False
        position, smaller_is_better = choice
        current, best = metric['current'][position], metric['best'][position]
        return current < best if smaller_is_better else current > best

    @abstractmethod
    def train(self, train_dataloader) -> float:
        pass

    @abstractmethod
    def validate(self, valid_dataloader):
        pass

    @abstractmethod
    def evaluate(self, test_dataloader):
        pass

    # -- resume (not in the reference, which saves weights only: SURVEY.md §8 f4) ---------------
    def save_checkpoint(self, path, **extra):
        """Weights (the reference's ``state_dict`` keys) + optimizer state (Adam moments and step
        counts) + anything the caller wants to find again (epoch, best metric, ...)."""
        torch.save({"model": self.model.state_dict(), "optimizer": self.optimizer.state_dict(), "extra": extra}, path)

    def load_checkpoint(self, path):
        """Restore what :meth:`save_checkpoint` wrote; training continues as if it had never stopped (to
        float rounding) when fed the same batches.  Returns the ``extra`` dict."""
        ck = torch.load(path, map_location=self.device, weights_only=True)
        self.model.load_state_dict(ck["model"])
        self.optimizer.load_state_dict(ck["optimizer"])
        return ck.get("extra", {})

    def load_best_model(self):
        # reference base_trainer.py:155-157 (weights_only: the file holds tensors only)
        logger.info("[Trainer] Load best model...")
        state = torch.load(f'{self.cfg.model_dir}/best_model.pt', map_location=self.device, weights_only=True)
        self.model.load_state_dict(state)


class TripletTrainer(BaseTrainer):
    """What the BPR-triplet trainers (MF, NGCF, DCN) share: the loss, the batch unpacking and the reference's
    three-argument epoch loop, whose metrics come from ``evaluate(valid_eval_data, 'valid')``."""

    def _loss(self):
        return BPRLoss()

    def run(self, train_dataloader, valid_dataloader, valid_eval_data):
        # reference mf_trainer.py:34-97, ngcf_trainer.py:36-99, dcn_trainer.py:36-97
        logger.info("[Trainer] run...")
        best = (1e+6, .0, .0, .0, .0)
        endurance = 0
        for epoch in range(self.cfg.epochs):
            train_loss = self.train(train_dataloader)
            valid_loss = self.validate(valid_dataloader)
            current = (valid_loss,) + tuple(self.evaluate(valid_eval_data, 'valid'))
            self._log_epoch(epoch, train_loss, *current)
            if self._is_surpass_best_metric(current=current, best=best):
                logger.info("[Trainer] update best model...")
                best = current
                endurance = 0
                self._save_best()
            else:
                endurance += 1
                if endurance > self.cfg.patience:
                    logger.info("[Trainer] ealry stopping...")
                    break

    def _batch(self, data):
        dev = self.device
        return (data['user_id'].to(dev, non_blocking=True), data['pos_item'].to(dev, non_blocking=True),
                data['neg_item'].to(dev, non_blocking=True))
