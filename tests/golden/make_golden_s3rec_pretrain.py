#!/usr/bin/env python3
"""Generate tests/golden/s3rec_pretrain_small.npz by RUNNING THE REFERENCE's S3Rec / S3RecPreTrainer on CPU in the
build container.  Same provenance rules as make_golden.py, whose logging / config stand-ins it reuses (imported, not
edited), and the sizes of s3rec_small.npz: 300 items, embed_size 32, max_seq_len 12, 2 heads, 2 blocks, batches of 8
(the third has 5 rows), ``dropout_ratio`` 0.  Data only.

Two things of the reference cannot run as published and are replaced HERE, in subclasses written in this file:
* ``S3Rec.encode`` calls ``_self_attention_block`` without its two mask arguments (models/s3rec.py:117-118).  The
  subclass passes the masks ``finetune`` builds (models/s3rec.py:91-97); nothing else of the model is touched.
* the two masking methods of the trainer draw from the host RNG; the subclass returns RECORDED arrays, chosen so that
  every branch occurs: a masked and an unmasked padded position, a segment whose end is L - 1 (the last start the
  reference's ``randint`` can give), a segment starting at 0, and, per row, the negative segment from the SAME row at
  another start (the only way the reference's ``while neg_user_idx != i`` ends).
``aap_actual`` / ``mip_actual`` are built as data/datasets/s3rec_dataset.py:35-39 builds them, as float32 (the
reference's float64 targets would promote its float32 loss to float64; the float64 twin below is that reading).

Everything starts from the ``pert:`` state of s3rec_small.npz and uses the X of its three validation batches.
Recorded, from the float32 model (``32``) and its float64 twin (``64``):
* ``out32:*`` / ``out64:*``  the four dense outputs of ``model.pretrain`` on the first batch (aap, mip, map, sp_pos,
  sp_neg) and ``loss32`` / ``loss64`` = (aap, mip, map, sp) losses of trainers/s3rec_trainer.py:137-158; their sum is
  asserted equal to what ``trainer.train([batch])`` returns on an untouched copy;
* ``grad32:*`` / ``grad64:*``  every parameter's gradient after one backward of that sum, ``grad_none`` the names whose
  ``grad`` is None (``map_weight.weight`` among them);
* ``train_losses32`` / ``train_losses64``  what two calls of ``trainer.train`` over the three batches return (Adam,
  lr 1e-3), ``final:*`` the float32 ``state_dict`` after them;
* the inputs: ``attr_ptr`` / ``attr_idx`` (the item id -> categories CSR of the generated ``item2attributes``) and per
  batch ``b{i}_X``, ``b{i}_masks``, ``b{i}_seg``, ``b{i}_pos``, ``b{i}_neg``.

Usage:  python tests/golden/make_golden_s3rec_pretrain.py        (seconds -> tests/golden/s3rec_pretrain_small.npz)
"""
from __future__ import annotations

import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs the stand-ins and puts the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import trainers.s3rec_trainer as ref_trainer  # noqa: E402
import utils as ref_utils  # noqa: E402
from models.s3rec import S3Rec  # noqa: E402

LR, EPOCHS = 1e-3, 2
BCE = torch.nn.functional.binary_cross_entropy_with_logits


class RepairedS3Rec(S3Rec):
    def encode(self, X):
        padding_mask = (X <= 0)
        L = self.cfg.max_seq_len
        attn_mask = torch.triu(torch.zeros(L, L) + torch.finfo(torch.float32).min, diagonal=1)
        return self._self_attention_block(self._embedding_layer(X), padding_mask, attn_mask)


class RecordedPreTrainer(ref_trainer.S3RecPreTrainer):
    """The reference's trainer with the two masking methods answering from ``self.recorded`` (a list of batches)."""

    def _take(self, sequences):
        for b in self.recorded:
            if b["X"].shape == sequences.shape and bool((b["X"] == sequences).all()):
                return b
        raise KeyError("no recorded masks for this batch")

    def item_level_masking(self, sequences):
        b = self._take(sequences)
        return b["masks"], b["masks"] * sequences

    def segment_masking(self, sequences):
        b = self._take(sequences)
        return b["seg"], b["pos"], b["neg"]


def make_attributes(num_items, count, seed=7):
    rs = np.random.RandomState(seed)
    out = {0: {"categories": []}}
    for k in range(1, num_items + 1):
        out[k] = {"categories": sorted(rs.choice(count, size=1 + rs.randint(4), replace=False).tolist())}
    return out


def make_masks(X, i, L):
    """The recorded masks of batch i (see the module docstring for what they must contain)."""
    rs = np.random.RandomState(100 + i)
    B = X.shape[0]
    masks = rs.rand(B, L) < 0.3
    pads = np.argwhere(X == 0)
    if len(pads) >= 2:
        masks[tuple(pads[0])], masks[tuple(pads[-1])] = True, False
    seg, pos, neg = X.copy(), np.zeros_like(X), np.zeros_like(X)
    for b in range(B):
        n = 2 + rs.randint(L // 2 - 2)                                 # [2, L // 2 - 1]
        start = (L - n - 1) if b == 0 else 0 if b == 1 else rs.randint(L - n)
        neg_start = rs.randint(L - n)
        seg[b, start:start + n] = 0
        pos[b, L - n:] = X[b, start:start + n]
        neg[b, L - n:] = X[b, neg_start:neg_start + n]
    return masks, seg, pos, neg


def dense_actuals(X, item2attributes, count, num_items, dtype):
    aap = np.array([[[1 if a in item2attributes[int(item)]["categories"] else 0 for a in range(count)] for item in row]
                    for row in X], dtype="float")
    mip = np.zeros(X.shape + (num_items + 1,), dtype="float")
    for b, row in enumerate(X):
        for i, item in enumerate(row):
            mip[b, i, item] = 1
    return torch.from_numpy(aap).to(dtype), torch.from_numpy(mip).to(dtype)


def four_losses(model, b):
    """trainers/s3rec_trainer.py:134-158 on one batch: (the dense outputs, the four losses)."""
    aap, mip, map_, (sp_pos, sp_neg) = model.pretrain(b["masks"] * b["X"], b["seg"], b["pos"], b["neg"])
    on, off = b["masks"].unsqueeze(-1), b["masks"].logical_not().unsqueeze(-1)
    n = b["X"].size(0)
    losses = (BCE(aap, b["aap_actual"] * on), BCE(mip * off, b["mip_actual"] * off), BCE(map_ * off, b["aap_actual"] * off),
              BCE(torch.concat([sp_neg, sp_pos]), torch.concat([torch.zeros(n), torch.ones(n)]).to(aap.dtype)))
    return dict(aap=aap, mip=mip, map=map_, sp_pos=sp_pos, sp_neg=sp_neg), losses


def golden_s3rec_pretrain(out_path):
    small = np.load(os.path.join(HERE, "s3rec_small.npz"))
    c = dict(zip(small["cfg_names"].tolist(), small["cfg_values"].tolist()))
    L, A, I = c["max_seq_len"], c["attributes_count"], c["num_items"]
    cfg = mg.DictConfig(seed=c["seed"], shuffle=False, model_dir=tempfile.mkdtemp(), device="cpu", epochs=EPOCHS,
                        pretrain_epochs=EPOCHS, batch_size=8, lr=LR, optimizer="adam", patience=5, top_n=c["top_n"],
                        weight_decay=0, best_metric="loss", wandb=False, model_name="S3Rec", embed_size=c["embed_size"],
                        max_seq_len=L, num_heads=c["num_heads"], num_blocks=c["num_blocks"], dropout_ratio=0.0,
                        load_pretrain=False, pretrain=True, mask_portion=0.2)
    state = {k[5:]: torch.from_numpy(small[k]) for k in small.files if k.startswith("pert:")}
    item2attributes = make_attributes(I, A)
    out, batches = {}, {torch.float32: [], torch.float64: []}
    for i in range(3):
        X = small[f"valid{i}_X"]
        masks, seg, pos, neg = make_masks(X, i, L)
        out.update({f"b{i}_X": X, f"b{i}_masks": masks, f"b{i}_seg": seg, f"b{i}_pos": pos, f"b{i}_neg": neg})
        for dt in batches:
            aap_actual, mip_actual = dense_actuals(X, item2attributes, A, I, dt)
            batches[dt].append(dict(X=torch.from_numpy(X), masks=torch.from_numpy(masks), seg=torch.from_numpy(seg),
                                    pos=torch.from_numpy(pos), neg=torch.from_numpy(neg), aap_actual=aap_actual,
                                    mip_actual=mip_actual))
    lists = [item2attributes[k]["categories"] for k in range(I + 1)]
    out["attr_ptr"] = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    out["attr_idx"] = np.array([a for l in lists for a in l], np.int64)

    ref_trainer.S3Rec = RepairedS3Rec                          # what S3RecPreTrainer.__init__ constructs
    ref_utils.set_seed(cfg.seed)
    trainers = {}

    def make_trainer(dt):
        trainer = RecordedPreTrainer(cfg, I, item2attributes, A)
        trainer.recorded = batches[dt]
        trainer.model.load_state_dict(state, strict=True)
        if dt == torch.float64:
            trainer.model = trainer.model.double()
            trainer.optimizer = trainer._optimizer(cfg.optimizer, trainer.model, cfg.lr)
        return trainer

    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        torch.set_default_dtype(dt)
        try:
            trainer = make_trainer(dt)
            model = trainer.model
            model.train()
            outs, losses = four_losses(model, batches[dt][0])
            assert outs["mip"].dtype == dt
            model.zero_grad()
            sum(losses).backward()
            for k, v in outs.items():
                out[f"out{tag}:{k}"] = v.detach().numpy().copy()
            out[f"loss{tag}"] = np.array([float(l.detach()) for l in losses], dtype=np.float64)
            for name, prm in model.named_parameters():
                if prm.grad is not None:
                    out[f"grad{tag}:{name}"] = prm.grad.detach().numpy().copy()
            none = [n for n, prm in model.named_parameters() if prm.grad is None]
            model.zero_grad()
            # the four losses above ARE the reference's step: its own train() on an untouched copy returns their sum
            got = make_trainer(dt).train([batches[dt][0]])
            assert abs(got - float(sum(losses).detach())) <= (1e-6 if dt == torch.float32 else 1e-12), (got, float(sum(losses).detach()))
            trainers[tag] = (trainer, none)
        finally:
            torch.set_default_dtype(torch.float32)
    assert trainers["32"][1] == trainers["64"][1] and "map_weight.weight" in trainers["32"][1]
    out["grad_none"] = np.array(trainers["32"][1])
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        torch.set_default_dtype(dt)
        try:
            trainer = trainers[tag][0]
            out[f"train_losses{tag}"] = np.asarray([trainer.train(batches[dt]) for _ in range(EPOCHS)], dtype=np.float64)
            if tag == "32":                                     # the twin's final state would take the file past 1 MiB
                out.update({f"final:{k}": v.detach().numpy().copy() for k, v in trainer.model.state_dict().items()})
        finally:
            torch.set_default_dtype(torch.float32)
    np.savez_compressed(out_path, versions=mg.VERSIONS, lr=np.float64(LR), epochs=np.int64(EPOCHS), **out)
    print(f"[s3rec pretrain] losses32={out['loss32'].tolist()} train={out['train_losses32'].tolist()} "
          f"none={out['grad_none'].tolist()} {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    golden_s3rec_pretrain(os.path.join(HERE, "s3rec_pretrain_small.npz"))
