#!/usr/bin/env python3
"""Generate tests/golden/s3rec_train_small.npz by RUNNING THE REFERENCE's S3Rec / S3RecTrainer in training mode on
CPU in the build container.  Same provenance rules as make_golden.py, whose logging / config stand-ins it reuses
(imported, not edited), and the sizes of make_golden_s3rec.py: 300 items, embed_size 32, max_seq_len 12, 2 heads,
2 blocks.  ``dropout_ratio`` is 0, so the reference's train() mode is deterministic.  Data only.

Everything starts from the ``pert:`` state of s3rec_small.npz and uses its three validation batches.  Recorded:
* ``grad32:*`` / ``grad64:*``  the gradient of every parameter after one ``finetune`` + ``BPRLoss`` + ``backward``
  on the first validation batch, from the float32 model and from its float64 twin;
* ``grad_none``  the names of the parameters whose ``grad`` is None after that backward;
* ``train_losses``  what two calls of ``trainer.train`` over the three batches return (Adam, lr 1e-3), and
  ``final:*`` the ``state_dict`` after them.

Usage:  python tests/golden/make_golden_s3rec_train.py        (seconds -> tests/golden/s3rec_train_small.npz)
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

import utils as ref_utils  # noqa: E402
from loss import BPRLoss  # noqa: E402
from models.s3rec import S3Rec  # noqa: E402
from trainers.s3rec_trainer import S3RecTrainer  # noqa: E402

LR, EPOCHS = 1e-3, 2


def golden_s3rec_train(out_path):
    small = np.load(os.path.join(HERE, "s3rec_small.npz"))
    c = dict(zip(small["cfg_names"].tolist(), small["cfg_values"].tolist()))
    tmp = tempfile.mkdtemp()
    cfg = mg.DictConfig(seed=c["seed"], shuffle=False, model_dir=tmp, device="cpu", epochs=EPOCHS, batch_size=8, lr=LR,
                        optimizer="adam", patience=5, top_n=c["top_n"], weight_decay=0, best_metric="loss",
                        wandb=False, model_name="S3Rec", embed_size=c["embed_size"], max_seq_len=c["max_seq_len"],
                        num_heads=c["num_heads"], num_blocks=c["num_blocks"], dropout_ratio=0.0, load_pretrain=False,
                        pretrain=False, mask_portion=0.2)
    state = {k[5:]: torch.from_numpy(small[k]) for k in small.files if k.startswith("pert:")}
    batches = [{k: torch.from_numpy(small[f"valid{i}_{k}"]) for k in ("X", "pos_items", "neg_items")} for i in range(3)]

    ref_utils.set_seed(cfg.seed)
    trainer = S3RecTrainer(cfg, c["num_items"], None, c["attributes_count"])
    model = trainer.model
    model.load_state_dict(state, strict=True)
    model64 = S3Rec(cfg, c["num_items"], c["attributes_count"])
    model64.load_state_dict(state, strict=True)
    model64 = model64.double()

    out = {}
    for prefix, m, dt in (("grad32", model, torch.float32), ("grad64", model64, torch.float64)):
        m.train()
        m.zero_grad()
        torch.set_default_dtype(dt)
        try:
            pos, neg = m.finetune(*batches[0].values())
            loss = BPRLoss()(pos, neg)
            loss.backward()
        finally:
            torch.set_default_dtype(torch.float32)
        assert pos.dtype == dt
        for name, prm in m.named_parameters():
            if prm.grad is not None:
                out[f"{prefix}:{name}"] = prm.grad.detach().numpy().copy()
        out[f"{prefix}_loss"] = np.float64(loss.item())
    out["grad_none"] = np.array([n for n, prm in model.named_parameters() if prm.grad is None])
    assert out["grad_none"].tolist() == [n for n, prm in model64.named_parameters() if prm.grad is None]
    model.zero_grad()

    losses = [trainer.train(batches) for _ in range(EPOCHS)]
    out["train_losses"] = np.asarray(losses, dtype=np.float64)
    out.update({f"final:{k}": v.detach().numpy().copy() for k, v in model.state_dict().items()})
    np.savez_compressed(out_path, versions=mg.VERSIONS, lr=np.float64(LR), epochs=np.int64(EPOCHS), **out)
    print(f"[s3rec train] losses={losses} none={out['grad_none'].tolist()} {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    golden_s3rec_train(os.path.join(HERE, "s3rec_train_small.npz"))
