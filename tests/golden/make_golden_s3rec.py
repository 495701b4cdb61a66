#!/usr/bin/env python3
"""Generate tests/golden/s3rec_small.npz by RUNNING THE REFERENCE's S3Rec / S3RecTrainer on CPU in the build
container.  Same provenance rules as make_golden.py, whose logging / config stand-ins it reuses (imported, not
edited).  Data only: two state_dicts, a few hand-shaped batches and what the reference computed from them.

Recorded, at num_items 300, attributes_count 20, embed_size 32, max_seq_len 12, 2 heads, 2 blocks:
* ``init:*``  the seeded initial state_dict;
* ``pert:*``  the same with the LayerNorm weights and every bias moved by 0.1 randn (fresh LayerNorms are the
  identity and would hide their affine part) — the state every output below was computed with;
* three validation batches (an all-padding row, a one-item row, a full row, interior padding ...) with the
  ``finetune`` outputs in float32 and in float64 (``model.double()`` under ``torch.set_default_dtype(float64)``)
  and the trainer's ``validate`` return;
* two test batches (one positive, 99 distinct negatives) with the ``evaluate`` scores in both precisions and the
  trainer's four metrics.
The reference ranks with an unstable argsort, so the test batches are redrawn until no two candidate scores of a
row are closer than 1e-4 in float64: a near-tie would make its own record arbitrary.

Usage:  python tests/golden/make_golden_s3rec.py        (seconds -> tests/golden/s3rec_small.npz)
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
from models.s3rec import S3Rec  # noqa: E402
from trainers.s3rec_trainer import S3RecTrainer  # noqa: E402

NUM_ITEMS, ATTRS, E, L, HEADS, BLOCKS, TOP_N, NEG = 300, 20, 32, 12, 2, 2, 10, 99
MIN_GAP = 1e-4


def _state(prefix, model):
    return {f"{prefix}:{k}": v.detach().numpy().copy() for k, v in model.state_dict().items()}


def _sequences(rs, rows):
    """[rows, L] ids: row 0 all padding, 1 one item (last position), 2 full, 3 interior padding, the rest
    left-padded histories of random length."""
    X = np.zeros((rows, L), dtype=np.int64)
    for r in range(rows):
        ids = rs.randint(1, NUM_ITEMS + 1, L)
        if r == 0:
            ids[:] = 0
        elif r == 1:
            ids[:-1] = 0
        elif r == 3:
            ids[rs.choice(np.arange(1, L - 1), 4, replace=False)] = 0
        elif r > 3:
            ids[:rs.randint(0, L - 1)] = 0
        X[r] = ids
    return X


def _double(model, cfg):
    """A float64 twin (the config stand-in does not deep-copy: build a second model and hand it the state)."""
    m = S3Rec(cfg, NUM_ITEMS, ATTRS)
    m.load_state_dict(model.state_dict(), strict=True)
    return m.double()


def golden_s3rec(out_path, seed=42):
    tmp = tempfile.mkdtemp()
    cfg = mg.DictConfig(seed=seed, shuffle=False, model_dir=tmp, device="cpu", epochs=1, batch_size=8, lr=1e-3,
                        optimizer="adam", patience=5, top_n=TOP_N, weight_decay=0, best_metric="loss", wandb=False,
                        model_name="S3Rec", embed_size=E, max_seq_len=L, num_heads=HEADS, num_blocks=BLOCKS,
                        dropout_ratio=0.1, load_pretrain=False, pretrain=False, mask_portion=0.2)
    ref_utils.set_seed(cfg.seed)
    trainer = S3RecTrainer(cfg, NUM_ITEMS, None, ATTRS)
    model = trainer.model
    init = _state("init", model)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for name, t in model.state_dict().items():
            if "layernorm" in name or name.endswith(".bias"):
                t.add_(0.1 * torch.randn(t.shape, generator=g))
    pert = _state("pert", model)
    model.eval()
    model64 = _double(model, cfg).eval()

    def both(fn_name, *args):
        with torch.no_grad():
            a = getattr(model, fn_name)(*args)
            torch.set_default_dtype(torch.float64)
            try:
                b = getattr(model64, fn_name)(*args)
            finally:
                torch.set_default_dtype(torch.float32)
        assert a[0].dtype == torch.float32 and b[0].dtype == torch.float64
        return [t.numpy().copy() for t in a], [t.numpy().copy() for t in b]

    out = {}
    rs = np.random.RandomState(5)
    valid = []
    for i, rows in enumerate((8, 8, 5)):
        X = _sequences(rs, rows)
        pos = rs.randint(0, NUM_ITEMS + 1, (rows, L)).astype(np.int64)
        neg = rs.randint(0, NUM_ITEMS + 1, (rows, L)).astype(np.int64)
        valid.append({"X": torch.from_numpy(X), "pos_items": torch.from_numpy(pos), "neg_items": torch.from_numpy(neg)})
        f32, f64 = both("finetune", *valid[-1].values())
        out.update({f"valid{i}_X": X, f"valid{i}_pos_items": pos, f"valid{i}_neg_items": neg,
                    f"valid{i}_pos_preds_f32": f32[0], f"valid{i}_neg_preds_f32": f32[1],
                    f"valid{i}_pos_preds_f64": f64[0], f"valid{i}_neg_preds_f64": f64[1]})
    out["validate"] = np.float64(trainer.validate(valid))

    for draw in range(100000):
        rs = np.random.RandomState(1000 + draw)
        test, rec, ok = [], {}, True
        for i, rows in enumerate((4, 3)):
            X = _sequences(rs, rows + 1)[1:]                      # no all-padding row: its last position is padding too,
            X[0, -1] = rs.randint(1, NUM_ITEMS + 1)               # and every row ends on a real item
            cand = np.stack([rs.choice(np.arange(1, NUM_ITEMS + 1), NEG + 1, replace=False) for _ in range(rows)])
            pos, neg = cand[:, 0].astype(np.int64), cand[:, 1:].astype(np.int64)
            test.append({"X": torch.from_numpy(X), "pos_item": torch.from_numpy(pos), "neg_items": torch.from_numpy(neg)})
            f32, f64 = both("evaluate", *test[-1].values())
            scores = np.sort(np.concatenate(f64, axis=1), axis=1)
            ok = ok and float(np.diff(scores, axis=1).min()) >= MIN_GAP
            rec.update({f"test{i}_X": X, f"test{i}_pos_item": pos, f"test{i}_neg_items": neg,
                        f"test{i}_pos_pred_f32": f32[0], f"test{i}_neg_preds_f32": f32[1],
                        f"test{i}_pos_pred_f64": f64[0], f"test{i}_neg_preds_f64": f64[1]})
        if ok:
            break
    assert ok, "no draw without a near-tie"
    out.update(rec)
    out["test_draw"] = np.int64(draw)
    metrics = trainer.evaluate(test)
    out["test_metrics"] = np.asarray(metrics, dtype=np.float64)
    np.savez_compressed(
        out_path, versions=mg.VERSIONS,
        cfg_names=np.array(["num_items", "attributes_count", "embed_size", "max_seq_len", "num_heads", "num_blocks",
                            "top_n", "seed"]),
        cfg_values=np.array([NUM_ITEMS, ATTRS, E, L, HEADS, BLOCKS, TOP_N, seed], dtype=np.int64),
        **init, **pert, **out)
    print(f"[s3rec] validate={out['validate']:.6f} test draw {draw} metrics={metrics} "
          f"{os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    golden_s3rec(os.path.join(HERE, "s3rec_small.npz"))
