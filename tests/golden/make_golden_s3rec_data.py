#!/usr/bin/env python3
"""Generate tests/golden/s3rec_data_small.npz by RUNNING THE REFERENCE's S3RecDataPipeline.split and S3RecDataset on
CPU in the build container.  Same provenance rules as make_golden.py, whose logging / config stand-ins it reuses
(imported, not edited).  Data only: a tiny frame and what the reference made of it.

The frame: 12 users, 150 items, max_seq_len L = 6, behaviour rows of length 1, 2, 3, 4, 5, L+2, L+3, L+4, 2L and three
more (7, 11, 20), raw 0-based ids with a repeat inside some rows.  Recorded:
* ``beh_ptr`` / ``beh_idx``  the rows as CSR;
* ``{train,valid,test}_X`` / ``_Y``  the six padded windows of ``split`` ([12, L] each);
* under ``np.random.seed(seed)``, reading users 0..11 of the train dataset, then of the valid dataset, then of the
  test dataset: ``train_neg_items`` / ``valid_neg_items`` [12, L], ``test_neg_items`` [12, 99], ``test_pos_item`` [12].

Usage:  python tests/golden/make_golden_s3rec_data.py        (seconds -> tests/golden/s3rec_data_small.npz)
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs the stand-ins and puts the reference on sys.path)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

from data.datasets.s3rec_data_pipeline import S3RecDataPipeline  # noqa: E402
from data.datasets.s3rec_dataset import S3RecDataset  # noqa: E402

NUM_ITEMS, L, ATTRS, SEED = 150, 6, 5, 42
LENGTHS = (1, 2, 3, 4, 5, L + 2, L + 3, L + 4, 2 * L, 7, 11, 20)


def golden_s3rec_data(out_path):
    rs = np.random.RandomState(11)
    rows = []
    for n in LENGTHS:
        row = rs.randint(0, NUM_ITEMS, n)
        if n >= 4:
            row[-2] = row[0]                                   # a repeat inside the row
        rows.append([int(v) for v in row])
    df = pd.DataFrame({"behaviors": rows})
    pipe = S3RecDataPipeline(mg.DictConfig(max_seq_len=L))
    parts = dict(zip(("train", "valid", "test"), pipe.split(df)))
    item2attribute = {i: {"categories": [i % ATTRS] if i else []} for i in range(NUM_ITEMS + 1)}
    out = {"beh_ptr": np.r_[0, np.cumsum(LENGTHS)].astype(np.int64), "beh_idx": np.concatenate(rows).astype(np.int64)}
    for mode, part in parts.items():
        out[f"{mode}_X"] = np.array(part["X"].tolist(), dtype=np.int64)
        out[f"{mode}_Y"] = np.array(part["Y"].tolist(), dtype=np.int64)
    np.random.seed(SEED)
    for mode, part in parts.items():
        ds = S3RecDataset(part, item2attribute, ATTRS, num_items=NUM_ITEMS, train=mode != "test")
        items = [ds[u] for u in range(len(ds))]
        assert all(np.array_equal(it["X"], out[f"{mode}_X"][u]) for u, it in enumerate(items))
        out[f"{mode}_neg_items"] = np.array([it["neg_items"] for it in items], dtype=np.int64)
        if mode == "test":
            out["test_pos_item"] = np.array([it["pos_item"] for it in items], dtype=np.int64)
        else:
            assert all(np.array_equal(it["pos_items"], out[f"{mode}_Y"][u]) for u, it in enumerate(items))
    np.savez_compressed(out_path, versions=mg.VERSIONS, cfg_names=np.array(["num_items", "max_seq_len", "seed"]),
                        cfg_values=np.array([NUM_ITEMS, L, SEED], dtype=np.int64), **out)
    print(f"[s3rec data] {len(LENGTHS)} users, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    golden_s3rec_data(os.path.join(HERE, "s3rec_data_small.npz"))
