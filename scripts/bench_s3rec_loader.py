#!/usr/bin/env python3
"""The S3Rec batch producers at Yelp2018 shape (31,668 users, 38,048 items, max_seq_len 50; synthetic interactions,
47 per user on average): the device loader (csrc/s3rec_batches.hip) next to the host DataLoader(S3RecDataset), and
what share of a fine-tuning epoch the device loader takes.  Writes profiles/s3rec_loader_yelp2018.json and prints it
as one line.

    python scripts/bench_s3rec_loader.py [--repeats 7] [--warmup 2] [--host-users 512]

Measured (medians over ``repeats`` runs after ``warmup`` runs, host clock around a window that ends in a device
synchronise):
* ``train_epoch_batches_ms``  one epoch of batch production by S3RecBatchLoader, train mode, batch 256 — the
  permutation, the one launch, the slicing, the flag read;
* ``train_epoch_kernel_ms``   the launch alone (device events);
* ``test_pass_ms`` / ``test_pass_kernel_ms``  the same for one test pass with 99 negatives;
* ``finetune_epoch_ms``       one fine-tuning epoch (S3RecTrainer.train, E = 64, 2 heads, 2 blocks, dropout 0.1, Adam,
  batch 256) fed by the device loader; ``loader_share_of_epoch`` = train_epoch_batches_ms / finetune_epoch_ms (derived);
* ``host_*``                  DataLoader(S3RecDataset) producing the batches of the first ``host_users`` users, and
  that time scaled to all users (labelled scaled: derived, not measured).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402

L, BATCH = 50, 256


def _median_ms(fn, repeats, warmup):
    times = []
    for it in range(warmup + repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= warmup:
            times.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(times), 4), [round(v, 4) for v in times]


def _kernel_ms(fn, repeats, warmup):
    times = []
    for it in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            times.append(a.elapsed_time(b))
    return round(statistics.median(times), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-users", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s3rec_loader_yelp2018.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_s3rec_loader: no GPU (the device loader has no CPU path to time)")
    from torch.utils.data import DataLoader
    from yelprecommendation_amd.data.datasets.s3rec_data_pipeline import S3RecDataPipeline
    from yelprecommendation_amd.data.datasets.s3rec_dataset import S3RecDataset
    from yelprecommendation_amd.data.s3rec_batches import S3RecBatchLoader, S3RecSequences
    from yelprecommendation_amd.data.synthetic import YELP2018_ITEMS as NI, YELP2018_USERS as NU, make_interactions_torch
    from yelprecommendation_amd.trainers.s3rec_trainer import S3RecTrainer
    from yelprecommendation_amd.utils import make_config, set_seed
    dev = torch.device("cuda")
    u, i = make_interactions_torch(NU, NI, 47.0, seed=1234, device=dev)
    store = S3RecSequences(u, i, NU, NI, L, seed=42)
    res = {"workload": "s3rec_yelp2018_loader", "shape": [NU, NI, L], "interactions": int(u.numel()), "batch": BATCH,
           "repeats": a.repeats, "warmup": a.warmup, "date": time.strftime("%Y-%m-%d"),
           "device": torch.cuda.get_device_name(0)}

    train_loader = S3RecBatchLoader(store, "train", BATCH, shuffle=True, seed=42)
    test_loader = S3RecBatchLoader(store, "test", BATCH, seed=0)
    res["train_epoch_batches_ms"], res["train_epoch_batches_ms_runs"] = _median_ms(lambda: list(train_loader), a.repeats, a.warmup)
    res["test_pass_ms"], res["test_pass_ms_runs"] = _median_ms(lambda: list(test_loader), a.repeats, a.warmup)
    res["train_epoch_kernel_ms"] = _kernel_ms(lambda: store.draw("train", 1), a.repeats, a.warmup)
    res["test_pass_kernel_ms"] = _kernel_ms(lambda: store.draw("test", 1, n_neg=99), a.repeats, a.warmup)
    store.check()

    set_seed(0)
    cfg = make_config("S3Rec", device="cuda", model_dir=tempfile.mkdtemp(prefix="yr_bench_s3rec_loader."), lr=1e-4,
                      load_pretrain=False, batch_size=BATCH)
    trainer = S3RecTrainer(cfg, NI, None, 100)
    res["finetune_epoch_ms"], res["finetune_epoch_ms_runs"] = _median_ms(lambda: trainer.train(train_loader), max(3, a.repeats // 2), 1)
    res["loader_share_of_epoch"] = round(res["train_epoch_batches_ms"] / res["finetune_epoch_ms"], 5)
    res["loader_share_of_epoch_is"] = "derived: train_epoch_batches_ms / finetune_epoch_ms"

    # the host path on the first host_users users (the reference's producer: a Python `in list` test per draw)
    n = min(a.host_users, NU)
    ptr = store.beh_ptr[:n + 1].cpu().numpy()
    idx = store.beh_idx[:int(ptr[-1])].cpu().numpy()
    frame = pd.DataFrame({"behaviors": [idx[s:e].tolist() for s, e in zip(ptr[:-1], ptr[1:])]})
    parts = S3RecDataPipeline(cfg).split(frame)
    np.random.seed(0)
    for name, part, train in (("train", parts[0], True), ("test", parts[2], False)):
        dl = DataLoader(S3RecDataset(part, None, None, num_items=NI, train=train), batch_size=BATCH, shuffle=train)
        ms, _ = _median_ms(lambda: list(dl), 3, 1)
        res[f"host_{name}_ms_{n}_users"] = ms
        res[f"host_{name}_ms_scaled_to_{NU}_users"] = round(ms * NU / n, 1)
    res["host_scaled_is"] = f"derived: the {n}-user time x {NU} / {n}"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
