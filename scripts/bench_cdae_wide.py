#!/usr/bin/env python3
"""CDAE at the hidden sizes 256 / 512 / 1024, Yelp2018 shape (31,668 users x 38,048 items, 47 interactions per user,
batches of 256 rows, neg_times 5): a training epoch and a validation pass of CDAETrainer on two routes —

    lists   batches as lists straight from the per-user CSR, sampled NS-BCE decoder, transposed W_h with item marks,
            row-marked Adam, all-user fused evaluation (what train.py fast_loader=true runs at these widths)
    parent  what the commit before the wide kernels ran at that width with fast_loader=true: dense [B, I] rows and
            masks from the loader; at 256 the sampled decoder on them (compaction pass, row marks), at 512 / 1024 the
            dense decoder (three full-catalogue products per step), no transposed W_h, no row marks (every Adam launch
            reads and clears all of dW_h, dV, dW_o), per-batch full-catalogue validation

as milliseconds per step (epoch / batches: the loader's work is part of the route) and per validation pass.  Medians of
interleaved repeats, warm-up excluded.  Every width runs in a child process of its own under a time limit; the first
one that fails ends the run.

    python scripts/bench_cdae_wide.py [--repeats 5] [--out profiles/cdae_wide_yelp2018.json]
"""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDE = (256, 512, 1024)
B, NEG_TIMES = 256, 5


def child(H, repeats):
    import torch
    from yelprecommendation_amd.data.cdae_batches import CDAEBatchLoader, CDAEInteractions
    from yelprecommendation_amd.data.synthetic import YELP2018_ITEMS as NI, YELP2018_USERS as NU, make_interactions_torch
    from yelprecommendation_amd.train import cdae_takes_list_batches
    from yelprecommendation_amd.trainers import CDAETrainer
    from yelprecommendation_amd.utils import make_config
    dev = torch.device("cuda")
    u, i = make_interactions_torch(NU, NI, 47.0, seed=1234, device=dev)
    data = CDAEInteractions.from_interactions(u, i, NU, NI, seed=1, device=dev)
    tmp = tempfile.mkdtemp(prefix="yr_cdae_wide.")
    routes = {}
    for name in ("lists", "parent"):
        lists = name == "lists"
        over = {} if lists or H <= 256 else {"train_decoder": "dense", "transposed_wh": False}
        cfg = make_config("CDAE", hidden_size=H, device="cuda", model_dir=tmp, lr=1e-4, batch_size=B, eval_batch_group=32,
                          negative_sampling=True, neg_times=NEG_TIMES, loss_name="bce", top_n=10, list_batches=lists, **over)
        assert cdae_takes_list_batches(cfg, NI) == lists
        torch.manual_seed(1)
        trainer = CDAETrainer(cfg, NI, NU)
        if not lists and H > 256:                      # no row marks at these widths before: dW_h and dV read and cleared whole
            from yelprecommendation_amd.cdae_step import CDAEStep
            trainer._step = CDAEStep(trainer.model, trainer.optimizer, True, decoder="dense", transposed_wh=False,
                                     row_marks=False)
        step = trainer._fused_step()
        assert step.row_marks == (lists or H <= 256)
        assert step.decoder == ("dense" if not lists and H > 256 else "sampled")
        train = CDAEBatchLoader(data, "train", B, NEG_TIMES, shuffle=True, seed=3, lists=lists,
                                dropout=trainer.model.corruption_level)
        valid = CDAEBatchLoader(data, "valid", B, NEG_TIMES, shuffle=False, seed=4, lists=lists)
        routes[name] = (trainer, train, valid)
    steps = -(-NU // B)
    fns = {}
    for name, (trainer, train, valid) in routes.items():
        fns[(name, "step_ms")] = (lambda trainer=trainer, train=train: trainer.train(train))
        fns[(name, "validate_ms")] = (lambda trainer=trainer, valid=valid: trainer.validate(valid))
    samples = {k: [] for k in fns}
    for r in range(repeats + 1):                       # repeat 0 is the warm-up
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r > 0:
                samples[k].append((time.perf_counter() - t0) * 1e3 / (steps if k[1] == "step_ms" else 1))
    out = {name: {what: round(statistics.median(samples[(name, what)]), 4) for what in ("step_ms", "validate_ms")}
           for name in routes}
    out["parent_over_lists"] = {what: round(out["parent"][what] / out["lists"][what], 2) for what in ("step_ms", "validate_ms")}
    out["steps_per_epoch"] = steps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdae_wide_yelp2018.json"))
    ap.add_argument("--child", type=int, metavar="H")
    ap.add_argument("--limit", type=int, default=300, help="seconds per measurement process")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.child, a.repeats)))
        return 0
    import torch
    res = {"workload": "cdae_wide_yelp2018", "batch_size": B, "neg_times": NEG_TIMES, "repeats": a.repeats,
           "measured_on": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
           "step_ms": "training epoch / batches, loader included", "widths": {}}
    for H in WIDE:
        # a fresh process per width, under its own time limit; a failure ends the run
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(H),
                            "--repeats", str(a.repeats)], capture_output=True, text=True)
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"H = {H} failed (exit {p.returncode}); stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            return 1
        res["widths"][str(H)] = json.loads(line[0][7:])
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
