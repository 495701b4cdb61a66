#!/usr/bin/env python3
"""CDAE without negative sampling (plain BCE over every catalogue position) at the hidden sizes 64 / 128, Yelp2018
shape (31,668 users x 38,048 items, 47 interactions per user, batches of 256 rows): a training epoch and a validation
pass of CDAETrainer on two routes —

    lists   batches as lists straight from the per-user CSR; the step takes the catalogue sweep (yr_cdae_catalogue_bce:
            no [B, I] array), validation one loss-only sweep over all users and the fused top-k (what train.py
            fast_loader=true negative_sampling=false runs at these widths)
    dense   list_batches=false: dense [B, I] rows from the loader, the dense decoder (a [B, I] gradient array, three
            products, a compaction pass), per-batch full-catalogue validation

as milliseconds per step (epoch / batches: the loader's work is part of the route), per validation pass, and the peak
device memory of each; beside them the sweep's own time (device events) for a training batch (four products of
2 B I H flops: the pre-activations twice, dz, dW_o) and for the validation pass (one product over all users), with its
TFLOP/s against the 157.3 TFLOP/s f32 matrix peak.  Medians of interleaved repeats, warm-up excluded.  Every width runs
in a child process of its own under a time limit; the first one that fails ends the run.

    python scripts/bench_cdae_plain.py [--repeats 5] [--out profiles/cdae_plain_bce_yelp2018.json]
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

WIDTHS = (64, 128)
B = 256
PEAK_F32_MATRIX_TFLOPS = 157.3


def child(H, repeats):
    import torch
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.data.cdae_batches import CDAEBatchLoader, CDAEInteractions
    from yelprecommendation_amd.data.synthetic import YELP2018_ITEMS as NI, YELP2018_USERS as NU, make_interactions_torch
    from yelprecommendation_amd.trainers import CDAETrainer
    from yelprecommendation_amd.utils import make_config
    dev = torch.device("cuda")
    u, i = make_interactions_torch(NU, NI, 47.0, seed=1234, device=dev)
    data = CDAEInteractions.from_interactions(u, i, NU, NI, seed=1, device=dev)
    tmp = tempfile.mkdtemp(prefix="yr_cdae_plain.")
    routes = {}
    for name in ("lists", "dense"):
        lists = name == "lists"
        cfg = make_config("CDAE", hidden_size=H, device="cuda", model_dir=tmp, lr=1e-4, batch_size=B, eval_batch_group=32,
                          negative_sampling=False, loss_name="bce", top_n=10, list_batches=lists)
        torch.manual_seed(1)
        trainer = CDAETrainer(cfg, NI, NU)
        step = trainer._fused_step()
        assert step.decoder == "dense" and step.catalogue
        train = CDAEBatchLoader(data, "train", B, shuffle=True, seed=3, lists=lists, dropout=trainer.model.corruption_level,
                                negative_sampling=False)
        valid = CDAEBatchLoader(data, "valid", B, shuffle=False, seed=4, lists=lists, negative_sampling=False)
        routes[name] = (trainer, train, valid)
    steps = -(-NU // B)
    fns = {}
    for name, (trainer, train, valid) in routes.items():
        fns[(name, "step_ms")] = (lambda trainer=trainer, train=train: trainer.train(train))
        fns[(name, "validate_ms")] = (lambda trainer=trainer, valid=valid: trainer.validate(valid))
    samples = {k: [] for k in fns}
    peak = {k: 0 for k in fns}
    for r in range(repeats + 1):                       # repeat 0 is the warm-up
        for k, fn in fns.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r > 0:
                samples[k].append((time.perf_counter() - t0) * 1e3 / (steps if k[1] == "step_ms" else 1))
                peak[k] = max(peak[k], torch.cuda.max_memory_allocated())
    out = {name: {what: round(statistics.median(samples[(name, what)]), 4) for what in ("step_ms", "validate_ms")}
           for name in routes}
    for name in routes:
        out[name]["epoch_plus_validate_ms"] = round(out[name]["step_ms"] * steps + out[name]["validate_ms"], 3)
        out[name]["peak_memory_mb"] = {what: round(peak[(name, what)] / 2 ** 20, 1) for what in ("step_ms", "validate_ms")}
    out["dense_over_lists"] = {what: round(out["dense"][what] / out["lists"][what], 2)
                               for what in ("step_ms", "validate_ms", "epoch_plus_validate_ms")}
    out["steps_per_epoch"] = steps

    # the sweep alone, by device events: a training batch (loss + three gradients) and the validation pass (loss only)
    model = routes["lists"][0].model
    Wo, bo = model.output_layer.weight.data, model.output_layer.bias.data
    act = model._output_act
    sweeps = {}
    for what, rows, part, grads, products in (("train_batch", B, "train", True, 4), ("validation_pass", NU, "train_valid", False, 1)):
        users = torch.arange(rows, device=dev)
        z = torch.rand(rows, H, device=dev)
        ptr, idx = data.csr(part)
        n = engine.cdae_catalogue_bce_workspace_floats(rows, NI, H)
        ws = torch.empty(n if grads else n // (1 + H), dtype=torch.float32, device=dev)
        ms = []
        for r in range(repeats + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            engine.cdae_catalogue_bce(z, Wo, bo, users, ptr, idx, act, grads=grads, workspace=ws)
            e1.record()
            torch.cuda.synchronize()
            if r > 1:
                ms.append(e0.elapsed_time(e1))
        t = statistics.median(ms)
        tf = products * 2.0 * rows * NI * H / (t * 1e-3) / 1e12
        sweeps[what] = {"ms": round(t, 4), "products_of_2BIH_flops": products, "tflops": round(tf, 2),
                        "of_f32_matrix_peak": round(tf / PEAK_F32_MATRIX_TFLOPS, 3)}
    out["sweep"] = sweeps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdae_plain_bce_yelp2018.json"))
    ap.add_argument("--child", type=int, metavar="H")
    ap.add_argument("--limit", type=int, default=300, help="seconds per measurement process")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.child, a.repeats)))
        return 0
    import torch
    res = {"workload": "cdae_plain_bce_yelp2018", "batch_size": B, "negative_sampling": False, "repeats": a.repeats,
           "measured_on": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
           "script": "scripts/bench_cdae_plain.py", "step_ms": "training epoch / batches, loader included",
           "f32_matrix_peak_tflops": PEAK_F32_MATRIX_TFLOPS, "widths": {}}
    for H in WIDTHS:
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
