#!/usr/bin/env python3
"""What deterministic=true costs a CDAE training step on list batches, Yelp2018 shape (31,668 users x 38,048 items, 47
interactions per user, batches of 256 rows, neg_times 5, NS-BCE) at the hidden sizes 64 / 128 / 512 / 1024:

    default         the sampled decoder and the fused hidden backward with their global float atomics
    deterministic   csrc/cdae_owned.hip: entries sorted by column, every gradient summed by its owner in row order

as milliseconds per step (one CDAETrainer.train epoch / batches: the loader's work is part of both).  A warm-up epoch,
then ``--windows`` epochs per mode, the two modes ALTERNATED inside one process; median, minimum and maximum of the
windows.  The warm-up epochs double as the equality check at the timed size: two deterministic trainers from one seed
must end their epoch with torch.equal parameters (the script fails otherwise).  Every width runs in a child process of
its own under a time limit; the first one that fails ends the run.

    python scripts/bench_cdae_deterministic.py [--windows 7] [--out profiles/cdae_deterministic_yelp2018.json]
    python scripts/bench_cdae_deterministic.py --modes default --out OTHER.json     # a commit without the mode
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

WIDTHS = (64, 128, 512, 1024)
B, NEG_TIMES = 256, 5


def child(H, windows, modes):
    import torch
    from yelprecommendation_amd.data.cdae_batches import CDAEBatchLoader, CDAEInteractions
    from yelprecommendation_amd.data.synthetic import YELP2018_ITEMS as NI, YELP2018_USERS as NU, make_interactions_torch
    from yelprecommendation_amd.trainers import CDAETrainer
    from yelprecommendation_amd.utils import make_config
    dev = torch.device("cuda")
    u, i = make_interactions_torch(NU, NI, 47.0, seed=1234, device=dev)
    data = CDAEInteractions.from_interactions(u, i, NU, NI, seed=1, device=dev)
    tmp = tempfile.mkdtemp(prefix="yr_cdae_det.")

    def make(mode):
        over = {"deterministic": True} if mode == "deterministic" else {}
        cfg = make_config("CDAE", hidden_size=H, device="cuda", model_dir=tmp, lr=1e-4, batch_size=B,
                          negative_sampling=True, neg_times=NEG_TIMES, loss_name="bce", top_n=10, **over)
        torch.manual_seed(1)
        trainer = CDAETrainer(cfg, NI, NU)
        loader = CDAEBatchLoader(data, "train", B, NEG_TIMES, shuffle=True, seed=3, lists=True,
                                 dropout=trainer.model.corruption_level)
        return trainer, loader

    def epoch(trainer, loader):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = trainer.train(loader)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, loss

    steps = -(-NU // B)
    runs = {m: make(m) for m in modes}
    out = {"steps_per_epoch": steps}
    warm = {m: epoch(*runs[m]) for m in modes}                     # warm-up, not timed
    if "deterministic" in modes:
        # the same first epoch from the same seed on a second trainer: every parameter bit for bit
        again, loader = make("deterministic")
        _, loss = epoch(again, loader)
        first = runs["deterministic"][0]
        assert getattr(first._fused_step(), "deterministic", False), "the deterministic trainer does not run the mode"
        same = loss == warm["deterministic"][1] and all(
            torch.equal(a, b) for a, b in zip(first.model.state_dict().values(), again.model.state_dict().values()))
        assert same, "two deterministic epochs from one seed differ"
        out["deterministic_epochs_bit_equal"] = True
        del again, loader
    samples = {m: [] for m in modes}
    for _ in range(windows):
        for m in modes:                                            # alternated: drift hits both alike
            samples[m].append(epoch(*runs[m])[0] / steps)
    for m in modes:
        s = samples[m]
        out[m] = {"step_ms": round(statistics.median(s), 4), "min": round(min(s), 4), "max": round(max(s), 4), "windows": len(s)}
    if len(modes) == 2:
        out["deterministic_over_default"] = round(out["deterministic"]["step_ms"] / out["default"]["step_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--modes", default="default,deterministic")
    ap.add_argument("--widths", default=",".join(str(h) for h in WIDTHS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdae_deterministic_yelp2018.json"))
    ap.add_argument("--child", type=int, metavar="H")
    ap.add_argument("--limit", type=int, default=240, help="seconds per measurement process")
    a = ap.parse_args()
    modes = tuple(a.modes.split(","))
    assert a.windows >= 5 and set(modes) <= {"default", "deterministic"}
    if a.child:
        print("RESULT " + json.dumps(child(a.child, a.windows, modes)))
        return 0
    import torch
    res = {"workload": "cdae_deterministic_yelp2018", "batch_size": B, "neg_times": NEG_TIMES, "windows": a.windows,
           "measured_on": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
           "step_ms": "training epoch / batches, loader included; median, min and max over the windows", "widths": {}}
    for H in (int(h) for h in a.widths.split(",")):
        # a fresh process per width, under its own time limit; a failure ends the run
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(H),
                            "--windows", str(a.windows), "--modes", a.modes], capture_output=True, text=True)
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"H = {H} failed (exit {p.returncode}); stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            return 1
        res["widths"][str(H)] = json.loads(line[0][7:])
        print(H, res["widths"][str(H)], flush=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
