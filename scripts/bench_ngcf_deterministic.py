#!/usr/bin/env python3
"""What deterministic=true costs the fused NGCF training step, Yelp2018 shape (31,668 users + 38,048 items, 47
interactions per user, D = 64, three propagation layers, Adam) at batches of 32, 4,096 and 65,536 triplets:

    default         yr_ngcf_bpr_step: float atomics in the score gradient, dW and the push product; row sets listed in
                    arrival order
    deterministic   yr_ngcf_bpr_step_ordered (csrc/ngcf_owned.hip): owner passes, ordered row sets, pull product only

as milliseconds per step (``--steps`` NGCFStep.step calls on one batch between two device synchronisations).  Warm-up
steps, then ``--windows`` windows per mode, the two modes ALTERNATED inside one process; median, minimum and maximum of
the windows, and the workspace bytes of both modes.  The warm-up doubles as the equality check at the timed size: two
deterministic steps objects from one seed must agree bit for bit in every parameter after it (the script fails
otherwise).  Every batch size runs in a child process of its own under a time limit; the first one that fails ends
the run.

    python scripts/bench_ngcf_deterministic.py [--windows 7] [--out profiles/ngcf_deterministic_yelp2018.json]
    python scripts/bench_ngcf_deterministic.py --trace 4096 deterministic     # 60 steps for a kernel trace, no timing

``--bench-this`` / ``--bench-parent``: files of ``bench.py --workload ngcf`` result lines (this commit, the parent
commit, alternated in one session) — folded into the profile as ``default_mode``: every figure, the medians, the parent's
own spread and whether this commit's median is at most the parent's slowest repeat.
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

BATCHES = (32, 4096, 65536)
DIM, LAYERS = 64, 3


def _make(B):
    import torch
    from yelprecommendation_amd.data.synthetic import YELP2018_ITEMS as NI, YELP2018_USERS as NU, make_interactions_torch
    from yelprecommendation_amd.graph import LaplacianCSR
    from yelprecommendation_amd.models.ngcf import NGCF
    from yelprecommendation_amd.ngcf_step import NGCFStep
    from yelprecommendation_amd.optim import Adam
    from yelprecommendation_amd.utils import make_config
    dev = torch.device("cuda")
    u, i = make_interactions_torch(NU, NI, 47.0, seed=1234, device=dev)
    r = torch.randint(1, 6, u.shape, device=dev)
    graph = LaplacianCSR.from_interactions(u.cpu().numpy(), i.cpu().numpy(), r.cpu().numpy(), NU, NI, dev)
    cfg = make_config("NGCF", embed_size=DIM, num_orders=LAYERS, device="cuda", model_dir=tempfile.mkdtemp(prefix="yr_ngcf_det."))
    g = torch.Generator(device=dev).manual_seed(5)
    # batches as a loader over the train rows yields them: (user, one of its items, uniform negative)
    pick = torch.randint(0, u.numel(), (B,), device=dev, generator=g)
    batch = (u[pick].contiguous(), i[pick].contiguous(), torch.randint(0, NI, (B,), device=dev, generator=g))

    def make(mode):
        torch.manual_seed(1)
        model = NGCF(cfg, NU, NI).to(dev)
        opt = Adam(model.parameters(), lr=1e-4)
        return model, NGCFStep(model, opt, graph, model._subset_fraction(), deterministic=mode == "deterministic")
    return make, batch


def child(B, windows, steps, warmup, modes):
    import torch
    make, batch = _make(B)

    def window(step, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step.step(*batch)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    runs = {m: make(m) for m in modes}
    out = {}
    for m in modes:                                                # warm-up, not timed
        window(runs[m][1], warmup)
        runs[m][1].check()
        out[m + "_workspace_bytes"] = int(runs[m][1]._ws.numel())
    if "deterministic" in modes:
        model2, again = make("deterministic")
        window(again, warmup)
        same = all(torch.equal(a, b) for a, b in zip(runs["deterministic"][0].state_dict().values(), model2.state_dict().values()))
        assert again.deterministic and same, "two deterministic runs from one seed differ"
        out["deterministic_runs_bit_equal"] = True
        del model2, again
    samples = {m: [] for m in modes}
    for _ in range(windows):
        for m in modes:                                            # alternated: drift hits both alike
            samples[m].append(window(runs[m][1], steps))
    for m in modes:
        s = samples[m]
        out[m] = {"step_ms": round(statistics.median(s), 4), "min": round(min(s), 4), "max": round(max(s), 4), "windows": len(s)}
    if len(modes) == 2:
        out["deterministic_over_default"] = round(out["deterministic"]["step_ms"] / out["default"]["step_ms"], 3)
    return out


def trace(B, mode):
    """60 steps after 10 of warm-up, for a kernel trace taken around this process."""
    import torch
    make, batch = _make(B)
    _, step = make(mode)
    for _ in range(70):
        step.step(*batch)
    torch.cuda.synchronize()
    step.check()


def _bench_lines(path):
    vals = []
    for line in open(path):
        line = line.strip()
        if line.startswith("{"):
            vals.append(json.loads(line))
    return vals


def default_mode(this_path, parent_path):
    """bench.py --workload ngcf (the autograd route over the default kernels) on both commits."""
    out = {"source": "bench.py --workload ngcf, both commits alternated in one session; ms per step"}
    for key in ("4096", "32", "4096_whole_graph", "32_whole_graph"):
        this = [r["step_ms"][key] for r in _bench_lines(this_path)]
        parent = [r["step_ms"][key] for r in _bench_lines(parent_path)]
        out[key] = {"this": this, "parent": parent, "this_median": statistics.median(this),
                    "parent_median": statistics.median(parent), "parent_spread": [min(parent), max(parent)],
                    "this_over_parent": round(statistics.median(this) / statistics.median(parent), 4),
                    "this_median_at_most_parent_max": statistics.median(this) <= max(parent)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=300, help="steps per window")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--modes", default="default,deterministic")
    ap.add_argument("--batches", default=",".join(str(b) for b in BATCHES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ngcf_deterministic_yelp2018.json"))
    ap.add_argument("--child", type=int, metavar="B")
    ap.add_argument("--trace", nargs=2, metavar=("B", "MODE"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per measurement process")
    ap.add_argument("--bench-this")
    ap.add_argument("--bench-parent")
    a = ap.parse_args()
    modes = tuple(a.modes.split(","))
    assert a.windows >= 5 and set(modes) <= {"default", "deterministic"}
    if a.trace:
        trace(int(a.trace[0]), a.trace[1])
        return 0
    if a.child is not None:
        print("RESULT " + json.dumps(child(a.child, a.windows, a.steps, a.warmup, modes)))
        return 0
    import torch
    res = {"workload": "ngcf_deterministic_yelp2018", "embed_size": DIM, "layers": LAYERS, "windows": a.windows,
           "steps_per_window": a.steps, "measured_on": datetime.date.today().isoformat(),
           "device": torch.cuda.get_device_name(0),
           "step_ms": "NGCFStep.step on one batch, host clock around a window that ends in a device synchronise; "
                      "median, min and max over the windows", "batches": {}}
    for B in (int(b) for b in a.batches.split(",")):
        # a fresh process per batch size, under its own time limit; a failure ends the run
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(B),
                            "--windows", str(a.windows), "--steps", str(a.steps), "--warmup", str(a.warmup),
                            "--modes", a.modes], capture_output=True, text=True)
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"B = {B} failed (exit {p.returncode}); stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            return 1
        res["batches"][str(B)] = json.loads(line[0][7:])
        print(B, res["batches"][str(B)], flush=True)
    if a.bench_this and a.bench_parent:
        res["default_mode"] = default_mode(a.bench_this, a.bench_parent)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
