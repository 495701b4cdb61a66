"""Two builds of the engine library on the paths that run yr_cdae_train_lists, at Yelp2018 size, alternating:

    python scratch/cdae_lists_ab.py LIB_A LIB_B [runs per library, default 3]

Every run is a fresh process (YR_ENGINE_LIB selects the library) that times, as medians over repeated calls, the list
kernel alone over 4,096 rows (scratch/lists_time.py), CDAETrainer.validate() and .evaluate() over list batches
(scratch/cdae_valid_epoch.py) and the fused training step of bench.py --workload cdae.  The parent prints every raw
figure, the medians per library and library A's own spread (max - min), the yardstick for "B is not slower than A".
The first child that fails ends the run."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("lists_us", "validate_ms", "evaluate_ms", "step_ms")


def child():
    sys.path.insert(0, ROOT)
    import torch
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.cdae_step import CDAEStep
    from yelprecommendation_amd.data.cdae_batches import CDAEBatchLoader, CDAEInteractions
    from yelprecommendation_amd.data.synthetic import YELP2018_ITEMS as NI, YELP2018_USERS as NU, make_interactions_torch
    from yelprecommendation_amd.models.cdae import CDAE
    from yelprecommendation_amd.optim import Adam
    from yelprecommendation_amd.trainers import CDAETrainer
    from yelprecommendation_amd.utils import make_config

    dev = torch.device("cuda")
    u, i = make_interactions_torch(NU, NI, 47.0, seed=1234, device=dev)
    data = CDAEInteractions.from_interactions(u, i, NU, NI, seed=1, device=dev)

    def median_of(fn, reps, calls=1, warmup=2):
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / calls)
        return statistics.median(ts)

    out = {}
    users = torch.randperm(NU, device=dev)[:4096].contiguous()
    ptr, idx = data.csr("train")
    extra, pool = data.csr("valid"), {}
    out["lists_us"] = 1e6 * median_of(
        lambda: engine.TrainLists(ptr, idx, users, NU, NI, 5, 11, 12, 0.0, extra=extra, pool=pool), reps=15, calls=20)

    B = 256
    cfg = make_config("CDAE", hidden_size=128, device="cuda", model_dir="/tmp/yr_cdae_epoch", lr=1e-4, batch_size=B,
                      eval_batch_group=32, negative_sampling=True, neg_times=5, loss_name="bce", top_n=10)
    trainer = CDAETrainer(cfg, NI, NU)
    valid = CDAEBatchLoader(data, "valid", batch_size=B, neg_times=5, seed=4, lists=True)
    test = CDAEBatchLoader(data, "test", batch_size=B, seed=5, lists=True)
    out["validate_ms"] = 1e3 * median_of(lambda: trainer.validate(valid), reps=15)
    out["evaluate_ms"] = 1e3 * median_of(lambda: trainer.evaluate(test), reps=15)

    # the step of bench.py --workload cdae (dense batch in, decoder on the loss positions)
    model = CDAE(make_config("CDAE", hidden_size=128, device="cuda", model_dir="/tmp/yr_bench", lr=1e-4), NI, NU)
    model.train()
    fused, k = CDAEStep(model, Adam(model.parameters(), lr=1e-4), True, decoder="sampled", transposed_wh=True), [0]
    bu = torch.randperm(NU, device=dev)[:B]
    x = (torch.rand(B, NI, device=dev) < 0.0008).float()
    neg = (torch.rand(B, NI, device=dev) < 0.004).float() * (1 - x)

    def step():
        k[0] += 1
        fused.step(bu, x, neg, seed=k[0], p=model.corruption_level)
    out["step_ms"] = 1e3 * median_of(step, reps=15, calls=20, warmup=10)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    libs = {"A": os.path.abspath(sys.argv[1]), "B": os.path.abspath(sys.argv[2])}
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    got = {name: [] for name in libs}
    for r in range(runs):
        for name, lib in libs.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True,
                               env=dict(os.environ, YR_ENGINE_LIB=lib), timeout=240)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-2000:], p.stderr[-2000:], sep="\n")
                sys.exit(f"run {r} of library {name} failed with status {p.returncode}: stopping")
            res = json.loads(line[0][7:])
            got[name].append(res)
            print(f"run {r} {name} " + "  ".join(f"{key} {res[key]:.3f}" for key in KEYS), flush=True)
    for name, lib in libs.items():
        print(f"{name} = {lib}")
    for key in KEYS:
        a, b = ([res[key] for res in got[name]] for name in ("A", "B"))
        spread, delta = max(a) - min(a), statistics.median(b) - statistics.median(a)
        print(f"{key}: median A {statistics.median(a):.3f}  B {statistics.median(b):.3f}  B - A {delta:+.3f}  "
              f"spread of A {spread:.3f}  -> {'ok' if delta <= spread else 'B SLOWER'}")


if __name__ == "__main__":
    child() if sys.argv[1:] == ["--child"] else main()
