#!/usr/bin/env python3
"""BPR-MF at the wide embedding widths (256 / 512 / 1024), Yelp2018 shape (31,668 users x 38,048 items): the time of
a training step at 32 / 4,096 / 65,536 triplets next to the float-atomic bound of DESIGN 4.9, and the fused
evaluation of all users at k = 10 in both precisions, cold and hinted, next to the executed-flop share of the matrix
peak and to the same build's D = 128 time.  Medians of interleaved repeats, warm-up excluded.  Every measurement
runs in a child process of its own under a time limit; the first one that fails ends the run.

    python scripts/bench_mf_wide.py [--repeats 7] [--out profiles/mf_wide_yelp2018.json]
"""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NU, NI = 31668, 38048
WIDE = (256, 512, 1024)
BATCHES = (32, 4096, 65536)
F32_PEAK, BF16_PEAK = 157.3e12, 2516.6e12      # MI355X dense matrix peaks (v_mfma_f32_32x32x2_f32 / ..x16_bf16)
ATOMIC_BYTES_PER_S = 1.3e12                    # memory-side float atomics, added bytes


def _events(fn, inner):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def _interleaved(fns, repeats, inner, warmup=2):
    """{name: median seconds per call}; the candidates take turns inside every repeat."""
    import torch
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            samples[k].append(_events(fn, inner))
    return {k: statistics.median(v) for k, v in samples.items()}


def child_step(d, repeats):
    import torch
    from yelprecommendation_amd.bpr_step import BPRMFStep
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    U = (torch.rand(NU, d, generator=g, device=dev) - 0.5) * 0.05
    I = (torch.rand(NI, d, generator=g, device=dev) - 0.5) * 0.05
    step = BPRMFStep(U, I, lr=1e-3, impl="auto")
    fns = {}
    for B in BATCHES:
        u = torch.randint(0, NU, (B,), generator=g, device=dev)
        p = (torch.rand(B, generator=g, device=dev).pow(3) * NI).long().clamp_(max=NI - 1)
        n = torch.randint(0, NI, (B,), generator=g, device=dev)
        fns[B] = (lambda u=u, p=p, n=n: step.step(u, p, n))
    t = _interleaved(fns, repeats, inner=10)
    step.check()
    out = {}
    for B in BATCHES:
        bound = B * 3 * 4 * d / ATOMIC_BYTES_PER_S         # three rows of 4 D bytes added per triplet
        out[f"b{B}"] = {"step_us": round(t[B] * 1e6, 1), "atomic_bound_us": round(bound * 1e6, 2),
                        "ratio_to_bound": round(t[B] / bound, 2), "g_triplets_per_s": round(B / t[B] * 1e-9, 4)}
    return out


def child_eval(d, repeats):
    import torch
    from yelprecommendation_amd import engine
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(2)
    users = torch.arange(NU, device=dev)
    deg = 40
    ptr = torch.arange(NU + 1, device=dev, dtype=torch.int64) * deg
    idx = engine.sort_mask_rows(ptr, torch.randint(0, NI, (NU * deg,), generator=g, device=dev))
    tabs = {}
    for dd in (d, 128):
        tabs[dd] = ((torch.rand(NU, dd, generator=g, device=dev) - 0.5) * 0.1,
                    (torch.rand(NI, dd, generator=g, device=dev) - 0.5) * 0.1)
    fns = {}
    for dd, (U, I) in tabs.items():
        for prec in ("f32", "bf16x3"):
            hint = engine.mf_eval_topk(U, I, users, ptr, idx, 10, precision=prec)
            fns[(dd, prec, "cold")] = (lambda U=U, I=I, prec=prec: engine.mf_eval_topk(U, I, users, ptr, idx, 10, precision=prec))
            fns[(dd, prec, "hinted")] = (lambda U=U, I=I, prec=prec, hint=hint:
                                         engine.mf_eval_topk(U, I, users, ptr, idx, 10, precision=prec, hint=hint))
    t = _interleaved(fns, repeats, inner=2, warmup=1)
    out = {}
    for prec in ("f32", "bf16x3"):
        for kind in ("cold", "hinted"):
            s, base = t[(d, prec, kind)], t[(128, prec, kind)]
            flops = 2.0 * NU * NI * d * (6 if prec == "bf16x3" else 1)
            out[f"{prec}_{kind}"] = {"ms": round(s * 1e3, 3), "d128_ms": round(base * 1e3, 3),
                                     "ratio_to_d128": round(s / base, 2), "expected_ratio": d // 128,
                                     "fraction_of_matrix_peak": round(flops / s / (BF16_PEAK if prec == "bf16x3" else F32_PEAK), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mf_wide_yelp2018.json"))
    ap.add_argument("--child", nargs=2, metavar=("KIND", "D"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per measurement process")
    a = ap.parse_args()
    if a.child:
        kind, d = a.child[0], int(a.child[1])
        print("RESULT " + json.dumps((child_step if kind == "step" else child_eval)(d, a.repeats)))
        return 0
    import torch
    res = {"workload": "mf_wide_yelp2018", "shape": [NU, NI], "k": 10, "repeats": a.repeats,
           "measured_on": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
           "atomic_bound": "3 rows x 4 D bytes per triplet at 1.3 TB/s of added bytes (derived, DESIGN 4.9)", "widths": {}}
    for d in WIDE:
        res["widths"][str(d)] = {}
        for kind in ("step", "eval"):
            # a fresh process per measurement, under its own time limit; a failure ends the run
            p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", kind,
                                str(d), "--repeats", str(a.repeats)], capture_output=True, text=True)
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(f"{kind} at D = {d} failed (exit {p.returncode}); stopping\n{p.stderr[-2000:]}", file=sys.stderr)
                return 1
            res["widths"][str(d)][kind] = json.loads(line[0][7:])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
