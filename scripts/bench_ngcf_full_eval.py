#!/usr/bin/env python3
"""NGCF full-catalogue evaluation at Yelp2018 shape (31,668 users x 38,048 items, embed_size 64, num_orders 2: three
layer tables, W = 192, top_n 10) on the synthetic graph of data/synthetic.py, next to the two other routes to the same
lists on the same GPU.  Writes profiles/ngcf_full_eval_yelp2018.json and prints it as one line.

    python scripts/bench_ngcf_full_eval.py [--windows 7] [--warmup 2] [--reps 5]

Medians over ``--windows`` windows after ``--warmup``; in every window the routes run one after the other (alternating),
each ``--reps`` times between two device events (the figure is the time per call):
* ``sweep_cold_ms`` / ``sweep_hinted_ms``   (a) engine.ngcf_eval_topk over all users, without a hint and with the previous
                       lists as hints (the model has not moved: the best case of a hint); flops 2 x rows x items x W
                       against the f32 matrix peak (the peak is the data sheet's figure, not measured);
* ``dense``            (b) the parent commit's only route to all users: per chunk of 4,096 users and per layer
                       ``mf_scores_gemm``, ``_iadd``, then ``topk_masked``;
* ``concat``           (c) ``torch.cat`` of the layers zero-padded to 256 columns (``copy_ms``) through
                       ``mf_eval_topk(precision="f32")`` (``sweep_cold_ms`` / ``sweep_hinted_ms``);
* ``propagate_ms``     (d) ``NGCF.propagate`` alone;
* ``evaluate_full_ms`` (e) ``NGCFTrainer.evaluate_full`` end to end (host clock, ends in the read-back of the metrics;
                       hints from the previous call);
* peak device memory of (a), (b) and (c) above what is resident.
The three routes must agree except at float near-ties (f32 summation orders); the rows that differ are counted.
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

EMBED, ORDERS, TOP_N = 64, 2, 10
PEAK_F32_MATRIX_TFLOPS = 157.3          # data sheet (MI355X f32 matrix), as scripts/bench_s3rec_full_eval.py uses it
DENSE_CHUNK = 4096
PAD_WIDTH = 256


def _setup(dev):
    """Trainer over the synthetic Yelp2018 graph and an eval frame of ALL users: mask = the user's interactions but
    the last one, pos = that last one."""
    from yelprecommendation_amd.data.synthetic import YELP2018_ITEMS as NI, YELP2018_USERS as NU, make_interactions_torch
    from yelprecommendation_amd.graph import LaplacianCSR
    from yelprecommendation_amd.trainers import NGCFTrainer
    from yelprecommendation_amd.utils import make_config, set_seed
    u, i = make_interactions_torch(NU, NI, 47.0, device=dev)
    u, i = u.cpu().numpy(), i.cpu().numpy()
    r = np.random.RandomState(0).randint(1, 6, u.shape[0])
    graph = LaplacianCSR.from_interactions(u, i, r, NU, NI, dev)
    order = np.argsort(u, kind="stable")
    u, i = u[order], i[order]
    starts = np.searchsorted(u, np.arange(NU + 1))
    ids = np.flatnonzero(starts[1:] - starts[:-1] >= 2)
    pos = [[int(i[starts[x + 1] - 1])] for x in ids]
    masks = [i[starts[x]:starts[x + 1] - 1].tolist() for x in ids]
    frame = pd.DataFrame({"pos_items": pos, "mask_items": masks}, index=ids)
    set_seed(0)
    cfg = make_config("NGCF", embed_size=EMBED, num_orders=ORDERS, device="cuda", top_n=TOP_N,
                      model_dir=tempfile.mkdtemp(prefix="yr_bench_ngcf_full_eval."))
    return NGCFTrainer(cfg, NI, NU, graph), graph, frame, NU, NI


def _median(runs):
    return round(statistics.median(runs), 4)


def dense_route(layers, nu, users, ptr, idx, k):
    """(b): the dense route of NGCFTrainer.recommend as the parent commit has it, in chunks of 4,096 users."""
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.models.ngcf import _iadd
    n = users.numel()
    out = torch.empty((n, k), dtype=torch.int64, device=users.device)
    rows = torch.arange(n, dtype=torch.int64, device=users.device)
    for lo in range(0, n, DENSE_CHUNK):
        hi = min(lo + DENSE_CHUNK, n)
        chunk = users[lo:hi].contiguous()
        scores = None
        for E in layers:
            s = engine.mf_scores_gemm(E[:nu], E[nu:], chunk)
            scores = s if scores is None else _iadd(scores, s)
        engine.topk_masked(scores, ptr, idx, k, out=out[lo:hi], mask_rows=rows[lo:hi])
    return out


def concat_tables(layers):
    """(c), the copy: the layers side by side, zero-padded to a width the one-table sweep takes."""
    cat = torch.zeros((layers[0].shape[0], PAD_WIDTH), dtype=torch.float32, device=layers[0].device)
    cat[:, :len(layers) * layers[0].shape[1]] = torch.cat(layers, 1)
    return cat


def bench(a):
    from yelprecommendation_amd import engine
    dev = torch.device("cuda")
    trainer, graph, frame, NU, NI = _setup(dev)
    model = trainer.model.eval()
    users, ptr, idx = trainer._eval_sets.eval_set(frame, sort_masks=True)[2:5]
    n, k, W = users.numel(), TOP_N, EMBED * (ORDERS + 1)
    res = {"workload": "ngcf_yelp2018_full_eval", "shape": [NU, NI, EMBED, ORDERS, k], "eval_rows": n, "width": W,
           "mask_entries": int(idx.numel()), "graph_nnz": int(graph.nnz), "windows": a.windows, "warmup": a.warmup,
           "reps": a.reps, "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        layers = model.propagate(graph)
        pieces = {
            "sweep_cold": lambda st: st.__setitem__("a", engine.ngcf_eval_topk(layers, NU, users, ptr, idx, k)),
            "sweep_hinted": lambda st: engine.ngcf_eval_topk(layers, NU, users, ptr, idx, k, hint=st["a"]),
            "dense": lambda st: st.__setitem__("b", dense_route(layers, NU, users, ptr, idx, k)),
            "concat_copy": lambda st: st.__setitem__("cat", concat_tables(layers)),
            "concat_sweep_cold": lambda st: st.__setitem__("c", engine.mf_eval_topk(
                st["cat"][:NU], st["cat"][NU:], users, ptr, idx, k, precision="f32")),
            "concat_sweep_hinted": lambda st: engine.mf_eval_topk(
                st["cat"][:NU], st["cat"][NU:], users, ptr, idx, k, precision="f32", hint=st["c"]),
            "propagate": lambda st: model.propagate(graph),
        }
        ms = {name: [] for name in pieces}
        st = {}
        for it in range(a.warmup + a.windows):
            for name, fn in pieces.items():
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record()
                for _ in range(a.reps):
                    fn(st)
                e1.record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1) / a.reps)
        # peak memory above what is resident, each route alone
        got_a, got_b, got_c = st["a"], st["b"], st["c"]
        st.clear()
        for name, fn in (("sweep_peak_mib", lambda: engine.ngcf_eval_topk(layers, NU, users, ptr, idx, k)),
                         ("dense_peak_mib", lambda: dense_route(layers, NU, users, ptr, idx, k)),
                         ("concat_peak_mib", lambda: (lambda cat: engine.mf_eval_topk(
                             cat[:NU], cat[NU:], users, ptr, idx, k, precision="f32"))(concat_tables(layers)))):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            res[name] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)
        res["rows_where_sweep_and_dense_differ"] = int((got_a != got_b).any(1).sum())
        res["rows_where_sweep_and_concat_differ"] = int((got_a != got_c).any(1).sum())
    flops = 2.0 * n * NI * W
    for name, runs in ms.items():
        res[name + "_ms"], res[name + "_ms_windows"] = _median(runs), [round(v, 4) for v in runs]
    res["sweep_matrix_gflop"] = round(flops / 1e9, 2)
    for form in ("cold", "hinted"):
        tf = flops / (res[f"sweep_{form}_ms"] * 1e-3) / 1e12
        res[f"sweep_{form}_tflops"] = round(tf, 2)
        res[f"sweep_{form}_of_f32_matrix_peak"] = round(tf / PEAK_F32_MATRIX_TFLOPS, 4)
    res["f32_matrix_peak_tflops_data_sheet_not_measured"] = PEAK_F32_MATRIX_TFLOPS
    res["concat_total_cold_ms"] = round(res["concat_copy_ms"] + res["concat_sweep_cold_ms"], 4)
    res["concat_total_hinted_ms"] = round(res["concat_copy_ms"] + res["concat_sweep_hinted_ms"], 4)
    res["dense_over_sweep_cold"] = round(res["dense_ms"] / res["sweep_cold_ms"], 2)
    res["concat_total_cold_over_sweep_cold"] = round(res["concat_total_cold_ms"] / res["sweep_cold_ms"], 3)
    res["concat_sweep_cold_over_sweep_cold"] = round(res["concat_sweep_cold_ms"] / res["sweep_cold_ms"], 3)
    res["dense_chunk_users"] = DENSE_CHUNK
    # (e) evaluate_full end to end
    runs = []
    for it in range(a.warmup + a.windows):
        torch.cuda.synchronize()
        t = time.perf_counter()
        four = trainer.evaluate_full(frame)
        runs.append((time.perf_counter() - t) * 1e3)
    runs = runs[a.warmup:]
    res["evaluate_full_ms"], res["evaluate_full_ms_windows"] = _median(runs), [round(v, 3) for v in runs]
    res["evaluate_full_metrics_untrained"] = [round(v, 6) for v in four]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ngcf_full_eval_yelp2018.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ngcf_full_eval: no GPU (there is no CPU path to time)")
    if a.windows < 5:
        raise SystemExit("bench_ngcf_full_eval: at least 5 windows")
    res = bench(a)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
