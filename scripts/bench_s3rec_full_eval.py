#!/usr/bin/env python3
"""S3Rec full-catalogue evaluation at Yelp2018 shape (31,668 sequences, 38,048 items, max_seq_len 50, embed_size 64,
2 heads, 2 blocks) next to the obvious DENSE path of the same model on the same GPU.  Writes
profiles/s3rec_full_eval_yelp2018.json and prints it as one line.

    python scripts/bench_s3rec_full_eval.py [--windows 7] [--warmup 2] [--batch 4096]

Medians over ``--windows`` windows after ``--warmup``, device events around each piece:
* ``encoder_ms``       the ``last_only`` encoder over all sequences (one launch);
* ``rank_sweep_ms``    yr_s3rec_catalogue_rank alone over all rows, the users' histories excluded; its 2 N R E matrix
                       flops against the 157.3 TFLOP/s f32 matrix peak;
* ``list_sweep_ms``    yr_mf_eval_topk alone (10-entry lists, the same histories as mask lists);
* ``dense``            the baseline, run in the same loop alternating with the sweep: per chunk of 4,096 users
                       ``h_last @ item_embedding.weight.T`` (``gemm_ms``), an index-put of the history and the pad
                       (``mask_ms``), then ``(scores > pos).sum(1)`` with the tie term (``count_ms``);
* ``evaluate_full_ms`` ``S3RecTrainer.evaluate_full`` end to end through ``S3RecBatchLoader`` (host clock, ends in the
                       read-back of the metrics);
* peak device memory of the sweep and of the dense path above what is resident.
The dense ranks and the sweep's must agree except at float near-ties (two f32 summation orders); the count of rows that
differ is recorded.
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

import torch  # noqa: E402

NU, NI, L, E, HEADS, BLOCKS = 31668, 38048, 50, 64, 2, 2
PEAK_F32_MATRIX_TFLOPS = 157.3
DENSE_CHUNK = 4096


def _cfg(**kw):
    from yelprecommendation_amd.utils import Config
    base = dict(device="cuda", model_dir=tempfile.mkdtemp(prefix="yr_bench_s3rec_full_eval."), top_n=10, best_metric="loss",
                embed_size=E, max_seq_len=L, num_heads=HEADS, num_blocks=BLOCKS, dropout_ratio=0.1, load_pretrain=False,
                optimizer="adam", lr=1e-3, epochs=1, patience=5, seed=0)
    base.update(kw)
    return Config(**base)


def _store(dev):
    """Behaviour rows of Yelp2018's size: 31,668 users, about 1.5 M interactions, 4 .. 95 per user."""
    from yelprecommendation_amd.data.s3rec_batches import S3RecSequences
    g = torch.Generator().manual_seed(7)
    n = torch.randint(4, 96, (NU,), generator=g)
    users = torch.repeat_interleave(torch.arange(NU), n)
    items = torch.randint(0, NI, (int(n.sum()),), generator=g)
    return S3RecSequences(users.to(dev), items.to(dev), NU, NI, L)


def _events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def _median(runs):
    return round(statistics.median(runs), 4)


def dense_ranks(h_last, W, target, ptr, idx, ev=None):
    """The baseline: chunks of 4,096 users; returns the ranks and, with ``ev``, adds (gemm, mask, count) ms to it."""
    N, R = h_last.shape[0], W.shape[0]
    out = torch.empty(N, dtype=torch.int64, device=h_last.device)
    col = torch.arange(R, device=h_last.device)
    for lo in range(0, N, DENSE_CHUNK):
        hi = min(lo + DENSE_CHUNK, N)
        e = _events(4)
        e[0].record()
        scores = h_last[lo:hi] @ W.T
        e[1].record()
        t = target[lo:hi]
        pos = scores.gather(1, t.clamp(min=0)[:, None])
        a, b = int(ptr[lo]), int(ptr[hi])
        rows = torch.repeat_interleave(torch.arange(hi - lo, device=h_last.device), ptr[lo + 1:hi + 1] - ptr[lo:hi])
        cols = idx[a:b]
        keep = cols != t[rows]                                        # the target is never excluded
        scores.index_put_((rows[keep], cols[keep]), torch.tensor(float("-inf"), device=h_last.device))
        scores[:, 0] = float("-inf")                                  # the pad row
        e[2].record()
        rank = (scores > pos).sum(1) + ((scores == pos) & (col[None, :] < t[:, None])).sum(1)
        out[lo:hi] = torch.where(t >= 1, rank, torch.full_like(rank, -1))
        e[3].record()
        if ev is not None:
            torch.cuda.synchronize()
            for k in range(3):
                ev[k] += e[k].elapsed_time(e[k + 1])
    return out


def bench(a):
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.data.s3rec_batches import S3RecBatchLoader
    from yelprecommendation_amd.trainers.s3rec_trainer import S3RecTrainer
    from yelprecommendation_amd.utils import set_seed
    dev = torch.device("cuda")
    set_seed(0)
    trainer = S3RecTrainer(_cfg(), NI)
    model = trainer.model.eval()
    store = _store(dev)
    ptr, idx = store.history("test")
    X, target, _ = store.draw("test", 0, n_neg=1)
    W = model.item_embedding.weight.detach()
    users = torch.arange(NU, device=dev)
    res = {"workload": "s3rec_yelp2018_full_eval", "shape": [NU, NI, L, E, HEADS, BLOCKS], "history_entries": int(idx.numel()),
           "windows": a.windows, "warmup": a.warmup, "date": time.strftime("%Y-%m-%d"),
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        h_last = model._encode(X, last_only=True)
        # the lists' mask CSR: the same histories, 0-based in weight[1:]
        mptr, midx = ptr, (idx - 1).contiguous()
        enc, rank_ms, list_ms, dense = [], [], [], {"gemm_ms": [], "mask_ms": [], "count_ms": []}
        for it in range(a.warmup + a.windows):
            e = _events(4)
            e[0].record()
            model._encode(X, last_only=True)
            e[1].record()
            rank = engine.s3rec_catalogue_rank(h_last, W, target, ptr, idx, users, first_col=1)
            e[2].record()
            engine.mf_eval_topk(h_last, W[1:], users, mptr, midx, 10)
            e[3].record()
            acc = [0.0, 0.0, 0.0]
            d_rank = dense_ranks(h_last, W, target, ptr, idx, ev=acc)
            torch.cuda.synchronize()
            if it >= a.warmup:
                enc.append(e[0].elapsed_time(e[1]))
                rank_ms.append(e[1].elapsed_time(e[2]))
                list_ms.append(e[2].elapsed_time(e[3]))
                for k, name in enumerate(dense):
                    dense[name].append(acc[k])
        # peak memory above what is resident, each path alone
        for name, fn in (("rank_sweep_peak_mib", lambda: engine.s3rec_catalogue_rank(h_last, W, target, ptr, idx, users)),
                         ("dense_peak_mib", lambda: dense_ranks(h_last, W, target, ptr, idx))):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            res[name] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)
        differ = int((rank != d_rank).sum())
        res["rows_where_dense_and_sweep_differ"] = differ
        res["largest_rank_difference"] = int((rank - d_rank).abs().max())
    model.check_indices()
    flops = 2.0 * NU * (NI + 1) * E
    res["encoder_ms"], res["encoder_ms_windows"] = _median(enc), [round(v, 4) for v in enc]
    res["rank_sweep_ms"], res["rank_sweep_ms_windows"] = _median(rank_ms), [round(v, 4) for v in rank_ms]
    res["rank_sweep_matrix_gflop"] = round(flops / 1e9, 2)
    res["rank_sweep_tflops"] = round(flops / (res["rank_sweep_ms"] * 1e-3) / 1e12, 2)
    res["rank_sweep_of_f32_matrix_peak"] = round(res["rank_sweep_tflops"] / PEAK_F32_MATRIX_TFLOPS, 4)
    res["rank_sweep_bound_ms"] = round(flops / (PEAK_F32_MATRIX_TFLOPS * 1e12) * 1e3, 3)
    res["list_sweep_ms"], res["list_sweep_ms_windows"] = _median(list_ms), [round(v, 4) for v in list_ms]
    res["dense"] = {k: _median(v) for k, v in dense.items()}
    res["dense"]["total_ms"] = round(sum(res["dense"].values()), 4)
    res["dense"]["chunk_users"] = DENSE_CHUNK
    res["dense_count_over_rank_sweep"] = round(res["dense"]["count_ms"] / res["rank_sweep_ms"], 3)
    res["dense_total_over_rank_sweep"] = round(res["dense"]["total_ms"] / res["rank_sweep_ms"], 3)
    # evaluate_full end to end
    runs = []
    for it in range(a.warmup + a.windows):
        loader = S3RecBatchLoader(store, "test", batch_size=a.batch, n_neg=1)
        torch.cuda.synchronize()
        t = time.perf_counter()
        four = trainer.evaluate_full(loader, history=(ptr, idx))
        runs.append((time.perf_counter() - t) * 1e3)
    runs = runs[a.warmup:]
    res["evaluate_full_ms"], res["evaluate_full_ms_windows"] = _median(runs), [round(v, 3) for v in runs]
    res["evaluate_full_batch"] = a.batch
    res["evaluate_full_metrics_untrained"] = [round(v, 6) for v in four]
    res["evaluate_full_n_users"] = trainer.last_full_eval["n_users"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s3rec_full_eval_yelp2018.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_s3rec_full_eval: no GPU (there is no CPU path to time)")
    if a.windows < 5:
        raise SystemExit("bench_s3rec_full_eval: at least 5 windows")
    res = bench(a)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
