#!/usr/bin/env python3
"""S3Rec scoring at Yelp2018 shape (31,668 sequences, 38,048 items, max_seq_len 50, embed_size 64, 2 heads, 2 blocks,
99 sampled negatives): S3RecTrainer.validate and .evaluate over all sequences at batch 256 and 4,096 (batches resident
on the device), the encoder launch alone, and its share of the f32 matrix peak.  Prints one JSON line.

    python scripts/bench_s3rec.py [--steps 5] [--warmup 1]

Flops of the encoder per sequence and block at this shape: Q, K, V 3 x heads x 2 L E^2 = 2.46 M, attention (Q K^T and
P V, full L x L) heads x 4 L^2 E = 1.28 M, output projection 2 L (heads E) E = 0.82 M, FFN 4 L E^2 = 1.64 M: 6.2 M,
i.e. 0.39 TFLOP per pass over the sequences and 2.5 ms at the 157.3 TFLOP/s f32 matrix peak.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

F32_PEAK = 157.3e12          # MI355X dense f32 matrix peak (v_mfma_f32_*)


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps


def encoder_flops(n, L, E, heads, blocks):
    per_block = 3 * heads * 2 * L * E * E + heads * 4 * L * L * E + 2 * L * heads * E * E + 4 * L * E * E
    return float(n) * blocks * per_block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    from yelprecommendation_amd.trainers.s3rec_trainer import S3RecTrainer
    from yelprecommendation_amd.utils import Config, set_seed
    n, ni, L, E, heads, blocks, C = 31668, 38048, 50, 64, 2, 2, 99
    cfg = Config(device="cuda", model_dir=tempfile.mkdtemp(prefix="yr_bench_s3rec."), top_n=10, best_metric="loss",
                 embed_size=E, max_seq_len=L, num_heads=heads, num_blocks=blocks, dropout_ratio=0.1,
                 load_pretrain=False)
    set_seed(0)
    tr = S3RecTrainer(cfg, ni, None, 100)
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    # left-padded histories of 1 .. L items, as the reference's dataset builds them
    X = torch.randint(1, ni + 1, (n, L), device=dev, generator=g)
    length = torch.randint(1, L + 1, (n, 1), device=dev, generator=g)
    X = X * (torch.arange(L, device=dev).unsqueeze(0) >= L - length)
    pos_items = torch.randint(0, ni + 1, (n, L), device=dev, generator=g)
    neg_items = torch.randint(0, ni + 1, (n, L), device=dev, generator=g)
    pos_item = torch.randint(1, ni + 1, (n,), device=dev, generator=g)
    cand = torch.randint(1, ni + 1, (n, C), device=dev, generator=g)
    flops = encoder_flops(n, L, E, heads, blocks)
    res = {"workload": "s3rec_yelp2018_scoring", "shape": [n, ni, L, E, heads, blocks, C],
           "encoder_tflop_per_pass": round(flops / 1e12, 4), "bound_ms_at_f32_matrix_peak": round(flops / F32_PEAK * 1e3, 3)}
    for B in (256, 4096):
        valid = [{"X": X[s:s + B], "pos_items": pos_items[s:s + B], "neg_items": neg_items[s:s + B]}
                 for s in range(0, n, B)]
        test = [{"X": X[s:s + B], "pos_item": pos_item[s:s + B], "neg_items": cand[s:s + B]} for s in range(0, n, B)]
        tv = _time(lambda: tr.validate(valid), a.steps, a.warmup)
        te = _time(lambda: tr.evaluate(test), a.steps, a.warmup)

        def encode_all():
            with torch.no_grad():
                for d in valid:
                    tr.model._encode(d["X"], last_only=False)
        tr.model.eval()
        tk = _time(encode_all, a.steps, a.warmup)
        res[f"validate_ms_b{B}"] = round(tv * 1e3, 2)
        res[f"evaluate_ms_b{B}"] = round(te * 1e3, 2)
        res[f"encoder_ms_b{B}"] = round(tk * 1e3, 2)
        res[f"encoder_fraction_of_f32_peak_b{B}"] = round(flops / tk / F32_PEAK, 3)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
