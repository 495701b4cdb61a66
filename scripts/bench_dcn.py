#!/usr/bin/env python3
"""DCN at Yelp2018 shape (31,668 users x 38,048 items, D = 64, hidden [1024, 1024], one cross order): train-step time
at three batch sizes, validation (1,000 users) and test (all users) evaluation times, and the fused scorer's share of
the f32 matrix peak.  Prints one JSON line.

    python scripts/bench_dcn.py [--steps 20] [--warmup 3] [--test-users 31668]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--test-users", type=int, default=31668)
    a = ap.parse_args()
    from yelprecommendation_amd.data.synthetic import make_item_attributes
    from yelprecommendation_amd.trainers.dcn_trainer import DCNTrainer
    from yelprecommendation_amd.utils import make_config, set_seed
    nu, ni, D, H = 31668, 38048, 64, [1024, 1024]
    attrs = make_item_attributes(ni)
    Lmax = max(len(v["categories"]) for v in attrs.values())
    cat = np.zeros((ni, Lmax), np.int32)
    for i in range(ni):
        c = attrs[str(i)]["categories"]
        cat[i, :len(c)] = np.asarray(c) + 1
    sc = np.array([attrs[str(i)]["statecity"] for i in range(ni)], np.int32)
    counts = [int(cat.max()), int(sc.max()) + 1]
    cfg = make_config("DCN", device="cuda", embed_size=D, hidden_dims=H, cross_orders=1, model_dir="/tmp/yr_bench_dcn")
    set_seed(0)
    tr = DCNTrainer(cfg, ni, nu, None, counts, cat_ids=torch.from_numpy(cat), sc_ids=torch.from_numpy(sc))
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    res = {"workload": "dcn_yelp2018", "shape": [nu, ni, D] + H + [1]}
    for B in (32, 4096, 65536):
        u = torch.randint(0, nu, (B,), device=dev, generator=g)
        p = torch.randint(0, ni, (B,), device=dev, generator=g)
        n = torch.randint(0, ni, (B,), device=dev, generator=g)

        def step():
            tr.model.bpr_loss_backward(u, p, n, loss_accum=tr._loss_accum)
            tr.optimizer.step(zero_grad=True)
        res[f"train_step_us_b{B}"] = round(_time(step, a.steps, a.warmup) * 1e6, 1)
    tr.model.check_indices()

    def eval_users(n):
        users = torch.arange(n, device=dev)
        ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        idx = torch.zeros(0, dtype=torch.int64, device=dev)
        return lambda: tr.recommend(users, ptr, idx)
    res["valid_eval_ms_1000_users"] = round(_time(eval_users(1000), max(2, a.steps // 5), 1) * 1e3, 2)
    res["test_eval_s_all_users"] = round(_time(eval_users(a.test_users), 1, 0), 3)
    res["test_users"] = a.test_users
    # the scorer alone (W2 GEMM flops: 2 H1 H2 per pair)
    prep = tr.model.score_prep()
    users = torch.arange(1024, device=dev)
    out = torch.empty(1024, ni, device=dev)
    t = _time(lambda: tr.model.score_catalogue(users, out, prep=prep), max(2, a.steps // 5), 1)
    flops = 2.0 * H[0] * H[1] * 1024 * ni
    res["scorer_ms_1024_users"] = round(t * 1e3, 2)
    res["scorer_fraction_of_f32_peak"] = round(flops / t / F32_PEAK, 3)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
