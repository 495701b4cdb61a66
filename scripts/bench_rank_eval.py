#!/usr/bin/env python3
"""Rank evaluation at Yelp2018 shape (31,668 users x 38,048 items) on the synthetic data set's own test split — the
real target lists (the held-out 20 % of every user) and mask lists (the rest) of train.py's pipeline — next to the only
routes the parent commit has for top_n = 50, on the same GPU in the same session.  Writes
profiles/rank_eval_yelp2018.json and prints it as one line.

    python scripts/bench_rank_eval.py [--windows 7] [--warmup 2] [--reps 3]

Three models, untrained (Xavier tables; NGCF's layers from one propagation): MF at D = 64 and 128, NGCF at D = 64 with
two propagation orders (three layer tables).  Medians over ``--windows`` windows after ``--warmup``; in every window the
routes run one after the other, each ``--reps`` times between two device events (the figure is the time per call):
* ``rank_sweep_ms``        engine.catalogue_ranks alone (its four launches); flops 2 x slots x items x L D against the
                           f32 matrix peak (the data sheet's figure, not measured), and the same with rows for slots;
* ``metrics_ms``           engine.metrics_from_ranks for ks = (10, 20, 50, 100), read-back included;
* ``dense_top50_ms``       the parent's route at top_n = 50: MF ``engine.mf_recommend(fused=False)`` + ``rank_metrics``;
                           NGCF ``NGCFTrainer._recommend_chunked`` (what ``recommend(fused=False)`` does, in the chunks
                           ``evaluate_full`` cuts all users into — one [users, items] array does not fit) + ``rank_metrics``;
* ``fused_top10_ms``       the fused top-10 sweep (mf_eval_topk / ngcf_eval_topk, no hint), for scale;
* ``evaluate_ranks_ms``    ``trainer.evaluate_ranks(ks=(10, 20, 50, 100))`` end to end on the host clock (NGCF: its
                           propagation included; ``propagate_ms`` is that part alone);
* peak device memory of the rank route and of the dense route above what is resident.
An untrained model spreads a user's targets over the whole order, so most items fall between the slot's best and worst
target and take the binary search: the slow case of the sweep.  ``mf64_trained``: MF at D = 64 after ``--epochs`` epochs
of the trainer's own loop, where the targets sit near the top and most items settle with one compare.
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

KS = (10, 20, 50, 100)
PEAK_F32_MATRIX_TFLOPS = 157.3          # data sheet (MI355X f32 matrix), as scripts/bench_s3rec_full_eval.py uses it


def _median(runs):
    return round(statistics.median(runs), 4)


def _timed(pieces, a):
    ms = {name: [] for name in pieces}
    for it in range(a.warmup + a.windows):
        for name, fn in pieces.items():
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                ms[name].append(e0.elapsed_time(e1) / a.reps)
    return ms


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)


def _build(model_name, embed, extra=()):
    from yelprecommendation_amd import train
    from yelprecommendation_amd.utils import make_config, set_seed
    cfg = make_config(model_name, synthetic="yelp2018", fast_loader=True, device="cuda", embed_size=embed, top_n=50,
                      batch_size=65536, lr=1e-2, model_dir=tempfile.mkdtemp(prefix="yr_bench_rank_eval."),
                      **dict(extra))
    args = train.build(cfg)
    set_seed(cfg.seed)
    return cfg, args


def measure(trainer, frame, layers_of, a, ngcf):
    from yelprecommendation_amd import engine
    users, mask_ptr, mask_idx, pos_ptr, pos_idx = trainer._eval_sets.eval_set(frame, sort_masks=True)[2:7]
    users = users.contiguous()
    lengths = (pos_ptr[1:] - pos_ptr[:-1]).cpu().tolist()
    res = {"eval_rows": int(users.numel()), "targets": int(pos_idx.numel()), "mask_entries": int(mask_idx.numel()),
           "targets_per_row_max": int(max(lengths)), "slots": engine.catalogue_rank_slots(lengths)}
    with torch.no_grad():
        lu, li = layers_of()
        L, D, ni = len(lu), lu[0].shape[1], li[0].shape[0]
        st = {}

        def sweep():
            st["rank"] = engine.catalogue_ranks(lu, li, users, pos_ptr, pos_idx, mask_ptr, mask_idx)

        if ngcf:
            layers = trainer.model.propagate(trainer.laplacian_matrix)
            dense = lambda: engine.rank_metrics(trainer._recommend_chunked(users, mask_ptr, mask_idx), pos_ptr, pos_idx)
            fused = lambda: engine.ngcf_eval_topk(layers, trainer.num_users, users, mask_ptr, mask_idx, 10)
        else:
            dense = lambda: engine.rank_metrics(engine.mf_recommend(lu[0], li[0], users, mask_ptr, mask_idx, 50,
                                                                    fused=False), pos_ptr, pos_idx)
            fused = lambda: engine.mf_eval_topk(lu[0], li[0], users, mask_ptr, mask_idx, 10)
        sweep()
        pieces = {"rank_sweep": sweep,
                  "metrics": lambda: engine.metrics_from_ranks(st["rank"], pos_ptr, KS, num_items=ni, mask_ptr=mask_ptr),
                  "dense_top50": dense, "fused_top10": fused}
        if ngcf:
            pieces["propagate"] = lambda: trainer.model.propagate(trainer.laplacian_matrix)
        ms = _timed(pieces, a)
        res["rank_route_peak_mib"] = _peak(lambda: engine.metrics_from_ranks(
            engine.catalogue_ranks(lu, li, users, pos_ptr, pos_idx, mask_ptr, mask_idx), pos_ptr, KS, num_items=ni,
            mask_ptr=mask_ptr))
        res["dense_top50_peak_mib"] = _peak(dense)
    for name, runs in ms.items():
        res[name + "_ms"], res[name + "_ms_windows"] = _median(runs), [round(v, 4) for v in runs]
    for what, rows in (("slots", res["slots"]), ("rows", res["eval_rows"])):
        tf = 2.0 * rows * ni * L * D / (res["rank_sweep_ms"] * 1e-3) / 1e12
        res[f"rank_sweep_tflops_by_{what}"] = round(tf, 2)
        res[f"rank_sweep_of_f32_matrix_peak_by_{what}"] = round(tf / PEAK_F32_MATRIX_TFLOPS, 4)
    runs = []
    for it in range(a.warmup + a.windows):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = trainer.evaluate_ranks(frame, ks=KS)
        runs.append((time.perf_counter() - t) * 1e3)
    runs = runs[a.warmup:]
    res["evaluate_ranks_ms"], res["evaluate_ranks_ms_windows"] = _median(runs), [round(v, 3) for v in runs]
    res["dense_top50_over_rank_route"] = round(res["dense_top50_ms"] / (res["rank_sweep_ms"] + res["metrics_ms"]), 2)
    res["metrics"] = {str(k): [round(v, 6) for v in out[k]] for k in KS}
    res["mrr"], res["auc"] = round(out.mrr, 6), round(out.auc, 6)
    return res


def bench(a):
    from yelprecommendation_amd import train
    from yelprecommendation_amd.trainers import MFTrainer, NGCFTrainer
    res = {"workload": "rank_eval_yelp2018", "ks": list(KS), "windows": a.windows, "warmup": a.warmup, "reps": a.reps,
           "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0),
           "f32_matrix_peak_tflops_data_sheet_not_measured": PEAK_F32_MATRIX_TFLOPS}
    cfg, args = _build("NGCF", 64, {"num_orders": 2, "full_eval": True})
    frame, ni, nu = args.test_eval_data, args.model_info["num_items"], args.model_info["num_users"]
    res["shape"] = [nu, ni]
    mf_layers = lambda t: lambda: ([t.model.user_embedding.weight.detach()], [t.model.item_embedding.weight.detach()])
    for embed in (64, 128):
        c = cfg.copy()
        c.update(model_name="MF", embed_size=embed)
        t = MFTrainer(c, ni, nu)
        res[f"mf{embed}"] = measure(t, frame, mf_layers(t), a, ngcf=False)
    t = NGCFTrainer(cfg, ni, nu, args.data_pipeline.laplacian_matrix)

    def ngcf_layers():
        layers = t.model.propagate(t.laplacian_matrix)
        return [E[:nu] for E in layers], [E[nu:] for E in layers]
    res["ngcf64_k2"] = measure(t, frame, ngcf_layers, a, ngcf=True)
    del t
    if a.epochs > 0:                                                  # MF D = 64 after a few epochs of its own loop
        c, margs = _build("MF", 64, {"epochs": a.epochs, "rank_eval": True})
        t, _ = train.train(c, margs)
        res["mf64_trained"] = measure(t, margs.test_eval_data, mf_layers(t), a, ngcf=False)
        res["mf64_trained"]["epochs"] = a.epochs
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_eval_yelp2018.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rank_eval: no GPU (there is no CPU path to time)")
    if a.windows < 5:
        raise SystemExit("bench_rank_eval: at least 5 windows")
    res = bench(a)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
