#!/usr/bin/env python3
"""S3Rec fine-tuning steps at Yelp2018 shape (38,048 items, max_seq_len 50, embed_size 64, 2 heads, 2 blocks,
dropout 0.1, Adam) at batch 32 (the reference's), 256 and 4,096, next to the same step written in eager PyTorch ops
(float32, torch.optim.Adam) on the same GPU.  Writes profiles/s3rec_train_yelp2018.json and prints it as one line.

    python scripts/bench_s3rec_train.py [--steps 20] [--warmup 3] [--batches 32,256,4096] [--converge]

Per batch size: ``hip_step_ms`` is finetune + BPRLoss + backward + Adam.step through the model's surface, host clock
around a window that ends in a device synchronise; the phases (forward = stash-keeping encoder + scores + loss,
backward kernel = score gradient + yr_s3rec_backward, gradient products and column sums, item gradient, Adam) are
device-event times of the same launches driven one after the other, so they leave out what autograd adds around
them.  ``eager_step_ms`` is the baseline: the arithmetic of tests/s3rec_grad_ref64.py (the reference's
models/s3rec.py) in torch ops with nn.functional.dropout, autograd and torch.optim.Adam.

--converge: a seeded S3RecTrainer.run at the reference's defaults (dropout 0.1, Adam 1e-4, batch 32) on synthetic
next-item sequences; records the validation loss per epoch.
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

NI, L, E, HEADS, BLOCKS, P_DROP = 38048, 50, 64, 2, 2, 0.1


def _cfg(**kw):
    from yelprecommendation_amd.utils import Config
    base = dict(device="cuda", model_dir=tempfile.mkdtemp(prefix="yr_bench_s3rec_train."), top_n=10, best_metric="loss",
                embed_size=E, max_seq_len=L, num_heads=HEADS, num_blocks=BLOCKS, dropout_ratio=P_DROP,
                load_pretrain=False, optimizer="adam", lr=1e-4, epochs=3, patience=5)
    base.update(kw)
    return Config(**base)


def _batch(B, dev, g):
    """Left-padded histories of 1 .. L items, as the reference's dataset builds them."""
    X = torch.randint(1, NI + 1, (B, L), device=dev, generator=g)
    length = torch.randint(1, L + 1, (B, 1), device=dev, generator=g)
    X = X * (torch.arange(L, device=dev).unsqueeze(0) >= L - length)
    return X, torch.randint(0, NI + 1, (B, L), device=dev, generator=g), torch.randint(0, NI + 1, (B, L), device=dev,
                                                                                       generator=g)


def eager_finetune(model, X, pos_items, neg_items, p_drop):
    """reference models/s3rec.py:53-100,184-214 in torch ops on the model's own parameters."""
    pad = (X <= 0).unsqueeze(-1).to(torch.float32)
    h = model.item_embedding.weight[X] + model.positional_encoding
    keep = torch.tril(torch.ones((L, L), dtype=torch.bool, device=X.device))
    for mha, ln1, f1, f2, ln2 in zip(model.multihead_attns, model.layernorm1s, model.ffn1s, model.ffn2s,
                                     model.layernorm2s):
        att = []
        for q, k, v in zip(mha.q_weights, mha.k_weights, mha.v_weights):
            S = (h @ q.weight.T) @ ((h @ k.weight.T) * pad).transpose(1, 2) / math.sqrt(E)
            att.append(torch.softmax(S.masked_fill(~keep, -math.inf), dim=-1) @ (h @ v.weight.T))
        attn = F.dropout(F.linear(torch.cat(att, -1), mha.output.weight, mha.output.bias), p_drop, True)
        x1 = F.layer_norm(h + attn, (E,), ln1.weight, ln1.bias, 1e-5)
        f = F.dropout(F.linear(torch.relu(F.linear(x1, f1.weight, f1.bias)), f2.weight, f2.bias), p_drop, True)
        h = F.layer_norm(h + f, (E,), ln2.weight, ln2.bias, 1e-5)
    hr = h.reshape(-1, E)
    return ((model.item_embedding.weight[pos_items.reshape(-1)] * hr).sum(-1),
            (model.item_embedding.weight[neg_items.reshape(-1)] * hr).sum(-1))


def _wall(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def hip_phases(model, opt, X, pos_items, neg_items, steps, warmup):
    """ms per phase, device events around the launches of one step driven by hand."""
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.loss import BPRLoss
    B = X.shape[0]
    names = ("forward", "backward_kernel", "grad_gemms_colsums", "item_grad", "adam")
    total = dict.fromkeys(names, 0.0)
    table, pos_enc = model.item_embedding.weight, model.positional_encoding
    for it in range(warmup + steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        packed = model._params()
        ev[0].record()
        h, ws = engine.s3rec_encode_train(table.detach(), pos_enc.detach(), packed, X, HEADS, BLOCKS, seed=it + 1, p=P_DROP)
        pos, neg = engine.s3rec_seq_scores(table.detach(), h, pos_items, neg_items)
        pos, neg = pos.requires_grad_(), neg.requires_grad_()
        loss = BPRLoss()(pos, neg)
        ev[1].record()
        loss.backward()
        dh = engine.s3rec_score_grad(table.detach(), pos_items, neg_items, pos.grad, neg.grad)
        d_emb = engine.s3rec_backward(packed, X, dh.view(B, L, E), ws, HEADS, BLOCKS, seed=it + 1, p=P_DROP)
        ev[2].record()
        pg = engine.s3rec_param_grads(ws, B, L, E, HEADS, BLOCKS)
        d_pos = engine.colsum(d_emb.view(B, L * E)).view(L, E)
        ev[3].record()
        d_item = torch.zeros_like(table)
        engine.s3rec_item_grad(X, pos_items, neg_items, d_emb, h, pos.grad, neg.grad, d_item)
        ev[4].record()
        table.grad, pos_enc.grad, at = d_item, d_pos, 0
        for t in model._block_tensors():
            t.grad = pg[at:at + t.numel()].view(t.shape)
            at += t.numel()
        opt.step()
        ev[5].record()
        torch.cuda.synchronize()
        if it >= warmup:
            for k, name in enumerate(names):
                total[name] += ev[k].elapsed_time(ev[k + 1])
    return {k: round(v / steps, 4) for k, v in total.items()}


def bench(a):
    from yelprecommendation_amd.loss import BPRLoss
    from yelprecommendation_amd.trainers.s3rec_trainer import S3RecTrainer
    from yelprecommendation_amd.utils import set_seed
    dev = torch.device("cuda")
    res = {"workload": "s3rec_yelp2018_finetune_step", "shape": [NI, L, E, HEADS, BLOCKS], "dropout": P_DROP,
           "optimizer": "adam", "steps": a.steps, "warmup": a.warmup, "date": time.strftime("%Y-%m-%d"),
           "device": torch.cuda.get_device_name(0)}
    loss_fn = BPRLoss()
    for B in a.batches:
        set_seed(0)
        tr = S3RecTrainer(_cfg(), NI, None, 100)
        model, opt = tr.model.train(), tr.optimizer
        X, pos_items, neg_items = _batch(B, dev, torch.Generator(device=dev).manual_seed(B))

        def hip_step():
            pos, neg = model.finetune(X, pos_items, neg_items)
            opt.zero_grad()
            loss_fn(pos, neg).backward()
            opt.step()
        hip = [_wall(hip_step, a.steps, a.warmup) for _ in range(3)]
        model.check_indices()
        phases = hip_phases(model, opt, X, pos_items, neg_items, a.steps, a.warmup)

        set_seed(0)
        eager_model = S3RecTrainer(_cfg(), NI, None, 100).model.train()
        eager_opt = torch.optim.Adam(eager_model.parameters(), lr=1e-4)

        def eager_step():
            pos, neg = eager_finetune(eager_model, X, pos_items, neg_items, P_DROP)
            eager_opt.zero_grad()
            (-F.logsigmoid(pos - neg)).mean().backward()
            eager_opt.step()
        eager = [_wall(eager_step, a.steps, a.warmup) for _ in range(3)]
        res[f"b{B}"] = {"hip_step_ms": round(min(hip), 4), "hip_step_ms_runs": [round(v, 4) for v in hip],
                        "hip_phase_ms": phases, "eager_step_ms": round(min(eager), 4),
                        "eager_step_ms_runs": [round(v, 4) for v in eager],
                        "eager_over_hip": round(min(eager) / min(hip), 3)}
    return res


def converge(a):
    """A seeded run at the reference's defaults on learnable synthetic data: the next item of a sequence is its
    successor in the catalogue."""
    from yelprecommendation_amd.trainers.s3rec_trainer import S3RecTrainer
    from yelprecommendation_amd.utils import set_seed
    set_seed(0)
    tr = S3RecTrainer(_cfg(epochs=a.epochs), NI, None, 100)
    g = torch.Generator().manual_seed(3)

    def data(n):
        start = torch.randint(0, 3000, (n, 1), generator=g)
        seq = (start + torch.arange(L + 1)) % NI + 1
        length = torch.randint(2, L + 1, (n, 1), generator=g)
        real = torch.arange(L).unsqueeze(0) >= L - length
        X, pos = seq[:, :L] * real, seq[:, 1:] * real
        neg = torch.randint(1, NI + 1, (n, L), generator=g) * real
        return [{"X": X[s:s + 32], "pos_items": pos[s:s + 32], "neg_items": neg[s:s + 32]} for s in range(0, n, 32)]
    train, valid = data(a.sequences), data(512)
    losses = [tr.validate(valid)]
    for _ in range(a.epochs):
        tr.train(train)
        losses.append(tr.validate(valid))
    return {"workload": "s3rec_finetune_convergence", "batch": 32, "lr": 1e-4, "dropout": P_DROP,
            "train_sequences": a.sequences, "valid_loss_sum_before_and_per_epoch": [round(v, 5) for v in losses]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=lambda s: [int(v) for v in s.split(",")], default=[32, 256, 4096])
    ap.add_argument("--converge", action="store_true")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--sequences", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s3rec_train_yelp2018.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_s3rec_train: no GPU (there is no CPU path to time)")
    res = converge(a) if a.converge else bench(a)
    if not a.converge:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
