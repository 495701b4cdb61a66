"""GPU: S3Rec pre-training above the kernel — ``S3Rec.encode`` under grad against the float64 restatement of the
encoder (tests/s3rec_grad_ref64.py), ``pretrain`` (dense) and ``pretrain_loss`` (fused) against what the reference
recorded (tests/golden/s3rec_pretrain_small.npz) and against each other, the pre-trainer on the recorded masks, its
checkpointing and early stop, the masking law on the device, and ``train.main`` with ``pretrain=true`` end to end.
Bars: anything downstream of the encoder uses the project's rule, 8 x |f32 - f64| of the restatement per tensor
(tests/s3rec_pretrain_ref64.py), never measured on a kernel."""
import functools
import os
import types

import numpy as np
import pytest
import torch

import s3rec_grad_ref64 as gr
import s3rec_pretrain_ref64 as R
import s3rec_ref64 as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = gr.DROPOUT_SEED
ENCODE_CONFIGS = [("E16-L7-h1-b1-B3", 0.0), ("E64-L50-h2-b2-B257", 0.0), ("E32-L33-h4-b3-B3", 0.1),
                  ("E16-L7-h1-b1-B3", 0.5)]
HEADS, BLOCKS = 2, 2


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _cfg(E, L, heads, blocks, p=0.0):
    return types.SimpleNamespace(embed_size=E, max_seq_len=L, num_heads=heads, num_blocks=blocks, dropout_ratio=p,
                                 device="cuda")


def _model(params, case, device, p=0.0):
    from yelprecommendation_amd.models.s3rec import S3Rec
    model = S3Rec(_cfg(case["E"], case["L"], case["heads"], case["blocks"], p),
                  params["item_embedding.weight"].shape[0] - 1, params["attribute_embedding.weight"].shape[0])
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}, strict=True)
    return model.to(device)


def _ratio(name, got, want, bar):
    want = np.asarray(want, np.float64)
    err = float(np.max(np.abs(got.detach().double().cpu().numpy().reshape(want.shape) - want)))
    print(f"{name}: max|err| {err:.3e}, bar {bar:.3e}, err/bar {err / bar if bar > 0 else (0.0 if err == 0 else np.inf):.3f}")
    assert np.isfinite(err) and err <= bar, f"{name}: {err:.3e} > bar {bar:.3e}"


def _all(checks):
    """Every tensor is measured and printed before the first one over its bar fails the test."""
    over = []
    for args in checks:
        try:
            _ratio(*args)
        except AssertionError as e:
            over.append(str(e))
    assert not over, "\n".join(over)


# ------------------------------------------------------------------------------------------------ encode under grad
@functools.lru_cache(maxsize=None)
def _encode_reference(cid, p):
    case = next(c for c in ref.CASES if c["id"] == cid)
    params, batch = gr.case_setup(case)
    X = batch["X"]
    B, L = X.shape
    w = np.random.RandomState(case["index"]).standard_normal((B, L, case["E"]))
    masks = gr.dropout_masks(SEED, p, B, L, case["E"], case["blocks"]) if p > 0 else None
    res = {}
    for dt in (torch.float64, torch.float32):
        t = gr.tensors(params, dt)
        h = gr.encode(t, X, case["heads"], case["blocks"], p, masks)
        (h * torch.as_tensor(w, dtype=dt)).sum().backward()
        res[dt] = (h.detach().numpy(), {k: v.grad.numpy().copy() for k, v in t.items() if v.grad is not None})
    (h64, g64), (h32, g32) = res[torch.float64], res[torch.float32]
    bars = {k: gr.BAR_FACTOR * float(np.max(np.abs(g32[k].astype(np.float64) - g64[k]))) for k in g64}
    return case, params, X, w, h64, g64, bars


@pytest.mark.parametrize("cid,p", ENCODE_CONFIGS, ids=[f"{c}-p{p}" for c, p in ENCODE_CONFIGS])
def test_encode_under_grad(device, cid, p):
    from yelprecommendation_amd import engine
    case, params, X, w, h64, g64, bars = _encode_reference(cid, p)
    model = _model(params, case, device, p).train()
    Xd, wd = torch.from_numpy(X).to(device), torch.from_numpy(w.astype(np.float32)).to(device)
    h = model.encode(Xd, dropout_seed=SEED)
    assert h.shape == (X.shape[0], X.shape[1], case["E"]) and h.requires_grad
    direct, _ = engine.s3rec_encode_train(model.item_embedding.weight.detach(), model.positional_encoding.detach(),
                                          model._params(), Xd, case["heads"], case["blocks"], seed=SEED, p=p)
    assert torch.equal(h.detach(), direct)                           # bit for bit (at p = 0 and under the same seed)
    (h * wd).sum().backward(retain_graph=True)
    model.check_indices()
    got = {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
    assert sorted(got) == sorted(g64)                                 # the two embeddings' other halves and *_weight: None
    _all([(f"{cid} p={p} {gr.group(k)} {k}", got[k], g64[k], bars[k]) for k in got])
    model.zero_grad(set_to_none=True)                                 # two backward calls, one answer
    (h * wd).sum().backward()
    for k, v in model.named_parameters():
        if v.grad is not None:
            assert torch.equal(v.grad, got[k]), k


def test_encode_in_eval_mode_is_the_scoring_encoder(device):
    case, params, X, *_ = _encode_reference("E16-L7-h1-b1-B3", 0.0)
    model = _model(params, case, device).eval()
    Xd = torch.from_numpy(X).to(device)
    with torch.no_grad():
        h = model.encode(Xd)
    assert not h.requires_grad and torch.equal(h, model.train().encode(Xd).detach())      # dropout_ratio 0
    with pytest.raises(NotImplementedError):
        model.eval().encode(Xd)                                      # eval() with grad enabled: neither mode


# ------------------------------------------------------------------------------------------------ the step
@pytest.fixture(scope="module")
def rec():
    g = np.load(os.path.join(HERE, "golden", "s3rec_pretrain_small.npz"))
    small = np.load(os.path.join(HERE, "golden", "s3rec_small.npz"))
    cfg = dict(zip(small["cfg_names"].tolist(), small["cfg_values"].tolist()))
    state = {k[5:]: small[k] for k in small.files if k.startswith("pert:")}
    batches = [dict(X=g[f"b{i}_X"], masks=g[f"b{i}_masks"], seg=g[f"b{i}_seg"], pos=g[f"b{i}_pos"], neg=g[f"b{i}_neg"])
               for i in range(3)]
    args = (state, batches[0], g["attr_ptr"], g["attr_idx"], HEADS, BLOCKS)
    r64, r32 = R.step_and_grads(*args, dtype=torch.float64), R.step_and_grads(*args, dtype=torch.float32)
    return dict(g=g, cfg=cfg, state=state, batches=batches, r64=r64, r32=r32)


def _rec_model(rec, device):
    c = rec["cfg"]
    return _model(rec["state"], dict(E=c["embed_size"], L=c["max_seq_len"], heads=HEADS, blocks=BLOCKS), device).train()


def _dev_batch(b, device):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in b.items()}


def _dense_losses(model, b):
    """trainers/s3rec_trainer.py:134-158 on the model's dense outputs."""
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    aap, mip, map_, (sp_pos, sp_neg) = model.pretrain(b["masks"] * b["X"], b["seg"], b["pos"], b["neg"])
    on, off = b["masks"].unsqueeze(-1).float(), (~b["masks"]).unsqueeze(-1).float()
    A, I = aap.shape[-1], mip.shape[-1]
    ptr, idx = b["attr_ptr"], b["attr_idx"]
    X = b["X"].reshape(-1)
    counts = (ptr[X + 1] - ptr[X])
    rows = torch.repeat_interleave(torch.arange(X.numel(), device=X.device), counts)
    offs = torch.arange(rows.numel(), device=X.device) - torch.repeat_interleave(torch.cumsum(counts, 0) - counts, counts)
    aap_actual = torch.zeros((X.numel(), A), device=X.device)
    aap_actual[rows, idx[torch.repeat_interleave(ptr[X], counts) + offs]] = 1.0
    aap_actual = aap_actual.view(*b["X"].shape, A)
    mip_actual = torch.nn.functional.one_hot(b["X"], I).float()
    n = b["X"].shape[0]
    sp_actual = torch.cat([torch.zeros(n, device=X.device), torch.ones(n, device=X.device)])
    return (aap, mip, map_, sp_pos, sp_neg), (bce(aap, aap_actual * on), bce(mip * off, mip_actual * off),
                                              bce(map_ * off, aap_actual * off), bce(torch.cat([sp_neg, sp_pos]), sp_actual))


def test_the_dense_outputs_match_the_record(device, rec):
    model = _rec_model(rec, device)
    b = _dev_batch(rec["batches"][0], device)
    outs = model.pretrain(b["masks"] * b["X"], b["seg"], b["pos"], b["neg"])
    flat = dict(zip(R.OUTPUTS, (outs[0], outs[1], outs[2], outs[3][0], outs[3][1])))
    assert flat["aap"].shape == (8, 12, 20) and flat["mip"].shape == (8, 12, 301) and flat["sp_pos"].shape == (8,)
    _all([(f"dense {k}", flat[k], rec["g"][f"out64:{k}"], R.bar_of(rec["r32"][k], rec["r64"][k])) for k in R.OUTPUTS])


def test_the_fused_losses_and_gradients_match_the_record_and_the_dense_path(device, rec):
    g, r64, r32 = rec["g"], rec["r64"], rec["r32"]
    b = _dev_batch(rec["batches"][0], device)
    b["attr_ptr"], b["attr_idx"] = torch.from_numpy(g["attr_ptr"]).to(device), torch.from_numpy(g["attr_idx"]).to(device)
    fused = _rec_model(rec, device)
    losses = fused.pretrain_loss(b["X"], b["masks"], b["masks"] * b["X"], b["pos"], b["neg"], b["attr_ptr"], b["attr_idx"])
    sum(losses).backward()
    fused.check_indices()
    dense = _rec_model(rec, device)
    _, dlosses = _dense_losses(dense, b)
    sum(dlosses).backward()
    names = R.LOSSES[:4]
    # a scalar's bar needs samples: the same loss on the three recorded batches; the fused path adds the kernel's own
    # closed-form bar on the restatement's F and T (tests/s3rec_pretrain_ref64.py: loss_bars, fused_loss_bars)
    ref_args = (rec["state"], rec["batches"], g["attr_ptr"], g["attr_idx"], HEADS, BLOCKS)
    loss_bar = R.loss_bars(*ref_args)
    kernel_bar = R.fused_loss_bars(rec["state"], rec["batches"][0], *ref_args[2:], r64=r64)
    checks = [(f"fused {k}", losses[i], g["loss64"][i], loss_bar[k] + kernel_bar[k]) for i, k in enumerate(names)]
    checks += [(f"dense {k}", dlosses[i], g["loss64"][i], loss_bar[k]) for i, k in enumerate(names)]
    for model, what in ((fused, "fused"), (dense, "dense")):
        none = sorted(k for k, v in model.named_parameters() if v.grad is None)
        assert none == sorted(g["grad_none"].tolist()), what
        for k, v in model.named_parameters():
            if v.grad is not None:
                checks.append((f"{what} {gr.group(k)} {k}", v.grad, g[f"grad64:{k}"], R.bar_of(r32["grads"][k], r64["grads"][k])))
    _all(checks)
    # the two paths against each other: both inside the bar of the same float64 value, so within two bars
    for (k, a), (_, d) in zip(fused.named_parameters(), dense.named_parameters()):
        if a.grad is not None:
            assert float((a.grad - d.grad).abs().max()) <= 2 * R.bar_of(r32["grads"][k], r64["grads"][k]), k


# ------------------------------------------------------------------------------------------------ the trainer
def _trainer(rec, tmp_path, recorded=True, **kw):
    from yelprecommendation_amd.trainers.s3rec_trainer import S3RecPreTrainer
    c = rec["cfg"]
    tcfg = Cfg(embed_size=c["embed_size"], max_seq_len=c["max_seq_len"], num_heads=HEADS, num_blocks=BLOCKS,
               dropout_ratio=0.0, device="cuda", model_dir=str(tmp_path), top_n=c["top_n"], best_metric="loss",
               load_pretrain=True, optimizer="adam", lr=1e-3, epochs=2, pretrain_epochs=2, patience=5, mask_portion=0.2,
               seed=c["seed"])
    sp_negative = kw.pop("sp_negative", "same_row")
    tcfg.update(kw)
    os.makedirs(tmp_path, exist_ok=True)
    g = rec["g"]
    lists = {k: {"categories": g["attr_idx"][g["attr_ptr"][k]:g["attr_ptr"][k + 1]].tolist()} for k in range(c["num_items"] + 1)}
    batches = rec["batches"]

    class Recorded(S3RecPreTrainer):
        """The recorded masks in place of the drawn ones."""

        def _take(self, sequences):
            return next(_dev_batch(b, sequences.device) for b in batches
                        if b["X"].shape == tuple(sequences.shape) and (b["X"] == sequences.cpu().numpy()).all())

        def item_level_masking(self, sequences):
            b = self._take(sequences)
            return b["masks"], b["masks"] * sequences

        def segment_masking(self, sequences):
            b = self._take(sequences)
            return b["seg"], b["pos"], b["neg"]

    trainer = (Recorded if recorded else S3RecPreTrainer)(tcfg, c["num_items"], lists, c["attributes_count"],
                                                          sp_negative=sp_negative)
    trainer.model.load_state_dict({k: torch.from_numpy(v) for k, v in rec["state"].items()}, strict=True)
    assert torch.equal(trainer.attr_ptr.cpu(), torch.from_numpy(g["attr_ptr"]))
    return trainer


def test_the_pretrainer_reproduces_the_recorded_epochs(device, rec, tmp_path):
    g = rec["g"]
    epochs, lr = int(g["epochs"]), float(g["lr"])
    args = (rec["state"], rec["batches"], g["attr_ptr"], g["attr_idx"], HEADS, BLOCKS, epochs, lr)
    l64, s64 = R.train(*args, torch.float64)
    l32, s32 = R.train(*args, torch.float32)
    trainer = _trainer(rec, tmp_path)
    data = [{"X": torch.from_numpy(b["X"])} for b in rec["batches"]]
    losses = [trainer.train(data) for _ in range(epochs)]
    # the bar of ONE batch loss from all of them as one tensor, times the batches of an epoch (test_gpu_s3rec_train.py)
    per_loss = R.BAR_FACTOR * max(abs(a - b) for e in range(epochs) for a, b in zip(l32[e], l64[e]))
    bar = len(data) * per_loss
    over = []
    for e in range(epochs):
        err = abs(losses[e] - float(g["train_losses32"][e]))
        print(f"epoch {e}: loss {losses[e]:.9f}, recorded {float(g['train_losses32'][e]):.9f}, float64 "
              f"{float(g['train_losses64'][e]):.9f}, err {err:.3e}, bar {bar:.3e}, err/bar {err / bar:.3f}")
        assert abs(float(g["train_losses32"][e]) - sum(l64[e])) <= bar        # the record itself lies inside
        if err > bar:
            over.append(f"epoch {e}: {err:.3e} > {bar:.3e}")
    final = trainer.model.state_dict()
    assert sorted(final) == sorted(s64)
    for name in s64:
        b = R.BAR_FACTOR * float(np.max(np.abs(s32[name].astype(np.float64) - s64[name])))
        try:
            _ratio(f"final {gr.group(name)} {name}", final[name], g[f"final:{name}"].astype(np.float64), b)
        except AssertionError as e:
            over.append(str(e))
    assert not over, "\n".join(over)
    assert torch.equal(final["map_weight.weight"].cpu(), torch.from_numpy(rec["state"]["map_weight.weight"]))


def test_pretrain_saves_the_best_model_stops_early_and_finetuning_starts_from_it(device, rec, tmp_path):
    from yelprecommendation_amd.trainers.s3rec_trainer import S3RecTrainer
    data = [{"X": torch.from_numpy(b["X"])} for b in rec["batches"]]
    trainer = _trainer(rec, tmp_path, pretrain_epochs=3)
    trainer.pretrain(data)
    path = tmp_path / "best_pretrain_model.pt"
    saved = torch.load(path, map_location="cpu", weights_only=True)
    for k, v in trainer.model.state_dict().items():                  # the loss fell every epoch: the last model is the best
        assert torch.equal(saved[k], v.cpu()), k
    assert not torch.equal(saved["item_embedding.weight"], torch.from_numpy(rec["state"]["item_embedding.weight"]))
    tuner = S3RecTrainer(trainer.cfg, rec["cfg"]["num_items"], None, rec["cfg"]["attributes_count"])
    for k, v in tuner.model.state_dict().items():                    # load_pretrain picked the file up
        assert torch.equal(saved[k], v.cpu()), k
    trainer.load_best_model()
    # early stop: a loss that cannot improve (lr 0) ends after patience + 2 epochs: one best, patience + 1 without
    calls = []
    stuck = _trainer(rec, tmp_path / "s", pretrain_epochs=50, patience=1, lr=0.0)
    inner = stuck.train
    stuck.train = lambda loader: calls.append(1) or inner(loader)
    stuck.pretrain(data)
    assert len(calls) == 3


@pytest.mark.parametrize("sp_negative", ["same_row", "other_row"])
def test_the_masking_law_on_the_device(device, rec, tmp_path, sp_negative):
    L = rec["cfg"]["max_seq_len"]
    X = torch.from_numpy(np.random.RandomState(5).randint(1, 301, (96, L))).to(device)   # no pad: unambiguous segments
    runs = []
    for _ in range(2):
        trainer = _trainer(rec, tmp_path, recorded=False, sp_negative=sp_negative, mask_portion=0.3)
        runs.append(tuple(trainer.item_level_masking(X)) + tuple(trainer.segment_masking(X)))
    for a, b in zip(*runs):
        assert a.is_cuda and torch.equal(a, b)                       # the same seed, the same masks
    masks, item_masked, seg, pos, neg = (t.cpu().numpy() for t in runs[0])
    Xn = X.cpu().numpy()
    assert (item_masked == masks * Xn).all() and 0.2 < masks.mean() < 0.4
    lens = (pos != 0).sum(1)
    assert lens.min() >= 2 and lens.max() <= L // 2 - 1 and set(lens.tolist()) == set(range(2, L // 2))
    starts = set()
    for b in range(Xn.shape[0]):
        n = int(lens[b])
        gone = np.flatnonzero(seg[b] == 0)
        assert gone.size == n and (np.diff(gone) == 1).all() and gone[-1] <= L - 2      # contiguous, start <= L - n - 1
        starts.add(int(gone[0]))
        assert (seg[b][seg[b] != 0] == Xn[b][seg[b] != 0]).all()
        assert (pos[b, :L - n] == 0).all() and (pos[b, L - n:] == Xn[b, gone]).all()     # right-aligned, zeros elsewhere
        assert (neg[b, :L - n] == 0).all()
        src = [r for r in range(Xn.shape[0]) if any((neg[b, L - n:] == Xn[r, s:s + n]).all() for s in range(L - n))]
        assert src and ((b in src) if sp_negative == "same_row" else (b not in src)), (b, src)
    assert 0 in starts


# ------------------------------------------------------------------------------------------------ end to end
ISSUE_SHAPE = ["model_name=S3Rec", "synthetic=40x60x9", "max_seq_len=6", "pretrain=true", "pretrain_epochs=2", "epochs=1",
               "device=cuda"]


@pytest.mark.parametrize("fast_loader", [True, False])
def test_train_main_with_pretraining(device, tmp_path, fast_loader):
    """``train.main`` with ``pretrain=true`` through both loaders: it finishes, leaves both checkpoint files and
    returns finite metrics.  The frame is ``synthetic=300x200x12`` (the one tests/test_gpu_s3rec_batches.py runs), not
    the ``40x60x9`` of the stated run: the evaluation that ends ``train.main`` draws 99 mutually distinct negatives
    per user (reference s3rec_dataset.py:21-29), which 60 items cannot give — the host loader's rejection loop never
    ends there, as the reference's does not, and the device loader raises — and a frame of 40 users leaves items of
    a larger catalogue without an interaction, which the device loader refuses too.  Everything else is the stated
    run; the 60-item shape itself pre-trains and fine-tunes in the test below."""
    from yelprecommendation_amd import train
    args = [a if not a.startswith("synthetic=") else "synthetic=300x200x12" for a in ISSUE_SHAPE]
    metrics = train.main(args + [f"fast_loader={'true' if fast_loader else 'false'}", f"model_dir={tmp_path}"])
    assert (tmp_path / "best_pretrain_model.pt").exists() and (tmp_path / "best_model.pt").exists()
    assert len(metrics) == 4 and all(np.isfinite(m) for m in metrics)


@pytest.mark.parametrize("fast_loader", [True, False])
def test_the_stated_shape_pretrains_and_finetunes(device, tmp_path, fast_loader):
    """``synthetic=40x60x9 max_seq_len=6`` as far as 60 items can go: train.py's own steps up to the evaluation —
    pre-train on the train loader, load the best pre-trained model, fine-tune from it."""
    from torch.utils.data import DataLoader
    from yelprecommendation_amd import train
    from yelprecommendation_amd.trainers.s3rec_trainer import S3RecPreTrainer, S3RecTrainer
    from yelprecommendation_amd.utils import make_config
    over = train._parse_overrides(ISSUE_SHAPE[1:] + [f"model_dir={tmp_path}"])
    cfg = make_config("S3Rec", **over)
    args = train.build(cfg)
    if fast_loader:
        from yelprecommendation_amd.data.s3rec_batches import S3RecBatchLoader
        store = args.train_dataset.to_sequences(device, cfg.max_seq_len, seed=cfg.seed)
        loaders = [S3RecBatchLoader(store, m, cfg.batch_size, shuffle=cfg.shuffle, seed=cfg.seed) for m in ("train", "valid")]
    else:
        loaders = [DataLoader(d, batch_size=cfg.batch_size, shuffle=cfg.shuffle) for d in (args.train_dataset, args.valid_dataset)]
    attrs = (args.model_info["num_items"], args.data_pipeline.item2attributes, args.data_pipeline.attributes_count)
    pre = S3RecPreTrainer(cfg, *attrs)
    first = pre.train(loaders[0])
    pre.pretrain(loaders[0])
    assert np.isfinite(first) and (tmp_path / "best_pretrain_model.pt").exists()
    pre.load_best_model()
    tuner = S3RecTrainer(cfg, *attrs)
    for (k, a), (_, b) in zip(tuner.model.state_dict().items(), pre.model.state_dict().items()):
        assert torch.equal(a, b), k                                  # fine-tuning starts from the pre-trained model
    tuner.run(*loaders)
    assert (tmp_path / "best_model.pt").exists()
