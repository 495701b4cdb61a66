"""GPU: S3Rec training (csrc/s3rec.hip: yr_s3rec_encode_train, yr_s3rec_backward, yr_s3rec_score_grad,
yr_s3rec_item_grad and the gradient products / column sums around them) against the float64 torch restatement
(tests/s3rec_grad_ref64.py) on its configurations, the model's autograd surface and the trainer against what the
reference recorded (tests/golden/s3rec_train_small.npz), the bitwise properties and the refusals.  Bars:
s3rec_grad_ref64's, 8 x the restatement's own float32 error per configuration and tensor (tests/
test_s3rec_grad_ref64.py shows what that bar still catches)."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest
import torch

import s3rec_grad_ref64 as gr
import s3rec_ref64 as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "s3rec_small.npz")
GOLDEN_TRAIN = os.path.join(HERE, "golden", "s3rec_train_small.npz")
GUARD = 256
CONFIGS = gr.configs()
IDS = [gr.config_id(c, p) for c, p in CONFIGS]
SEED = gr.DROPOUT_SEED


def _cfg(E, L, heads, blocks, p=0.0):
    return types.SimpleNamespace(embed_size=E, max_seq_len=L, num_heads=heads, num_blocks=blocks, dropout_ratio=p,
                                 device="cuda")


def _model(params, case, device, p=0.0):
    from yelprecommendation_amd.models.s3rec import S3Rec
    num_items = params["item_embedding.weight"].shape[0] - 1
    model = S3Rec(_cfg(case["E"], case["L"], case["heads"], case["blocks"], p), num_items,
                  params["attribute_embedding.weight"].shape[0])
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}, strict=True)
    return model.to(device)


@functools.lru_cache(maxsize=None)
def _reference(index, p):
    """(params, batch, float64 result, gradient bars, forward bar) of a configuration, computed once and shared."""
    case = ref.CASES[index]
    params, batch = gr.case_setup(case)
    hb = (case["heads"], case["blocks"])
    r64 = gr.loss_and_grads(params, batch, *hb, dtype=torch.float64, p_drop=p, seed=SEED)
    r32 = gr.loss_and_grads(params, batch, *hb, dtype=torch.float32, p_drop=p, seed=SEED)
    for v in r64["grads"].values():
        if v is not None:
            v.setflags(write=False)
    return params, batch, r64, gr.bars(r32["grads"], r64["grads"]), ref.bar(r32["h"], r64["h"])


def _guarded(shape, device):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), ref.SENTINEL, dtype=torch.float32, device=device)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == ref.SENTINEL).all()) and bool((buf[-GUARD:] == ref.SENTINEL).all())


def _ratio(name, got, want, bar):
    """max |err| / bar, printed; a zero bar (both restatements exactly zero) asks for exactly zero."""
    err = float(np.max(np.abs(got.double().cpu().numpy().reshape(want.shape) - want)))
    print(f"{name}: max|err| {err:.3e}, bar {bar:.3e}, err/bar {err / bar if bar > 0 else (0.0 if err == 0 else np.inf):.3f}")
    assert np.isfinite(err) and err <= bar, f"{name}: {err:.3e} > bar {bar:.3e}"


def _check_grads(what, got, r64, bars):
    """Every tensor is measured and printed before the first one over its bar fails the test."""
    assert sorted(got) == sorted(bars), what
    over = []
    for name, g in got.items():
        try:
            _ratio(f"{what} {gr.group(name)} {name}", g, r64["grads"][name], bars[name])
        except AssertionError as e:
            over.append(str(e))
    assert not over, "\n".join(over)


def _engine_grads(model, case, t, p, device, guards=False):
    """Every gradient through the engine entry points: {state_dict name: tensor}, plus h and d_emb."""
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.loss import BPRLoss
    E, L, B, heads, blocks = case["E"], case["L"], case["B"], case["heads"], case["blocks"]
    table, pos_enc, packed = model.item_embedding.weight.detach(), model.positional_encoding.detach(), model._params()
    flag = engine.new_error_flag(device)
    n_ws = engine.s3rec_train_workspace_floats(B, L, E, heads, blocks)
    wbuf, ws = _guarded((n_ws,), device)
    hbuf, h = _guarded((B, L, E), device)
    engine.s3rec_encode_train(table, pos_enc, packed, t["X"], heads, blocks, seed=SEED, p=p, workspace=ws, out=h,
                              err_flag=flag)
    pos, neg = engine.s3rec_seq_scores(table, h, t["pos_items"], t["neg_items"], err_flag=flag)
    pos, neg = pos.requires_grad_(), neg.requires_grad_()
    BPRLoss()(pos, neg).backward()
    dh = engine.s3rec_score_grad(table, t["pos_items"], t["neg_items"], pos.grad, neg.grad, err_flag=flag)
    dbuf, d_emb = _guarded((B, L, E), device)
    engine.s3rec_backward(packed, t["X"], dh.view(B, L, E), ws, heads, blocks, seed=SEED, p=p, d_emb=d_emb)
    packed_grad = engine.s3rec_param_grads(ws, B, L, E, heads, blocks)
    d_pos = engine.colsum(d_emb.view(B, L * E)).view(L, E)
    d_item = torch.zeros_like(table)
    engine.s3rec_item_grad(t["X"], t["pos_items"], t["neg_items"], d_emb, h, pos.grad, neg.grad, d_item, err_flag=flag)
    if guards:
        assert _guards_intact(wbuf) and _guards_intact(hbuf) and _guards_intact(dbuf)
    assert int(flag.item()) == 0
    grads = {"item_embedding.weight": d_item, "positional_encoding": d_pos}
    by_tensor = {id(v): k for k, v in model.named_parameters()}
    at = 0
    for tensor in model._block_tensors():
        n = tensor.numel()
        grads[by_tensor[id(tensor)]] = packed_grad[at:at + n].view(tensor.shape)
        at += n
    assert at == packed_grad.numel()
    return grads, h, d_emb


# ------------------------------------------------------------------------------------------------ the forward
@pytest.mark.parametrize("case,p", CONFIGS, ids=IDS)
def test_encode_train_matches(device, case, p):
    from yelprecommendation_amd import engine
    params, batch, r64, _, hbar = _reference(case["index"], p)
    E, L, B, heads, blocks = case["E"], case["L"], case["B"], case["heads"], case["blocks"]
    model = _model(params, case, device)
    X = torch.from_numpy(batch["X"]).to(device)
    table, pos_enc, packed = model.item_embedding.weight.detach(), model.positional_encoding.detach(), model._params()
    n_ws = engine.s3rec_train_workspace_floats(B, L, E, heads, blocks)
    assert n_ws == blocks * B * L * ((12 + 8 * heads) * E + 4)
    wbuf, ws = _guarded((n_ws,), device)
    hbuf, h = _guarded((B, L, E), device)
    engine.s3rec_encode_train(table, pos_enc, packed, X, heads, blocks, seed=SEED, p=p, workspace=ws, out=h)
    assert _guards_intact(wbuf) and _guards_intact(hbuf)
    if p == 0:
        assert torch.equal(h, engine.s3rec_encode(table, pos_enc, packed, X, heads, blocks))    # bit for bit
    _ratio(f"{gr.config_id(case, p)} h", h, r64["h"], hbar)
    views = engine.s3rec_workspace_views(ws, B, L, E, heads, blocks)
    assert torch.equal(views[0]["h_in"].view(B, L, E), table[X.clamp(min=0)] + pos_enc)           # one f32 addition


# ------------------------------------------------------------------------------------------------ the gradients
@pytest.mark.parametrize("case,p", CONFIGS, ids=IDS)
def test_every_gradient_matches_ref64(device, case, p):
    from yelprecommendation_amd.loss import BPRLoss
    params, batch, r64, bars, _ = _reference(case["index"], p)
    t = {k: torch.from_numpy(v).to(device) for k, v in batch.items()}
    cid = gr.config_id(case, p)
    model = _model(params, case, device, p)
    grads, _, _ = _engine_grads(model, case, t, p, device, guards=True)
    _check_grads(f"{cid} engine", grads, r64, bars)

    # the model's surface: finetune + BPRLoss + backward
    model.train()
    pos, neg = model.finetune(t["X"], t["pos_items"], t["neg_items"], dropout_seed=SEED)
    assert pos.shape == neg.shape == (case["B"] * case["L"],) and pos.requires_grad
    loss = BPRLoss()(pos, neg)
    loss.backward()
    model.check_indices()
    got = {k: v.grad for k, v in model.named_parameters() if v.grad is not None}
    assert sorted(k for k, v in model.named_parameters() if v.grad is None) == \
        sorted(k for k, v in r64["grads"].items() if v is None)
    _check_grads(f"{cid} model", got, r64, bars)


# ------------------------------------------------------------------------------------------------ properties
def _big():
    return next(c for c in ref.CASES if c["B"] == 257)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_two_calls_one_answer_and_a_sequence_alone(device, p):
    case = _big()
    params, batch, _, bars, _ = _reference(case["index"], p)
    t = {k: torch.from_numpy(v).to(device) for k, v in batch.items()}
    model = _model(params, case, device, p)
    g1, h1, d1 = _engine_grads(model, case, t, p, device)
    g2, h2, d2 = _engine_grads(model, case, t, p, device)
    assert torch.equal(h1, h2) and torch.equal(d1, d2)
    for name in g1:
        assert torch.equal(g1[name], g2[name]), name            # the item table too: its sums run in a fixed order
    if p > 0:
        g3, h3, _ = _engine_grads(_model(params, case, device, 0.0), case, t, 0.0, device)
        assert not torch.equal(h1, h3)
    # a sequence's d_emb alone equals its d_emb inside the batch, bit for bit: same dh_out, its own row of the masks
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.loss import BPRLoss
    E, L, B, heads, blocks = case["E"], case["L"], case["B"], case["heads"], case["blocks"]
    table, pos_enc, packed = model.item_embedding.weight.detach(), model.positional_encoding.detach(), model._params()
    pos, neg = engine.s3rec_seq_scores(table, h1, t["pos_items"], t["neg_items"])
    pos, neg = pos.requires_grad_(), neg.requires_grad_()
    BPRLoss()(pos, neg).backward()
    dh = engine.s3rec_score_grad(table, t["pos_items"], t["neg_items"], pos.grad, neg.grad).view(B, L, E)
    rows = (0,) if p > 0 else (0, 1, 2, 128, 256)     # the mask depends on the flat index: only row 0 keeps its own
    for row in rows:
        X1 = t["X"][row:row + 1].contiguous()
        h, ws = engine.s3rec_encode_train(table, pos_enc, packed, X1, heads, blocks, seed=SEED, p=p)
        assert torch.equal(h[0], h1[row]), row
        alone = engine.s3rec_backward(packed, X1, dh[row:row + 1].contiguous(), ws, heads, blocks, seed=SEED, p=p)
        assert torch.equal(alone[0], d1[row]), row


def test_gradients_accumulate_over_two_backward_calls(device):
    from yelprecommendation_amd.loss import BPRLoss
    case = next(c for c in ref.CASES if (c["E"], c["L"], c["B"]) == (16, 7, 3))
    params, batch, r64, bars, _ = _reference(case["index"], 0.0)
    t = {k: torch.from_numpy(v).to(device) for k, v in batch.items()}
    model = _model(params, case, device).train()                    # dropout_ratio 0
    for _ in range(2):
        BPRLoss()(*model.finetune(t["X"], t["pos_items"], t["neg_items"])).backward()
    for name, prm in model.named_parameters():
        if prm.grad is not None:
            _ratio(f"twice {name}", prm.grad, 2 * r64["grads"][name], 2 * bars[name])


def test_eval_mode_is_for_scoring(device):
    case = next(c for c in ref.CASES if (c["E"], c["L"], c["B"]) == (16, 7, 3))
    params, batch, _, _, _ = _reference(case["index"], 0.0)
    t = {k: torch.from_numpy(v).to(device) for k, v in batch.items()}
    model = _model(params, case, device).eval()
    with pytest.raises(NotImplementedError, match="train\\(\\)"):
        model.finetune(t["X"], t["pos_items"], t["neg_items"])
    with torch.no_grad():
        pos, _ = model.finetune(t["X"], t["pos_items"], t["neg_items"])
    assert not pos.requires_grad
    assert torch.equal(pos, model.train().finetune(t["X"], t["pos_items"], t["neg_items"])[0].detach())   # p = 0


def test_dropout_draws_a_fresh_repeatable_seed(device):
    case = next(c for c in ref.CASES if (c["E"], c["L"], c["B"]) == (16, 7, 3))
    params, batch, _, _, _ = _reference(case["index"], 0.0)
    t = {k: torch.from_numpy(v).to(device) for k, v in batch.items()}

    def two_calls():
        torch.manual_seed(1234)
        model = _model(params, case, device, 0.5).train()
        return [model.finetune(t["X"], t["pos_items"], t["neg_items"])[0].detach() for _ in range(2)]
    a, b = two_calls(), two_calls()
    assert not torch.equal(a[0], a[1])                              # a fresh seed per call
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])      # the same stream under the same torch seed


# ------------------------------------------------------------------------------------------------ bad ids
@pytest.mark.parametrize("where", ["X", "pos_items", "neg_items"])
def test_a_bad_id_raises_and_leaves_the_other_rows(device, where):
    """A bad id reads a zero embedding row and receives nothing: the restatement with one more (zero) row in the table,
    the bad id pointing at it, gives the gradients of every real row."""
    from yelprecommendation_amd.loss import BPRLoss
    case = next(c for c in ref.CASES if (c["E"], c["L"], c["B"]) == (32, 33, 3) and c["heads"] == 2 and c["blocks"] == 2)
    params, batch = gr.case_setup(case)
    hb = (case["heads"], case["blocks"])
    bad = {k: v.copy() for k, v in batch.items()}
    bad[where][2, 5] = ref.NUM_ITEMS + 9
    model = _model(params, case, device).train()
    t = {k: torch.from_numpy(v).to(device) for k, v in bad.items()}
    BPRLoss()(*model.finetune(t["X"], t["pos_items"], t["neg_items"])).backward()
    with pytest.raises(IndexError, match="S3Rec"):
        model.check_indices()
    model.check_indices()                                            # the flag is cleared
    ext = dict(params)
    ext["item_embedding.weight"] = np.concatenate([params["item_embedding.weight"],
                                                   np.zeros((1, case["E"]), np.float32)])
    twin = {k: v.copy() for k, v in batch.items()}
    twin[where][2, 5] = ref.NUM_ITEMS + 1
    r64 = gr.loss_and_grads(ext, twin, *hb, dtype=torch.float64)
    r32 = gr.loss_and_grads(ext, twin, *hb, dtype=torch.float32)
    for r in (r64, r32):
        r["grads"]["item_embedding.weight"] = r["grads"]["item_embedding.weight"][:-1]
    bars = gr.bars(r32["grads"], r64["grads"])
    _check_grads(f"bad {where}", {k: v.grad for k, v in model.named_parameters() if v.grad is not None}, r64, bars)


# ------------------------------------------------------------------------------------------------ the trainer
@pytest.fixture(scope="module")
def golden():
    g, t = np.load(GOLDEN), np.load(GOLDEN_TRAIN)
    cfg = dict(zip(g["cfg_names"].tolist(), g["cfg_values"].tolist()))
    state = {k[5:]: g[k] for k in g.files if k.startswith("pert:")}
    batches = [{k: g[f"valid{i}_{k}"] for k in ("X", "pos_items", "neg_items")} for i in range(3)]
    return cfg, state, batches, t


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _trainer(cfg, state, tmp_path, **kw):
    from yelprecommendation_amd.trainers.s3rec_trainer import S3RecTrainer
    tcfg = Cfg(embed_size=cfg["embed_size"], max_seq_len=cfg["max_seq_len"], num_heads=cfg["num_heads"],
               num_blocks=cfg["num_blocks"], dropout_ratio=0.0, device="cuda", model_dir=str(tmp_path),
               top_n=cfg["top_n"], best_metric="loss", load_pretrain=True, optimizer="adam", lr=1e-3, epochs=2,
               patience=5)
    tcfg.update(kw)
    os.makedirs(tmp_path, exist_ok=True)
    torch.save({k: torch.from_numpy(v) for k, v in state.items()}, tmp_path / "best_pretrain_model.pt")
    return S3RecTrainer(tcfg, cfg["num_items"], None, cfg["attributes_count"])


def test_model_gradients_match_the_record(device, golden):
    from yelprecommendation_amd.loss import BPRLoss
    cfg, state, batches, t = golden
    case = dict(E=cfg["embed_size"], L=cfg["max_seq_len"], heads=cfg["num_heads"], blocks=cfg["num_blocks"])
    model = _model(state, case, device).train()
    b = {k: torch.from_numpy(v).to(device) for k, v in batches[0].items()}
    BPRLoss()(*model.finetune(b["X"], b["pos_items"], b["neg_items"])).backward()
    hb = (case["heads"], case["blocks"])
    r64 = gr.loss_and_grads(state, batches[0], *hb, dtype=torch.float64)
    r32 = gr.loss_and_grads(state, batches[0], *hb, dtype=torch.float32)
    bars = gr.bars(r32["grads"], r64["grads"])
    assert sorted(k for k, v in model.named_parameters() if v.grad is None) == sorted(t["grad_none"].tolist())
    for name, prm in model.named_parameters():
        if prm.grad is not None:
            _ratio(f"record {name}", prm.grad, t[f"grad64:{name}"], bars[name])


def test_trainer_reproduces_the_recorded_epochs(device, golden, tmp_path):
    cfg, state, batches, t = golden
    hb = (cfg["num_heads"], cfg["num_blocks"])
    epochs, lr = int(t["epochs"]), float(t["lr"])
    l64, s64 = gr.train(state, batches, *hb, epochs, lr, torch.float64)
    l32, s32 = gr.train(state, batches, *hb, epochs, lr, torch.float32)
    trainer = _trainer(cfg, state, tmp_path)
    data = [{k: torch.from_numpy(v) for k, v in b.items()} for b in batches]
    losses = [trainer.train(data) for _ in range(epochs)]
    # An epoch's loss is the sum of its batch losses.  The bar of ONE batch loss, from all of them as one tensor (a
    # maximum needs samples: a single |f32 - f64| can be anything down to zero), times the batches of an epoch.
    per_loss = gr.BAR_FACTOR * max(abs(a - b) for e in range(epochs) for a, b in zip(l32[e], l64[e]))
    bar = len(batches) * per_loss
    over = []
    for e in range(epochs):
        err = abs(losses[e] - float(t["train_losses"][e]))
        print(f"epoch {e}: loss {losses[e]:.9f}, recorded {float(t['train_losses'][e]):.9f}, float64 restatement "
              f"{sum(l64[e]):.9f}, err {err:.3e}, bar {bar:.3e}, err/bar {err / bar:.3f}")
        assert abs(float(t["train_losses"][e]) - sum(l64[e])) <= bar      # the record itself lies inside
        if err > bar:
            over.append(f"epoch {e}: {err:.3e} > {bar:.3e}")
    final = trainer.model.state_dict()
    assert sorted(final) == sorted(s64)
    for name in s64:
        bar = gr.BAR_FACTOR * float(np.max(np.abs(s32[name].astype(np.float64) - s64[name])))
        try:
            _ratio(f"final {gr.group(name)} {name}", final[name], t[f"final:{name}"].astype(np.float64), bar)
        except AssertionError as e:
            over.append(str(e))
    assert not over, "\n".join(over)


def test_run_saves_the_best_model_and_validate_sees_the_step(device, golden, tmp_path):
    from yelprecommendation_amd.models.s3rec import S3Rec
    cfg, state, batches, _ = golden
    trainer = _trainer(cfg, state, tmp_path)
    data = [{k: torch.from_numpy(v) for k, v in b.items()} for b in batches]
    before = trainer.validate(data)
    packed = trainer.model._params()
    trainer.train(data)
    assert trainer.model._params() is not packed                     # the step wrote the parameters: re-packed
    after = trainer.validate(data)
    assert after < before                                            # three Adam steps on the same batches
    fresh = S3Rec(trainer.cfg, cfg["num_items"], cfg["attributes_count"])
    fresh.load_state_dict(trainer.model.state_dict(), strict=True)
    trainer2 = _trainer(cfg, state, tmp_path / "b")
    trainer2.model = fresh.to(device)
    assert trainer2.validate(data) == after                          # validate used the stepped parameters
    trainer.run(data, data)
    saved = torch.load(tmp_path / "best_model.pt", map_location="cpu", weights_only=True)
    S3Rec(trainer.cfg, cfg["num_items"], cfg["attributes_count"]).load_state_dict(saved, strict=True)
    trainer.load_best_model()
    assert trainer.validate(data) < after


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_without_a_launch(device):
    from yelprecommendation_amd import _lib, engine
    lib = _lib.load()
    B, L, E, H, NB = 2, 12, 32, 2, 2
    n_ws = engine.s3rec_train_workspace_floats(B, L, E, H, NB)
    f = lambda n: torch.zeros(n, dtype=torch.float32, device=device)      # noqa: E731
    table, pos, params, out, ws = f(51 * E), f(L * E), f(NB * engine.s3rec_block_floats(E, H) + 4), f(B * L * E), f(n_ws)
    X = torch.zeros((B, L), dtype=torch.int64, device=device)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                         # noqa: E731

    def fwd(table=ptr(table), pos=ptr(pos), params=ptr(params), X=ptr(X), L=L, E=E, out=ptr(out), ws=ptr(ws), n=n_ws):
        return lib.yr_s3rec_encode_train(table, pos, params, X, B, L, E, H, NB, 50, 0, 0.0, out, ws, n, None, None)

    def bwd(params=ptr(params), X=ptr(X), dh=ptr(out), L=L, E=E, ws=ptr(ws), n=n_ws, d=ptr(out)):
        return lib.yr_s3rec_backward(params, X, dh, B, L, E, H, NB, 0, 0.0, ws, n, d, None)
    bad, unsupported = -2, -1
    for null in ("table", "pos", "params", "X", "out", "ws"):
        assert fwd(**{null: None}) == bad, null
    for null in ("params", "X", "dh", "ws", "d"):
        assert bwd(**{null: None}) == bad, null
    misaligned = ctypes.c_void_p(params.data_ptr() + 4)
    assert fwd(params=misaligned) == bad and bwd(params=misaligned) == bad
    assert fwd(E=48) == unsupported and bwd(E=48) == unsupported
    assert fwd(L=65) == unsupported and bwd(L=65) == unsupported
    assert fwd(n=0) == bad and bwd(n=0) == bad and fwd(n=n_ws - 1) == bad
    assert lib.yr_s3rec_train_workspace_floats(B, L, 48, H, NB) == unsupported
    assert lib.yr_s3rec_train_workspace_floats(B, 65, E, H, NB) == unsupported
    assert lib.yr_s3rec_score_grad(None, ptr(X), ptr(X), ptr(out), ptr(out), B * L, E, 50, ptr(out), None, None) == bad
    assert lib.yr_s3rec_item_grad(ptr(X), ptr(X), ptr(out), ptr(out), ptr(out), ptr(out), B * L, E, 50, ptr(ws), None,
                                  None, None) == bad
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0 and float(ws.abs().sum()) == 0    # nothing ran
