"""GPU: the S3Rec scoring kernels (csrc/s3rec.hip) against the float64 restatement (tests/s3rec_ref64.py) on its case
list, the model and the trainer against what the reference recorded (tests/golden/s3rec_small.npz), the bitwise
properties of the encoder and the refusals.  Bars: s3rec_ref64's, 8 x the restatement's own float32 error per case
and tensor (tests/test_s3rec_ref64.py shows what that bar still catches)."""
import functools
import os
import types

import numpy as np
import pytest
import torch

import s3rec_ref64 as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s3rec_small.npz")
GUARD = 256


def _cfg(E, L, heads, blocks, **kw):
    base = dict(embed_size=E, max_seq_len=L, num_heads=heads, num_blocks=blocks, dropout_ratio=0.1, device="cuda")
    base.update(kw)
    return types.SimpleNamespace(**base)


def _model(params, E, L, heads, blocks, device):
    from yelprecommendation_amd.models.s3rec import S3Rec
    num_items = params["item_embedding.weight"].shape[0] - 1
    model = S3Rec(_cfg(E, L, heads, blocks), num_items, params["attribute_embedding.weight"].shape[0])
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}, strict=True)
    return model.to(device).eval()


@functools.lru_cache(maxsize=None)
def _reference(index):
    """(params, batch, float64 outputs, bars) of a case, computed once and shared."""
    case = ref.CASES[index]
    p = ref.make_params(case["E"], case["L"], case["heads"], case["blocks"], seed=index)
    b = ref.make_batch(case)
    o64 = ref.case_outputs(case, np.float64, params=p, batch=b)
    o32 = ref.case_outputs(case, np.float32, params=p, batch=b)
    bars = {k: ref.bar(o32[k], o64[k]) for k in o64}
    for v in o64.values():
        v.setflags(write=False)
    return p, b, o64, bars


def _guarded(shape, device):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), ref.SENTINEL, dtype=torch.float32, device=device)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == ref.SENTINEL).all()) and bool((buf[-GUARD:] == ref.SENTINEL).all())


def _close(name, got, want, bar):
    err = float(np.max(np.abs(got.double().cpu().numpy() - want)))
    print(f"{name}: max|err| {err:.3e}, bar {bar:.3e}, err/bar {err / bar:.3f}")
    assert np.isfinite(err) and err <= bar, f"{name}: {err:.3e} > bar {bar:.3e}"


@pytest.mark.parametrize("case", ref.CASES, ids=[c["id"] for c in ref.CASES])
def test_kernels_match_ref64(device, case):
    from yelprecommendation_amd import engine
    p, b, o64, bars = _reference(case["index"])
    E, L, B, C = case["E"], case["L"], case["B"], case["C"]
    model = _model(p, E, L, case["heads"], case["blocks"], device)
    t = {k: torch.from_numpy(v).to(device) for k, v in b.items()}
    table, pos_enc, packed = model.item_embedding.weight.detach(), model.positional_encoding.detach(), model._params()
    flag = engine.new_error_flag(device)

    buf, h = _guarded((B, L, E), device)
    engine.s3rec_encode(table, pos_enc, packed, t["X"], case["heads"], case["blocks"], out=h, err_flag=flag)
    assert _guards_intact(buf)
    _close(f"{case['id']} h", h, o64["h"], bars["h"])                      # every position of every sequence

    lbuf, h_last = _guarded((B, E), device)
    engine.s3rec_encode(table, pos_enc, packed, t["X"], case["heads"], case["blocks"], last_only=True, out=h_last,
                        err_flag=flag)
    assert _guards_intact(lbuf) and torch.equal(h_last, h[:, L - 1])

    pbuf, sp = _guarded((B * L,), device)
    nbuf, sn = _guarded((B * L,), device)
    engine.s3rec_seq_scores(table, h, t["pos_items"], t["neg_items"], out=(sp, sn), err_flag=flag)
    assert _guards_intact(pbuf) and _guards_intact(nbuf)
    _close(f"{case['id']} seq", torch.stack([sp, sn]), o64["seq"], bars["seq"])

    pbuf, cp = _guarded((B, 1), device)
    nbuf, cn = _guarded((B, C), device)
    engine.s3rec_candidate_scores(table, h_last, t["pos_item"], t["cand"], out=(cp, cn), err_flag=flag)
    assert _guards_intact(pbuf) and _guards_intact(nbuf)
    _close(f"{case['id']} cand", torch.cat([cp, cn], dim=1), o64["cand"], bars["cand"])
    assert int(flag.item()) == 0

    # the model's surface gives the same numbers in the reference's shapes
    with torch.no_grad():
        mp, mn = model.finetune(t["X"], t["pos_items"], t["neg_items"])
        ep, en = model.evaluate(t["X"], t["pos_item"], t["cand"])
    assert mp.shape == (B * L,) and mn.shape == (B * L,) and ep.shape == (B, 1) and en.shape == (B, C)
    assert torch.equal(mp, sp) and torch.equal(mn, sn) and torch.equal(ep, cp) and torch.equal(en, cn)
    model.check_indices()


# ------------------------------------------------------------------------------------------------ golden
@pytest.fixture(scope="module")
def golden(device):
    g = np.load(GOLDEN)
    cfg = dict(zip(g["cfg_names"].tolist(), g["cfg_values"].tolist()))
    state = {k[5:]: g[k] for k in g.files if k.startswith("pert:")}
    return g, cfg, state


def test_model_matches_the_float64_record(device, golden):
    g, cfg, state = golden
    E, L, hb = cfg["embed_size"], cfg["max_seq_len"], (cfg["num_heads"], cfg["num_blocks"])
    model = _model(state, E, L, *hb, device)
    with torch.no_grad():
        for i in range(3):
            args = [g[f"valid{i}_{k}"] for k in ("X", "pos_items", "neg_items")]
            got = model.finetune(*(torch.from_numpy(a).to(device) for a in args))
            r32 = ref.finetune(state, *args, *hb, dtype=np.float32)
            r64 = ref.finetune(state, *args, *hb, dtype=np.float64)
            assert got[0].shape == got[1].shape == g[f"valid{i}_pos_preds_f64"].shape
            rec = np.stack([g[f"valid{i}_pos_preds_f64"], g[f"valid{i}_neg_preds_f64"]])
            _close(f"valid{i}", torch.stack(got), rec, ref.bar(np.stack(r32), np.stack(r64)))
        for i in range(2):
            args = [g[f"test{i}_{k}"] for k in ("X", "pos_item", "neg_items")]
            got = model.evaluate(*(torch.from_numpy(a).to(device) for a in args))
            r32 = ref.evaluate(state, *args, *hb, dtype=np.float32)
            r64 = ref.evaluate(state, *args, *hb, dtype=np.float64)
            for name, v in zip(("pos_pred", "neg_preds"), got):
                assert tuple(v.shape) == g[f"test{i}_{name}_f64"].shape
            rec = np.concatenate([g[f"test{i}_pos_pred_f64"], g[f"test{i}_neg_preds_f64"]], axis=1)
            _close(f"test{i}", torch.cat(got, dim=1), rec,
                   ref.bar(np.concatenate(r32, axis=1), np.concatenate(r64, axis=1)))
    model.check_indices()


def test_trainer_matches_the_recorded_loss_and_metrics(device, golden, tmp_path):
    from yelprecommendation_amd.trainers.s3rec_trainer import S3RecTrainer
    g, cfg, state = golden

    class Cfg(dict):
        __getattr__ = dict.__getitem__
    tcfg = Cfg(embed_size=cfg["embed_size"], max_seq_len=cfg["max_seq_len"], num_heads=cfg["num_heads"],
               num_blocks=cfg["num_blocks"], dropout_ratio=0.1, device="cuda", model_dir=str(tmp_path),
               top_n=cfg["top_n"], best_metric="loss", load_pretrain=True)
    # a checkpoint as the reference saves it, picked up by name at construction
    torch.save({k: torch.from_numpy(v) for k, v in state.items()}, tmp_path / "best_pretrain_model.pt")
    trainer = S3RecTrainer(tcfg, cfg["num_items"], None, cfg["attributes_count"])
    valid = [{k: torch.from_numpy(g[f"valid{i}_{k}"]) for k in ("X", "pos_items", "neg_items")} for i in range(3)]
    test = [{k: torch.from_numpy(g[f"test{i}_{k}"]) for k in ("X", "pos_item", "neg_items")} for i in range(2)]
    loss = trainer.validate(valid)
    print(f"validate {loss:.9f}, recorded {float(g['validate']):.9f}")
    assert abs(loss - float(g["validate"])) <= 1e-5 * abs(float(g["validate"]))
    metrics = trainer.evaluate(test)
    np.testing.assert_allclose(np.asarray(metrics, dtype=np.float64), g["test_metrics"], rtol=0, atol=1e-12)
    torch.save(trainer.model.state_dict(), tmp_path / "best_model.pt")
    trainer.load_best_model()
    assert trainer.validate(valid) == loss


# ------------------------------------------------------------------------------------------------ properties
def _big_case():
    return next(c for c in ref.CASES if c["B"] == 257)


def test_a_sequence_alone_equals_itself_inside_a_batch(device):
    case = _big_case()
    p, b, _, _ = _reference(case["index"])
    model = _model(p, case["E"], case["L"], case["heads"], case["blocks"], device)
    X = torch.from_numpy(b["X"]).to(device)
    with torch.no_grad():
        whole = model._encode(X, last_only=False)
        again = model._encode(X, last_only=False)
        assert torch.equal(whole, again)                         # two calls, one answer
        for row in (0, 1, 2, 128, 256):
            alone = model._encode(X[row:row + 1].contiguous(), last_only=False)
            assert torch.equal(alone[0], whole[row]), row


def test_a_later_item_changes_no_earlier_position(device):
    case = next(c for c in ref.CASES if (c["E"], c["L"], c["B"]) == (64, 50, 3))
    p, b, _, _ = _reference(case["index"])
    model = _model(p, case["E"], case["L"], case["heads"], case["blocks"], device)
    X = torch.from_numpy(b["X"]).to(device)
    L = case["L"]
    with torch.no_grad():
        base = model._encode(X, last_only=False)
        for j in (1, 31, 32, 33, L - 1):
            Y = X.clone()
            Y[:, j] = torch.where(Y[:, j] > 0, torch.zeros_like(Y[:, j]), torch.full_like(Y[:, j], 7))   # real <-> padding
            h = model._encode(Y, last_only=False)
            assert torch.equal(h[:, :j], base[:, :j]), j
            assert not torch.equal(h[:, j:], base[:, j:]), j


def test_repacks_when_a_parameter_is_written(device):
    case = next(c for c in ref.CASES if (c["E"], c["L"], c["B"]) == (16, 7, 3))
    p, b, _, _ = _reference(case["index"])
    model = _model(p, case["E"], case["L"], case["heads"], case["blocks"], device)
    X = torch.from_numpy(b["X"]).to(device)
    with torch.no_grad():
        model._encode(X, last_only=False)
        packed = model._params()
        assert model._params() is packed                         # nothing written: no second copy
        model.ffn1s[0].bias.add_(0.25)
        p2 = dict(p)
        p2["ffn1s.0.bias"] = p["ffn1s.0.bias"] + np.float32(0.25)
        h = model._encode(X, last_only=False)
    want = ref.encode(p2, b["X"], case["heads"], case["blocks"])
    _close("after an in-place write", h, want, ref.bar(ref.encode(p2, b["X"], case["heads"], case["blocks"],
                                                                   dtype=np.float32), want))


# ------------------------------------------------------------------------------------------------ refusals
def test_training_is_refused(device):
    case = next(c for c in ref.CASES if (c["E"], c["L"], c["B"]) == (16, 7, 3))
    p, b, _, _ = _reference(case["index"])
    model = _model(p, case["E"], case["L"], case["heads"], case["blocks"], device)
    t = {k: torch.from_numpy(v).to(device) for k, v in b.items()}
    with pytest.raises(NotImplementedError, match="training is not built"):
        model.finetune(t["X"], t["pos_items"], t["neg_items"])                 # eval() mode, grad enabled
    model.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="training is not built"):
        model.evaluate(t["X"], t["pos_item"], t["cand"])                       # no_grad, training mode
    from yelprecommendation_amd.models.s3rec import S3Rec
    for bad in (dict(E=48), dict(L=65), dict(heads=5), dict(blocks=5)):
        shape = dict(E=32, L=12, heads=2, blocks=2)
        shape.update(bad)
        with pytest.raises(NotImplementedError, match="S3Rec"):
            S3Rec(_cfg(**shape), 100, 7)


def test_a_bad_id_raises_the_flag_and_reads_nothing(device):
    case = next(c for c in ref.CASES if (c["E"], c["L"], c["B"]) == (16, 7, 3))
    p, b, o64, bars = _reference(case["index"])
    model = _model(p, case["E"], case["L"], case["heads"], case["blocks"], device)
    t = {k: torch.from_numpy(v).to(device) for k, v in b.items()}
    with torch.no_grad():
        for bad in (ref.NUM_ITEMS + 1, 1 << 40, -3):
            X = t["X"].clone()
            X[2, 3] = bad
            h = model._encode(X, last_only=False)
            assert bool(torch.isfinite(h).all())
            assert torch.equal(h[:2], model._encode(t["X"], last_only=False)[:2])      # the other sequences are untouched
            with pytest.raises(IndexError, match="item"):
                model.check_indices()
            model.check_indices()                                                      # the flag was cleared
            pos = t["pos_items"].clone()
            pos[1, 2] = bad
            sp, _ = model.finetune(t["X"], pos, t["neg_items"])
            assert float(sp[1 * case["L"] + 2]) == 0.0
            with pytest.raises(IndexError, match="item"):
                model.check_indices()
            cand = t["cand"].clone()
            cand[0, 0] = bad
            _, cn = model.evaluate(t["X"], t["pos_item"], cand)
            assert float(cn[0, 0]) == 0.0
            with pytest.raises(IndexError, match="item"):
                model.check_indices()
