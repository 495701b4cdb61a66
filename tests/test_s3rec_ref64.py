"""CPU: the S3Rec restatement (tests/s3rec_ref64.py) against what the reference recorded (tests/golden/
s3rec_small.npz), the strength of the bar the GPU tests use, the seeded construction of models/s3rec.py and the
argument checks of the three entry points.  No GPU."""
import os
import types

import numpy as np
import pytest
import torch

import s3rec_ref64 as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s3rec_small.npz")


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    cfg = dict(zip(g["cfg_names"].tolist(), g["cfg_values"].tolist()))
    return g, cfg


def _state(g, prefix):
    return {k[len(prefix) + 1:]: g[k] for k in g.files if k.startswith(prefix + ":")}


def _golden_outputs(g, cfg, dtype):
    """[(name, restated, recorded f64, recorded f32)] over the three validation and the two test batches, the scores
    grouped as s3rec_ref64 compares them: (pos_preds, neg_preds) stacked, [pos_pred | neg_preds] side by side."""
    p = _state(g, "pert")
    hb = (cfg["num_heads"], cfg["num_blocks"])
    out = []
    for i in range(3):
        got = ref.finetune(p, g[f"valid{i}_X"], g[f"valid{i}_pos_items"], g[f"valid{i}_neg_items"], *hb, dtype=dtype)
        out.append((f"valid{i}", np.stack(got), *(np.stack([g[f"valid{i}_pos_preds_{t}"], g[f"valid{i}_neg_preds_{t}"]])
                                                   for t in ("f64", "f32"))))
    for i in range(2):
        got = ref.evaluate(p, g[f"test{i}_X"], g[f"test{i}_pos_item"], g[f"test{i}_neg_items"], *hb, dtype=dtype)
        out.append((f"test{i}", np.concatenate(got, axis=1),
                    *(np.concatenate([g[f"test{i}_pos_pred_{t}"], g[f"test{i}_neg_preds_{t}"]], axis=1)
                      for t in ("f64", "f32"))))
    return out


def test_restatement_equals_the_float64_record(golden):
    g, cfg = golden
    for name, got, rec64, _ in _golden_outputs(g, cfg, np.float64):
        assert got.shape == rec64.shape, name
        scale = np.max(np.abs(rec64))
        assert np.max(np.abs(got - rec64)) <= 1e-10 * scale, name


def test_float32_record_is_inside_the_bar(golden):
    """The reference's own float32 run is one more f32 evaluation order: it must sit inside the bar that the
    restatement's float32 run sets."""
    g, cfg = golden
    r64 = _golden_outputs(g, cfg, np.float64)
    r32 = _golden_outputs(g, cfg, np.float32)
    for (name, v64, _, rec32), (_, v32, _, _) in zip(r64, r32):
        assert v32.dtype == np.float32
        bar = ref.bar(v32, v64)
        err = float(np.max(np.abs(rec32.astype(np.float64) - v64)))
        print(f"{name}: reference f32 err {err:.3e}, bar {bar:.3e}")
        assert 0 < bar and err <= bar, name


def test_record_has_no_near_ties(golden):
    g, _ = golden
    for i in range(2):
        s = np.sort(np.concatenate([g[f"test{i}_pos_pred_f64"], g[f"test{i}_neg_preds_f64"]], axis=1), axis=1)
        assert np.diff(s, axis=1).min() >= 1e-4


@pytest.mark.parametrize("case", ref.CASES, ids=[c["id"] for c in ref.CASES])
def test_wrong_semantics_cross_the_bar(case):
    """Each wrong reading in VARIANTS moves the compared tensor of the case by more than the case's bar — the bar
    taken from the unperturbed restatement alone."""
    p = ref.make_params(case["E"], case["L"], case["heads"], case["blocks"], seed=case["index"])
    b = ref.make_batch(case)
    o64 = ref.case_outputs(case, np.float64, params=p, batch=b)
    o32 = ref.case_outputs(case, np.float32, params=p, batch=b)
    bars = {k: ref.bar(o32[k], o64[k]) for k in ("h", "cand")}
    assert bars["h"] > 0 and bars["cand"] > 0
    for variant in ref.VARIANTS:
        if not ref.applies(variant, case):
            continue
        ov = ref.case_outputs(case, np.float64, variant=variant, params=p, batch=b)
        k = "cand" if variant == "evaluate_at_L_minus_2" else "h"
        moved, bar = float(np.max(np.abs(ov[k] - o64[k]))), bars[k]
        print(f"{case['id']} {variant}: moved {moved:.3e}, bar {bar:.3e}, ratio {moved / bar:.1f}")
        assert moved > bar, f"{variant} ({ref.VARIANTS[variant]}) hides under the bar: {moved:.3e} <= {bar:.3e}"


def test_case_list_covers_the_loop_ends():
    seen = {(c["E"], c["L"]) for c in ref.CASES}
    assert {(E, L) for E in ref.WIDTHS for L in ref.LENGTHS} <= seen
    assert {(c["heads"], c["blocks"]) for c in ref.CASES if (c["E"], c["L"]) == (32, 33)} >= {
        (h, b) for h in (1, 2, 4) for b in (1, 3)}
    assert {c["B"] for c in ref.CASES} >= {1, 3, 257} and {c["C"] for c in ref.CASES} == set(ref.CANDIDATES)
    kinds = set()
    for c in ref.CASES:
        X = ref.make_batch(c)["X"]
        assert X.min() >= 0 and X.max() <= ref.NUM_ITEMS
        for row in X:
            real = row > 0
            kinds.add("all_padding" if not real.any() else "full" if real.all() else
                      "one_last" if real.sum() == 1 and real[-1] else "one_first" if real.sum() == 1 and real[0]
                      else "interior")
        kinds.add("last_row") if (X == ref.NUM_ITEMS).all(axis=1).any() else None
    assert kinds >= {"all_padding", "full", "one_last", "one_first", "interior", "last_row"}


def _cfg(**kw):
    base = dict(embed_size=32, max_seq_len=12, num_heads=2, num_blocks=2, dropout_ratio=0.1, device="cpu")
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_seeded_construction_matches_the_reference(golden):
    """Same modules in the same order with the same initialisers: the reference's RNG stream, bit for bit."""
    from yelprecommendation_amd.models.s3rec import S3Rec
    g, cfg = golden
    torch.manual_seed(cfg["seed"])
    model = S3Rec(_cfg(embed_size=cfg["embed_size"], max_seq_len=cfg["max_seq_len"], num_heads=cfg["num_heads"],
                       num_blocks=cfg["num_blocks"]), cfg["num_items"], cfg["attributes_count"])
    want = _state(g, "init")
    got = model.state_dict()
    assert list(got) == [k[5:] for k in g.files if k.startswith("init:")]
    for name, t in got.items():
        assert tuple(t.shape) == want[name].shape, name
        assert np.array_equal(t.numpy(), want[name]), name
    # and a reference checkpoint loads by name
    model.load_state_dict({k: torch.from_numpy(v) for k, v in _state(g, "pert").items()}, strict=True)


def test_parameter_names_of_the_default_shape():
    from yelprecommendation_amd.models.s3rec import S3Rec
    model = S3Rec(_cfg(embed_size=64, max_seq_len=50), 100, 7)
    names = list(model.state_dict())
    assert len(names) == 39
    assert names[:3] == ["positional_encoding", "item_embedding.weight", "attribute_embedding.weight"]
    assert model.item_embedding.weight.shape == (101, 64)
    assert "multihead_attns.1.k_weights.1.weight" in names and "multihead_attns.0.output.bias" in names
    assert names[-4:] == ["aap_weight.weight", "mip_weight.weight", "map_weight.weight", "sp_weight.weight"]


@pytest.mark.parametrize("bad", [dict(embed_size=48), dict(max_seq_len=65), dict(num_heads=5), dict(num_blocks=5),
                                 dict(max_seq_len=0)])
def test_unsupported_configuration_raises_at_construction(bad):
    from yelprecommendation_amd.models.s3rec import S3Rec
    with pytest.raises(NotImplementedError, match="S3Rec"):
        S3Rec(_cfg(**bad), 100, 7)


def test_training_surface_is_refused_without_a_device():
    from yelprecommendation_amd.models.s3rec import S3Rec
    model = S3Rec(_cfg(), 100, 7)
    X = torch.zeros((2, 12), dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="training is not built"):
        model.finetune(X, X, X)                                  # training mode
    model.eval()
    with pytest.raises(NotImplementedError, match="training is not built"):
        model.evaluate(X, X[:, 0], X)                            # grad enabled
    for fn in (model.encode, model.pretrain):
        with pytest.raises(NotImplementedError, match="pre-training"):
            fn(X)


def test_trainer_refuses_to_train(tmp_path):
    from yelprecommendation_amd.trainers.s3rec_trainer import S3RecTrainer

    class Cfg(dict):
        __getattr__ = dict.__getitem__
    cfg = Cfg(embed_size=32, max_seq_len=12, num_heads=2, num_blocks=2, dropout_ratio=0.1, device="cpu",
              model_dir=str(tmp_path), top_n=10, best_metric="loss", load_pretrain=True)
    trainer = S3RecTrainer(cfg, 100, None, 7)                    # no pre-trained file: nothing to load
    for fn in (trainer.train, lambda dl: trainer.run(dl, dl)):
        with pytest.raises(NotImplementedError, match="training is not built"):
            fn([])
    assert trainer._is_surpass_best_metric(current=(1.0,), best=(2.0,))
    torch.save(trainer.model.state_dict(), tmp_path / "best_model.pt")
    torch.save(trainer.model.state_dict(), tmp_path / "best_pretrain_model.pt")
    trainer.load_best_model()
    trainer._load_best_pretrain_model()


def test_argument_checks_without_gpu():
    """-1 for what the kernels do not take, -2 for null pointers with work to do, 0 for an empty batch: all before
    any launch."""
    from yelprecommendation_amd import _lib
    lib = _lib.load()
    enc = lambda B=4, L=12, E=32, heads=2, blocks=2: lib.yr_s3rec_encode(    # noqa: E731
        None, None, None, None, B, L, E, heads, blocks, 100, 0, None, None, None)
    assert enc(E=48) == -1 and enc(L=65) == -1 and enc(heads=5) == -1 and enc(blocks=5) == -1
    assert enc() == -2 and enc(B=-1) == -2 and enc(L=0) == -2
    assert enc(B=0) == 0
    assert lib.yr_s3rec_seq_scores(None, None, None, None, 8, 48, 100, None, None, None, None) == -1
    assert lib.yr_s3rec_seq_scores(None, None, None, None, 8, 32, 100, None, None, None, None) == -2
    assert lib.yr_s3rec_seq_scores(None, None, None, None, 0, 32, 100, None, None, None, None) == 0
    assert lib.yr_s3rec_candidate_scores(None, None, None, None, 4, 99, 48, 100, None, None, None, None) == -1
    assert lib.yr_s3rec_candidate_scores(None, None, None, None, 4, 99, 32, 100, None, None, None, None) == -2
    assert lib.yr_s3rec_candidate_scores(None, None, None, None, 4, 0, 32, 100, None, None, None, None) == -2
    assert lib.yr_s3rec_candidate_scores(None, None, None, None, 0, 99, 32, 100, None, None, None, None) == 0
