"""GPU: NGCF's full-catalogue evaluation — the sweep over the layer tables (engine.ngcf_eval_topk,
csrc/eval_topk.hip ngcf_eval_topk_kernel) against float64 on certified ladders (tests/ngcf_eval_cases.py: exact list
equality), against the one-table sweep, with bad ids, through NGCFTrainer (recommend(fused=True), evaluate_full,
cfg.full_eval) and at the Yelp2018 shape."""
import numpy as np
import pandas as pd
import pytest
import torch

import eval_ladders as el
import ngcf_eval_cases as nc
import replay

pytestmark = pytest.mark.gpu


def _tensors(case, D, layers, device):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    tables, num_users = nc.layer_tables(case, D, layers)
    return [t(E) for E in tables], num_users, t(case.users), t(case.mask_ptr), t(case.mask_idx)


def _top64(S, masks, k):
    """Top k of float64 score rows by (-score, id), each row's masked items excluded."""
    S = S.copy()
    for r, m in enumerate(masks):
        S[r, np.asarray(m, np.int64)] = -np.inf
    return el.order_rows(S, k)


# ---- 1. certified ladders ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", nc.SPECS, ids=nc.spec_id)
def test_layered_sweep_equals_float64_on_certified_ladders(device, spec):
    """engine.ngcf_eval_topk == the certified float64 lists, exactly: every mask value, catalogue slices on / off, hint
    lists none / the expected lists / the expected lists with the k-th entry replaced by the (k+1)-th / junk ids with
    -1 and N + 7 (the hint variants of test_eval_ladders.py).  Certified cases: no tolerance, no quota."""
    from yelprecommendation_amd import engine
    D, layers, N, n, k = spec
    case = nc.build(spec)
    L, num_users, users, ptr, idx = _tensors(case, D, layers, device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    rs = np.random.RandomState(D + k)
    junk = rs.randint(0, N, (n, k)).astype(np.int64)
    junk[:, 0] = -1
    if k > 1:
        junk[1::2, 1] = N + 7
        junk[2::3, -1] = junk[2::3, 0]
    for mv in el.MASK_VALUES:
        want = case.expected[mv]
        top1 = el.order_rows(case.scores64(mask_value=mv), k + 1)
        swapped = top1[:, :k].copy()
        swapped[:, k - 1] = top1[:, k]
        hints = {"none": None, "expected": want, "kth_swapped": swapped, "junk": junk}
        for sliced in (True, False):
            for name, hint in hints.items():
                got = engine.ngcf_eval_topk(L, num_users, users, ptr, idx, k, mask_value=mv, sliced=sliced,
                                            hint=None if hint is None else t(hint)).cpu().numpy()
                bad = np.flatnonzero((got != want).any(axis=1))
                assert len(bad) == 0, (f"mask={mv} sliced={sliced} hint={name}: {len(bad)} of {n} rows differ, first "
                                       f"row {bad[0]} ({case.kinds[case.family[bad[0]]]}): {got[bad[0]].tolist()} != "
                                       f"{want[bad[0]].tolist()}")


# ---- 2. one layer is MF --------------------------------------------------------------------------------------------------

def test_one_layer_is_the_one_table_sweep(device):
    from yelprecommendation_amd import engine
    spec = (64, 1, 4100, 130, 10)
    case = nc.build(spec)
    L, num_users, users, ptr, idx = _tensors(case, 64, 1, device)
    for mv in el.MASK_VALUES:
        got = engine.ngcf_eval_topk(L, num_users, users, ptr, idx, 10, mask_value=mv)
        mf = engine.mf_eval_topk(L[0][:num_users], L[0][num_users:], users, ptr, idx, 10, mask_value=mv, precision="f32")
        assert torch.equal(got, mf)


# ---- 3. bad ids ----------------------------------------------------------------------------------------------------------

def test_bad_user_id_raises_and_harms_no_other_row(device):
    """A user id equal to num_users: flagged (IndexError through the call's own flag), its row comes back empty (-1),
    every other row is what a clean call returns; more than eight layer buffers are refused on the host."""
    from yelprecommendation_amd import engine
    spec = (64, 3, 4100, 300, 10)
    case = nc.build(spec)
    L, num_users, users, ptr, idx = _tensors(case, 64, 3, device)
    want = case.expected[el.MASK_VALUE]
    for sliced in (True, False):
        bad = users.clone()
        bad[7] = num_users
        bad[299] = -1
        out = torch.full((300, 10), -7, dtype=torch.int64, device=device)
        with pytest.raises(IndexError, match="user"):
            engine.ngcf_eval_topk(L, num_users, bad, ptr, idx, 10, out=out, sliced=sliced)
        got = out.cpu().numpy()
        assert (got[[7, 299]] == -1).all()
        keep = np.setdiff1d(np.arange(300), [7, 299])
        assert np.array_equal(got[keep], want[keep])
    with pytest.raises(engine.EngineError):
        engine.ngcf_eval_topk([L[0]] * 9, num_users, users, ptr, idx, 10)
    with pytest.raises(engine.EngineError):
        engine.ngcf_eval_topk(L, num_users, users, ptr, idx, 17)
    assert engine.ngcf_eval_supports(16) and not engine.ngcf_eval_supports(17)


# ---- 4. trainer ----------------------------------------------------------------------------------------------------------

NU, NI, EMBED, ORDERS = 300, 517, 32, 2


@pytest.fixture(scope="module")
def small(device, tmp_path_factory):
    """300 users x 517 items, about 8 interactions per user, D = 32, two propagation orders (W = 96); an eval frame of
    290 users in shuffled order, one with an empty mask list; the float64 scores of the model's layers."""
    from yelprecommendation_amd.graph import LaplacianCSR
    from yelprecommendation_amd.trainers import NGCFTrainer
    from yelprecommendation_amd.utils import make_config
    rs = np.random.RandomState(77)
    u = np.repeat(np.arange(NU), 8)
    i = rs.randint(0, NI, u.shape[0])
    pairs = np.unique(np.stack([u, i], 1), axis=0)
    u, i = pairs[:, 0], pairs[:, 1]
    graph = LaplacianCSR.from_interactions(u, i, rs.randint(1, 6, u.shape[0]), NU, NI, device)
    cfg = make_config("NGCF", embed_size=EMBED, num_orders=ORDERS, device="cuda", top_n=10,
                      model_dir=str(tmp_path_factory.mktemp("ngcf_full_eval")))
    torch.manual_seed(5)
    trainer = NGCFTrainer(cfg, NI, NU, graph)
    ids = rs.permutation(NU)[:290]
    masks = [list(rs.permutation(i[u == x])) for x in ids]          # the train items, unsorted
    masks[11] = []
    pos = [list(rs.choice(NI, rs.randint(1, 6), replace=False)) for _ in ids]
    frame = pd.DataFrame({"pos_items": pos, "mask_items": masks}, index=ids)
    with torch.no_grad():
        layers = [E.cpu().numpy().astype(np.float64) for E in trainer.model.propagate(graph)]
    assert len(layers) == ORDERS + 1 and layers[0].shape == (NU + NI, EMBED)
    Ucat = np.concatenate([E[:NU] for E in layers], 1)
    Icat = np.concatenate([E[NU:] for E in layers], 1)
    return trainer, frame, ids.astype(np.int64), masks, Ucat, Icat, Ucat[ids] @ Icat.T


def _near_ties(got, want, small_case):
    _, _, ids, masks, Ucat, Icat, _ = small_case
    return replay.assert_topk_equal_up_to_near_ties(got, want, Ucat, Icat, ids, masks, rel=2 * el.c_bound(96))


def test_trainer_recommend_fused_equals_float64(device, small):
    trainer, frame, ids, masks, Ucat, Icat, S = small
    want = _top64(S, masks, 10)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    ptr = np.zeros(len(masks) + 1, np.int64)
    ptr[1:] = np.cumsum([len(m) for m in masks])
    idx = np.array([x for m in masks for x in sorted(m)], np.int64)
    trainer.cfg.top_n = 10
    for _ in range(2):                                           # the second call takes the first one's lists as hints
        got = trainer.recommend(t(ids), t(ptr), t(idx), fused=True, hint_key="small").cpu().numpy()
        _near_ties(got, want, small)
    assert tuple(trainer._eval_hints["small"].shape) == (290, 10)
    # the default path is the dense one, as before: same lists up to near-ties
    _near_ties(trainer.recommend(t(ids), t(ptr), t(idx)).cpu().numpy(), want, small)


def test_trainer_evaluate_full_metrics_and_the_chunked_route(device, small):
    from yelprecommendation_amd import metric
    trainer, frame, ids, masks, Ucat, Icat, S = small
    actual = [list(x) for x in frame["pos_items"]]
    trainer.cfg.top_n = 10
    four = trainer.evaluate_full(frame, "test")
    lists = trainer.last_full_topk.cpu().numpy()
    _near_ties(lists, _top64(S, masks, 10), small)
    np.testing.assert_allclose(four, metric.ranking_metrics(actual, lists.tolist(), 10), rtol=0, atol=1e-9)
    # top_n = 20: the dense route, in chunks of 64 users (five chunks, the last one short)
    trainer.cfg.top_n = 20
    trainer.full_eval_chunk_users = 64
    try:
        four20 = trainer.evaluate_full(frame)
        lists20 = trainer.last_full_topk.cpu().numpy()
    finally:
        trainer.cfg.top_n = 10
        del trainer.full_eval_chunk_users
    assert lists20.shape == (290, 20)
    _near_ties(lists20, _top64(S, masks, 20), small)
    np.testing.assert_allclose(four20, metric.ranking_metrics(actual, lists20.tolist(), 20), rtol=0, atol=1e-9)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_full_eval_flag_and_the_global_rng(device, small):
    """cfg.full_eval unset: evaluate is the reference's sample — NumPy's global state ends where one
    np.random.randint(290, size=100) leaves it.  full_eval=True: the state is untouched and evaluate is evaluate_full."""
    trainer, frame = small[:2]
    trainer.cfg.top_n = 10
    assert not trainer.cfg.get("full_eval")
    np.random.seed(123)
    np.random.randint(290, size=100)
    after_one_draw = np.random.get_state()
    np.random.seed(123)
    sampled = trainer.evaluate(frame)
    assert _same_state(np.random.get_state(), after_one_draw)
    trainer.cfg.full_eval = True
    try:
        np.random.seed(123)
        before = np.random.get_state()
        for mode in ("valid", "test"):
            got = trainer.evaluate(frame, mode)
            assert _same_state(np.random.get_state(), before)
            assert got == trainer.evaluate_full(frame, mode)
    finally:
        trainer.cfg.full_eval = False
    assert len(sampled) == 4


@pytest.mark.parametrize("flag", [True, False], ids=["full", "sampled"])
def test_train_main_selects_and_tests_on_all_users_when_asked(device, tmp_path, monkeypatch, flag):
    """train.py model_name=NGCF full_eval=true: every evaluation of the run (one per epoch on the validation frame, one
    on the test frame) goes through evaluate_full over all rows of its frame; without the flag none does."""
    from yelprecommendation_amd import train
    from yelprecommendation_amd.trainers import NGCFTrainer
    seen = []
    inner = NGCFTrainer.evaluate_full

    def spy(self, eval_data, mode='valid'):
        out = inner(self, eval_data, mode)
        seen.append((mode, len(eval_data), tuple(self.last_full_topk.shape), out))
        return out
    monkeypatch.setattr(NGCFTrainer, "evaluate_full", spy)
    argv = ["model_name=NGCF", "synthetic=120x90x12", "fast_loader=true", "epochs=2", "batch_size=256", "embed_size=16",
            "num_orders=1", "lr=0.01", "seed=42", "best_metric=recall", f"model_dir={tmp_path}"]
    metrics = train.main(argv + (["full_eval=true"] if flag else []))
    assert len(metrics) == 4 and all(np.isfinite(m) and 0.0 <= m <= 1.0 for m in metrics)
    if not flag:
        assert seen == []
        return
    assert [s[0] for s in seen] == ["valid", "valid", "test"]
    for mode, rows, shape, out in seen:
        assert shape == (rows, 10) and rows > 100
    assert tuple(metrics) == tuple(seen[-1][3])


# ---- 5. the full shape ---------------------------------------------------------------------------------------------------

def test_full_shape_spot_check(device):
    """31,668 x 38,048, D = 64, three layers of N(0, 0.3^2), 20 masked items per user, k = 10, one fused call over all
    users (248 row blocks x 3 catalogue slices): 128 rows drawn with a fixed seed against their float64 lists, and the
    same call with the first result as hint returns identical lists."""
    from yelprecommendation_amd import engine
    nu, ni, d, k = 31668, 38048, 64, 10
    g = torch.Generator(device=device).manual_seed(11)
    L = [torch.randn(nu + ni, d, device=device, generator=g) * 0.3 for _ in range(3)]
    # 20 distinct masked items per user, ascending: one from each of 20 strata of 1,902 items
    idx = (torch.randint(0, 1902, (nu, 20), device=device, generator=g)
           + 1902 * torch.arange(20, device=device)).reshape(-1).contiguous()
    ptr = 20 * torch.arange(nu + 1, device=device, dtype=torch.int64)
    users = torch.randperm(nu, device=device, generator=g)
    got = engine.ngcf_eval_topk(L, nu, users, ptr, idx, k)
    rows = np.random.RandomState(3).choice(nu, 128, replace=False)
    uid = users.cpu().numpy()[rows]
    Lh = [E.cpu().numpy().astype(np.float64) for E in L]
    Ucat = np.concatenate([E[uid] for E in Lh], 1)
    Icat = np.concatenate([E[nu:] for E in Lh], 1)
    masks = idx.reshape(nu, 20).cpu().numpy()[rows]
    want = _top64(Ucat @ Icat.T, masks, k)
    replay.assert_topk_equal_up_to_near_ties(got.cpu().numpy()[rows], want, Ucat, Icat, np.arange(128), masks,
                                             rel=2 * el.c_bound(192))
    again = engine.ngcf_eval_topk(L, nu, users, ptr, idx, k, hint=got)
    assert torch.equal(again, got)
