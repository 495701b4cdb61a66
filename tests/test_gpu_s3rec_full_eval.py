"""GPU: S3Rec full-catalogue evaluation above the rank kernel — ``S3Rec.rank_catalogue`` / ``recommend`` against the
float64 encoder restatement (tests/s3rec_ref64.py) followed by the rank restatement (tests/s3rec_rank_ref64.py),
``S3RecSequences.history`` against a Python set construction, ``S3RecTrainer.evaluate_full`` through both loaders
against metric.ranking_metrics on the float64 lists and against its own formulas, the refusals, and train.py's flag.

The band of a rank here has two parts: the f32 sweep's c_E A, and the encoder before it — the kernel's rows differ from
the float64 rows by the encoder's own float32 error, bounded as everywhere in the S3Rec tests by s3rec_ref64.bar (8 x the
distance between the restatement in float32 and in float64); s3rec_rank_ref64.bands takes it as ``h_err``."""
import os
import types

import numpy as np
import pytest
import torch

import replay
import s3rec_rank_ref64 as R
import s3rec_ref64 as ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s3rec_small.npz")
NUM_ITEMS, L, K = 40, 8, 10


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _behaviours(num_items=NUM_ITEMS, seed=4):
    """Per-user raw item rows: shorter than every cut, empty, repeats, longer than L, nearly the whole catalogue."""
    rs = np.random.RandomState(seed)
    rows = [[3, 7], [], [5, 5, 7, 5, 9, 7, 5, 11, 9], rs.randint(0, num_items, 30).tolist(),
            rs.permutation(num_items)[:num_items - 3].tolist(), [1, 2, 3], [1, 2, 3, 4]]
    rows += [rs.randint(0, num_items, rs.randint(4, 21)).tolist() for _ in range(16)]
    return rows


def _history_sets(rows, mode):
    cut = {"train": 3, "valid": 2, "test": 1}[mode]
    return [sorted({v + 1 for v in r[:max(0, len(r) - cut)]}) for r in rows]


@pytest.fixture(scope="module")
def world(device):
    """The small model (E = 16, L = 8, one head, one block, 40 items), the behaviour rows on the device, the test
    batches and their float64 reference, computed once."""
    from yelprecommendation_amd.data.s3rec_batches import S3RecSequences
    from yelprecommendation_amd.models.s3rec import S3Rec
    E, heads, blocks = 16, 1, 1
    params = ref.make_params(E, L, heads, blocks, num_items=NUM_ITEMS, seed=21)
    cfg = types.SimpleNamespace(embed_size=E, max_seq_len=L, num_heads=heads, num_blocks=blocks, dropout_ratio=0.1,
                                device="cuda")
    model = S3Rec(cfg, NUM_ITEMS, params["attribute_embedding.weight"].shape[0])
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}, strict=True)
    model = model.to(device).eval()
    rows = _behaviours()
    users = np.repeat(np.arange(len(rows)), [len(r) for r in rows])
    items = np.array([v for r in rows for v in r], dtype=np.int64)
    store = S3RecSequences(torch.from_numpy(users).to(device), torch.from_numpy(items).to(device), len(rows), NUM_ITEMS, L)
    X, pos, _ = store.draw("test", 0, n_neg=2)
    store.check()
    return dict(model=model, params=params, hb=(heads, blocks), rows=rows, store=store, X=X, pos=pos, E=E)


def _reference(w, history_sets):
    """Float64: h_last, the encoder's error bound, the rank bands and the lists of every user of the test batches."""
    X, pos = w["X"].cpu().numpy(), w["pos"].cpu().numpy()
    h64 = ref.encode(w["params"], X, *w["hb"], dtype=np.float64)[:, -1]
    h32 = ref.encode(w["params"], X, *w["hb"], dtype=np.float32)[:, -1]
    h_err = ref.bar(h32, h64)
    T = np.asarray(w["params"]["item_embedding.weight"], dtype=np.float32)
    B, Rr = X.shape[0], T.shape[0]
    ptr = np.zeros(B + 1, dtype=np.int64)
    hs = history_sets if history_sets is not None else [[] for _ in range(B)]
    np.cumsum([len(s) for s in hs], out=ptr[1:])
    idx = np.array([v for s in hs for v in s], dtype=np.int64)
    g = dict(H=h64.astype(np.float32), T=T, target=pos.astype(np.int64), ptr=ptr, idx=idx, rows=None, K=B, first_col=1,
             R=Rr, N=B, E=w["E"])
    b = R.bands(g, h_err=h_err + float(np.abs(h64 - h64.astype(np.float32)).max()))
    S = h64 @ T.astype(np.float64).T
    lists = np.full((B, K), -1, dtype=np.int64)
    for n in range(B):
        free = [r for r in range(1, Rr) if r not in set(hs[n])]
        order = sorted(free, key=lambda r: (-S[n, r], r))[:K]
        lists[n, :len(order)] = order
    return dict(h64=h64, h_err=h_err, bands=b, lists=lists, T=T, hs=hs, pos=pos)


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _csr(sets, device):
    ptr = np.zeros(len(sets) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in sets], out=ptr[1:])
    return _t(ptr, device), _t(np.array([v for s in sets for v in s], dtype=np.int64), device)


@pytest.mark.parametrize("mode", ["train", "valid", "test"])
def test_history_is_the_set_construction(world, mode):
    ptr, idx = world["store"].history(mode)
    want = _history_sets(world["rows"], mode)
    ptr, idx = ptr.cpu().numpy(), idx.cpu().numpy()
    assert ptr.shape == (len(want) + 1,) and idx.dtype == np.int64
    for u, s in enumerate(want):
        assert idx[ptr[u]:ptr[u + 1]].tolist() == s, (mode, u)
    assert world["store"].history(mode)[1] is world["store"].history(mode)[1]          # built once
    if mode == "test":
        assert want[0] == [4] and want[1] == [] and want[2] == [6, 8, 10, 12] and len(want[4]) == NUM_ITEMS - 4
    with pytest.raises(ValueError):
        world["store"].history("all")


@pytest.mark.parametrize("with_history", [True, False], ids=["history", "no-history"])
def test_rank_catalogue_and_recommend_against_float64(device, world, with_history):
    w, model = world, world["model"]
    hs = _history_sets(w["rows"], "test") if with_history else None
    want = _reference(w, hs)
    history = w["store"].history("test") if with_history else None
    with torch.no_grad():
        rank = model.rank_catalogue(w["X"], w["pos"], history=history)
        lists = model.recommend(w["X"], K, history=history)
        both = model.rank_and_recommend(w["X"], w["pos"], K, history=history)
        # users: the rows of the CSR, here a reversed batch
        rev = torch.arange(w["X"].shape[0] - 1, -1, -1, device=device)
        rank_rev = model.rank_catalogue(w["X"][rev].contiguous(), w["pos"][rev].contiguous(), history=history, users=rev)
    model.check_indices()
    assert rank.dtype == torch.int64 and lists.dtype == torch.int64 and tuple(lists.shape) == (w["X"].shape[0], K)
    assert torch.equal(both[0], rank) and torch.equal(rank_rev, rank[rev])
    rank, lists = rank.cpu().numpy(), lists.cpu().numpy()
    b = want["bands"]
    assert ((rank >= b["lo"]) & (rank <= b["hi"])).all(), (rank, b["lo"], b["hi"])
    assert (rank[want["pos"] == 0] == -1).all() and (want["pos"] == 0).sum() >= 3          # users 0, 1, 5: no target
    print(f"band widths {np.bincount((b['hi'] - b['lo'])[b['has']])}, encoder bar {want['h_err']:.3g}")
    # the lists: 1..num_items, never the pad, never the history, -1 only where the free items run out
    free = np.array([NUM_ITEMS - len(s) for s in want["hs"]])
    full = free >= K
    assert (lists[full] >= 1).all() and (lists <= NUM_ITEMS).all() and (lists != 0).all()
    for n in range(lists.shape[0]):
        assert not set(lists[n].tolist()) & set(want["hs"][n])
        if not full[n]:
            assert (lists[n, free[n]:] == -1).all() and lists[n, :free[n]].tolist() == want["lists"][n, :free[n]].tolist()
    if with_history:
        assert (~full).any()
    masked = [np.array(s, dtype=np.int64) for s in want["hs"]]
    differed = replay.assert_topk_equal_up_to_near_ties(lists[full], want["lists"][full], want["h64"][full], want["T"],
                                                        np.arange(int(full.sum())), masked=[m for m, f in zip(masked, full) if f])
    print(f"{differed} of {int(full.sum())} lists differ at a near-tie")
    # the rank sweep keeps the target where the lists' mask would drop it: with the target kept, rank < K is membership
    lists_t = both[1].cpu().numpy()
    single = b["has"] & (b["lo"] == b["hi"])
    member = (lists_t == want["pos"][:, None]).any(1)
    assert ((rank < K) == member)[single].all()


def test_the_recorded_checkpoint(device):
    """tests/golden/s3rec_small.npz: the reference's own model and test batches, ranks inside the float64 band."""
    from yelprecommendation_amd.models.s3rec import S3Rec
    g = np.load(GOLDEN)
    cfg = dict(zip(g["cfg_names"].tolist(), g["cfg_values"].tolist()))
    state = {k[5:]: g[k] for k in g.files if k.startswith("pert:")}
    hb = (cfg["num_heads"], cfg["num_blocks"])
    mcfg = types.SimpleNamespace(embed_size=cfg["embed_size"], max_seq_len=cfg["max_seq_len"], num_heads=hb[0],
                                 num_blocks=hb[1], dropout_ratio=0.1, device="cuda")
    model = S3Rec(mcfg, cfg["num_items"], cfg["attributes_count"])
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=True)
    model = model.to(device).eval()
    X = np.concatenate([g[f"test{i}_X"] for i in range(2)])
    pos = np.concatenate([g[f"test{i}_pos_item"].reshape(-1) for i in range(2)]).astype(np.int64)
    w = dict(params=state, hb=hb, X=_t(X, device), pos=_t(pos, device), E=cfg["embed_size"])
    hs = [sorted(set(x[x > 0].tolist())) for x in X]                  # the sequence itself as the history
    want = _reference(w, hs)
    with torch.no_grad():
        rank = model.rank_catalogue(w["X"], w["pos"], history=_csr(hs, device)).cpu().numpy()
    model.check_indices()
    b = want["bands"]
    assert ((rank >= b["lo"]) & (rank <= b["hi"])).all(), (rank, b["lo"], b["hi"])
    assert (b["hi"] - b["lo"])[b["has"]].mean() <= 0.5


def _trainer(world, tmp_path):
    from yelprecommendation_amd.trainers.s3rec_trainer import S3RecTrainer
    tcfg = Cfg(embed_size=world["E"], max_seq_len=L, num_heads=world["hb"][0], num_blocks=world["hb"][1], dropout_ratio=0.1,
               device="cuda", model_dir=str(tmp_path), top_n=K, best_metric="loss", load_pretrain=True)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in world["params"].items()}, tmp_path / "best_pretrain_model.pt")
    return S3RecTrainer(tcfg, NUM_ITEMS, None, world["params"]["attribute_embedding.weight"].shape[0])


def test_evaluate_full_through_both_loaders(device, world, tmp_path):
    import pandas as pd
    from torch.utils.data import DataLoader
    from yelprecommendation_amd.data.datasets.s3rec_data_pipeline import S3RecDataPipeline
    from yelprecommendation_amd.data.datasets.s3rec_dataset import S3RecDataset
    from yelprecommendation_amd.data.s3rec_batches import S3RecBatchLoader
    from yelprecommendation_amd.metric import ranking_metrics
    w = world
    trainer = _trainer(w, tmp_path)
    history = w["store"].history("test")
    fast = S3RecBatchLoader(w["store"], "test", batch_size=7, n_neg=2)
    before = trainer.evaluate(S3RecBatchLoader(w["store"], "test", batch_size=7, n_neg=2))
    four = trainer.evaluate_full(fast, history=history)
    full = trainer.last_full_eval
    assert trainer.evaluate(S3RecBatchLoader(w["store"], "test", batch_size=7, n_neg=2)) == before   # evaluate is untouched
    # the host loader: the same users, the same ranks
    pipe = S3RecDataPipeline(types.SimpleNamespace(max_seq_len=L))
    test_df = pipe.split(pd.DataFrame({"behaviors": w["rows"]}))[2]

    class NoDraw(S3RecDataset):
        """The reference's loop needs 99 free ids and this catalogue has 40; evaluate_full reads no negatives."""

        def _negative_sampling(self, behaviors):
            return [1]
    host = DataLoader(NoDraw(test_df, num_items=NUM_ITEMS, train=False), batch_size=5)
    four_host = trainer.evaluate_full(host, history=history)
    assert torch.equal(trainer.last_full_eval["ranks"], full["ranks"]) and four_host == four
    # a valid loader: the target is the last entry of pos_items
    trainer.evaluate_full(S3RecBatchLoader(w["store"], "valid", batch_size=7), history=w["store"].history("valid"))
    Xv, posv, _ = w["store"].draw("valid", 0)
    with torch.no_grad():
        want_v = trainer.model.rank_catalogue(Xv, posv[:, -1].contiguous(), history=w["store"].history("valid"))
    assert torch.equal(trainer.last_full_eval["ranks"], want_v)
    # the four metrics: metric.ranking_metrics on the float64 lists (the target kept in its own list)
    hs = _history_sets(w["rows"], "test")
    want = _reference(w, [[v for v in s if v != t] for s, t in zip(hs, w["pos"].cpu().numpy().tolist())])
    actual = [[int(t)] if t > 0 else [] for t in want["pos"]]
    ref4 = ranking_metrics(actual, want["lists"].tolist(), K)
    np.testing.assert_allclose(four, ref4, rtol=0, atol=1e-12)
    # the dict: its formulas on the returned ranks, float64, means over the rows with a target
    ranks = full["ranks"].cpu().numpy()
    b = want["bands"]
    assert ((ranks >= b["lo"]) & (ranks <= b["hi"])).all()
    rho = ranks[ranks >= 0].astype(np.float64)
    assert full["n_users"] == rho.size == int((want["pos"] > 0).sum()) and full["n_skipped"] == ranks.size - rho.size >= 3
    for k in (1, 5, 10, K):
        assert full[f"HR@{k}"] == pytest.approx(np.mean(rho < k), abs=1e-15)
        assert full[f"NDCG@{k}"] == pytest.approx(np.mean((rho < k) / np.log2(rho + 2.0)), abs=1e-15)
    assert full["MRR"] == pytest.approx(np.mean(1.0 / (rho + 1.0)), abs=1e-15)
    assert 0.0 < full["MRR"] <= 1.0 and full["HR@1"] <= full["HR@5"] <= full["HR@10"]


def test_the_refusals(device, world):
    model = world["model"]
    X, pos = world["X"], world["pos"]
    for call in (lambda: model.rank_catalogue(X, pos), lambda: model.recommend(X, K)):
        with pytest.raises(NotImplementedError):                      # grad enabled
            call()
        model.train()
        try:
            with torch.no_grad(), pytest.raises(NotImplementedError):  # train() mode
                call()
        finally:
            model.eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="CPU"):
        model.rank_catalogue(X.cpu(), pos.cpu())
    with torch.no_grad(), pytest.raises(NotImplementedError, match="CPU"):
        model.recommend(X.cpu(), K)
    with torch.no_grad():
        bad = pos.clone()
        bad[0] = NUM_ITEMS + 1
        assert int(model.rank_catalogue(X, bad)[0]) == -1
    with pytest.raises(IndexError, match="S3Rec"):
        model.check_indices()
    with torch.no_grad():                                             # a CSR row that does not exist
        model.rank_catalogue(X, pos, history=world["store"].history("test"),
                             users=torch.full((X.shape[0],), 10 ** 6, device=device))
    with pytest.raises(IndexError, match="S3Rec"):
        model.check_indices()
    model.check_indices()


@pytest.mark.parametrize("fast,flag", [("true", True), ("false", True), ("false", False)],
                         ids=["fast-full", "host-full", "host-plain"])
def test_train_main_runs_the_full_evaluation_when_asked(device, tmp_path, monkeypatch, fast, flag):
    from yelprecommendation_amd import train
    from yelprecommendation_amd.trainers.s3rec_trainer import S3RecTrainer
    seen = []
    inner = S3RecTrainer.evaluate_full

    def spy(self, loader, history=None):
        out = inner(self, loader, history=history)
        seen.append((self, history))
        return out
    monkeypatch.setattr(S3RecTrainer, "evaluate_full", spy)
    argv = ["model_name=S3Rec", "synthetic=60x150x10", f"fast_loader={fast}", "epochs=1", "batch_size=32", "embed_size=16",
            "max_seq_len=12", "num_heads=1", "num_blocks=1", "dropout_ratio=0", "lr=0.001", "seed=42",
            "load_pretrain=false", f"model_dir={tmp_path}"] + (["full_eval=true"] if flag else [])
    metrics = train.main(argv)
    assert len(metrics) == 4 and all(np.isfinite(m) and 0.0 <= m <= 1.0 for m in metrics)
    assert len(seen) == (1 if flag else 0)
    if flag:
        trainer, history = seen[0]
        full = trainer.last_full_eval
        assert history is not None and history[0].numel() == 61
        assert full["ranks"].numel() == 60 and full["n_users"] + full["n_skipped"] == 60 and full["n_users"] > 0
        assert int(full["ranks"].max()) < 150 and 0.0 < full["MRR"] <= 1.0
