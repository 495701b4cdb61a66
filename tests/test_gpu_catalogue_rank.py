"""GPU: the catalogue rank sweep (engine.catalogue_ranks, csrc/catalogue_rank.hip) and the metrics from ranks
(engine.metrics_from_ranks, csrc/metrics.hip) against float64 (tests/catalogue_rank_ref64.py) on the cases of
tests/catalogue_rank_cases.py — whose plans test_catalogue_rank_host.py asserts — against the S3Rec rank kernel, against
the fused top-k sweeps on certified ladders, and through MFTrainer / NGCFTrainer / train.py."""
import logging

import numpy as np
import pandas as pd
import pytest
import torch

import catalogue_rank_cases as cc
import catalogue_rank_ref64 as ref
import eval_ladders as el
import ngcf_eval_cases as nc

pytestmark = pytest.mark.gpu

KS = (1, 3, 10, 20, 50, 200)
GUARD, RANK_FILL, SCORE_FILL = 64, -777, 7.25


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _call(c, device, **kw):
    """engine.catalogue_ranks on a case of catalogue_rank_cases (numpy in, tensors out)."""
    from yelprecommendation_amd import engine
    return engine.catalogue_ranks([_t(U, device) for U in c.layers_user], [_t(I, device) for I in c.layers_item],
                                  _t(c.users, device), _t(c.pos_ptr, device), _t(c.pos_idx, device),
                                  _t(c.mask_ptr, device), _t(c.mask_idx, device), **kw)


def _rows(flat, ptr):
    return [flat[ptr[r]:ptr[r + 1]] for r in range(len(ptr) - 1)]


# ---- 1. exact inputs: equal to float64 --------------------------------------------------------------------------------

def _check_exact(c, device):
    nnz = len(c.pos_idx)
    rank_buf = torch.full((nnz + 2 * GUARD,), RANK_FILL, dtype=torch.int64, device=device)
    score_buf = torch.full((nnz + 2 * GUARD,), SCORE_FILL, dtype=torch.float32, device=device)
    rank, score = _call(c, device, out=rank_buf[GUARD:GUARD + nnz], score_out=score_buf[GUARD:GUARD + nnz])
    got, got_s = rank.cpu().numpy(), score.cpu().numpy()
    bad = np.flatnonzero(got != c.rank)
    assert len(bad) == 0, f"{len(bad)} of {nnz} ranks differ, first entry {bad[0]}: {got[bad[0]]} != {c.rank[bad[0]]}"
    assert np.array_equal(got_s.astype(np.float64), c.score)
    for buf, fill in ((rank_buf, RANK_FILL), (score_buf, SCORE_FILL)):
        assert (buf[:GUARD] == fill).all() and (buf[GUARD + nnz:] == fill).all()
    if c.N >= 2:                                                      # the repeated user id: equal ranks for both rows
        a, b = _rows(got, c.pos_ptr)[0], _rows(got, c.pos_ptr)[-1]
        assert np.array_equal(a, b)
    return got


@pytest.mark.parametrize("spec", cc.EXACT_SPECS, ids=cc.spec_id)
def test_exact_inputs_equal_float64(device, spec):
    from yelprecommendation_amd import engine
    c = cc.build_exact(spec)
    got = _check_exact(c, device)
    # the metrics of these ranks, every cutoff (k above the unmasked count and above the catalogue included)
    if len(c.pos_idx):
        res = engine.metrics_from_ranks(_t(got, device), _t(c.pos_ptr, device), KS, num_items=c.items,
                                        mask_ptr=_t(c.mask_ptr, device))
        rows = _rows(c.rank, c.pos_ptr)
        want = ref.metrics_from_ranks(rows, KS, [c.items - len(m) for m in c.masks])
        for k in KS:
            np.testing.assert_allclose(res[k], want[k], rtol=0, atol=1e-12)
        assert abs(res.mrr - want["mrr"]) < 1e-12
        assert abs(res.auc - want["auc"]) < 1e-12 or (np.isnan(res.auc) and np.isnan(want["auc"]))


def test_all_zero_tables_every_score_ties(device):
    _check_exact(cc.build_exact((64, 2, 65, 33), zero=True), device)
    _check_exact(cc.build_exact((16, 1, 33, 2049), zero=True), device)


# ---- 2. the grid loop -------------------------------------------------------------------------------------------------

def test_more_units_than_one_launch(device):
    """65,537 rows of one target each over 8 items at D = 16: 2,049 row tiles x 1 chunk, one more unit than the grid
    holds.  Equal to float64 (integer tables), and torch.equal to the same rows evaluated alone."""
    from yelprecommendation_amd import engine
    c = cc.build_grid()
    n = cc.GRID_ROWS
    U, I = _t(c.U, device), _t(c.I, device)
    ptr = torch.arange(n + 1, dtype=torch.int64, device=device)
    users, tg, mk = _t(c.users, device), _t(c.targets, device), _t(c.masked, device)
    rank = engine.catalogue_ranks([U], [I], users, ptr, tg, ptr, mk)
    S = c.U.astype(np.float64)[c.users] @ c.I.astype(np.float64).T
    st = S[np.arange(n), c.targets][:, None]
    ids = np.arange(cc.GRID_ITEMS)[None, :]
    ahead = ((S > st) | ((S == st) & (ids < c.targets[:, None]))) & (ids != c.masked[:, None])
    assert np.array_equal(rank.cpu().numpy(), ahead.sum(1))
    for lo, hi in ((0, 40), (n - 33, n), (32 * 2047 - 5, 32 * 2047 + 7)):
        alone = engine.catalogue_ranks([U], [I], users[lo:hi].contiguous(), ptr[:hi - lo + 1], tg[lo:hi].contiguous(),
                                       ptr[:hi - lo + 1], mk[lo:hi].contiguous())
        assert torch.equal(alone, rank[lo:hi])


# ---- 3. random f32 inputs: inside the float64 interval ------------------------------------------------------------------

@pytest.mark.parametrize("spec", cc.RANDOM_SPECS, ids=lambda s: "D{}-L{}-N{}-I{}-m{}".format(*s))
def test_random_inputs_inside_the_float64_interval(device, spec):
    c = cc.build_random(spec)
    got = _call(c, device).cpu().numpy()
    hidden = float(np.mean(c.lo != c.hi))
    print(f"{spec}: {hidden:.4f} of {len(got)} pairs have lo != hi")
    assert hidden <= cc.RANDOM_CAP
    bad = np.flatnonzero((got < c.lo) | (got > c.hi))
    assert len(bad) == 0, f"{len(bad)} ranks outside [lo, hi], first {bad[0]}: {got[bad[0]]} not in " \
                          f"[{c.lo[bad[0]]}, {c.hi[bad[0]]}]"


# ---- 4. one target per row, one table: the S3Rec rank kernel ------------------------------------------------------------

@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_single_target_equals_the_s3rec_rank_kernel(device, D):
    """Same H, T, targets and exclusion lists (the target never excluded), first_col = 0: torch.equal ranks and scores."""
    from yelprecommendation_amd import engine
    rs = np.random.RandomState(D)
    N, R = 70, 2100
    H = _t(rs.standard_normal((N, D)).astype(np.float32), device)
    T_np = rs.standard_normal((R, D)).astype(np.float32)
    T_np[100] = T_np[101] = T_np[99]                                  # bit-identical rows around a target
    T = _t(T_np, device)
    target = rs.randint(0, R, N).astype(np.int64)
    target[:3] = (100, 99, 101)
    excl = [sorted(set(rs.choice(R, 30, replace=False).tolist()) - {int(t)}) if r % 4 else [] for r, t in
            enumerate(target)]
    eptr, eidx = ref.csr(excl)
    want, want_s = engine.s3rec_catalogue_rank(H, T, _t(target, device), _t(eptr, device), _t(eidx, device),
                                               first_col=0, want_score=True)
    ptr = torch.arange(N + 1, dtype=torch.int64, device=device)
    got, got_s = engine.catalogue_ranks([H], [T], torch.arange(N, dtype=torch.int64, device=device), ptr,
                                        _t(target, device), _t(eptr, device), _t(eidx, device), want_score=True)
    assert torch.equal(got, want) and torch.equal(got_s, want_s)


# ---- 5. certified ladders: the fused top-k sweeps ------------------------------------------------------------------------

def _ladder_targets(case, rs):
    """Per row: some members of the certified list, items beyond it, a masked item when the row has one — shuffled."""
    k, N = case.k, case.N
    want = case.expected[el.MASK_VALUE]
    pos = []
    for r in range(len(case.users)):
        inside = rs.permutation(want[r])[:rs.randint(0, min(k, 6) + 1)].tolist()
        beyond = rs.choice(N, rs.randint(0, 20), replace=False).tolist()
        masked = case.masks[r][:1].tolist() if r % 2 else []
        tg = list(dict.fromkeys(int(x) for x in inside + beyond + masked))
        pos.append([tg[i] for i in rs.permutation(len(tg))])
    return pos


def _check_ladder(case, layers_user, layers_item, fused, pos, device):
    from yelprecommendation_amd import engine
    k = case.k
    pos_ptr, pos_idx = ref.csr(pos)
    d_ptr, d_idx = _t(pos_ptr, device), _t(pos_idx, device)
    rank = engine.catalogue_ranks(layers_user, layers_item, _t(case.users, device), d_ptr, d_idx,
                                  _t(case.mask_ptr, device), _t(case.mask_idx, device))
    assert np.array_equal(fused.cpu().numpy(), case.expected[el.MASK_VALUE])
    res = engine.metrics_from_ranks(rank, d_ptr, (k,))
    want = engine.rank_metrics(fused, d_ptr, d_idx)
    np.testing.assert_allclose(res.ten(k).cpu().numpy(), want.cpu().numpy(), rtol=0, atol=1e-12)
    lists = fused.cpu().numpy()
    for r, rk in enumerate(_rows(rank.cpu().numpy(), pos_ptr)):
        inside = set(lists[r].tolist())
        for t, x in zip(pos[r], rk):
            assert (x < k) == (t in inside), f"row {r}: target {t} has rank {x}, k = {k}, in the list: {t in inside}"
            if t in inside:
                assert lists[r][x] == t                                # and its rank is its place in the list


@pytest.mark.parametrize("D,N,rows,k", [(64, 4100, 130, 10), (32, 2100, 70, 16), (128, 4100, 70, 16), (16, 700, 40, 10)])
def test_certified_mf_ladders(device, D, N, rows, k):
    from yelprecommendation_amd import engine
    case = el.build_case(D, N, rows, k, mask_values=(el.MASK_VALUE,), seed=300 + D + k)
    U, I = _t(case.U, device), _t(case.I, device)
    fused = engine.mf_eval_topk(U, I, _t(case.users, device), _t(case.mask_ptr, device), _t(case.mask_idx, device), k)
    _check_ladder(case, [U], [I], fused, _ladder_targets(case, np.random.RandomState(k)), device)


@pytest.mark.parametrize("spec", nc.SPECS, ids=nc.spec_id)
def test_certified_ngcf_ladders(device, spec):
    from yelprecommendation_amd import engine
    D, layers, N, n, k = spec
    case = nc.build(spec)
    tables, nu = nc.layer_tables(case, D, layers)
    L = [_t(E, device) for E in tables]
    fused = engine.ngcf_eval_topk(L, nu, _t(case.users, device), _t(case.mask_ptr, device), _t(case.mask_idx, device), k)
    _check_ladder(case, [E[:nu] for E in L], [E[nu:] for E in L], fused,
                  _ladder_targets(case, np.random.RandomState(k + layers)), device)


# ---- 6. repeatability, bad ids -------------------------------------------------------------------------------------------

def test_two_calls_agree_and_bad_ids_harm_no_neighbour(device):
    from yelprecommendation_amd import engine
    c = cc.build_random((64, 2, 70, 2100, 4))
    a, sa = _call(c, device, want_score=True)
    b, sb = _call(c, device, want_score=True)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    clean = a.cpu().numpy()
    # a user id past the table and a negative one; a target past the catalogue and a negative one
    users = c.users.copy()
    rows_bad = [r for r in (3, 40) if len(c.pos[r])]
    users[rows_bad[0]] = c.num_users
    users[rows_bad[-1]] = -1
    idx = c.pos_idx.copy()
    ok_rows = [r for r in range(c.N) if r not in rows_bad and len(c.pos[r]) > 1]
    e1, e2 = c.pos_ptr[ok_rows[0]], c.pos_ptr[ok_rows[5]] + 1
    idx[e1], idx[e2] = c.items, -5
    args = ([_t(U, device) for U in c.layers_user], [_t(I, device) for I in c.layers_item], _t(users, device),
            _t(c.pos_ptr, device), _t(idx, device), _t(c.mask_ptr, device), _t(c.mask_idx, device))
    flag = engine.new_error_flag(device)
    got, score = engine.catalogue_ranks(*args, want_score=True, err_flag=flag)
    assert int(flag.item()) == engine.FLAG_BAD_USER | engine.FLAG_BAD_ITEM
    got, score = got.cpu().numpy(), score.cpu().numpy()
    refused = np.zeros(len(idx), bool)
    for r in rows_bad:
        refused[c.pos_ptr[r]:c.pos_ptr[r + 1]] = True
    refused[[e1, e2]] = True
    assert (got[refused] == -1).all() and (score[refused] == 0).all()
    # every other entry is the clean call's — the rows of e1 / e2 included: the items the refused entries replaced
    # are still in the catalogue, and a row's targets are items like any other to each other
    assert np.array_equal(got[~refused], clean[~refused])
    assert np.array_equal(score[~refused], sa.cpu().numpy()[~refused])
    with pytest.raises(IndexError, match="user"):
        engine.catalogue_ranks(*args)
    with pytest.raises(engine.EngineError):
        engine.catalogue_ranks([args[0][0]] * 9, [args[1][0]] * 9, *args[2:])
    wide = torch.zeros((4, 256), device=device)
    with pytest.raises(engine.EngineError):
        engine.catalogue_ranks([wide], [wide], *args[2:])


# ---- 7. trainers ---------------------------------------------------------------------------------------------------------

NU, NI = 300, 517


def _frame(rs, inter_u, inter_i):
    ids = rs.permutation(NU)[:290]
    masks = [list(rs.permutation(inter_i[inter_u == x])) for x in ids]          # the train items, unsorted
    masks[11] = []
    pos = []
    for n, m in enumerate(masks):
        free = np.setdiff1d(np.arange(NI), np.asarray(m, np.int64))
        count = (0, 1, 3, 7, 20, 40)[n % 6] if n != 11 else 5
        pos.append([int(x) for x in rs.choice(free, count, replace=False)])
    return pd.DataFrame({"pos_items": pos, "mask_items": masks}, index=ids), ids.astype(np.int64), masks, pos


def _interactions(rs):
    u = np.repeat(np.arange(NU), 8)
    i = rs.randint(0, NI, u.shape[0])
    pairs = np.unique(np.stack([u, i], 1), axis=0)
    return pairs[:, 0], pairs[:, 1]


@pytest.fixture(scope="module")
def mf_small(device, tmp_path_factory):
    from yelprecommendation_amd.trainers import MFTrainer
    from yelprecommendation_amd.utils import make_config
    rs = np.random.RandomState(91)
    u, i = _interactions(rs)
    cfg = make_config("MF", embed_size=32, device="cuda", top_n=10, model_dir=str(tmp_path_factory.mktemp("mf_rank")))
    torch.manual_seed(7)
    trainer = MFTrainer(cfg, NI, NU)
    with torch.no_grad():                                             # scores of order one, as after training
        trainer.model.user_embedding.weight.normal_(0, 0.5)
        trainer.model.item_embedding.weight.normal_(0, 0.5)
    frame, ids, masks, pos = _frame(rs, u, i)
    Ut = trainer.model.user_embedding.weight.detach().cpu().numpy()
    It = trainer.model.item_embedding.weight.detach().cpu().numpy()
    return trainer, frame, ids, masks, pos, [Ut], [It]


@pytest.fixture(scope="module")
def ngcf_small(device, tmp_path_factory):
    from yelprecommendation_amd.graph import LaplacianCSR
    from yelprecommendation_amd.trainers import NGCFTrainer
    from yelprecommendation_amd.utils import make_config
    rs = np.random.RandomState(77)
    u, i = _interactions(rs)
    graph = LaplacianCSR.from_interactions(u, i, rs.randint(1, 6, u.shape[0]), NU, NI, device)
    cfg = make_config("NGCF", embed_size=32, num_orders=2, device="cuda", top_n=10, full_eval=True,
                      model_dir=str(tmp_path_factory.mktemp("ngcf_rank")))
    torch.manual_seed(5)
    trainer = NGCFTrainer(cfg, NI, NU, graph)
    frame, ids, masks, pos = _frame(rs, u, i)
    with torch.no_grad():
        layers = [E.cpu().numpy() for E in trainer.model.propagate(graph)]
    return trainer, frame, ids, masks, pos, [E[:NU] for E in layers], [E[NU:] for E in layers]


def _intervals(small):
    """(lo, hi) of every target's rank from the float64 scores of the model's tables and the bar."""
    trainer, frame, ids, masks, pos, lu, li = small
    S, A = ref.scores64(lu, li, ids)
    eps = ref.bar(len(lu), lu[0].shape[1]) * A
    lo, hi = zip(*(ref.rank_bounds_row(S[r], eps[r], masks[r], pos[r]) for r in range(len(pos))))
    return np.concatenate(lo), np.concatenate(hi), S


def _check_trainer(small, dense_topk):
    from yelprecommendation_amd import engine
    trainer, frame, ids, masks, pos, lu, li = small
    cfg = trainer.cfg
    # (a) at k = 10 the rank route gives evaluate's four figures
    assert not cfg.get("rank_eval")
    want = trainer.evaluate(frame)
    res = trainer.evaluate_ranks(frame, ks=(10,))
    np.testing.assert_allclose(res[10][:4], want, rtol=0, atol=1e-12)
    assert trainer.evaluate_ranks(frame)[10] == res[10]               # ks defaults to (cfg.top_n,)
    assert 0.0 < res.mrr <= 1.0 and 0.0 <= res.auc <= 1.0 and 0.0 <= res[10][4] <= 1.0
    # (b) rank_eval at top_n = 50 against the dense route (the parent's only route there), wherever float64 certifies
    lo, hi, S = _intervals(small)
    ks = (10, 20, 50, 100)
    users, mask_ptr, mask_idx, pos_ptr, pos_idx = trainer._eval_sets.eval_set(frame, sort_masks=True)[2:7]
    ptr = pos_ptr.cpu().numpy()
    certified_rows = np.array([r for r in range(len(pos)) if (lo[ptr[r]:ptr[r + 1]] == hi[ptr[r]:ptr[r + 1]]).all()])
    sub = frame.iloc[certified_rows]                                  # the rows whose every rank float64 certifies
    cfg.top_n, cfg.rank_eval = 50, True
    try:
        four = trainer.evaluate(frame, "test")
        many = trainer.evaluate_ranks(frame, ks=ks)
        dense = dense_topk(trainer, frame)
        four_sub = trainer.evaluate(sub)
    finally:
        cfg.top_n, cfg.rank_eval = 10, False
    assert tuple(four) == tuple(many[50][:4])
    # the trainer's figures are the metrics of the ranks the sweep gives on the model's tables, and those ranks lie
    # inside their float64 intervals: this bounds every row, certified or not
    rank = engine.catalogue_ranks([_t(x, users.device) for x in lu], [_t(x, users.device) for x in li], users,
                                  pos_ptr, pos_idx, mask_ptr, mask_idx).cpu().numpy()
    assert ((lo <= rank) & (rank <= hi)).all()
    mine = ref.metrics_from_ranks(_rows(rank, ptr), ks, [NI - len(m) for m in masks])
    for k in ks:
        np.testing.assert_allclose(many[k], mine[k], rtol=0, atol=1e-12)
    assert abs(many.mrr - mine["mrr"]) < 1e-12 and abs(many.auc - mine["auc"]) < 1e-12
    # every certified target: inside the dense top-50 exactly when its rank is below 50, and at that place
    lists = dense.cpu().numpy()
    assert lists.shape == (len(pos), 50)
    certified = np.flatnonzero(lo == hi)
    uncertified = len(lo) - len(certified)
    print(f"{type(trainer).__name__}: {uncertified} of {len(lo)} ranks not certified by float64, "
          f"{len(certified_rows)} of {len(pos)} rows wholly certified")
    assert uncertified <= cc.RANDOM_CAP * len(lo)                     # the cap of the random cases holds here too
    row_of = np.repeat(np.arange(len(pos)), np.diff(ptr))
    flat = np.concatenate([np.asarray(p, np.int64) for p in pos])
    inside = below = 0
    for e in certified:
        r, t = row_of[e], flat[e]
        where = np.flatnonzero(lists[r] == t)
        assert (rank[e] < 50) == (len(where) == 1), f"row {r}, target {t}: rank {rank[e]}, dense places {where}"
        if len(where):
            assert where[0] == rank[e]
            inside += 1
        else:
            below += 1
    assert inside > 0 and below > 0                                   # the comparison ran on both sides of k = 50
    # the wholly certified rows as a frame of their own: the two routes' four metrics agree to 1e-12
    assert len(certified_rows) >= len(pos) // 2 and any(len(pos[r]) > 16 for r in certified_rows)
    sub_ptr, sub_idx = ref.csr([pos[r] for r in certified_rows])
    want_sub = engine.rank_metrics(dense[_t(certified_rows, dense.device)].contiguous(), _t(sub_ptr, dense.device),
                                   _t(sub_idx, dense.device))[:4].tolist()
    np.testing.assert_allclose(four_sub, want_sub, rtol=0, atol=1e-12)


def test_mf_trainer_rank_route(device, mf_small):
    from yelprecommendation_amd import engine

    def dense(trainer, frame):
        users, mask_ptr, mask_idx = trainer._eval_sets.eval_set(frame, sort_masks=True)[2:5]
        U, I = trainer.model.user_embedding.weight.detach(), trainer.model.item_embedding.weight.detach()
        return engine.mf_recommend(U, I, users, mask_ptr, mask_idx, 50, fused=False)
    _check_trainer(mf_small, dense)


def test_ngcf_trainer_rank_route(device, ngcf_small):
    def dense(trainer, frame):
        users, mask_ptr, mask_idx = trainer._eval_sets.eval_set(frame, sort_masks=True)[2:5]
        return trainer._recommend_chunked(users, mask_ptr, mask_idx)       # top_n = 50: the parent's only route
    _check_trainer(ngcf_small, dense)


def test_refusals_come_before_any_launch(device, mf_small, monkeypatch, tmp_path):
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.trainers import MFTrainer
    from yelprecommendation_amd.utils import make_config
    trainer, frame = mf_small[:2]

    def no_launch(*a, **k):
        raise AssertionError("a launch after a refusal")
    monkeypatch.setattr(engine, "catalogue_ranks", no_launch)
    monkeypatch.setattr(trainer, "world_size", 2)
    with pytest.raises(NotImplementedError, match="world_size"):
        trainer.evaluate_ranks(frame)
    wide = MFTrainer(make_config("MF", embed_size=256, device="cuda", model_dir=str(tmp_path)), NI, NU)
    with pytest.raises(NotImplementedError, match="256"):
        wide.evaluate_ranks(frame)


def test_train_main_logs_every_cutoff(device, tmp_path, caplog):
    from yelprecommendation_amd import train
    argv = ["model_name=MF", "synthetic=120x90x12", "fast_loader=true", "epochs=2", "batch_size=256", "embed_size=16",
            "lr=0.01", "seed=42", "top_n=50", "rank_eval=true", "eval_ks=[10,20,50]", f"model_dir={tmp_path}"]
    with caplog.at_level(logging.INFO, logger="yelprecommendation_amd"):
        metrics = train.main(argv)
    assert len(metrics) == 4 and all(np.isfinite(m) and 0.0 <= m <= 1.0 for m in metrics)
    text = caplog.text
    for k in (10, 20, 50):
        assert f"precision@{k} " in text and f"HR@{k}" in text
    assert "eval_ks=[10, 20, 50]" in text and "MRR" in text and "AUC" in text
