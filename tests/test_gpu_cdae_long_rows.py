"""The CDAE list kernels (csrc/cdae_sparse.hip, cdae_hidden_bwd of csrc/cdae.hip) on rows longer than one staging
pass (kListCap = 2,048 entries) and at every split count of the sampled decoder, each entry point called directly and
compared with the float64 reference of tests/cdae_ref64.py at the bars stated there (tests/test_cdae_ref64.py shows
that those bars notice a lost, repeated or skipped list entry).  Every case prints max |err| / bar per output."""
import numpy as np
import pytest
import torch

import cdae_ref64 as R
from oracle import cdae as ocdae

pytestmark = pytest.mark.gpu


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _n(a):
    return a.detach().cpu().numpy()


def _counts(k, I):
    return [I if c < 0 else c for c in k]


def _report(what, ratios):
    print(f"{what}: max |err| / bar " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v < 1.0}
    assert not bad, (what, bad)


def _loss_lists(engine, device, target, negmask):
    """The loss lists of (target, negmask) in buffers of their own, checked against the dense inputs first (a list
    fault is then told apart from a consumer fault)."""
    B, I = target.shape
    n = B * engine.SPARSE_PARTS * engine.sparse_part_columns(I)
    L = (torch.empty(n, dtype=torch.int32, device=device), torch.empty(n, dtype=torch.float32, device=device),
         torch.empty(B * engine.SPARSE_PARTS, dtype=torch.int32, device=device))
    rows = engine.SparseRows(target, 0, 0.0, negative_mask=negmask, loss_lists=L)
    assert torch.equal(rows.to_dense(), target)
    both = engine.SparseRows.from_buffers(L[0], L[1] + 1.0, L[2], B, I).to_dense()       # as TrainLists.loss_dense
    assert torch.equal((both == 2.0).float(), target) and torch.equal((both == 1.0).float(), negmask)
    return L


def _spread(device, engine, value):
    """A spread count whose value sits in several of its 64 slots."""
    c = torch.zeros(engine.COUNT_WORDS, dtype=torch.int32, device=device)
    stride = engine.COUNT_WORDS // engine.COUNT_SLOTS
    c[0], c[5 * stride], c[63 * stride] = value - 9, 7, 2
    return c


def _count_value(engine, count):
    stride = engine.COUNT_WORDS // engine.COUNT_SLOTS
    c = count.view(engine.COUNT_SLOTS, stride)
    assert int(c[:, 1:].abs().sum()) == 0                     # only the 64 slot words are written
    return int(c[:, 0].sum())


# ---- a. encoder -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("I,H,act,transposed,p", R.ENCODER_CASES)
def test_encoder_on_long_rows(device, I, H, act, transposed, p):
    """cdae_sparse_encode_kernel<false / true> on rows of 0, 1, 2047, 2048, 2049, 4096, 4097 and I entries: up to
    three staging passes, the h0 loop beyond one round (H = 300), an out-of-range user (flag, no V row)."""
    from yelprecommendation_amd import engine
    c = R.encoder_case(I, H, act, transposed, p)
    x = _t(c["x"], device)
    x_in = engine.dropout_seeded(x, c["seed"], p) if p > 0 else x
    rows = engine.SparseRows(x, c["seed"], p)
    assert torch.equal(rows.to_dense(), x_in)
    per_row = rows.count.view(-1, engine.SPARSE_PARTS).sum(1).cpu().tolist()
    assert per_row == (x_in != 0).sum(1).cpu().tolist() and (p > 0 or per_row == _counts(R.ENC_COUNTS, I))
    assert max(per_row) > R.LIST_CAP
    xin = _n(x_in)
    Wh, bh, V = R.encoder_params(c["rs"], H, I, R.ENCODER_USERS, xin)
    flag = engine.new_error_flag(device)
    W = _t(Wh.T if transposed else Wh, device)
    z = engine.cdae_sparse_encode(rows, W, _t(bh, device), _t(V, device), _t(c["user"], device), act, err_flag=flag,
                                  transposed=transposed)
    assert int(flag.item()) == engine.FLAG_BAD_USER
    _report(f"encoder I={I} H={H} act={act} transposed={transposed} p={p}",
            {"z": R.ratio(_n(z), R.encode(Wh, bh, V, c["user"], xin, act))})


# ---- b. sampled decoder with gradients ------------------------------------------------------------------------------

def _decode(engine, device, c, B, H, I, act, grads=True, dz_fill=0.0):
    f32 = torch.float32
    L = _loss_lists(engine, device, _t(c["target"], device), _t(c["negmask"], device))
    assert L[2].view(B, -1).sum(1).cpu().tolist() == _counts(c["counts"], I)
    splits = engine.cdae_sampled_decode_splits(B)
    z, Wo = _t(c["z"], device), _t(c["Wo"], device)
    bo = None if c["bo"] is None else _t(c["bo"], device)
    dz = torch.full((B, H), dz_fill, dtype=f32, device=device) if grads else None
    dWo = torch.zeros(I, H, dtype=f32, device=device) if grads else None
    dbo = torch.zeros(I, dtype=f32, device=device) if grads else None
    partials = torch.full((B * splits,), float("nan"), dtype=f32, device=device)
    count = torch.zeros(engine.COUNT_WORDS, dtype=torch.int32, device=device)
    engine.cdae_sampled_decode(L, z, Wo, bo, act, dz, dWo, dbo, partials, count)
    return L, splits, dz, dWo, dbo, partials, count


def _decode_ratios(engine, ref, B, splits, dz, dWo, dbo, partials, count):
    assert _count_value(engine, count) == ref["count"]
    out = {"partials": R.ratio(_n(partials).reshape(B, splits), ref["partials"], R.loss_bar),
           "loss": R.ratio(_n(partials).astype(np.float64).sum(), ref["loss"], R.loss_bar)}
    if dz is not None:
        out.update(dz=R.ratio(_n(dz), ref["dz"]), dWo=R.ratio(_n(dWo), ref["dWo"]), dbo=R.ratio(_n(dbo), ref["dbo"]))
    return out


@pytest.mark.parametrize("B,I,H,act,with_bo,long", R.DECODE_CASES)
def test_sampled_decoder_every_split_count_and_long_rows(device, B, I, H, act, with_bo, long):
    """cdae_sampled_decode_kernel<32, 4 | 8, false, false> (a half-wave per position) with gradients: splits 8, 8, 7,
    6, 5, 4, 3, 2, 1, 1 on short rows, and the multi-pass walk of the long rows at splits 8, 3 and 1; dz, dW_o, db_o,
    every loss partial, their sum and the spread count.  splits = 1 stores dz: a sentinel in dz on entry changes
    nothing."""
    from yelprecommendation_amd import engine
    c = R.decode_case(B, I, H, act, with_bo, long)
    _, splits, dz, dWo, dbo, partials, count = _decode(engine, device, c, B, H, I, act)
    assert splits == (R.DECODE_SPLITS[B] if B in R.DECODE_SPLITS else {9: 8, 300: 1}[B])
    ref = R.sampled_decode(c["z"], c["Wo"], c["bo"], c["target"], c["negmask"], act, splits=splits)
    _report(f"decoder B={B} splits={splits} I={I} H={H} act={act} bo={with_bo}",
            _decode_ratios(engine, ref, B, splits, dz, dWo, dbo, partials, count))
    if splits == 1:
        again = _decode(engine, device, c, B, H, I, act, dz_fill=7.5)
        assert torch.equal(again[2], dz)


def test_sampled_decoder_refuses_wide_hidden_layers(device):
    from yelprecommendation_amd import engine
    c = R.decode_case(4, 301, 260, 1, True, False)
    with pytest.raises(engine.EngineError):
        _decode(engine, device, c, 4, 260, 301, 1)


# ---- c. sampled decoder, loss only ----------------------------------------------------------------------------------

@pytest.mark.parametrize("B,I,H,act", R.LOSS_ONLY_CASES)
def test_loss_only_decoder_and_the_loss_finalizers(device, B, I, H, act):
    """dz = dWo = dbo = None: the LOSS_ONLY instances of cdae_sampled_decode_kernel (H % 4 == 0) and the gradient
    instance run without gradient buffers (H = 130) on the long rows and on rows of 31 ... 65 positions (the 32-slot
    settle() hand-off); then cdae_loss_finalize and cdae_loss_finalize_batched (batch_rows = 7 does not divide the
    rows; run twice on the same buffers; ``arrive`` left at zero) against float64 means per batch."""
    from yelprecommendation_amd import engine
    c = R.decode_case(B, I, H, act, True, True, settle=True)
    L, splits, _, _, _, partials, count = _decode(engine, device, c, B, H, I, act, grads=False)
    ref = R.sampled_decode(c["z"], c["Wo"], c["bo"], c["target"], c["negmask"], act, splits=splits)
    ratios = _decode_ratios(engine, ref, B, splits, None, None, None, partials, count)
    n_part = B * splits
    stats = torch.zeros(2, dtype=torch.float32, device=device)
    accum = torch.full((1,), 1.5, dtype=torch.float64, device=device)
    engine.cdae_loss_finalize(partials, n_part, count, stats, accum)
    cnt = ref["count"]
    mean = R.Out(ref["loss"].v / cnt, ref["loss"].n + n_part, ref["loss"].s / cnt)
    assert float(stats[1]) == cnt
    ratios["finalize"] = R.ratio(float(stats[0]), mean, R.loss_bar)
    ratios["finalize accum"] = R.ratio(float(accum.item()) - 1.5, mean, R.loss_bar)
    # batched: workgroup q owns rows [7 q, 7 q + 7)
    rows_per = 7
    nb = -(-B // rows_per)
    P, per_row = ref["partials"], np.asarray(_counts(c["counts"], I), np.float64)
    v, s, n = np.zeros(nb), np.zeros(nb), np.zeros(nb)
    for q in range(nb):
        sl = slice(q * rows_per, min(B, (q + 1) * rows_per))
        k = per_row[sl].sum()
        if k > 0:
            v[q], s[q] = P.v[sl].sum() / k, P.s[sl].sum() / k
        n[q] = P.n[sl].max() + P.v[sl].size
    want = R.Out(v, n, s)
    means = torch.full((nb,), float("nan"), dtype=torch.float32, device=device)
    arrive = torch.zeros(1, dtype=torch.int32, device=device)
    accum = torch.zeros(1, dtype=torch.float64, device=device)
    for k in (1, 2):
        engine.cdae_loss_finalize_batched(partials, splits, L[2], B, rows_per, means, arrive, accum)
        assert int(arrive.item()) == 0
        ratios[f"batched means {k}"] = R.ratio(_n(means), want, R.loss_bar)
        err = abs(float(accum.item()) - k * v.sum())
        ratios[f"batched accum {k}"] = float(R.over(err, k * R.loss_bar(want).sum()))
    _report(f"loss only B={B} splits={splits} I={I} H={H} act={act}", ratios)


# ---- d. cdae_hidden_bwd ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", R.HIDDEN_B)
def test_hidden_bwd_row_strides_and_tails(device, B):
    """The 1,024-thread kernel walks rows in strides of 128 (16 waves x 8 rows in flight) and clamps the tail: B on
    both sides of 16 and 128, H on both sides of a 64-column workgroup; duplicate users, an out-of-range user;
    dz in place, db_h, dV, the marks, and the loss workgroup's stats / loss_accum."""
    from yelprecommendation_amd import engine
    f32 = torch.float32
    worst = {}
    for H in R.HIDDEN_H:
        c = R.hidden_case(B, H)
        nu, cnt = R.HIDDEN_USERS, 37
        dz, dV = _t(c["dz"], device), torch.zeros(nu, H, dtype=f32, device=device)
        marks = torch.zeros(nu, dtype=torch.uint8, device=device)
        dbh = torch.full((H,), float("nan"), dtype=f32, device=device)
        stats = torch.zeros(2, dtype=f32, device=device)
        accum = torch.full((1,), 2.5, dtype=torch.float64, device=device)
        partials = _t(c["partials"], device)
        engine.cdae_hidden_bwd(dz, _t(c["z"], device), c["act"], _t(c["user"], device), dV, marks, dbh, partials,
                               partials.numel(), _spread(device, engine, cnt), stats, accum, scale_dz=c["scale_dz"])
        ref = R.hidden_bwd(c["dz"], c["z"], c["act"], c["user"], cnt if c["scale_dz"] else None, None, nu)
        p64 = c["partials"].astype(np.float64)
        mean = R.Out(p64.sum() / cnt, p64.size + 1, np.abs(p64).sum() / cnt)
        assert np.array_equal(_n(marks), ref["user_marks"]) and float(stats[1]) == cnt
        got = {"dz": R.ratio(_n(dz), ref["dz"]), "dbh": R.ratio(_n(dbh), ref["dbh"]), "dV": R.ratio(_n(dV), ref["dV"]),
               "loss": R.ratio(float(stats[0]), mean, R.loss_bar),
               "accum": R.ratio(float(accum.item()) - 2.5, mean, R.loss_bar)}
        for k, v in got.items():
            worst[k] = max(worst.get(k, 0.0), v)
    _report(f"hidden_bwd B={B} H={R.HIDDEN_H}", worst)


# ---- e. dW_h kernels on the long rows -------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel,H,act,scale_dz", R.DWH_CASES)
def test_dwh_kernels_on_long_rows(device, kernel, H, act, scale_dz):
    """cdae_hidden_bwd_dwh_t (H = 256, 100 and the h1 half at 320), cdae_sparse_dwh_t and cdae_sparse_dwh on rows of
    up to three staging passes: dW_h (either layout), db_h, dV; the item marks are exactly the listed columns (also
    on a batch without the every-column row); cdae_sparse_dwh twice on different batches (claim epochs), its
    transposed scratch all zero afterwards."""
    from yelprecommendation_amd import engine
    f32 = torch.float32
    I, nu, cnt = R.I_LONG, R.HIDDEN_USERS, 37
    worst = {}
    for batch, drop_full in ((0, False), (1, False), (0, True)):
        c = R.dwh_case(H, batch)
        x = c["x"].copy()
        if drop_full:
            x[[k for k, n in enumerate(R.ENC_COUNTS) if n < 0]] = 0.0
        rows = engine.SparseRows(_t(x, device))
        assert torch.equal(rows.to_dense(), _t(x, device))
        dz, z, user = _t(c["dz"], device), _t(c["z"], device), _t(c["user"], device)
        fused = kernel == "hidden_bwd_dwh_t"
        ref = R.hidden_bwd(c["dz"], c["z"], act if fused else 0, c["user"], cnt if (fused and scale_dz) else None, x, nu)
        got = {}
        if kernel == "sparse_dwh":
            dWh = torch.zeros(H, I, dtype=f32, device=device)
            engine.cdae_sparse_dwh(rows, dz, dWh)
            sc = engine._dwh_scratch[(dz.device, I, H)]
            listed = np.flatnonzero(ref["item_marks"])
            assert float(sc[0].abs().sum()) == 0.0
            assert int(sc[3].item()) == len(listed) and np.array_equal(np.sort(_n(sc[2][:len(listed)])), listed)
            got["dWh"] = R.ratio(_n(dWh), ref["dWh"])
        else:
            dWhT = torch.zeros(I, H, dtype=f32, device=device)
            items = torch.zeros(I, dtype=torch.uint8, device=device)
            if fused:
                dV, dbh = torch.zeros(nu, H, dtype=f32, device=device), torch.zeros(H, dtype=f32, device=device)
                marks = torch.zeros(nu, dtype=torch.uint8, device=device)
                stats = torch.zeros(2, dtype=f32, device=device)
                accum = torch.full((1,), 2.5, dtype=torch.float64, device=device)
                partials = _t(np.random.RandomState(H).rand(R.N_LONG * 8).astype(np.float32), device)
                engine.cdae_hidden_bwd_dwh_t(rows, dz, z, act, user, _spread(device, engine, cnt), dV, marks, dbh, dWhT,
                                             items, partials, partials.numel(), stats, accum, scale_dz=scale_dz)
                p64 = _n(partials).astype(np.float64)
                mean = R.Out(p64.sum() / cnt, p64.size + 1, np.abs(p64).sum() / cnt)
                assert np.array_equal(_n(marks), ref["user_marks"]) and float(stats[1]) == cnt
                assert torch.equal(dz, _t(c["dz"], device))                       # read only
                got.update(dbh=R.ratio(_n(dbh), ref["dbh"]), dV=R.ratio(_n(dV), ref["dV"]),
                           loss=R.ratio(float(stats[0]), mean, R.loss_bar),
                           accum=R.ratio(float(accum.item()) - 2.5, mean, R.loss_bar))
            else:
                engine.cdae_sparse_dwh_t(rows, dz, dWhT, items)
            assert np.array_equal(_n(items), ref["item_marks"]) and (not drop_full or 0 < int(items.sum()) < I)
            got["dWhT"] = R.ratio(_n(dWhT).T, ref["dWh"])
        for k, v in got.items():
            worst[k] = max(worst.get(k, 0.0), v)
    _report(f"{kernel} H={H} act={act} scale_dz={scale_dz}", worst)


# ---- f. whole step with a changing batch ----------------------------------------------------------------------------

@pytest.mark.parametrize("decoder,transposed", [("sampled", True), ("dense", False)])
def test_step_with_a_changing_batch_and_heavy_users(device, tmp_path, decoder, transposed):
    """One live CDAEStep takes batches of 300, 170, 41 and 300 rows (sampled decoder: 1, 3, 8 and 1 splits; dz, the
    counter, the partials and the loss lists are re-created at every change); row 0 of every batch has more than
    2,048 inputs after dropout and more than 2,048 loss positions, row 1 more than 2,048 loss positions.  After each
    step: loss, all five parameters and both Adam moments against oracle.cdae.CDAEState (bars of
    test_fused_step_equals_autograd_route), gradient buffers and marks clean."""
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.cdae_step import CDAEStep
    from yelprecommendation_amd.models.cdae import CDAE
    from yelprecommendation_amd.optim import Adam
    from yelprecommendation_amd.utils import make_config
    rs = np.random.RandomState(77)
    ni, nu, H, lr = R.I_LONG, 400, 128, 1e-4
    torch.manual_seed(5)
    model = CDAE(make_config("CDAE", hidden_size=H, device="cuda", model_dir=str(tmp_path), lr=lr), ni, nu)
    model.train()
    params = list(model.parameters())
    opt = Adam(params, lr=lr)
    ref = ocdae.CDAEState([_n(q).copy() for q in params], lr=lr)
    step = CDAEStep(model, opt, True, decoder=decoder, transposed_wh=transposed)
    assert step.decoder == decoder and step.transposed_wh == transposed
    p = model.corruption_level
    close = lambda a, b, what: torch.testing.assert_close(
        a, torch.from_numpy(b).to(a.device), rtol=2e-4, atol=1e-7 + 2e-5 * float(np.abs(b).max()), msg=lambda m: f"{what}: {m}")
    for k, B in enumerate((300, 170, 41, 300)):
        u = rs.permutation(nu)[:B].astype(np.int64); u[7] = u[2]
        x = (rs.rand(B, ni) < 0.005).astype(np.float32)
        x[0] = 0.0; x[0, rs.choice(ni, 5800, replace=False)] = 1.0
        x[1] = 0.0; x[1, rs.choice(ni, 400, replace=False)] = 1.0
        x[3] = 0.0
        neg = ((rs.rand(B, ni) < 0.025) * (1 - x)).astype(np.float32)
        neg[1] = 0.0; neg[1, rs.choice(np.flatnonzero(x[1] == 0), 2000, replace=False)] = 1.0
        seed = int(rs.randint(1, 1 << 40))
        xin = _n(engine.dropout_seeded(_t(x, device), seed, p)) if p > 0 else x
        assert (xin[0] != 0).sum() > R.LIST_CAP and ((x + neg)[:2] != 0).sum(1).min() > R.LIST_CAP
        want = float(ref.train_step(u, xin, x, neg))
        step.step(_t(u, device), _t(x, device), _t(neg, device), seed=seed, p=p)
        if decoder == "sampled":
            assert step.n_partials == B * engine.cdae_sampled_decode_splits(B)
        clean = [step.dV, step.dbh, step.touched_users] + ([step.dWo, step.dbo] if decoder == "sampled" else []) \
            + ([step._wht[3], step._wht[4]] if transposed else [step.dWh])
        assert all(float(g.float().abs().sum()) == 0.0 for g in clean)
        step.release()
        step.check()
        got = float(step.last_loss())
        print(f"step {k} B={B} {decoder}: loss {got:.7f} oracle {want:.7f} rel {abs(got - want) / want:.2e}")
        np.testing.assert_allclose(got, want, rtol=1e-5)
        for j, q in enumerate(params):
            close(q.data, ref.params[j], f"step {k} parameter {j}")
            close(opt.state[q]["exp_avg"], ref.opt.m[j], f"step {k} exp_avg {j}")
            close(opt.state[q]["exp_avg_sq"], ref.opt.v[j], f"step {k} exp_avg_sq {j}")


# ---- g. list-fed validation with heavy users ------------------------------------------------------------------------

def test_list_fed_validation_with_heavy_users(device, tmp_path):
    """CDAETrainer.validate / evaluate over CDAEBatchLoader(lists=True) where three users have 400 ... 900 items and
    neg_times = 5: their loss lists pass 2,048 entries in the grouped _scored_by_lists path (150 rows per launch:
    3 splits).  Against the dense per-batch route at the bars of
    test_list_route_of_validate_and_evaluate_equals_dense_route; the lists of yr_cdae_train_lists for those users:
    encoder list exact, negatives' count exact and disjoint from the positives."""
    from yelprecommendation_amd.data.cdae_batches import CDAEBatchLoader, CDAEInteractions
    from yelprecommendation_amd.trainers import CDAETrainer
    from yelprecommendation_amd.utils import make_config
    rs = np.random.RandomState(9)
    nu, ni, H, B, nt = 150, R.I_LONG, 64, 64, 5
    heavy = {5: 400, 70: 650, 149: 900}
    parts, taken = {}, np.zeros((nu, ni), bool)
    for name, hi in (("train", 30), ("valid", 8), ("test", 8)):
        counts = rs.randint(0, hi, nu)
        if name == "train":
            for u_, k in heavy.items():
                counts[u_] = k
        ptr = np.zeros(nu + 1, np.int64); ptr[1:] = np.cumsum(counts)
        idx = []
        for u_, k in enumerate(counts):
            pick = np.sort(rs.choice(np.flatnonzero(~taken[u_]), k, replace=False))
            taken[u_, pick] = True
            idx.append(pick)
        parts[name] = (torch.from_numpy(ptr), torch.from_numpy(np.concatenate(idx).astype(np.int64)))
    data = CDAEInteractions(nu, ni, parts, device)
    cfg = make_config("CDAE", hidden_size=H, device="cuda", model_dir=str(tmp_path), lr=1e-2, negative_sampling=True,
                      neg_times=nt, loss_name="bce", batch_size=B, top_n=10)
    trainer = CDAETrainer(cfg, ni, nu)
    trainer.train(CDAEBatchLoader(data, "train", batch_size=B, neg_times=nt, shuffle=True, seed=1, lists=True,
                                  dropout=trainer.model.corruption_level))          # a few steps off the init
    for mode in ("valid", "test"):
        as_lists = CDAEBatchLoader(data, mode, batch_size=B, neg_times=nt, seed=7, lists=True)
        dense, longest = [], 0
        for batch in CDAEBatchLoader(data, mode, batch_size=B, neg_times=nt, seed=7, lists=True):
            users = batch["user_id"]
            d = {"user_id": users, "item_lists": batch["item_lists"]}
            if mode == "valid":
                target, neg = batch["lists"].loss_dense()
                d.update(input_mask=data.dense("train", users), valid_mask=data.dense("valid", users), negative_mask=neg.clone())
                assert torch.equal(target, d["input_mask"] + d["valid_mask"])        # positives of the loss list
                assert float((neg * target).sum()) == 0.0 and torch.equal(neg.sum(1), nt * target.sum(1))
                longest = max(longest, int((neg + target).sum(1).max()))
            else:
                d.update(input_mask=data.dense("train_valid", users), test_mask=data.dense("test", users))
            assert torch.equal(batch["lists"].rows.to_dense(), d["input_mask"])      # the encoder's input
            dense.append(d)
        if mode == "valid":
            assert longest > 2 * R.LIST_CAP                                          # 900 items: three staging passes
            got, want = trainer.validate(as_lists), trainer.validate(dense)
            print("validate lists", got, "dense", want)
            np.testing.assert_allclose(got[0], want[0], rtol=1e-5)
            np.testing.assert_allclose(got[1:], want[1:], atol=1e-3, rtol=0)
            trainer.cfg.eval_batch_group = 1                                         # per batch: 8, 8 and 8 splits
            again = trainer.validate(CDAEBatchLoader(data, mode, batch_size=B, neg_times=nt, seed=7, lists=True))
            trainer.cfg.eval_batch_group = 32
            np.testing.assert_allclose(again[0], got[0], rtol=2e-6)
            assert tuple(again[1:]) == tuple(got[1:])
        else:
            got, want = trainer.evaluate(as_lists), trainer.evaluate(dense)
            print("evaluate lists", got, "dense", want)
            np.testing.assert_allclose(got, want, atol=1e-3, rtol=0)
