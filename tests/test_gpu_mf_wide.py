"""BPR-MF at the wide embedding widths (256 / 512 / 1024) on the GPU: the push-form kernels, the two-launch step
with touched-row marks on rows wider than one wave, the slab sweep of the fused evaluation against float64 on
certified ladders, the score GEMM, and the trainer.  Every case needs a width the narrow kernels refuse."""
import itertools
import os

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import bpr_mf as obpr

import eval_ladders as el
from mf_wide_cases import LADDER_SPECS, WIDE, ladder_case, spec_id
from replay import assert_topk_equal_up_to_near_ties
from test_eval_ladders import _check

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24


def _tables(rs, nu, ni, d, scale=0.3):
    return ((rs.standard_normal((nu, d)) * scale).astype(np.float32),
            (rs.standard_normal((ni, d)) * scale).astype(np.float32))


def _dot_bar(U, I, u, i):
    """float64 dot products of the f32 rows and the bar on an f32 result: any-order f32 accumulation of D products is
    off by at most (D + 1) 2^-24 sum |u_d i_d| to first order; a factor 2 of margin."""
    P = U[u].astype(np.float64) * I[i].astype(np.float64)
    return P.sum(axis=1), 2 * (U.shape[1] + 1) * U24 * np.abs(P).sum(axis=1)


# ---- 1. mf_score and its backward ------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", WIDE)
@pytest.mark.parametrize("B", [1, 257, 1000])
def test_mf_score(device, d, B):
    from yelprecommendation_amd import engine
    rs = np.random.RandomState(B + d)
    nu, ni = 301, 517
    U, I = _tables(rs, nu, ni, d)
    u = rs.randint(0, nu, size=B).astype(np.int64)
    i = rs.randint(0, ni, size=B).astype(np.int64)
    t = lambda a: torch.from_numpy(a).to(device)
    dU, dI, du, di = t(U), t(I), t(u), t(i)
    got = engine.mf_score(dU, dI, du, di).cpu().numpy().astype(np.float64)
    want, bar = _dot_bar(U, I, u, i)
    print(f"mf_score d={d} B={B}: max |err| / bar = {np.max(np.abs(got - want) / bar):.3f}")
    assert np.all(np.abs(got - want) <= bar)

    # backward: gradU[u[b]] += gout[b] I[i[b]], gradI[i[b]] += gout[b] U[u[b]].  Every contribution is one rounded
    # product; a row element with c contributions is their f32 sum in arrival order (c roundings at most, counting
    # the add onto zero): (c + 1) 2^-24 sum |contribution|, with the same factor 2.
    gout = rs.standard_normal(B).astype(np.float32)
    gU, gI = torch.zeros_like(dU), torch.zeros_like(dI)
    engine.mf_score_backward(dU, dI, du, di, t(gout), gU, gI)
    g64 = gout.astype(np.float64)[:, None]
    for got_g, idx, rows, other in ((gU, u, nu, I[i]), (gI, i, ni, U[u])):
        C = g64 * other.astype(np.float64)
        want_g, mag = np.zeros((rows, d)), np.zeros((rows, d))
        np.add.at(want_g, idx, C)
        np.add.at(mag, idx, np.abs(C))
        c = np.bincount(idx, minlength=rows)[:, None]
        assert np.all(np.abs(got_g.cpu().numpy() - want_g) <= 2 * (c + 1) * U24 * mag)


# ---- 2. fused forward + loss + backward ------------------------------------------------------------------------------

def _loss_and_grads64(U, I, u, p, n):
    """oracle.bpr_mf.loss_and_grads, evaluated in float64 (the oracle's own functions round to f32 on the way)."""
    U, I = U.astype(np.float64), I.astype(np.float64)
    x = np.sum(U[u] * (I[p] - I[n]), axis=1)
    loss = np.mean(np.maximum(-x, 0) + np.log1p(np.exp(-np.abs(x))))
    z = np.exp(-np.abs(x))
    g = (-np.where(x < 0, 1 / (1 + z), z / (1 + z)) / len(u))[:, None]
    # index_add as a product with 0/1 selection matrices (np.add.at takes minutes at 140,000 x 256)
    B, rows = len(u), np.arange(len(u))
    Su, Si = np.zeros((U.shape[0], B)), np.zeros((I.shape[0], B))
    Su[u, rows] = 1.0
    np.add.at(Si, (p, rows), 1.0)
    np.add.at(Si, (n, rows), -1.0)
    return loss, Su @ (g * (I[p] - I[n])), Si @ (g * U[u])


# B <= 16,384: the TILE = 16 kernel; 20,000: TILE = 64; 140,000 (d = 256 only): TILE = 256
FWD_BWD = [(d, B) for d in WIDE for B in (1, 7, 777, 4096, 20000)] + [(256, 140000)]


@pytest.mark.parametrize("d,B", FWD_BWD)
def test_bpr_fwd_bwd(device, d, B):
    from yelprecommendation_amd import engine
    rs = np.random.RandomState(1000 + B + d)
    nu, ni = 97, 131            # small tables => many duplicate rows inside the batch
    U, I = _tables(rs, nu, ni, d)
    u, p, n = (rs.randint(0, m, size=B).astype(np.int64) for m in (nu, ni, ni))
    # own test of the oracle restatement: float64 == the f32 oracle to f32 rounding (small batch only: cost)
    loss, gU, gI = _loss_and_grads64(U, I, u, p, n)
    if B <= 777:
        lo, gUo, gIo = obpr.loss_and_grads(U, I, u, p, n)
        np.testing.assert_allclose(lo, loss, rtol=1e-4)
        np.testing.assert_allclose(gUo, gU, rtol=1e-2, atol=1e-5)

    t = lambda a: torch.from_numpy(a).to(device)
    dU, dI, idx = t(U), t(I), [t(a) for a in (u, p, n)]
    gradU, gradI = torch.zeros_like(dU), torch.zeros_like(dI)
    partials = torch.full((engine.LOSS_PARTIALS,), 7.0, dtype=torch.float32, device=device)
    flag = engine.new_error_flag(device)
    engine.bpr_mf_fwd_bwd(dU, dI, *idx, gradU, gradI, partials, err_flag=flag)
    out = engine.loss_finalize(partials, 1.0 / B)
    assert int(flag.item()) == 0
    gotU, gotI = gradU.cpu().numpy(), gradI.cpu().numpy()
    for name, got, want in (("gradU", gotU, gU), ("gradI", gotI, gI)):
        excess = np.abs(got - want) - (1e-6 + 1e-4 * np.abs(want))
        print(f"bpr_fwd_bwd d={d} B={B} {name}: max (|err| - atol - rtol |want|) = {excess.max():.3e}")
    print(f"bpr_fwd_bwd d={d} B={B} loss rel err {abs(out.item() - loss) / abs(loss):.3e}")
    np.testing.assert_allclose(out.item(), loss, rtol=1e-5)
    np.testing.assert_allclose(gotU, gU, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(gotI, gI, rtol=1e-4, atol=1e-6)

    # forward-only mode (validate): same loss, no gradient buffers
    partials.fill_(3.0)
    engine.bpr_mf_fwd_bwd(dU, dI, *idx, None, None, partials)
    np.testing.assert_allclose(engine.loss_finalize(partials, 1.0 / B).item(), loss, rtol=1e-5)


def test_bpr_empty_and_bad_index(device):
    from yelprecommendation_amd import engine
    rs = np.random.RandomState(5)
    U, I = _tables(rs, 10, 12, 512)
    dU, dI = torch.from_numpy(U).to(device), torch.from_numpy(I).to(device)
    gradU, gradI = torch.zeros_like(dU), torch.zeros_like(dI)
    partials = torch.ones(engine.LOSS_PARTIALS, dtype=torch.float32, device=device)
    e = torch.zeros(0, dtype=torch.int64, device=device)
    engine.bpr_mf_fwd_bwd(dU, dI, e, e, e, gradU, gradI, partials)        # empty batch
    assert float(partials.sum().item()) == 0.0 and float(gradU.abs().sum().item()) == 0.0
    u = torch.tensor([0, 3, 10, 2], dtype=torch.int64, device=device)      # 10 is out of range
    p = torch.tensor([1, 2, 3, 12], dtype=torch.int64, device=device)      # 12 is out of range
    n = torch.tensor([4, 5, 6, -1], dtype=torch.int64, device=device)      # -1 is out of range
    flag = engine.new_error_flag(device)
    engine.bpr_mf_fwd_bwd(dU, dI, u, p, n, gradU, gradI, partials, err_flag=flag)
    assert int(flag.item()) == (engine.FLAG_BAD_USER | engine.FLAG_BAD_ITEM)
    # the two valid triplets still contributed, scaled by inv_batch = 1/4 (not 1/2)
    _, gU, gI = obpr.loss_and_grads(U, I, np.array([0, 3]), np.array([1, 2]), np.array([4, 5]))
    np.testing.assert_allclose(gradU.cpu().numpy(), gU * 0.5, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(gradI.cpu().numpy(), gI * 0.5, rtol=1e-4, atol=1e-7)
    with pytest.raises(IndexError):
        engine.raise_on_flag(flag)


# ---- 3. the two-launch step: scatter with marks + one Adam pass ---------------------------------------------------------

@pytest.mark.parametrize("d,nu,ni", [(256, 40, 56), (512, 40, 56), (1024, 40, 56), (1024, 3000, 3000)],
                         ids=["256", "512", "1024", "1024-several-workgroups"])
def test_scatter_step_with_marks(device, d, nu, ni):
    """Three steps of BPRMFStep(impl="auto") — at these widths always the push form — against the oracle after every
    step; step 2 touches none of step 1's user rows, step 3 returns to them.  Rows outside a step's batch get exactly
    the zero-gradient Adam update, and every mark reads 0 after the step.  3,000 x 3,000 rows at d = 1024: 1.5 M
    float4 in the Adam launch, more workgroups than the grid cap and several grid-stride iterations each."""
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.bpr_step import BPRMFStep
    rs = np.random.RandomState(7 * d + nu)
    U, I = _tables(rs, nu, ni, d, scale=0.2)
    lr = 5e-3
    ref = obpr.MFState(U, I, "adam", lr=lr)
    step = BPRMFStep(torch.from_numpy(U).to(device), torch.from_numpy(I).to(device), lr=lr, impl="auto")
    half = nu // 2
    user_ranges = ((0, half), (half, nu), (0, half))
    total = 0.0
    for k, (lo, hi) in enumerate(user_ranges):
        u = rs.randint(lo, hi, size=64).astype(np.int64)
        p = rs.randint(0, ni, size=64).astype(np.int64)
        n = rs.randint(0, ni, size=64).astype(np.int64)
        # the zero-gradient update of every row, by the plain dense kernel on copies
        zero = {}
        for name, P, M, V in (("U", step.U, step.mU, step.vU), ("I", step.I, step.mI, step.vI)):
            c = [x.clone() for x in (P, M, V)]
            engine.adam_dense(c[0], torch.zeros_like(c[0]), c[1], c[2], k + 1, lr)
            zero[name] = c
        total += float(ref.train_step(u, p, n))
        step.step(*(torch.from_numpy(a).to(device) for a in (u, p, n)))
        assert step.impl.startswith("atomic")
        step.check()
        assert int(step._touched.count_nonzero().item()) == 0
        assert float(step.gU.abs().sum().item()) == 0.0 and float(step.gI.abs().sum().item()) == 0.0
        np.testing.assert_allclose(step.U.cpu().numpy(), ref.U, rtol=1e-3, atol=1e-5)
        np.testing.assert_allclose(step.I.cpu().numpy(), ref.I, rtol=1e-3, atol=1e-5)
        np.testing.assert_allclose(step.mU.cpu().numpy(), ref.opt.m[0], rtol=1e-3, atol=1e-8)
        np.testing.assert_allclose(step.mI.cpu().numpy(), ref.opt.m[1], rtol=1e-3, atol=1e-8)
        np.testing.assert_allclose(step.vU.cpu().numpy(), ref.opt.v[0], rtol=1e-3, atol=1e-11)
        np.testing.assert_allclose(step.vI.cpu().numpy(), ref.opt.v[1], rtol=1e-3, atol=1e-11)
        for name, rows, touched, got in (("U", nu, u, (step.U, step.mU, step.vU)),
                                         ("I", ni, np.concatenate([p, n]), (step.I, step.mI, step.vI))):
            rest = torch.from_numpy(np.setdiff1d(np.arange(rows), touched)).to(device)
            assert len(rest) > 0
            for a, b in zip(got, zero[name]):
                assert torch.equal(a[rest], b[rest]), (k, name)
    np.testing.assert_allclose(step.epoch_loss(), total, rtol=2e-5)


# ---- 4. fused evaluation == float64 on certified ladders ----------------------------------------------------------------

@pytest.mark.parametrize("spec", LADDER_SPECS, ids=spec_id)
def test_fused_evaluation_equals_float64_on_certified_ladders(device, spec):
    """As test_eval_ladders.test_fused_evaluation_equals_float64_on_certified_ladders, for the slab sweep: exact list
    equality, both precisions, prescan flag off / on (the wide form runs none: same lists), catalogue slices on /
    off, the four hint kinds, every mask value; mf_recommend fused and unfused (the wide score GEMM) without bias."""
    from yelprecommendation_amd import engine
    D, N, n, k, bias = spec
    case = ladder_case(spec)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    U, I, users = t(case.U), t(case.I), t(case.users)
    b = t(case.bias) if bias else None
    ptr, idx = t(case.mask_ptr), t(case.mask_idx)
    exp_mask = case.expected[el.MASK_VALUE]
    top1 = el.order_rows(case.scores64(mask_value=el.MASK_VALUE), k + 1) if N > k else None
    rs = np.random.RandomState(D + k)
    junk = rs.randint(0, N, (n, k)).astype(np.int64)
    junk[:, 0] = -1
    if k > 1:
        junk[1::2, 1] = N + 7
        junk[2::3, -1] = junk[2::3, 0]
    hints = {"none": None, "expected": exp_mask, "junk": junk}
    if top1 is not None:
        swapped = top1[:, :k].copy()
        swapped[:, k - 1] = top1[:, k]
        hints["kth_swapped"] = swapped
    hint_names = list(hints)
    runs = []
    for precision in ("f32", "bf16x3"):
        forms = [None] if precision == "f32" else [None, "two_roles"]     # (one wide form: the flag is ignored)
        for form, prescan, sliced in itertools.product(forms, (False, True), (True, False)):
            if prescan and not sliced:
                continue                                # (sliced=False implies no prescan)
            runs.append(dict(precision=precision, form=form, prescan=prescan, sliced=sliced))
    for j, kw in enumerate(runs):
        if kw["prescan"]:
            combos = [("none", mv) for mv in el.MASK_VALUES]
        else:
            combos = [(h, el.MASK_VALUES[(j + (h == "none")) % len(el.MASK_VALUES)])
                      for h in (hint_names[(j + k) % len(hint_names)], hint_names[(j + k + 1) % len(hint_names)])]
        for h, mv in combos:
            hint = case.expected[mv] if h == "expected" else hints[h]
            _check(engine, case, (U, I, users, ptr, idx, b), mv, None if hint is None else t(hint), dict(kw, hint=h))
    if not bias:
        for fused in (False, True):
            got = engine.mf_recommend(U, I, users, ptr, idx, k, fused=fused).cpu().numpy()
            assert np.array_equal(got, exp_mask), f"mf_recommend(fused={fused})"


def test_fused_evaluation_refuses_long_lists_at_the_wide_widths(device):
    from yelprecommendation_amd import engine
    U = torch.zeros(4, 256, device=device)
    I = torch.zeros(40, 256, device=device)
    with pytest.raises(engine.EngineError, match="unsupported"):
        engine.mf_eval_topk(U, I, torch.arange(4, device=device), None, None, 17)


# ---- 5. the score GEMM ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", WIDE)
@pytest.mark.parametrize("n,ni", [(70, 333), (5, 4100)])
def test_mf_scores_gemm(device, d, n, ni):
    from yelprecommendation_amd import engine
    rs = np.random.RandomState(d + n)
    nu = 90
    U, I = _tables(rs, nu, ni, d)
    users = rs.randint(0, nu, size=n).astype(np.int64)
    S = engine.mf_scores_gemm(torch.from_numpy(U).to(device), torch.from_numpy(I).to(device),
                              torch.from_numpy(users).to(device)).cpu().numpy().astype(np.float64)
    assert S.shape == (n, ni)
    U64, I64 = U[users].astype(np.float64), I.astype(np.float64)
    want = U64 @ I64.T
    bar = 2 * (d + 1) * U24 * (np.abs(U64) @ np.abs(I64).T)
    assert np.all(np.abs(S - want) <= bar)


# ---- 6. the trainer --------------------------------------------------------------------------------------------------

def test_trainer_at_width_256(device, tmp_path):
    """MFTrainer at embed_size = 256 on the synthetic set of test_gpu_mf_trainer.py (300 x 500, 12 items per user):
    two epochs of batches of 256, epoch losses == the oracle replay (rtol 1e-4, that file's bar), evaluation lists
    == float64 up to near-ties, best-model and checkpoint round trips.
    Checkpoint: what is loaded equals what was saved bit for bit, and so does the first thing computed from it (the
    evaluation lists).  The CONTINUED training run is compared at test_checkpoint_resume_continues_the_run's bars,
    not bitwise: the step's float atomics add in arrival order (the fixed-order form is the pull form, which these
    widths do not have), so two runs of the same step from the same bits may differ in the last place."""
    from yelprecommendation_amd.data.synthetic import make_interactions_torch
    from yelprecommendation_amd.trainers import MFTrainer
    from yelprecommendation_amd.utils import make_config
    nu, ni, bs = 300, 500, 256
    iu, ii = (x.numpy() for x in make_interactions_torch(nu, ni, 12.0, seed=3))
    rs = np.random.RandomState(8)
    cfg = make_config("MF", device="cuda", model_dir=str(tmp_path), embed_size=256, batch_size=bs, lr=1e-3, top_n=10)
    torch.manual_seed(2)
    t = MFTrainer(cfg, ni, nu)
    ref = obpr.MFState(t.model.user_embedding.weight.detach().cpu().numpy(),
                       t.model.item_embedding.weight.detach().cpu().numpy(), "adam", lr=cfg.lr)

    def epoch():
        order = rs.permutation(len(iu))
        u, p, n = iu[order], ii[order], rs.randint(0, ni, size=len(iu)).astype(np.int64)
        sizes = [min(bs, len(u) - s) for s in range(0, len(u), bs)]
        batches = [{"user_id": torch.from_numpy(u[s:s + bs]), "pos_item": torch.from_numpy(p[s:s + bs]),
                    "neg_item": torch.from_numpy(n[s:s + bs])} for s in range(0, len(u), bs)]
        return (u, p, n, sizes), batches

    masks = [ii[iu == r] for r in range(nu)]
    frame = pd.DataFrame({"pos_items": [[int(rs.randint(0, ni))] for _ in range(nu)],
                          "mask_items": [m.tolist() for m in masks]}, index=pd.Index(np.arange(nu), name="user_id"))
    for e in range(2):
        (u, p, n, sizes), batches = epoch()
        want, _ = ref.train_epoch(u, p, n, sizes)
        np.testing.assert_allclose(t.train(batches), want, rtol=1e-4)
        (u, p, n, sizes), batches = epoch()
        want, _ = ref.valid_epoch(u, p, n, sizes)
        np.testing.assert_allclose(t.validate(batches), want, rtol=1e-4)
        t.evaluate(frame, "valid")                       # the second one runs with the first one's lists as hints
    np.testing.assert_allclose(t.model.user_embedding.weight.detach().cpu().numpy(), ref.U, rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(t.model.item_embedding.weight.detach().cpu().numpy(), ref.I, rtol=1e-3, atol=2e-5)

    def lists(tr):
        _, users, mask_ptr, mask_idx = tr._eval_arrays(frame)
        return tr.recommend(users, mask_ptr, mask_idx).cpu().numpy(), users.cpu().numpy()

    top, users = lists(t)
    Ug, Ig = (w.detach().cpu().numpy() for w in (t.model.user_embedding.weight, t.model.item_embedding.weight))
    S = Ug[users].astype(np.float64) @ Ig.astype(np.float64).T
    for r, uid in enumerate(users):
        S[r, masks[uid]] = el.MASK_VALUE
    ndiff = assert_topk_equal_up_to_near_ties(top, el.order_rows(S, 10), Ug, Ig, users, [masks[uid] for uid in users])
    assert ndiff <= nu // 100

    # best model: save, disturb, load
    t._save_best()
    keep = t.model.user_embedding.weight.detach().clone()
    t.model.user_embedding.weight.data.zero_()
    t.load_best_model()
    assert torch.equal(t.model.user_embedding.weight.detach(), keep)

    path = os.path.join(str(tmp_path), "ckpt.pt")
    t.save_checkpoint(path, epoch=2)
    b = MFTrainer(cfg, ni, nu)
    assert b.load_checkpoint(path) == {"epoch": 2}
    for (na, pa), (nb, pb) in zip(t.model.named_parameters(), b.model.named_parameters()):
        assert na == nb and torch.equal(pa, pb)
    sa, sb = t.optimizer.state_dict()["state"], b.optimizer.state_dict()["state"]
    for key in sa:
        assert sa[key]["step"] == sb[key]["step"]
        assert torch.equal(sa[key]["exp_avg"], sb[key]["exp_avg"])
        assert torch.equal(sa[key]["exp_avg_sq"], sb[key]["exp_avg_sq"])
    assert np.array_equal(lists(b)[0], top)
    _, batches = epoch()
    la, lb = t.train(batches), b.train(batches)
    bitwise = all(torch.equal(pa, pb) for pa, pb in zip(t.model.parameters(), b.model.parameters()))
    print(f"continued epoch after the checkpoint: losses {la!r} / {lb!r}, tables bit-equal: {bitwise}")
    assert abs(la - lb) <= 1e-6 * abs(la)
    for pa, pb in zip(t.model.parameters(), b.model.parameters()):
        torch.testing.assert_close(pa, pb, rtol=1e-5, atol=1e-7)
