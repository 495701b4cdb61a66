"""CDAE on list batches at the hidden sizes 512 and 1,024: the wave-per-position sampled decoder (with gradients and loss
only), the encoder and the fused hidden backward at those widths, row marks on 512- and 1,024-wide rows in
adam_dense_flat — each entry point called directly and compared with the float64 reference of tests/cdae_ref64.py at
its bars (tests/test_cdae_wide_host.py shows that those bars notice a lost list entry and, on the probe inputs, a hidden
unit lost from the decoder's dot product) — then CDAEStep, CDAETrainer and train.py at those widths.  Every kernel case
prints max |err| / bar per output."""
import numpy as np
import pytest
import torch

import cdae_ref64 as R
import cdae_wide_cases as W
from test_gpu_cdae_long_rows import _count_value, _counts, _decode, _decode_ratios, _n, _report, _spread, _t

pytestmark = pytest.mark.gpu


# ---- a. sampled decoder with gradients ------------------------------------------------------------------------------

def _decoder_with_gradients(device, c, B, I, H, act, what):
    from yelprecommendation_amd import engine
    _, splits, dz, dWo, dbo, partials, count = _decode(engine, device, c, B, H, I, act)
    assert splits == W.splits_of(B)
    ref = R.sampled_decode(c["z"], c["Wo"], c["bo"], c["target"], c["negmask"], act, splits=splits)
    _report(f"{what} B={B} splits={splits} I={I} H={H} act={act} bo={c['bo'] is not None}",
            _decode_ratios(engine, ref, B, splits, dz, dWo, dbo, partials, count))
    if splits == 1:
        again = _decode(engine, device, c, B, H, I, act, dz_fill=7.5)
        assert torch.equal(again[2], dz)


@pytest.mark.parametrize("B,I,H,act,with_bo,long", W.DECODE_CASES)
def test_wide_decoder_every_split_count_and_long_rows(device, B, I, H, act, with_bo, long):
    """cdae_sampled_decode_kernel<64, 8 | 16, true, false> (H = 512 | 1,024): splits 8, 7, 2, 1 on short rows and
    8, 8, 3, 1 on the long rows (0 ... 6,001 positions, three staging passes); dz, dW_o, db_o, every loss partial,
    their sum and the spread count.  splits = 1 stores dz: a sentinel in dz on entry changes nothing."""
    _decoder_with_gradients(device, R.decode_case(B, I, H, act, with_bo, long), B, I, H, act, "wide decoder")


@pytest.mark.parametrize("B,I,H,act,with_bo,long", W.PROBE_DECODE_CASES)
def test_wide_decoder_on_the_probe_units(device, B, I, H, act, with_bo, long):
    """The inputs on which a hidden unit lost from z . W_o[i] — a register slot, lane 0 or lane 63 of the wave's row
    layout — crosses a bar (test_cdae_wide_host.py)."""
    _decoder_with_gradients(device, W.probe_decode_case(B, I, H, act, with_bo, long), B, I, H, act, "probe units")


# ---- b. sampled decoder, loss only ----------------------------------------------------------------------------------

def _loss_only(device, c, B, I, H, act, what):
    from yelprecommendation_amd import engine
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
    rows_per = 7                                       # batched: workgroup q owns rows [7 q, 7 q + 7)
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
    _report(f"{what} B={B} splits={splits} I={I} H={H} act={act}", ratios)


@pytest.mark.parametrize("B,I,H,act", W.LOSS_ONLY_CASES)
def test_wide_loss_only_decoder_and_the_loss_finalizers(device, B, I, H, act):
    """dz = dWo = dbo = None: cdae_sampled_decode_kernel<64, ., true, true> at 8 splits on the long rows (up to 188
    positions per wave and pass: the 64-slot settle() hand-off is passed twice and ends in a partial round) and on
    rows of 31 ... 65 positions (one or two positions per wave, or none); then cdae_loss_finalize and
    cdae_loss_finalize_batched on its partials."""
    _loss_only(device, R.decode_case(B, I, H, act, True, True, settle=True), B, I, H, act, "wide loss only")


@pytest.mark.parametrize("B,I,H,act", W.PROBE_LOSS_ONLY_CASES)
def test_wide_loss_only_decoder_on_the_probe_units(device, B, I, H, act):
    _loss_only(device, W.probe_decode_case(B, I, H, act, True, True, settle=True), B, I, H, act, "probe units, loss only")


# ---- c. encoder -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("I,H,act,transposed,p", W.ENCODER_CASES)
def test_encoder_at_the_wide_widths(device, I, H, act, transposed, p):
    """cdae_sparse_encode_kernel<false / true> with two and four rounds of its loop over H, on the long rows."""
    from yelprecommendation_amd import engine
    c = R.encoder_case(I, H, act, transposed, p)
    x = _t(c["x"], device)
    rows = engine.SparseRows(x, c["seed"], p)
    assert torch.equal(rows.to_dense(), x)
    Wh, bh, V = R.encoder_params(c["rs"], H, I, R.ENCODER_USERS, c["x"])
    flag = engine.new_error_flag(device)
    z = engine.cdae_sparse_encode(rows, _t(Wh.T if transposed else Wh, device), _t(bh, device), _t(V, device),
                                  _t(c["user"], device), act, err_flag=flag, transposed=transposed)
    assert int(flag.item()) == engine.FLAG_BAD_USER
    _report(f"encoder I={I} H={H} act={act} transposed={transposed}",
            {"z": R.ratio(_n(z), R.encode(Wh, bh, V, c["user"], c["x"], act))})


# ---- d. the fused hidden backward -----------------------------------------------------------------------------------

@pytest.mark.parametrize("H,act,scale_dz", W.DWH_CASES)
def test_hidden_bwd_dwh_t_at_the_wide_widths(device, H, act, scale_dz):
    """cdae_hidden_bwd_dwh_t_kernel<2> at H = 512 and <4> at H = 1,024 on rows of up to three staging passes, both
    batches: dW_h^T, db_h, dV (no row and no mark for the out-of-range user), the item marks exactly the listed
    columns, the step's loss from the partials; dz is read only."""
    from yelprecommendation_amd import engine
    f32 = torch.float32
    I, nu, cnt = R.I_LONG, R.HIDDEN_USERS, 37
    worst = {}
    for batch in (0, 1):
        c = R.dwh_case(H, batch)
        rows = engine.SparseRows(_t(c["x"], device))
        dz, z, user = _t(c["dz"], device), _t(c["z"], device), _t(c["user"], device)
        ref = R.hidden_bwd(c["dz"], c["z"], act, c["user"], cnt if scale_dz else None, c["x"], nu)
        assert (c["user"] >= nu).any()
        dWhT = torch.zeros(I, H, dtype=f32, device=device)
        items = torch.zeros(I, dtype=torch.uint8, device=device)
        dV, dbh = torch.zeros(nu, H, dtype=f32, device=device), torch.zeros(H, dtype=f32, device=device)
        marks = torch.zeros(nu, dtype=torch.uint8, device=device)
        stats = torch.zeros(2, dtype=f32, device=device)
        accum = torch.full((1,), 2.5, dtype=torch.float64, device=device)
        partials = _t(np.random.RandomState(H + batch).rand(R.N_LONG * 8).astype(np.float32), device)
        engine.cdae_hidden_bwd_dwh_t(rows, dz, z, act, user, _spread(device, engine, cnt), dV, marks, dbh, dWhT, items,
                                     partials, partials.numel(), stats, accum, scale_dz=scale_dz)
        p64 = _n(partials).astype(np.float64)
        mean = R.Out(p64.sum() / cnt, p64.size + 1, np.abs(p64).sum() / cnt)
        assert np.array_equal(_n(marks), ref["user_marks"]) and float(stats[1]) == cnt
        assert np.array_equal(_n(items), ref["item_marks"])
        assert torch.equal(dz, _t(c["dz"], device))
        got = dict(dbh=R.ratio(_n(dbh), ref["dbh"]), dV=R.ratio(_n(dV), ref["dV"]),
                   dWhT=R.ratio(_n(dWhT).T, ref["dWh"]), loss=R.ratio(float(stats[0]), mean, R.loss_bar),
                   accum=R.ratio(float(accum.item()) - 2.5, mean, R.loss_bar))
        for k, v in got.items():
            worst[k] = max(worst.get(k, 0.0), v)
    _report(f"hidden_bwd_dwh_t H={H} act={act} scale_dz={scale_dz}", worst)


# ---- e. row marks on 512- and 1,024-wide rows -----------------------------------------------------------------------

SENTINEL = 12345.0


def _marked_launch(device, shapes, marked_rows, decoupled, wd, with_count):
    """One adam_dense_flat launch over ``shapes`` ((rows, width) marked on marked_rows[k], or a plain shape with
    marked_rows[k] None) against single unmarked yr_adam_dense launches fed what the marks stand for."""
    from yelprecommendation_amd import engine
    rs = np.random.RandomState(sum(int(np.prod(s)) for s in shapes) + int(decoupled) + 2 * int(with_count))
    mk = lambda s, scale=1.0: torch.from_numpy((rs.standard_normal(s) * scale).astype(np.float32)).to(device)
    P, G = [mk(s) for s in shapes], [mk(s, 0.1) for s in shapes]
    M, V = [mk(s, 0.01) for s in shapes], [mk(s, 0.01).abs() for s in shapes]
    count = _spread(device, engine, 37) if with_count else None
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(37.0, dtype=torch.float32)      # f32 division, as the kernel's
    marks, tensors, want = [], [], []
    for k, s in enumerate(shapes):
        rows_k = marked_rows[k]
        scaled = with_count and k % 2 == 0
        p, m, v = P[k].clone(), M[k].clone(), V[k].clone()
        if rows_k is None:
            mark = None
            gd = G[k].clone()
        else:
            mark = torch.zeros(s[0], dtype=torch.uint8, device=device)
            idx = torch.from_numpy(np.asarray(rows_k, np.int64)).to(device)
            mark[idx] = 1
            gd = torch.zeros_like(G[k]); gd[idx] = G[k][idx]
            keep = torch.ones(s[0], dtype=torch.bool, device=device); keep[idx] = False
            G[k][keep] = SENTINEL                                       # never read, never cleared
        if scaled:
            gd = gd * inv.to(device)
        engine.adam_dense(p.reshape(-1), gd.reshape(-1), m.reshape(-1), v.reshape(-1), 3, 1e-2, 0.9, 0.999, 1e-8, wd,
                          decoupled=decoupled)
        want.append((p, m, v))
        marks.append(mark)
        tensors.append((P[k], G[k], M[k], V[k], mark, 0, scaled))
    engine.adam_dense_flat(tensors, 3, 1e-2, 0.9, 0.999, 1e-8, wd, decoupled=decoupled, grad_count=count)
    for k, ((p, m, v), s) in enumerate(zip(want, shapes)):
        assert torch.equal(p, P[k]) and torch.equal(m, M[k]) and torch.equal(v, V[k]), (k, s)
        if marks[k] is not None:
            assert int(marks[k].sum()) == 0, (k, s)
            idx = torch.from_numpy(np.asarray(marked_rows[k], np.int64)).to(device)
            keep = torch.ones(s[0], dtype=torch.bool, device=device); keep[idx] = False
            assert float(G[k][idx].abs().sum()) == 0.0 and bool((G[k][keep] == SENTINEL).all()), (k, s)


@pytest.mark.parametrize("decoupled,wd", [(False, 0.0), (True, 0.01)])
@pytest.mark.parametrize("with_count", [False, True])
def test_wide_row_marks_in_adam_dense_flat(device, decoupled, wd, with_count):
    """adam_flat_kernel<., true>: marked tensors of 1, 3 and 5 rows of 1,024 floats and of 1, 4 and 9 rows of 512 (an odd
    count leaves half a chunk), a marked 64-wide tensor and an unmarked one with n % 4 != 0 in ONE launch, marks on a
    subset of the rows, a sentinel gradient in the unmarked rows: parameters and both moments bit-identical to single
    unmarked launches fed the gradient with the unmarked rows zeroed, sentinels untouched, marked gradient rows and all
    marks cleared; Adam and AdamW, with and without the 1 / count scaling.  Then 4,099 rows of 512 with every second
    row marked: many chunks in flight."""
    shapes = [(1, 1024), (3, 1024), (5, 1024), (1, 512), (4, 512), (9, 512), (37, 64), (7, 13)]
    rows = [[0], [0, 2], [1, 2, 4], [0], [1, 2], [0, 3, 4, 8], list(range(0, 37, 3)), None]
    _marked_launch(device, shapes, rows, decoupled, wd, with_count)
    _marked_launch(device, [(2, 1024), (3, 512)], [[], [1]], decoupled, wd, with_count)       # a tensor with no mark set
    _marked_launch(device, [(4099, 512), (5,)], [list(range(0, 4099, 2)), None], decoupled, wd, with_count)


# ---- f. the whole step ----------------------------------------------------------------------------------------------

def _close(a, b, what):
    torch.testing.assert_close(a, b, rtol=2e-4, atol=1e-7 + 2e-5 * float(b.abs().max()), msg=lambda m: f"{what}: {m}")


@pytest.mark.parametrize("ni,H", [(1001, 512), (1501, 1024)])
def test_wide_step_equals_float64_chain_and_autograd_route(device, tmp_path, ni, H):
    """CDAEStep at H = 512 / 1,024 — decoder="auto" is the sampled one, the transposed working copy of W_h with item
    marks is on, released and re-acquired mid-run — over four steps against the autograd route (model + loss module +
    optimizer.step) from the same init with the same dropout seeds: losses at 1e-5 relative, all parameters and both
    Adam moments at rtol 2e-4, atol 1e-7 + 2e-5 max |b|.  The first step also against the float64 chain
    encode -> sampled_decode -> hidden_bwd of cdae_ref64 at its bars: the loss, and every gradient read back from the
    first moment (exp_avg = (1 - beta1) g after one step)."""
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.cdae_step import CDAEStep
    from yelprecommendation_amd.loss import NSBCELoss
    from yelprecommendation_amd.models.cdae import CDAE
    from yelprecommendation_amd.optim import Adam
    from yelprecommendation_amd.utils import make_config
    rs = np.random.RandomState(ni + H)
    nu, B, steps = 90, 40, 4
    t = lambda a: torch.from_numpy(a).to(device)
    batches = []
    for _ in range(steps):
        u = rs.randint(0, nu, B).astype(np.int64); u[7] = u[2]
        x = (rs.rand(B, ni) < 0.02).astype(np.float32); x[3] = 0.0
        neg = ((rs.rand(B, ni) < 0.1) * (1 - x)).astype(np.float32)
        batches.append((u, x, neg, int(rs.randint(1, 1 << 40))))
    drop = lambda x, seed, p: engine.dropout_seeded(x, seed, p) if p > 0 else x
    out, first = {}, None
    for fused in (False, True):
        torch.manual_seed(3)
        model = CDAE(make_config("CDAE", hidden_size=H, device="cuda", model_dir=str(tmp_path), lr=1e-3), ni, nu)
        model.train()
        params = list(model.parameters())
        opt = Adam(params, lr=1e-3)
        init = [_n(q).copy() for q in params]
        losses = []
        if fused:
            step = CDAEStep(model, opt, True, transposed_wh=True)
            assert step.decoder == "sampled" and step.transposed_wh and step.row_marks
            for k, (u, x, neg, seed) in enumerate(batches):
                step.step(t(u), t(x), t(neg), seed=seed, p=model.corruption_level)
                losses.append(float(step.last_loss()))
                assert step._wht is not None
                clean = [step.dV, step.dbh, step.touched_users, step.dWo, step.dbo, step._wht[3], step._wht[4]]
                assert all(float(g.float().abs().sum()) == 0.0 for g in clean)
                if k == 0:
                    step.release()
                    first = (losses[0], [opt.state[q]["exp_avg"].clone() for q in params], init,
                             _n(drop(t(x), seed, model.corruption_level)), model._hidden_act, model._output_act)
                if k == 1:
                    step.release()                              # back to the module mid-run, re-acquired by the next step
            step.release()
            assert abs(step.epoch_loss() - sum(losses)) < 1e-5
            step.check()
        else:
            lossf = NSBCELoss()
            for u, x, neg, seed in batches:
                pred = model.encode_decode(t(u), drop(t(x), seed, model.corruption_level))
                loss = lossf(pred, t(x), t(neg))
                opt.zero_grad(); loss.backward(); opt.step()
                losses.append(float(loss.detach()))
        out[fused] = (losses, [q.detach().clone() for q in params], [opt.state[q]["exp_avg"].clone() for q in params],
                      [opt.state[q]["exp_avg_sq"].clone() for q in params])
    # the first step against the float64 chain
    loss0, m0, (Wh, bh, V, Wo, bo), xin, hact, oact = first
    u, x, neg, _ = batches[0]
    z = R.encode(Wh, bh, V, u, xin, hact)
    dec = R.sampled_decode(z.v, Wo, bo, x, neg, oact)
    cnt = dec["count"]
    hid = R.hidden_bwd(dec["dz"].v, z.v, hact, u, cnt, xin, nu)
    tenth = lambda o, div=1.0: R.Out(0.1 * o.v / div, o.n + 1, 0.1 * o.s / div)
    ratios = {"loss": R.ratio(loss0, R.Out(dec["loss"].v / cnt, dec["loss"].n + B, dec["loss"].s / cnt), R.loss_bar),
              "dWh": R.ratio(_n(m0[0]), tenth(hid["dWh"])), "dbh": R.ratio(_n(m0[1]), tenth(hid["dbh"])),
              "dV": R.ratio(_n(m0[2]), tenth(hid["dV"])), "dWo": R.ratio(_n(m0[3]), tenth(dec["dWo"], cnt)),
              "dbo": R.ratio(_n(m0[4]), tenth(dec["dbo"], cnt))}
    _report(f"first step ni={ni} H={H} against the float64 chain (gradients from exp_avg)", ratios)
    rel = max(abs(a - b) / abs(b) for a, b in zip(out[True][0], out[False][0]))
    print(f"four steps ni={ni} H={H}: largest relative loss difference to the autograd route {rel:.2e}")
    np.testing.assert_allclose(out[True][0], out[False][0], rtol=1e-5)
    for k, name in ((1, "parameter"), (2, "exp_avg"), (3, "exp_avg_sq")):
        for j, (a, b) in enumerate(zip(out[True][k], out[False][k])):
            _close(a, b, f"{name} {j}")


def test_wide_list_batches_train_like_dense_batches(device, tmp_path):
    """CDAEStep.step_lists on engine.TrainLists against CDAEStep.step on the dense row / negative mask the lists stand
    for (same dropout seed) at H = 512, as test_gpu_cdae.py::test_list_batches_train_like_dense_batches does at H = 64:
    losses at 1e-6 relative, all parameters over three steps at rtol 1e-5, atol 1e-7.
    Both routes run the same kernels on the same lists; what differs — as between two runs of one route — is the
    order in which the float atomics of dW_o, dz, dW_h and dV arrive, and Adam's step lr m / (sqrt(v) + eps) turns a
    gradient's RELATIVE error into a parameter difference of up to lr times it, which cancellation inside a gradient
    sum (positives pull a row of W_o down, negatives push it up) leaves unbounded by any fixed tolerance.  An element
    beyond rtol 1e-5, atol 1e-7 must therefore be explained by the float64 replay of the three steps
    (cdae_wide_cases.replay_steps): each route may end `allowance` from the replay, where the allowance is Adam run
    again in float64 with each step's gradient moved by its f32 bound 2 (n + 1) 2^-24 sum |terms|; the element passes
    only if both routes are within 2 x allowance of the replay (2: the later steps' gradients are taken at parameters
    that already differ), i.e. both are as far from the exact steps as f32 sums allow and no further.  Every such
    element is printed with its figures.  Measured over three runs: none, none, and 1 element of 769,536 of W_o with
    |lists - dense| = 1.12e-7 (1.0e-4 relative)."""
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.cdae_step import CDAEStep
    from yelprecommendation_amd.models.cdae import CDAE
    from yelprecommendation_amd.optim import Adam
    from yelprecommendation_amd.utils import make_config
    rs = np.random.RandomState(12)
    nu, ni, H, B, lr = 120, 1503, 512, 32, 1e-3
    counts = rs.randint(0, 25, nu)
    ptr = np.zeros(nu + 1, np.int64); ptr[1:] = np.cumsum(counts)
    idx = np.concatenate([np.sort(rs.choice(ni, c, replace=False)) for c in counts]).astype(np.int64)
    t = lambda a: torch.from_numpy(a).to(device)
    cfg = make_config("CDAE", hidden_size=H, device="cuda", model_dir=str(tmp_path), lr=lr, negative_sampling=True,
                      neg_times=3, loss_name="bce", batch_size=B)
    out, replay = {}, []
    for form in ("lists", "dense"):
        torch.manual_seed(4)
        model = CDAE(cfg, ni, nu); model.train()
        init = [_n(q).copy() for q in model.parameters()]
        step = CDAEStep(model, Adam(model.parameters(), lr=lr), transposed_wh=True)
        assert step.decoder == "sampled" and step.transposed_wh
        losses = []
        for k in range(3):
            users = t(np.random.RandomState(k).permutation(nu)[:B].astype(np.int64))
            L = engine.TrainLists(t(ptr), t(idx), users, nu, ni, 3, 100 + k, 200 + k, model.corruption_level)
            if form == "lists":
                step.step_lists(users, L)
            else:
                x, neg = L.loss_dense()
                p = model.corruption_level
                replay.append((_n(users), _n(engine.dropout_seeded(x, 200 + k, p) if p > 0 else x), _n(x), _n(neg)))
                step.step(users, x, neg, seed=200 + k, p=p)
            losses.append(float(step.last_loss()))
        step.release()
        step.check()
        out[form] = (losses, [q.detach().clone() for q in model.parameters()])
    np.testing.assert_allclose(out["lists"][0], out["dense"][0], rtol=1e-6)
    beyond = [(j, ~torch.isclose(a, b, rtol=1e-5, atol=1e-7)) for j, (a, b) in enumerate(zip(out["lists"][1], out["dense"][1]))]
    print("elements beyond rtol 1e-5, atol 1e-7:", [int(m.sum()) for _, m in beyond])
    exact, allow = W.replay_steps(init, replay, model._hidden_act, model._output_act, nu, lr)
    for form in ("lists", "dense"):                    # printed for every run: both routes against the replay
        far = [float((np.abs(_n(q).astype(np.float64) - exact[j]) / (2.0 * allow[j] + 1e-5 * np.abs(exact[j]) + 1e-7)).max())
               for j, q in enumerate(out[form][1])]
        print(f"{form}: max |route - float64 replay| / (2 x allowance + rtol 1e-5, atol 1e-7) per parameter", [f"{v:.3g}" for v in far])
    unexplained = []
    for j, mask in beyond:
        a, b, m = _n(out["lists"][1][j]).astype(np.float64), _n(out["dense"][1][j]).astype(np.float64), _n(mask)
        for e in zip(*np.nonzero(m)):
            ea, eb, al = abs(a[e] - exact[j][e]), abs(b[e] - exact[j][e]), allow[j][e]
            print(f"parameter {j} element {e}: lists {a[e]:.9g} dense {b[e]:.9g} float64 replay {exact[j][e]:.9g}; "
                  f"|lists - replay| {ea:.3g} |dense - replay| {eb:.3g} allowance {al:.3g}")
            if not (ea <= 2.0 * al and eb <= 2.0 * al):
                unexplained.append((j, e, ea, eb, al))
    assert not unexplained, unexplained


# ---- g. trainer and train.py ----------------------------------------------------------------------------------------

def test_wide_list_route_of_validate_and_evaluate_equals_dense_route(device, tmp_path):
    """CDAETrainer.validate / evaluate over list batches at H = 512 (encoder over two rounds of H, loss-only wide
    decoder, yr_mf_eval_topk_bias at D = 512 with the decoder bias) against the dense per-batch route: loss at 1e-5
    relative, the four metrics at 1e-3, the top-10 lists row by row up to float near-ties."""
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.data.cdae_batches import CDAEBatchLoader, CDAEInteractions
    from yelprecommendation_amd.trainers import CDAETrainer
    from yelprecommendation_amd.utils import make_config
    from replay import assert_topk_equal_up_to_near_ties
    rs = np.random.RandomState(3)
    nu, ni, H, B = 300, 1503, 512, 64
    parts = {}
    taken = np.zeros((nu, ni), bool)
    for name, hi in (("train", 30), ("valid", 8), ("test", 8)):
        counts = rs.randint(0, hi, nu)
        ptr = np.zeros(nu + 1, np.int64); ptr[1:] = np.cumsum(counts)
        idx = []
        for u_, c in enumerate(counts):
            pick = np.sort(rs.choice(np.flatnonzero(~taken[u_]), c, replace=False))
            taken[u_, pick] = True
            idx.append(pick)
        parts[name] = (torch.from_numpy(ptr), torch.from_numpy(np.concatenate(idx).astype(np.int64)))
    data = CDAEInteractions(nu, ni, parts, device)
    cfg = make_config("CDAE", hidden_size=H, device="cuda", model_dir=str(tmp_path), lr=1e-2, negative_sampling=True,
                      neg_times=3, loss_name="bce", batch_size=B, top_n=10)
    trainer = CDAETrainer(cfg, ni, nu)
    trainer.train(CDAEBatchLoader(data, "train", batch_size=B, neg_times=3, shuffle=True, seed=1, lists=True,
                                  dropout=trainer.model.corruption_level))          # a few steps off the init
    assert trainer._fused_step().decoder == "sampled" and trainer._fused_step().transposed_wh
    for mode in ("valid", "test"):
        as_lists = CDAEBatchLoader(data, mode, batch_size=B, neg_times=3, seed=7, lists=True)
        dense = []
        for batch in CDAEBatchLoader(data, mode, batch_size=B, neg_times=3, seed=7, lists=True):
            users = batch["user_id"]
            d = {"user_id": users, "item_lists": batch["item_lists"]}
            if mode == "valid":
                target, neg = batch["lists"].loss_dense()
                d.update(input_mask=data.dense("train", users), valid_mask=data.dense("valid", users), negative_mask=neg.clone())
                assert torch.equal(target, d["input_mask"] + d["valid_mask"])
            else:
                d.update(input_mask=data.dense("train_valid", users), test_mask=data.dense("test", users))
            dense.append(d)
        if mode == "valid":
            got, want = trainer.validate(as_lists), trainer.validate(dense)
            print("validate lists", got, "dense", want)
            np.testing.assert_allclose(got[0], want[0], rtol=1e-5)
            np.testing.assert_allclose(got[1:], want[1:], atol=1e-3, rtol=0)
        else:
            got, want = trainer.evaluate(as_lists), trainer.evaluate(dense)
            print("evaluate lists", got, "dense", want)
            np.testing.assert_allclose(got, want, atol=1e-3, rtol=0)
    model = trainer.model.eval()
    users = torch.arange(nu, device=device)
    x = data.dense("train_valid", users)
    with torch.no_grad():
        pred = model(users, x)
        z = engine.cdae_sparse_encode(engine.SparseRows(x), *(q.data for q in model._params()[:3]), users, model._hidden_act)
    sp, si = data.csr("train_valid")
    top_dense = engine.topk_masked(pred.contiguous(), sp, si, 10, mask_value=0.0)
    top_fused = engine.mf_eval_topk(z, model.output_layer.weight.data, users, sp, si, 10,
                                    item_bias=model.output_layer.bias.data)
    Ua = np.c_[_n(z), np.ones(nu, np.float32)]
    Ia = np.c_[_n(model.output_layer.weight.data), _n(model.output_layer.bias.data)]
    spn, sin = _n(sp), _n(si)
    masked = [sin[spn[r]:spn[r + 1]] for r in range(nu)]
    assert_topk_equal_up_to_near_ties(_n(top_fused), _n(top_dense), Ua, Ia, np.arange(nu), masked=masked)


def test_train_entry_point_at_hidden_size_1024(device, tmp_path, monkeypatch):
    """train.build + train.run with fast_loader=true hidden_size=1024: all three loaders are list loaders, the step
    uses the sampled decoder, the metrics are finite and in [0, 1]."""
    from yelprecommendation_amd import train
    from yelprecommendation_amd.data import cdae_batches
    from yelprecommendation_amd.utils import make_config
    made = []

    class Recorded(cdae_batches.CDAEBatchLoader):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(cdae_batches, "CDAEBatchLoader", Recorded)
    cfg = make_config("CDAE", synthetic="300x900x14", fast_loader=True, epochs=2, batch_size=64, hidden_size=1024,
                      device="cuda", model_dir=str(tmp_path), lr=0.01, loss_name="bce")
    trainer, metrics = train.run(cfg, train.build(cfg))
    assert len(made) == 3 and all(getattr(ld, "lists", False) for ld in made)
    step = trainer._fused_step()
    assert step.decoder == "sampled" and step.transposed_wh and step.row_marks
    assert len(metrics) == 4 and all(np.isfinite(m) and 0.0 <= m <= 1.0 for m in metrics)
