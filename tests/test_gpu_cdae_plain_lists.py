"""CDAE without negative sampling on list batches (the catalogue sweep of csrc/cdae_catalogue.hip in the step, the
trainer and train.py) against the dense route of the same model: CDAEStep.step_lists against CDAEStep.step,
CDAETrainer.validate / evaluate over list loaders against dense loaders, and the train.py entry point."""
import numpy as np
import pytest
import torch

import cdae_ref64 as R
import cdae_wide_cases as W
from oracle import cdae as ocdae

pytestmark = pytest.mark.gpu


def _n(t):
    return t.detach().cpu().numpy()


def _csr(rs, nu, ni, counts):
    ptr = np.zeros(nu + 1, np.int64)
    ptr[1:] = np.cumsum(counts)
    idx = np.concatenate([np.sort(rs.choice(ni, c, replace=False)) for c in counts] or [np.zeros(0)]).astype(np.int64)
    return ptr, idx


@pytest.mark.parametrize("H", [32, 128])
def test_plain_bce_list_batches_train_like_dense_batches(device, tmp_path, H):
    """Three steps of CDAEStep.step_lists under plain BCE (encoder from the lists, catalogue sweep, hidden backward,
    Adam) against CDAEStep.step on the dense form of the same lists with ``x_in`` given (no dropout draw differs):
    70 users, 2,100 items (more than one column chunk), batches of 32 (the last one short: 6 rows).  Losses and all
    five parameters at rtol 1e-5, atol 1e-7; an element beyond that must be explained by the float64 replay of the
    steps (cdae_wide_cases.replay_steps with every position selected), as in
    test_gpu_cdae_wide.py::test_wide_list_batches_train_like_dense_batches: the hidden backward adds dV, dW_h and db_h
    with float atomics in both routes, and the two routes hand it a dz that differs in its last bits.  The first step
    is also compared against oracle/cdae.py."""
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.cdae_step import CDAEStep
    from yelprecommendation_amd.models.cdae import CDAE
    from yelprecommendation_amd.optim import Adam
    from yelprecommendation_amd.utils import make_config
    rs = np.random.RandomState(21)
    nu, ni, B, lr = 70, 2100, 32, 1e-3
    ptr, idx = _csr(rs, nu, ni, rs.randint(0, 25, nu))
    t = lambda a: torch.from_numpy(a).to(device)
    cfg = make_config("CDAE", hidden_size=H, device="cuda", model_dir=str(tmp_path), lr=lr, negative_sampling=False,
                      loss_name="bce", batch_size=B)
    order = np.random.RandomState(5).permutation(nu).astype(np.int64)
    out, replay, first = {}, [], None
    for form in ("lists", "dense"):
        torch.manual_seed(4)
        model = CDAE(cfg, ni, nu); model.train()
        init = [_n(q).copy() for q in model.parameters()]
        step = CDAEStep(model, Adam(model.parameters(), lr=lr), negative_sampling=False, transposed_wh=True)
        assert step.decoder == "dense" and step.catalogue and step.transposed_wh
        losses = []
        for k in range(3):
            users = t(order[k * B:(k + 1) * B].copy())
            assert users.numel() == (B if k < 2 else nu - 2 * B)
            L = engine.TrainLists(t(ptr), t(idx), users, nu, ni, 0, 100 + k, 200 + k, model.corruption_level,
                                  targets=(t(ptr), t(idx)))
            if form == "lists":
                step.step_lists(users, L)
            else:
                x, neg = L.loss_dense()
                assert int(neg.sum().item()) == 0
                x_in = L.rows.to_dense()                   # the encoder's input of the lists: dropout already applied
                replay.append((_n(users), _n(x_in), _n(x), 1.0 - _n(x)))
                step.step(users, x, None, x_in=x_in)
            losses.append(float(step.last_loss()))
            if k == 0 and form == "lists":
                step.release()
                first = [_n(q).copy() for q in model.parameters()]
        step.release()
        step.check()
        out[form] = (losses, [q.detach().clone() for q in model.parameters()])
    print(f"H={H} losses lists {out['lists'][0]} dense {out['dense'][0]}")
    np.testing.assert_allclose(out["lists"][0], out["dense"][0], rtol=1e-5, atol=1e-7)
    # the first step against the oracle: plain BCE is NS-BCE with every position selected
    ref = ocdae.CDAEState(init, lr=lr, hidden_act="sigmoid" if model._hidden_act == 1 else "identity",
                          output_act="sigmoid" if model._output_act == 1 else "identity")
    u0, xin0, x0, _ = replay[0]
    want = float(ref.train_step(u0, xin0, x0, np.ones_like(x0)))
    np.testing.assert_allclose(out["lists"][0][0], want, rtol=1e-5)
    for p, r in zip(first, ref.params):
        np.testing.assert_allclose(p, r, rtol=1e-3, atol=2e-6)
    # the three steps, lists against dense
    beyond = [(j, ~torch.isclose(a, b, rtol=1e-5, atol=1e-7)) for j, (a, b) in enumerate(zip(out["lists"][1], out["dense"][1]))]
    print("elements beyond rtol 1e-5, atol 1e-7:", [int(m.sum()) for _, m in beyond])
    if not any(int(m.sum()) for _, m in beyond):
        return
    exact, allow = W.replay_steps(init, replay, model._hidden_act, model._output_act, nu, lr)
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


def test_other_widths_refuse_list_batches_under_plain_bce(device, tmp_path):
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.cdae_step import CDAEStep
    from yelprecommendation_amd.models.cdae import CDAE
    from yelprecommendation_amd.optim import Adam
    from yelprecommendation_amd.utils import make_config
    nu, ni = 8, 40
    cfg = make_config("CDAE", hidden_size=256, device="cuda", model_dir=str(tmp_path), lr=1e-3, negative_sampling=False,
                      loss_name="bce")
    model = CDAE(cfg, ni, nu)
    step = CDAEStep(model, Adam(model.parameters(), lr=1e-3), negative_sampling=False)
    ptr = torch.arange(nu + 1, dtype=torch.int64, device=device)
    idx = torch.arange(nu, dtype=torch.int64, device=device)
    users = torch.arange(nu, dtype=torch.int64, device=device)
    L = engine.TrainLists(ptr, idx, users, nu, ni, 0, 1, 2, 0.0, targets=(ptr, idx))
    with pytest.raises(NotImplementedError):
        step.step_lists(users, L)


def _store(rs, nu, ni, device):
    from yelprecommendation_amd.data.cdae_batches import CDAEInteractions
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
    return CDAEInteractions(nu, ni, parts, device)


@pytest.mark.parametrize("group", [32, 1])
def test_plain_bce_list_route_of_validate_and_evaluate_equals_dense_route(device, tmp_path, group):
    """CDAETrainer.validate / evaluate over CDAEBatchLoader(lists=True, negative_sampling=False) — the encoder per
    group of batches, ONE loss-only catalogue sweep over all users, the fused top-k — against the same methods over
    the dense loader of the same store (a [B, I] prediction, the BCE module and a masked top-k per batch): the loss
    within 1e-5 relative, the four metrics equal.  300 users in batches of 64 (a short last batch), shuffled, so the
    per-batch means are taken in the loader's order; ``group`` 1 is the per-batch loop."""
    from yelprecommendation_amd.data.cdae_batches import CDAEBatchLoader
    from yelprecommendation_amd.trainers import CDAETrainer
    from yelprecommendation_amd.utils import make_config
    nu, ni, H, B = 300, 2100, 64, 64
    data = _store(np.random.RandomState(3), nu, ni, device)
    cfg = make_config("CDAE", hidden_size=H, device="cuda", model_dir=str(tmp_path), lr=1e-2, negative_sampling=False,
                      loss_name="bce", batch_size=B, top_n=10, eval_batch_group=group)
    torch.manual_seed(11)
    trainer = CDAETrainer(cfg, ni, nu)
    train_loader = CDAEBatchLoader(data, "train", batch_size=B, shuffle=True, seed=1, lists=True,
                                   dropout=trainer.model.corruption_level, negative_sampling=False)
    first = trainer.train(train_loader)                      # a few steps off the init, through step_lists
    step = trainer._fused_step()
    assert step.decoder == "dense" and step.catalogue and np.isfinite(first)
    mk = lambda mode, lists: CDAEBatchLoader(data, mode, batch_size=B, shuffle=mode == "valid", seed=7, lists=lists,
                                             negative_sampling=False)
    got, want = trainer.validate(mk("valid", True)), trainer.validate(mk("valid", False))
    print("validate lists", got, "dense", want)
    np.testing.assert_allclose(got[0], want[0], rtol=1e-5)
    np.testing.assert_allclose(got[1:], want[1:], rtol=0, atol=1e-12)
    got, want = trainer.evaluate(mk("test", True)), trainer.evaluate(mk("test", False))
    print("evaluate lists", got, "dense", want)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_list_batches_of_plain_bce_carry_their_targets_and_no_negatives(device):
    from yelprecommendation_amd.data.cdae_batches import CDAEBatchLoader
    data = _store(np.random.RandomState(9), 40, 300, device)
    for mode, part in (("train", "train"), ("valid", "train_valid")):
        for batch in CDAEBatchLoader(data, mode, batch_size=16, lists=True, negative_sampling=False):
            L = batch["lists"]
            assert L.targets is not None and all(torch.equal(a, b) for a, b in zip(L.targets, data.csr(part)))
            target, neg = L.loss_dense()
            assert int(neg.sum().item()) == 0
    for batch in CDAEBatchLoader(data, "test", batch_size=16, lists=True, negative_sampling=False):
        assert batch["lists"].targets is None
    for batch in CDAEBatchLoader(data, "train", batch_size=16, lists=True):     # the default: NS-BCE lists as before
        assert batch["lists"].targets is None and int(batch["lists"].loss_dense()[1].sum().item()) > 0
    grouped = list(CDAEBatchLoader(data, "valid", batch_size=16, lists=True, negative_sampling=False).super_batches(2))
    assert [g["user_id"].numel() for g in grouped] == [32, 8] and all(g["lists"].targets is not None for g in grouped)


def test_train_entry_point_under_plain_bce(device, tmp_path, monkeypatch):
    """train.build + train.run with fast_loader=true negative_sampling=false: the three loaders are list loaders that
    draw no negatives, the step takes the catalogue sweep, and the training loss falls from the first epoch to the
    second (corruption_level 0: no dropout draw between the epochs' losses)."""
    from yelprecommendation_amd import train
    from yelprecommendation_amd.data import cdae_batches
    from yelprecommendation_amd.trainers import cdae_trainer
    from yelprecommendation_amd.utils import make_config
    made, losses = [], []

    class Recorded(cdae_batches.CDAEBatchLoader):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    plain_train = cdae_trainer.CDAETrainer.train

    def recorded_train(self, loader):
        losses.append(plain_train(self, loader))
        return losses[-1]

    monkeypatch.setattr(cdae_batches, "CDAEBatchLoader", Recorded)
    monkeypatch.setattr(cdae_trainer.CDAETrainer, "train", recorded_train)
    cfg = make_config("CDAE", synthetic="300x900x14", fast_loader=True, epochs=2, batch_size=64, hidden_size=64,
                      device="cuda", model_dir=str(tmp_path), lr=0.01, loss_name="bce", negative_sampling=False,
                      corruption_level=0)
    trainer, metrics = train.run(cfg, train.build(cfg))
    assert len(made) == 3 and all(ld.lists and not ld.negative_sampling for ld in made)
    step = trainer._fused_step()
    assert step.decoder == "dense" and step.catalogue and step.transposed_wh
    assert len(losses) == 2 and np.isfinite(losses).all() and losses[1] < losses[0], losses
    assert len(metrics) == 4 and all(np.isfinite(m) and 0.0 <= m <= 1.0 for m in metrics)
