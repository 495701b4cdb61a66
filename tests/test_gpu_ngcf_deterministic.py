"""deterministic=True for NGCF: NGCFStep (yr_ngcf_bpr_step_ordered), NGCFTrainer and the train.py entry point give the
same bits twice, stay as close to the default mode as the fused step is to the autograd route (the criteria of
test_gpu_ngcf.py::test_fused_step_equals_autograd_route: both pairs differ by summation order only), do not depend on
what their workspace held, and refuse what the mode does not cover."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

NU, NI = 2300, 1900
LR = 2e-3


def _random_graph(rs, nu, ni, deg, hot_items=0):
    u = np.repeat(np.arange(nu), deg)
    i = rs.randint(0, ni, size=u.shape[0])
    if hot_items:
        hot = rs.rand(i.shape[0]) < 0.3
        i[hot] = rs.randint(0, hot_items, size=int(hot.sum()))
    r = rs.randint(1, 6, size=u.shape[0])
    return u, i, r


_GRAPHS = {}


def _setup(device, batch):
    """The graph (2,300 x 1,900, five hot items) and the six batches of test_fused_step_equals_autograd_route."""
    from yelprecommendation_amd.graph import LaplacianCSR
    if batch not in _GRAPHS:
        rs = np.random.RandomState(batch + 1)
        u, i, r = _random_graph(rs, NU, NI, 9, hot_items=5)
        graph = LaplacianCSR.from_interactions(u, i, r, NU, NI, device, heavy_threshold=128)
        batches = [tuple(torch.from_numpy(rs.randint(0, m, batch + 3 * k)).to(device) for m in (NU, NI, NI))
                   for k in range(6)]
        batches[3] = tuple(t[:0] for t in batches[3])                # an empty batch: a step with zero gradients
        _GRAPHS.clear()
        _GRAPHS[batch] = (graph, batches)
    return _GRAPHS[batch]


def _six_steps(device, tmp_path, batch, fraction, optimizer, layers, embed, deterministic, poison=False):
    from yelprecommendation_amd.models.ngcf import NGCF
    from yelprecommendation_amd.ngcf_step import NGCFStep
    from yelprecommendation_amd.optim import Adam, AdamW
    from yelprecommendation_amd.utils import make_config
    graph, batches = _setup(device, batch)
    torch.manual_seed(8)
    cfg = make_config("NGCF", embed_size=embed, num_orders=layers, device="cuda", model_dir=str(tmp_path),
                      ngcf_subset_fraction=fraction)
    model = NGCF(cfg, NU, NI).to(device)
    with torch.no_grad():
        model.embedding.weight.mul_(0.1)
    opt = (AdamW(model.parameters(), lr=LR, weight_decay=0.05) if optimizer == "adamw"
           else Adam(model.parameters(), lr=LR))

    def snapshot():
        return ({k: p.detach().clone() for k, p in model.named_parameters()},
                {k: (opt.state[p]["step"], opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
                 for k, p in model.named_parameters()})
    step = NGCFStep(model, opt, graph, fraction, deterministic=deterministic)
    assert step.deterministic is deterministic
    if poison:                                                       # the largest workspace of the run, allocated once
        step._workspace(max(b[0].numel() for b in batches))
    losses, first = [], None
    for j, (bu, bp, bn) in enumerate(batches):
        if poison:
            step._ws.fill_(255)                                      # 0xFF in every byte: NaNs, huge counts, set flags
        step.step(bu, bp, bn)
        losses.append(step.last_loss().clone())
        if j == 0:
            first = snapshot()
    step.check()
    params, state = snapshot()
    assert len(params) == 1 + 2 * layers
    return dict(losses=torch.stack(losses), first=first, params=params, state=state)


def _assert_bit_equal(a, b, what):
    assert torch.equal(a["losses"], b["losses"]), (what, "losses")
    for k in a["params"]:
        assert torch.equal(a["params"][k], b["params"][k]), (what, "parameter", k)
        assert a["state"][k][0] == b["state"][k][0] == 6
        assert torch.equal(a["state"][k][1], b["state"][k][1]), (what, "exp_avg", k)
        assert torch.equal(a["state"][k][2], b["state"][k][2]), (what, "exp_avg_sq", k)


@pytest.mark.parametrize("batch,fraction,optimizer,layers,embed", [
    (24, 0.5, "adam", 3, 64), (700, 0.5, "adamw", 3, 64), (700, 0.0, "adam", 3, 64), (24, 1e9, "adam", 3, 64),
    (8190, 0.5, "adam", 2, 32)],
    ids=["24-0.5-adam", "700-0.5-adamw", "700-0.0-adam", "24-1000000000.0-adam", "8190-0.5-adam-2x32"])
def test_six_steps_repeat_bit_for_bit_and_stay_with_the_default_mode(device, tmp_path, batch, fraction, optimizer,
                                                                     layers, embed):
    """Six steps on changing batches (one of them empty), batch-aware propagation on, off and forced on every layer,
    Adam and AdamW, across the switch of the loss to partials (B > 8192): two deterministic runs are torch.equal in
    every loss, all 1 + 2K parameters and both moments; a third run whose workspace is filled with 0xFF bytes before
    every step changes no bit; against the default mode the criteria of test_fused_step_equals_autograd_route hold."""
    args = (device, tmp_path, batch, fraction, optimizer, layers, embed)
    a = _six_steps(*args, True)
    b = _six_steps(*args, True)
    _assert_bit_equal(a, b, "second run")
    _assert_bit_equal(a, _six_steps(*args, True, poison=True), "poisoned workspace")
    d = _six_steps(*args, False)
    # after ONE step from the same parameters the two modes differ by the order of the sums only (the comment of
    # test_fused_step_equals_autograd_route applies word for word)
    (pa1, sa1), (pb1, sb1) = a["first"], d["first"]
    for k in pa1:
        for which, a_, b_ in (("m", sa1[k][1], sb1[k][1]), ("v", sa1[k][2], sb1[k][2])):
            assert float((a_ - b_).norm()) <= 1e-5 * float(b_.norm()) + 1e-30, (which, k)
            assert float((a_ - b_).abs().max()) <= 1e-4 * float(b_.abs().max()) + 1e-30, (which, k)
        err = (pa1[k] - pb1[k]).abs()
        assert float((err <= 1e-6 + 1e-5 * pb1[k].abs()).float().mean()) >= 0.999, k
        assert float(err.max()) <= 2.1 * LR, k
    la, lb = a["losses"].cpu().numpy(), d["losses"].cpu().numpy()
    np.testing.assert_allclose(la[0], lb[0], rtol=3e-7)
    np.testing.assert_allclose(la, lb, rtol=2e-5)
    travel = LR * 6
    for k in a["params"]:
        pa, pb, sa, sb = a["params"][k], d["params"][k], a["state"][k], d["state"][k]
        assert sa[0] == sb[0] == 6
        err = (pa - pb).abs()
        assert float((err <= 1e-3 * pb.abs() + 0.02 * travel).float().mean()) >= 0.998, k
        assert float(err.max()) <= 0.1 * travel, (k, float(err.max()))
        assert float((sa[1] - sb[1]).norm()) <= 2e-2 * float(sb[1].norm()) + 1e-30, k


# ---- trainer ----------------------------------------------------------------------------------------------------------

def _trainer_run(device, model_dir, full_eval):
    from yelprecommendation_amd.graph import LaplacianCSR
    from yelprecommendation_amd.trainers import NGCFTrainer
    from yelprecommendation_amd.utils import make_config
    nu, ni = 300, 517
    rs = np.random.RandomState(77)
    u = np.repeat(np.arange(nu), 8)
    i = rs.randint(0, ni, u.shape[0])
    pairs = np.unique(np.stack([u, i], 1), axis=0)
    u, i = pairs[:, 0], pairs[:, 1]
    graph = LaplacianCSR.from_interactions(u, i, rs.randint(1, 6, u.shape[0]), nu, ni, device)
    cfg = make_config("NGCF", embed_size=32, num_orders=2, device="cuda", top_n=10, model_dir=model_dir, lr=1e-2,
                      deterministic=True, full_eval=full_eval)
    torch.manual_seed(5)
    trainer = NGCFTrainer(cfg, ni, nu, graph)
    ids = rs.permutation(nu)[:290]
    frame = pd.DataFrame({"pos_items": [list(rs.choice(ni, rs.randint(1, 6), replace=False)) for _ in ids],
                          "mask_items": [list(rs.permutation(i[u == x])) for x in ids]}, index=ids)

    def loader(n_batches, B):
        return [{"user_id": torch.from_numpy(rs.randint(0, nu, B)), "pos_item": torch.from_numpy(rs.randint(0, ni, B)),
                 "neg_item": torch.from_numpy(rs.randint(0, ni, B))} for _ in range(n_batches)]
    train_loader, valid_loader = loader(5, 200), loader(3, 150)
    np.random.seed(9)                                                # evaluate's sample when full_eval is false
    floats = []
    for _ in range(2):
        floats.append(trainer.train(train_loader))
        floats.append(trainer.validate(valid_loader))
        floats.extend(trainer.evaluate(frame))
        floats.extend(trainer.evaluate_full(frame, "test"))
    assert trainer._fused_step().deterministic
    state = {k: v.clone() for k, v in trainer.model.state_dict().items()}
    opt = [trainer.optimizer.state[q][k].clone() for q in trainer.model.parameters() for k in ("exp_avg", "exp_avg_sq")]
    return floats, state, opt


@pytest.mark.parametrize("full_eval", [True, False], ids=["full_eval", "sampled_eval"])
def test_trainer_repeats_bit_for_bit(device, tmp_path, full_eval):
    """Two epochs of train / validate / evaluate / evaluate_full, twice from the same seeds: every returned float equal
    with ==, the model and the optimizer state torch.equal."""
    fa, sa, oa = _trainer_run(device, str(tmp_path / "a"), full_eval)
    fb, sb, ob = _trainer_run(device, str(tmp_path / "b"), full_eval)
    print("train / validate / evaluate / evaluate_full floats:", fa)
    assert len(fa) == 20 and np.isfinite(fa).all() and fa == fb
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert len(oa) == 10 and all(torch.equal(x, y) for x, y in zip(oa, ob))


def test_train_entry_point_repeats_bit_for_bit(device, tmp_path):
    from yelprecommendation_amd import train
    from yelprecommendation_amd.utils import make_config
    got = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        os.makedirs(d, exist_ok=True)
        cfg = make_config("NGCF", synthetic="300x900x14", fast_loader=True, deterministic=True, epochs=2, batch_size=256,
                          embed_size=32, num_orders=2, device="cuda", model_dir=d, lr=0.01)
        trainer, metrics = train.run(cfg, train.build(cfg))
        assert trainer._fused_step().deterministic
        got.append((tuple(metrics), torch.load(os.path.join(d, "best_model.pt"), map_location="cpu")))
    (ma, ba), (mb, bb) = got
    print("test metrics:", ma)
    assert ma == mb
    assert ba.keys() == bb.keys() and all(torch.equal(ba[k], bb[k]) for k in ba)


@pytest.mark.parametrize("kw", [dict(optimizer="sgd"), dict(fused_step=False)], ids=["sgd", "autograd_route"])
def test_refuses_what_the_mode_lacks(device, tmp_path, kw):
    """deterministic=true where the fused step is not available: NotImplementedError that names what the mode needs,
    from train.py before training starts, from the trainer, and from NGCFStep itself — never an unordered run."""
    from yelprecommendation_amd import optim, train
    from yelprecommendation_amd.graph import LaplacianCSR
    from yelprecommendation_amd.models.ngcf import NGCF
    from yelprecommendation_amd.ngcf_step import NGCFStep
    from yelprecommendation_amd.trainers import NGCFTrainer
    from yelprecommendation_amd.utils import make_config
    base = dict(synthetic="300x900x14", fast_loader=True, deterministic=True, epochs=1, batch_size=256, embed_size=16,
                num_orders=1, device="cuda", model_dir=str(tmp_path), lr=0.01)
    cfg = make_config("NGCF", **{**base, **kw})
    called = []
    inner = NGCFTrainer.train
    NGCFTrainer.train = lambda self, loader: called.append(1) or inner(self, loader)
    try:
        with pytest.raises(NotImplementedError, match="fused step"):
            train.run(cfg, train.build(cfg))
    finally:
        NGCFTrainer.train = inner
    assert called == []
    rs = np.random.RandomState(0)
    u = np.repeat(np.arange(30), 4)
    graph = LaplacianCSR.from_interactions(u, rs.randint(0, 20, u.shape[0]), np.ones(u.shape[0], np.int64), 30, 20, device)
    with pytest.raises(NotImplementedError, match="fused step"):
        NGCFTrainer(cfg, 20, 30, graph)
    # a trainer built without the flag and switched afterwards still refuses, in train()
    plain = make_config("NGCF", **{**base, **kw, "deterministic": False})
    trainer = NGCFTrainer(plain, 20, 30, graph)
    trainer.cfg.deterministic = True
    with pytest.raises(NotImplementedError, match="fused step"):
        trainer.train([])
    if "optimizer" in kw:
        model = NGCF(plain, 30, 20).to(device)
        with pytest.raises(NotImplementedError, match="fused step"):
            NGCFStep(model, optim.SGD(model.parameters(), lr=0.01), graph, deterministic=True)
