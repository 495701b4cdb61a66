"""deterministic=True for DCN: DCN.bpr_loss_backward (yr_dcn_head_ordered + yr_dcn_owned_assemble_bwd), DCNTrainer and
the train.py entry point give the same bits twice, do not depend on what their workspaces held, meet the criteria of
test_gpu_dcn.py::test_whole_step_matches_reference_probe against the reference's capture (both modes differ from the
reference by summation order only), and refuse the one form the mode does not cover."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from test_gpu_dcn import _rand_model, _trainer

pytestmark = pytest.mark.gpu

NU, NI, NC, NS, LMAX = 230, 610, 12, 5, 4
LR = 2e-3


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "dcn_small.npz"))


_BATCHES = {}


def _batches(device, batch):
    """Six batches of changing size over 230 users and 610 items (a hot item on a fifth of the positives; the padding
    category's list spans several chunks), the fourth one empty."""
    if batch not in _BATCHES:
        rs = np.random.RandomState(batch + 1)
        out = []
        for k in range(6):
            B = batch + 3 * k
            ids = [rs.randint(0, m, B) for m in (NU, NI, NI)]
            ids[1][rs.rand(B) < 0.2] = 17
            out.append(tuple(torch.from_numpy(a.astype(np.int64)).to(device) for a in ids))
        out[3] = tuple(t[:0] for t in out[3])
        _BATCHES.clear()
        _BATCHES[batch] = out
    return _BATCHES[batch]


def _six_steps(device, batch, D, hidden, L, optimizer, poison=False):
    from yelprecommendation_amd import optim
    from yelprecommendation_amd.models.dcn import DCN
    from yelprecommendation_amd.utils import make_config
    st, cat, sc = _rand_model(D, hidden, L, NU, NI, NC, NS, LMAX, 3)
    m = DCN(make_config("DCN", device="cuda", embed_size=D, hidden_dims=list(hidden), cross_orders=L), NU, NI,
            [NC - 1, NS - 1])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    m = m.to(device)
    m.set_item_attributes(torch.from_numpy(cat), torch.from_numpy(sc))
    m.deterministic = True
    opt = {"adam": lambda: optim.Adam(m.parameters(), lr=LR),
           "adamw": lambda: optim.AdamW(m.parameters(), lr=LR, weight_decay=0.05),
           "sgd": lambda: optim.SGD(m.parameters(), lr=0.05)}[optimizer]()
    losses = []
    for u, p, n in _batches(device, batch):
        if poison:
            for ws in m._owned_ws.values():
                ws.fill_(255)                                        # 0xFF in every byte: NaNs, huge counts
        losses.append(m.bpr_loss_backward(u, p, n).clone())
        opt.step(zero_grad=True)
    m.check_indices()
    assert set(m._owned_ws) == {"head", "scatter"}
    params = {k: v.detach().clone() for k, v in m.named_parameters()}
    state = {k: {s: (t.clone() if torch.is_tensor(t) else t) for s, t in opt.state[v].items()}
             for k, v in m.named_parameters()}
    return dict(losses=torch.stack(losses), params=params, state=state)


def _assert_bit_equal(a, b, what):
    assert torch.isfinite(a["losses"]).all() and float(a["losses"][3]) == 0.0
    assert torch.equal(a["losses"], b["losses"]), (what, "losses")
    for k in a["params"]:
        assert torch.equal(a["params"][k], b["params"][k]), (what, "parameter", k)
        assert a["state"][k].keys() == b["state"][k].keys()
        for s, t in a["state"][k].items():
            assert torch.equal(t, b["state"][k][s]) if torch.is_tensor(t) else t == b["state"][k][s], (what, s, k)


@pytest.mark.parametrize("batch,D,hidden,L,optimizer", [
    (24, 16, [64], 1, "adam"), (700, 64, [64, 32], 3, "adamw"), (1100, 16, [64, 32], 1, "sgd"),
    (1100, 64, [64], 3, "adam")], ids=["24-16-adam", "700-64-adamw", "1100-16-sgd", "1100-64-adam"])
def test_six_steps_repeat_bit_for_bit(device, batch, D, hidden, L, optimizer):
    """Six steps on changing batches (one of them empty; 1100 triplets: past one trip of the head's 1,024 waves), one
    and two hidden layers, one and three cross orders, Adam, AdamW and SGD: two deterministic runs are torch.equal in
    every loss, parameter and optimizer state; a third run whose workspaces are filled with 0xFF bytes before every step
    changes no bit."""
    args = (device, batch, D, hidden, L, optimizer)
    a = _six_steps(*args)
    _assert_bit_equal(a, _six_steps(*args), "second run")
    _assert_bit_equal(a, _six_steps(*args, poison=True), "poisoned workspaces")
    if optimizer != "sgd":
        assert all(s["step"] == 6 for s in a["state"].values())


def test_whole_step_matches_reference_probe(g, device, tmp_path):
    """The criteria of test_gpu_dcn.py::test_whole_step_matches_reference_probe, word for word, for the deterministic
    step: the loss, every gradient and the parameters after one Adam step against the reference's capture."""
    tr = _trainer(g, tmp_path)
    m = tr.model
    m.deterministic = True
    u, p, n = (torch.from_numpy(g[k].astype(np.int64)).to(device) for k in ("probe_u", "probe_p", "probe_n"))
    loss = m.bpr_loss_backward(u, p, n)
    np.testing.assert_allclose(float(loss.item()), float(g["probe_loss"]), rtol=1e-5)
    for k, prm in m.named_parameters():
        want = g["grad:" + k]
        np.testing.assert_allclose(prm.grad.cpu().numpy(), want, rtol=1e-3, atol=1e-4 * max(1e-3, np.abs(want).max()),
                                   err_msg=k)
    tr.optimizer.step(zero_grad=True)
    lr = tr.cfg.lr
    for k, v in m.state_dict().items():
        tiny = np.abs(g["grad:" + k]) < 1e-6
        np.testing.assert_allclose(v.cpu().numpy()[~tiny], g["step1:" + k][~tiny], rtol=1e-5, atol=2e-6, err_msg=k)
        np.testing.assert_allclose(v.cpu().numpy()[tiny], g["step1:" + k][tiny], atol=1.01 * lr, err_msg=k)


def test_autograd_forward_refuses_the_flag(g, device, tmp_path):
    """DCN.forward(...).backward() is the per-row attribute form, which has no ordered scatter: NotImplementedError
    under the flag rather than an unordered run; the forward itself still works."""
    tr = _trainer(g, tmp_path)
    m = tr.model
    m.deterministic = True
    u, p = (torch.from_numpy(g[k].astype(np.int64)).to(device) for k in ("probe_u", "probe_p"))
    cats, sc = torch.from_numpy(g["cat_ids"]), torch.from_numpy(g["sc_ids"])
    pos = m(u, p, cats[p.cpu()].to(device), sc[p.cpu()].to(device))
    np.testing.assert_allclose(pos.detach().cpu().numpy().reshape(-1), g["probe_pos"], rtol=1e-5, atol=1e-6)
    with pytest.raises(NotImplementedError, match="deterministic"):
        pos.sum().backward()


# ---- trainer ----------------------------------------------------------------------------------------------------------

def _trainer_run(device, model_dir, optimizer):
    from yelprecommendation_amd.trainers.dcn_trainer import DCNTrainer
    from yelprecommendation_amd.utils import make_config
    nu, ni = 300, 517
    rs = np.random.RandomState(77)
    _, cat, sc = _rand_model(16, [64, 32], 2, nu, ni, NC, NS, LMAX, 4)
    cfg = make_config("DCN", embed_size=16, hidden_dims=[64, 32], cross_orders=2, device="cuda", top_n=10,
                      model_dir=model_dir, lr=1e-2, deterministic=True, optimizer=optimizer)
    torch.manual_seed(5)
    trainer = DCNTrainer(cfg, ni, nu, None, [NC - 1, NS - 1], cat_ids=torch.from_numpy(cat), sc_ids=torch.from_numpy(sc))
    assert trainer.model.deterministic is True
    ids = rs.permutation(nu)[:290]
    frame = pd.DataFrame({"pos_items": [list(rs.choice(ni, rs.randint(1, 6), replace=False)) for _ in ids],
                          "mask_items": [list(rs.choice(ni, 8, replace=False)) for _ in ids]},
                         index=pd.Index(ids, name="user_id"))

    def loader(n_batches, B):
        return [{"user_id": torch.from_numpy(rs.randint(0, nu, B)), "pos_item": torch.from_numpy(rs.randint(0, ni, B)),
                 "neg_item": torch.from_numpy(rs.randint(0, ni, B))} for _ in range(n_batches)]
    train_loader, valid_loader = loader(5, 200), loader(3, 150)
    floats = []
    for _ in range(2):
        floats.append(trainer.train(train_loader))
        floats.append(trainer.validate(valid_loader))
        floats.extend(trainer.evaluate(frame))
    state = {k: v.clone() for k, v in trainer.model.state_dict().items()}
    opt = [t.clone() for q in trainer.model.parameters() for t in trainer.optimizer.state[q].values()
           if torch.is_tensor(t)]
    return floats, state, opt


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_trainer_repeats_bit_for_bit(device, tmp_path, optimizer):
    """Two epochs of train / validate / evaluate, twice from the same seeds: every returned float equal with ==, the
    model and the optimizer state torch.equal."""
    fa, sa, oa = _trainer_run(device, str(tmp_path / "a"), optimizer)
    fb, sb, ob = _trainer_run(device, str(tmp_path / "b"), optimizer)
    print("train / validate / evaluate floats:", fa)
    assert len(fa) == 12 and np.isfinite(fa).all() and fa == fb
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert len(oa) == len(ob) and all(torch.equal(x, y) for x, y in zip(oa, ob))


def test_train_entry_point_repeats_bit_for_bit(device, tmp_path):
    from yelprecommendation_amd import train
    from yelprecommendation_amd.utils import make_config
    got = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        os.makedirs(d, exist_ok=True)
        cfg = make_config("DCN", synthetic="300x200x12", fast_loader=True, deterministic=True, epochs=2, batch_size=64,
                          embed_size=16, hidden_dims=[64, 32], cross_orders=2, device="cuda", model_dir=d, lr=0.001)
        trainer, metrics = train.run(cfg, train.build(cfg))
        assert trainer.model.deterministic is True
        got.append((tuple(metrics), torch.load(os.path.join(d, "best_model.pt"), map_location="cpu")))
    (ma, ba), (mb, bb) = got
    print("test metrics:", ma)
    assert ma == mb
    assert ba.keys() == bb.keys() and all(torch.equal(ba[k], bb[k]) for k in ba)
