"""GPU parity for NGCF: SpMM, the MFMA dense layer (forward and both backward kernels), the model's
bpr_forward / forward / embedding_propagation and a full NGCFTrainer run against the golden vectors
captured from the reference (tests/golden/ngcf_tiny.npz) and against the NumPy oracle at larger,
popularity-skewed sizes."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from oracle import ngcf as ongcf
from replay import ReplayLoader, epoch_slices

pytestmark = pytest.mark.gpu


# two captures of the reference: the tiny graph (D = 16, K = 2) and one with BASELINE configs[3]'s hyper-parameters
# (D = 64, K = 3 layers) on a 1,044-node graph (tests/golden/make_golden.py ngcf)
@pytest.fixture(scope="module", params=["ngcf_tiny.npz", "ngcf_mid.npz"])
def g(golden_dir, request):
    return np.load(os.path.join(golden_dir, request.param))


def _cfg(g, tmp_path, **kw):
    from yelprecommendation_amd.utils import make_config
    c = make_config("NGCF", embed_size=int(g["embed_size"]), num_orders=int(g["num_orders"]), lr=float(g["lr"]),
                    batch_size=int(g["batch_size"]), device="cuda", model_dir=str(tmp_path), seed=42)
    c.update(kw)
    return c


def _lap_torch(g):
    n = int(g["num_users"]) + int(g["num_items"])
    idx = torch.from_numpy(np.stack([g["lap_row"], g["lap_col"]]).astype(np.int64))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(g["lap_val"]), (n, n)).coalesce()


def _random_graph(rs, nu, ni, deg, hot_items=0):
    u = np.repeat(np.arange(nu), deg)
    i = rs.randint(0, ni, size=u.shape[0])
    if hot_items:
        hot = rs.rand(i.shape[0]) < 0.3
        i[hot] = rs.randint(0, hot_items, size=int(hot.sum()))
    r = rs.randint(1, 6, size=u.shape[0])
    return u, i, r


@pytest.mark.parametrize("d", [16, 32, 64, 128])
def test_spmm_matches_scipy(device, d):
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.graph import LaplacianCSR, laplacian_scipy
    rs = np.random.RandomState(d)
    nu, ni = 400, 120
    u, i, r = _random_graph(rs, nu, ni, 12, hot_items=3)       # 3 very popular items => heavy rows
    L = laplacian_scipy(u, i, r, nu, ni)
    graph = LaplacianCSR.from_scipy(L, device, heavy_threshold=64)
    assert graph.n_heavy >= 1 and graph.symmetric
    X = rs.standard_normal((nu + ni, d)).astype(np.float32)
    Y = engine.spmm_csr(graph, torch.from_numpy(X).to(device))
    np.testing.assert_allclose(Y.cpu().numpy(), L @ X, rtol=1e-4, atol=1e-5)
    acc = torch.from_numpy(X).to(device).clone()
    engine.spmm_csr(graph, torch.from_numpy(X).to(device), out=acc, accumulate=True)
    np.testing.assert_allclose(acc.cpu().numpy(), L @ X + X, rtol=1e-4, atol=1e-5)
    for dd in (16, 32, 64, 128):                                  # the sliced form at every width (1, 1, 2, 4 slices)
        xs = torch.randn(graph.n, dd, device=device)
        torch.testing.assert_close(engine.spmm_csr(graph, xs, form="sliced"), engine.spmm_csr(graph, xs, form="rows"),
                                   rtol=1e-5, atol=1e-6)
    # all-light path (no heavy list) gives the same result
    g2 = LaplacianCSR.from_scipy(L, device, heavy_threshold=10 ** 9)
    assert g2.n_heavy == 0
    np.testing.assert_allclose(engine.spmm_csr(g2, torch.from_numpy(X).to(device)).cpu().numpy(), L @ X,
                               rtol=1e-4, atol=1e-5)


def test_laplacian_builder_matches_reference_pipeline(g, device):
    from yelprecommendation_amd.graph import LaplacianCSR, laplacian_scipy
    U, I = int(g["num_users"]), int(g["num_items"])
    L = laplacian_scipy(g["tsv_user"], g["tsv_item"], g["tsv_rating"], U, I)
    ref = sp.csr_matrix((g["lap_val"], (g["lap_row"], g["lap_col"])), shape=(U + I, U + I))
    assert L.nnz == ref.nnz and abs(L - ref).max() <= 1e-7
    graph = LaplacianCSR.from_interactions(g["tsv_user"], g["tsv_item"], g["tsv_rating"], U, I, device)
    back = graph.to_torch_sparse()
    assert torch.equal(back.indices(), _lap_torch(g).indices())
    torch.testing.assert_close(back.values(), _lap_torch(g).values(), rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("d", [16, 32, 64, 128])
def test_dense_layer_fwd_bwd_matches_oracle(device, d):
    from yelprecommendation_amd import engine
    rs = np.random.RandomState(100 + d)
    n = 333
    E = rs.standard_normal((n, d)).astype(np.float32)
    Z = rs.standard_normal((n, d)).astype(np.float32)
    W1 = (rs.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
    W2 = (rs.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
    dOut = rs.standard_normal((n, d)).astype(np.float32)
    A, H = Z + E, E * Z
    P = A @ W1.T + H @ W2.T
    out_ref = np.where(P > 0, P, 0.01 * P)
    dP = dOut * np.where(P > 0, 1.0, 0.01)
    dA, dH = dP @ W1, dP @ W2
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    out = engine.ngcf_dense_fwd(t(E), t(Z), t(W1), t(W2))
    np.testing.assert_allclose(out.cpu().numpy(), out_ref, rtol=1e-4, atol=1e-5)
    dE0 = rs.standard_normal((n, d)).astype(np.float32)           # dE is accumulated into
    dE, dW1, dW2 = t(dE0), torch.zeros(d, d, device=device), torch.zeros(d, d, device=device)
    dZ = engine.ngcf_dense_bwd(t(dOut), out, t(E), t(Z), t(W1), t(W2), dE, dW1, dW2)
    np.testing.assert_allclose(dZ.cpu().numpy(), dA + dH * E, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(dE.cpu().numpy(), dE0 + dA + dH * Z, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(dW1.cpu().numpy(), dP.T @ A, rtol=1e-4, atol=2e-4)
    np.testing.assert_allclose(dW2.cpu().numpy(), dP.T @ H, rtol=1e-4, atol=2e-4)


def _load_init(model, g, prefix="init"):
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(torch.from_numpy(g[f"{prefix}__{name.replace('.', '__')}"]))


def test_model_probe_matches_reference(g, tmp_path, device):
    """bpr_forward / forward / embedding_propagation outputs, BPR loss and ALL parameter gradients on
    the golden probe batch (reference models/ngcf.py:30-72 + loss.py:25-27 + autograd)."""
    from yelprecommendation_amd.loss import BPRLoss
    from yelprecommendation_amd.models.ngcf import NGCF
    cfg = _cfg(g, tmp_path)
    model = NGCF(cfg, int(g["num_users"]), int(g["num_items"])).to(device)
    assert [n for n, _ in model.named_parameters()] == g["param_names"].tolist()
    _load_init(model, g)
    L = _lap_torch(g)
    u, p, n = (torch.from_numpy(g[k]).to(device) for k in ("probe_u", "probe_p", "probe_n"))
    pos, neg = model.bpr_forward(u, p, n, L)
    np.testing.assert_allclose(pos.detach().cpu().numpy(), g["probe_pos"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(neg.detach().cpu().numpy(), g["probe_neg"], rtol=1e-4, atol=1e-5)
    loss = BPRLoss()(pos, neg)
    np.testing.assert_allclose(loss.item(), float(g["probe_loss"]), rtol=1e-5)
    loss.backward()
    for name, prm in model.named_parameters():
        want = g[f"grad__{name.replace('.', '__')}"]
        np.testing.assert_allclose(prm.grad.cpu().numpy(), want, rtol=1e-3, atol=1e-6 + 1e-4 * np.abs(want).max())
    with torch.no_grad():
        fwd = model(u, p, L)
        e1 = model.embedding_propagation(model.embedding.weight, model.W1[0], model.W2[0], L)
    np.testing.assert_allclose(fwd.cpu().numpy(), g["probe_forward"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(e1.cpu().numpy(), g["probe_layer1"], rtol=1e-4, atol=1e-5)
    model.check_indices()


def test_seeded_init_matches_reference(g, tmp_path, device):
    from yelprecommendation_amd.trainers import NGCFTrainer
    from yelprecommendation_amd.utils import set_seed
    cfg = _cfg(g, tmp_path)
    set_seed(cfg.seed)
    t = NGCFTrainer(cfg, int(g["num_items"]), int(g["num_users"]), _lap_torch(g))
    for name, prm in t.model.named_parameters():
        np.testing.assert_array_equal(prm.detach().cpu().numpy(), g[f"init__{name.replace('.', '__')}"])


@pytest.mark.parametrize("fused", [True, False])
def test_trainer_run_matches_reference(g, tmp_path, device, fused):
    """Replay the reference's recorded batches through NGCFTrainer: per-epoch losses, final parameters
    and the 100-sampled-user metrics (same NumPy RNG positions) must match — with the whole batch step as one
    engine call (ngcf_step.NGCFStep, the default) and through the launch-by-launch autograd route."""
    from yelprecommendation_amd.trainers import NGCFTrainer
    cfg = _cfg(g, tmp_path, fused_step=fused)
    t = NGCFTrainer(cfg, int(g["num_items"]), int(g["num_users"]), _lap_torch(g))
    _load_init(t.model, g)
    users = g["valid_eval_users"]
    frame = pd.DataFrame({
        "pos_items": [g["valid_pos_idx"][g["valid_pos_ptr"][r]:g["valid_pos_ptr"][r + 1]].tolist() for r in range(len(users))],
        "mask_items": [g["valid_mask_idx"][g["valid_mask_ptr"][r]:g["valid_mask_ptr"][r + 1]].tolist() for r in range(len(users))],
    }, index=pd.Index(users, name="user_id"))
    tb, vb = g["train_batch_sizes"], g["valid_batch_sizes"]
    real_randint = np.random.randint
    for e, ((tb0, tb1, tr0, tr1), (vb0, vb1, vr0, vr1)) in enumerate(
            zip(epoch_slices(g["train_steps"], tb), epoch_slices(g["valid_steps"], vb))):
        tl = t.train(ReplayLoader(g["train_u"][tr0:tr1], g["train_p"][tr0:tr1], g["train_n"][tr0:tr1], tb[tb0:tb1]))
        vl = t.validate(ReplayLoader(g["valid_u"][vr0:vr1], g["valid_p"][vr0:vr1], g["valid_n"][vr0:vr1], vb[vb0:vb1]))
        np.testing.assert_allclose(tl, g["train_epoch_loss"][e], rtol=1e-4)
        np.testing.assert_allclose(vl, g["valid_epoch_loss"][e], rtol=1e-4)
        # validate() propagates once and scores every batch on the same layers; re-propagating per batch (the
        # reference's loop) must give the very same number
        t.cfg.propagate_once = False
        again = t.validate(ReplayLoader(g["valid_u"][vr0:vr1], g["valid_p"][vr0:vr1], g["valid_n"][vr0:vr1], vb[vb0:vb1]))
        t.cfg.propagate_once = True
        assert again == vl
        # feed evaluate() the positions the reference drew from its NumPy stream
        np.random.randint = lambda *a, **k: g["eval_positions"][e].copy()
        try:
            metrics = t.evaluate(frame, "valid")
        finally:
            np.random.randint = real_randint
        np.testing.assert_allclose(metrics, g["eval_metrics"][e], atol=1e-3, rtol=0)
    # Adam moves a parameter by at most lr per step whatever the size of its gradient: where a gradient nearly
    # cancels, summation-order noise becomes a visible fraction of lr — the absolute bar is 1 % of the maximum
    # travel lr x steps (never below the 2e-4 the tiny capture has always met)
    travel = float(g["lr"]) * int(np.sum(g["train_steps"]))
    for name, prm in t.model.named_parameters():
        want = g[f"final__{name.replace('.', '__')}"]
        got = prm.detach().cpu().numpy()
        if int(g["embed_size"]) < 64:
            np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-4)
            continue
        # the larger capture (D = 64, K = 3, float atomics in the backward): at least 99.8 % of every tensor inside
        # rtol 2e-3 + 1 % of the travel; the few elements whose gradient sits at Adam's eps — where m / sqrt(v) turns
        # noise into whole steps of lr — inside 5 % of the travel
        err = np.abs(got - want)
        tight = err <= 2e-3 * np.abs(want) + 0.01 * travel
        assert tight.mean() >= 0.998, (name, float(tight.mean()))
        assert float(err.max()) <= 0.05 * travel, (name, float(err.max()), travel)


def test_training_steps_match_oracle_on_skewed_graph(device, tmp_path):
    """Beyond the fixture: a larger popularity-skewed graph (heavy rows), D = 64, K = 3 (config 4's
    depth); three Adam steps against the NumPy oracle."""
    from yelprecommendation_amd.graph import LaplacianCSR, laplacian_scipy
    from yelprecommendation_amd.loss import BPRLoss
    from yelprecommendation_amd.models.ngcf import NGCF
    from yelprecommendation_amd.optim import Adam
    from yelprecommendation_amd.utils import make_config
    rs = np.random.RandomState(9)
    nu, ni, d, K, B = 900, 300, 64, 3, 512
    u, i, r = _random_graph(rs, nu, ni, 15, hot_items=2)
    L = laplacian_scipy(u, i, r, nu, ni)
    graph = LaplacianCSR.from_scipy(L, device, heavy_threshold=128)
    assert graph.n_heavy >= 1
    cfg = make_config("NGCF", embed_size=d, num_orders=K, device="cuda", model_dir=str(tmp_path))
    torch.manual_seed(3)
    model = NGCF(cfg, nu, ni)
    with torch.no_grad():
        model.embedding.weight.mul_(0.1)                     # N(0,1) rows blow the scores up at D = 64
    E0 = model.embedding.weight.detach().numpy().copy()
    W1 = [w.weight.detach().numpy().copy() for w in model.W1]
    W2 = [w.weight.detach().numpy().copy() for w in model.W2]
    model = model.to(device)
    ref = ongcf.NGCFState(E0, W1, W2, L, nu, lr=1e-3)
    opt = Adam(model.parameters(), lr=1e-3)
    for step in range(3):
        bu, bp, bn = rs.randint(0, nu, B), rs.randint(0, ni, B), rs.randint(0, ni, B)
        want = float(ref.train_step(bu, bp, bn))
        pos, neg = model.bpr_forward(*(torch.from_numpy(a.astype(np.int64)).to(device) for a in (bu, bp, bn)), graph)
        opt.zero_grad()
        loss = BPRLoss()(pos, neg)
        loss.backward()
        opt.step()
        np.testing.assert_allclose(loss.item(), want, rtol=2e-4)
    np.testing.assert_allclose(model.embedding.weight.detach().cpu().numpy(), ref.E, rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(model.W1[K - 1].weight.detach().cpu().numpy(), ref.W1[K - 1], rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(model.W2[0].weight.detach().cpu().numpy(), ref.W2[0], rtol=2e-3, atol=2e-4)


@pytest.mark.parametrize("d,layers,with_neg", [(16, 1, True), (32, 3, True), (64, 4, True), (64, 4, False),
                                               (128, 8, True)])
def test_layer_sum_scores_match_concat_definition(device, d, layers, with_neg):
    """yr_ngcf_score_fwd/_bwd vs the reference's definition (models/ngcf.py:44-58): concatenate the
    layer outputs, index users and items, multiply, sum — and its autograd; ragged batch sizes
    (not a multiple of the lane-group count) and repeated ids (atomics)."""
    from yelprecommendation_amd import engine
    rs = np.random.RandomState(layers * 1000 + d)
    nu, ni = 37, 53
    for B in (1, 7, 64, 1001):
        Es = [rs.standard_normal((nu + ni, d)).astype(np.float32) for _ in range(layers)]
        u = rs.randint(0, nu, B); p = rs.randint(0, ni, B); n = rs.randint(0, ni, B)
        gp = rs.standard_normal(B).astype(np.float32); gn = rs.standard_normal(B).astype(np.float32)
        # float64 statement of the definition
        cat = np.concatenate(Es, axis=1).astype(np.float64)
        want_pos = (cat[u] * cat[nu + p]).sum(1)
        want_neg = (cat[u] * cat[nu + n]).sum(1)
        dcat = np.zeros_like(cat)
        np.add.at(dcat, u, gp[:, None] * cat[nu + p]); np.add.at(dcat, nu + p, gp[:, None] * cat[u])
        if with_neg:
            np.add.at(dcat, u, gn[:, None] * cat[nu + n]); np.add.at(dcat, nu + n, gn[:, None] * cat[u])
        T = [torch.from_numpy(E).to(device) for E in Es]
        tu, tp, tn = (torch.from_numpy(x).to(device) for x in (u, p, n))
        flag = torch.zeros(1, dtype=torch.int32, device=device)
        res = engine.ngcf_score(T, nu, tu, tp, tn if with_neg else None, err_flag=flag)
        pos, neg = res if with_neg else (res, None)
        scale = np.abs(cat).max() ** 2 * cat.shape[1]
        np.testing.assert_allclose(pos.cpu().numpy(), want_pos, atol=2e-6 * scale)
        if with_neg:
            np.testing.assert_allclose(neg.cpu().numpy(), want_neg, atol=2e-6 * scale)
        dT = [torch.zeros_like(t) for t in T]
        engine.ngcf_score_backward(T, dT, nu, tu, tp, tn if with_neg else None, torch.from_numpy(gp).to(device),
                                   torch.from_numpy(gn).to(device) if with_neg else None, err_flag=flag)
        got = np.concatenate([t.cpu().numpy() for t in dT], axis=1)
        np.testing.assert_allclose(got, dcat, atol=1e-5 * max(1.0, np.abs(dcat).max()))
        assert int(flag.item()) == 0


def test_layer_sum_scores_flag_bad_ids(device):
    from yelprecommendation_amd import engine
    nu, ni, d = 10, 12, 64
    T = [torch.randn(nu + ni, d, device=device) for _ in range(2)]
    u = torch.tensor([0, 10, 3, -1], device=device); p = torch.tensor([1, 2, 12, 4], device=device)
    n = torch.tensor([0, 1, 2, 3], device=device)
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    pos, neg = engine.ngcf_score(T, nu, u, p, n, err_flag=flag)
    assert int(flag.item()) == engine.FLAG_BAD_USER | engine.FLAG_BAD_ITEM
    assert pos[1:].abs().max().item() == 0.0 and neg[1:].abs().max().item() == 0.0 and pos[0].item() != 0.0
    dT = [torch.zeros_like(t) for t in T]
    engine.ngcf_score_backward(T, dT, nu, u, p, n, torch.ones(4, device=device), torch.ones(4, device=device))
    touched = (dT[0].abs().sum(1) > 0).nonzero().flatten().tolist()
    assert touched == [0, nu + 0, nu + 1]                    # only the valid triplet (0, 1, 0) scatters
    with pytest.raises(engine.EngineError):
        engine.ngcf_score([T[0]] * 9, nu, u, p, n)


def test_full_size_spmm_properties(device):
    """BASELINE configs[3] graph size (69,716 nodes, ~3.1 M non-zeros, D = 64): the SpMM is linear,
    symmetric (<x, L y> == <L x, y>: L = D^-1/2 A D^-1/2), agrees with torch.sparse.mm, and
    accumulate adds."""
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.data.synthetic import YELP2018_ITEMS as NI, YELP2018_USERS as NU, make_interactions_torch
    from yelprecommendation_amd.graph import LaplacianCSR
    u, i = make_interactions_torch(NU, NI, 47.0, device=device)
    r = torch.randint(1, 6, u.shape, device=device)
    graph = LaplacianCSR.from_interactions(u.cpu().numpy(), i.cpu().numpy(), r.cpu().numpy(), NU, NI, device)
    assert graph.n == NU + NI and graph.symmetric and graph.nnz > 3_000_000
    g = torch.Generator(device=device).manual_seed(1)
    x = torch.randn(graph.n, 64, device=device, generator=g)
    y = torch.randn(graph.n, 64, device=device, generator=g)
    Lx, Ly = engine.spmm_csr(graph, x), engine.spmm_csr(graph, y)
    torch.testing.assert_close(engine.spmm_csr(graph, 2.0 * x - 3.0 * y), 2.0 * Lx - 3.0 * Ly, rtol=1e-4, atol=1e-4)
    a, b = (x.double() * Ly.double()).sum().item(), (Lx.double() * y.double()).sum().item()
    assert abs(a - b) <= 1e-5 * max(abs(a), abs(b), 1.0)
    ref = torch.sparse.mm(graph.to_torch_sparse().to(device), x)
    torch.testing.assert_close(Lx, ref, rtol=1e-4, atol=1e-5)
    acc = y.clone()
    engine.spmm_csr(graph, x, out=acc, accumulate=True)
    torch.testing.assert_close(acc, y + Lx, rtol=1e-5, atol=1e-5)
    # the feature-sliced form (slices of 32 floats pinned per XCD, rows by falling degree) gives the same product
    torch.testing.assert_close(engine.spmm_csr(graph, x, form="sliced"), Lx, rtol=1e-5, atol=1e-6)
    acc = y.clone()
    engine.spmm_csr(graph, x, out=acc, accumulate=True, form="sliced")
    torch.testing.assert_close(acc, y + Lx, rtol=1e-5, atol=1e-5)


def test_frontier_and_subset_kernels(device):
    """The batch-aware propagation's building blocks (ABI v28): frontier flags == the NumPy definition
    S_K = {u, U + p, U + n}, S_{k-1} = S_k + neighbours(S_k); the row list is a permutation of the flagged rows with
    its length on the device; the row-subset SpMM writes EXACTLY the full product's rows (bit for bit) and nothing
    else; the scatter form from a row list equals the product of a matrix whose other rows are zero; the row-list
    forms of the dense kernels equal the full kernels on the listed rows bit for bit."""
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.graph import LaplacianCSR, laplacian_scipy
    rs = np.random.RandomState(11)
    nu, ni, d = 900, 700, 64
    u, i, r = _random_graph(rs, nu, ni, 6, hot_items=4)
    L = laplacian_scipy(u, i, r, nu, ni)
    graph = LaplacianCSR.from_scipy(L, device, heavy_threshold=64)
    assert graph.n_heavy >= 1
    n = nu + ni
    t = lambda a: torch.from_numpy(a).to(device)
    bu, bp, bn = rs.randint(0, nu, 40), rs.randint(0, ni, 40), rs.randint(0, ni, 40)
    bp[:3] = (0, 1, 2)                                              # the heavy rows are in the batch
    want0 = np.zeros(n, np.int32)
    want0[bu] = 1; want0[nu + bp] = 1; want0[nu + bn] = 1
    s0 = engine.ngcf_frontier_mark(nu, ni, t(bu), t(bp), t(bn))
    f0 = s0.flags
    np.testing.assert_array_equal(f0.cpu().numpy(), want0)
    cnt = int(s0.count.item())
    assert s0.max_rows == 120 and cnt == int(want0.sum())
    assert sorted(s0.rows[:cnt].cpu().tolist()) == np.flatnonzero(want0).tolist()      # every member exactly once
    only_pos = engine.ngcf_frontier_mark(nu, ni, t(bu), t(bp), None)
    assert int(only_pos.count.item()) == int(only_pos.flags.sum()) == len(set(bu.tolist())) + len(set(bp.tolist()))
    adj = (abs(L) > 0).astype(np.int32)
    want1 = ((adj @ want0 > 0) | (want0 > 0)).astype(np.int32)
    s1 = engine.ngcf_frontier_expand(graph, s0)
    f1 = s1.flags
    np.testing.assert_array_equal(f1.cpu().numpy(), want1)
    c1 = int(s1.count.item())
    assert c1 == int(want1.sum()) and sorted(s1.rows[:c1].cpu().tolist()) == np.flatnonzero(want1).tolist()
    # SpMM, row subset
    X = t(rs.standard_normal((n, d)).astype(np.float32))
    full = engine.spmm_csr(graph, X)
    sub = engine.spmm_csr_subset(graph, X, torch.full_like(X, 7.0), row_active=f0)
    on = f0.bool()
    assert torch.equal(sub[on], full[on]) and bool((sub[~on] == 7.0).all())
    by_list = engine.spmm_csr_subset(graph, X, torch.full_like(X, 7.0), rows=s0)          # the set's list drives the launch
    assert torch.equal(by_list, sub)
    # accumulate adds to what is there, on the flagged rows only
    acc = engine.spmm_csr_subset(graph, X, torch.ones_like(X), row_active=f0, accumulate=True)
    ref = engine.spmm_csr(graph, X, out=torch.ones_like(X), accumulate=True)
    assert torch.equal(acc[on], ref[on]) and bool((acc[~on] == 1.0).all())
    Xz = X * f1.float()[:, None]
    want = engine.spmm_csr(graph, Xz)
    # the scatter form of the same restricted product (backward of a layer whose dZ lives on few rows)
    pushed = engine.spmm_csr_push_rows(graph, X, torch.zeros_like(X), s1)
    torch.testing.assert_close(pushed, want, rtol=1e-4, atol=1e-5)
    # dense part over the row list
    E, Z = X, full
    W1, W2 = (t((rs.standard_normal((d, d)) * 0.2).astype(np.float32)) for _ in range(2))
    out_full = engine.ngcf_dense_fwd(E, Z, W1, W2)
    out_sub = engine.ngcf_dense_fwd(E, Z, W1, W2, out=torch.full_like(E, 5.0), rows=s0)
    assert torch.equal(out_sub[on], out_full[on]) and bool((out_sub[~on] == 5.0).all())
    dEout = torch.zeros_like(E)
    dEout[on] = t(rs.standard_normal((cnt, d)).astype(np.float32))
    dE_f, dW1_f, dW2_f = torch.zeros_like(E), torch.zeros_like(W1), torch.zeros_like(W2)
    dZ_f = engine.ngcf_dense_bwd(dEout, out_full, E, Z, W1, W2, dE_f, dW1_f, dW2_f)
    dE_s, dW1_s, dW2_s = torch.zeros_like(E), torch.zeros_like(W1), torch.zeros_like(W2)
    dZ_s = engine.ngcf_dense_bwd(dEout, out_full, E, Z, W1, W2, dE_s, dW1_s, dW2_s, dZ=torch.full_like(E, 3.0), rows=s0)
    assert torch.equal(dZ_s[on], dZ_f[on]) and bool((dZ_s[~on] == 3.0).all()) and torch.equal(dE_s, dE_f)
    torch.testing.assert_close(dW1_s, dW1_f, rtol=1e-4, atol=1e-5)      # float atomics / another chunking of the rows
    torch.testing.assert_close(dW2_s, dW2_f, rtol=1e-4, atol=1e-5)
    # an empty batch: no flags, an empty list, nothing computed
    e = torch.zeros(0, dtype=torch.int64, device=device)
    se = engine.ngcf_frontier_mark(nu, ni, e, e, e)
    assert int(se.flags.sum()) == 0 and int(se.count.item()) == 0
    assert bool((engine.ngcf_dense_fwd(E, Z, W1, W2, out=torch.full_like(E, 5.0), rows=se) == 5.0).all())


@pytest.mark.parametrize("batch,fraction,subset_layers", [(12, 0.5, 2), (400, 0.5, 1), (12, 1e9, 3), (5000, 0.5, 0)])
def test_batch_aware_propagation_equals_full_graph_propagation(device, tmp_path, batch, fraction, subset_layers):
    """NGCF.bpr_forward / forward propagate layer k on the rows the batch's scores need (cfg.ngcf_subset_fraction,
    default 0.5) instead of the whole graph for every batch (reference trainers/ngcf_trainer.py:108 ->
    models/ngcf.py:30-45): the scores are BIT-IDENTICAL to the full-graph propagation's, the loss too, and every
    parameter gradient agrees to summation order — for a small batch (last two of three layers restricted), a
    medium one (last layer only), all layers forced, and a batch whose rows cover the graph (none restricted)."""
    from yelprecommendation_amd.graph import LaplacianCSR
    from yelprecommendation_amd.loss import BPRLoss
    from yelprecommendation_amd.models import ngcf as mngcf
    from yelprecommendation_amd.models.ngcf import NGCF
    from yelprecommendation_amd.utils import make_config
    rs = np.random.RandomState(batch)
    nu, ni = 2500, 2100
    u, i, r = _random_graph(rs, nu, ni, 9, hot_items=5)
    graph = LaplacianCSR.from_interactions(u, i, r, nu, ni, device, heavy_threshold=128)
    bu, bp, bn = (torch.from_numpy(rs.randint(0, m, batch)).to(device) for m in (nu, ni, ni))
    plan = mngcf._subset_plan(graph, nu, 3, bu, bp, bn, fraction)
    assert sum(s is not None for s in plan) == subset_layers and all(s is None for s in plan[:3 - subset_layers])
    res = {}
    for frac in (fraction, 0.0):
        torch.manual_seed(5)
        model = NGCF(make_config("NGCF", embed_size=64, num_orders=3, device="cuda", model_dir=str(tmp_path),
                                 ngcf_subset_fraction=frac), nu, ni).to(device)
        pos, neg = model.bpr_forward(bu, bp, bn, graph)
        loss = BPRLoss()(pos, neg)
        loss.backward()
        single = model.forward(bu, bp, graph)
        model.check_indices()
        res[frac] = (pos.detach(), neg.detach(), loss.detach(), single.detach(),
                     {k: p.grad.detach().clone() for k, p in model.named_parameters()})
    a, b = res[fraction], res[0.0]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert torch.equal(a[3], a[0])                                   # forward(u, i) == bpr_forward's positive scores
    for k in a[4]:
        scale = float(b[4][k].abs().max())
        torch.testing.assert_close(a[4][k], b[4][k], rtol=2e-4, atol=2e-6 * scale, msg=lambda m: f"{k}: {m}")
    assert float(a[4]["embedding.weight"].abs().sum()) > 0


@pytest.mark.parametrize("batch,fraction,optimizer,layers,embed", [
    (24, 0.5, "adam", 3, 64), (700, 0.5, "adamw", 3, 64), (700, 0.0, "adam", 3, 64), (24, 1e9, "adam", 3, 64),
    # seven layers, the most yr_ngcf_bpr_step takes (K + 1 layer buffers <= YR_NGCF_MAX_LAYERS): 14 weight matrices
    # in the step's one multi-tensor Adam launch
    (24, 0.5, "adam", 7, 16),
    # batches of 8190, 8193, ... triplets: across the switch (B > 8192) from the loss finished by its one workgroup to
    # partials, the clearing of the unused partial slots and yr_loss_finalize
    (8190, 0.5, "adam", 2, 32)],
    ids=["24-0.5-adam", "700-0.5-adamw", "700-0.0-adam", "24-1000000000.0-adam", "24-0.5-adam-7x16",
         "8190-0.5-adam-2x32"])
def test_fused_step_equals_autograd_route(device, tmp_path, batch, fraction, optimizer, layers, embed):
    """ngcf_step.NGCFStep (yr_ngcf_bpr_step: every launch of the step issued from C) against the autograd route
    (bpr_forward, zero_grad, BPRLoss, backward, optimizer.step) over six steps on changing batches: the same
    kernels on the same data — per-step losses bit-identical on the first step and equal to rounding after, all
    parameters and both Adam moments equal to summation order, step counts equal; batch-aware propagation on
    (small and medium batch), off, and forced on every layer; Adam and AdamW (weight decay)."""
    from yelprecommendation_amd.graph import LaplacianCSR
    from yelprecommendation_amd.loss import BPRLoss
    from yelprecommendation_amd.models.ngcf import NGCF
    from yelprecommendation_amd.ngcf_step import NGCFStep
    from yelprecommendation_amd.optim import Adam, AdamW
    from yelprecommendation_amd.utils import make_config
    rs = np.random.RandomState(batch + 1)
    nu, ni = 2300, 1900
    u, i, r = _random_graph(rs, nu, ni, 9, hot_items=5)
    graph = LaplacianCSR.from_interactions(u, i, r, nu, ni, device, heavy_threshold=128)
    batches = [tuple(torch.from_numpy(rs.randint(0, m, batch + 3 * k)).to(device) for m in (nu, ni, ni)) for k in range(6)]
    batches[3] = tuple(t[:0] for t in batches[3])                    # an empty batch: a step with zero gradients
    out, first = {}, {}
    for route in ("fused", "autograd"):
        torch.manual_seed(8)
        cfg = make_config("NGCF", embed_size=embed, num_orders=layers, device="cuda", model_dir=str(tmp_path),
                          ngcf_subset_fraction=fraction)
        model = NGCF(cfg, nu, ni).to(device)
        with torch.no_grad():
            model.embedding.weight.mul_(0.1)
        opt = (AdamW(model.parameters(), lr=2e-3, weight_decay=0.05) if optimizer == "adamw"
               else Adam(model.parameters(), lr=2e-3))
        losses = []

        def snapshot():
            return ({k: p.detach().clone() for k, p in model.named_parameters()},
                    {k: (opt.state[p]["step"], opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
                     for k, p in model.named_parameters()})
        if route == "fused":
            step = NGCFStep(model, opt, graph, fraction)
            for j, (bu, bp, bn) in enumerate(batches):
                step.step(bu, bp, bn)
                losses.append(float(step.last_loss().item()))
                if j == 0:
                    first[route] = snapshot()
            step.check()
            assert abs(step.epoch_loss() - sum(losses)) <= 1e-6 * abs(sum(losses))
        else:
            for j, (bu, bp, bn) in enumerate(batches):
                if bu.numel() == 0:
                    # the reference's loop on an empty batch: mean of nothing; here: a step with zero gradients
                    for p in model.parameters():
                        p.grad = torch.zeros_like(p)
                    opt.step()
                    losses.append(0.0)
                    continue
                pos, neg = model.bpr_forward(bu, bp, bn, graph)
                opt.zero_grad()
                loss = BPRLoss()(pos, neg)
                loss.backward()
                opt.step()
                losses.append(float(loss.item()))
                if j == 0:
                    first[route] = snapshot()
        out[route] = (losses,) + snapshot()
    # after ONE step from the same parameters the two routes differ by the order of the float atomics only: the
    # moments (linear / quadratic in the gradients) agree to rounding of the summed terms; a parameter element
    # whose gradient is at the noise level may take its +-lr step in the other direction (m / sqrt(v) = +-1 at t = 1)
    (pa1, sa1), (pb1, sb1) = first["fused"], first["autograd"]
    for k in pa1:
        for which, a_, b_ in (("m", sa1[k][1], sb1[k][1]), ("v", sa1[k][2], sb1[k][2])):
            assert float((a_ - b_).norm()) <= 1e-5 * float(b_.norm()) + 1e-30, (which, k)
            assert float((a_ - b_).abs().max()) <= 1e-4 * float(b_.abs().max()) + 1e-30, (which, k)
        err = (pa1[k] - pb1[k]).abs()
        assert float((err <= 1e-6 + 1e-5 * pb1[k].abs()).float().mean()) >= 0.999, k
        assert float(err.max()) <= 2.1 * 2e-3, k
    # after six steps the trajectories have drifted by what those elements feed back: losses to 2e-5, step counts equal,
    # at least 99.8 % of every parameter tensor inside 2 % of the travel lr x steps, nothing beyond 10 % of it
    (la, pa, sa), (lb, pb, sb) = out["fused"], out["autograd"]
    np.testing.assert_allclose(la[0], lb[0], rtol=3e-7)     # the same scores; the batch mean summed in another order
    np.testing.assert_allclose(la, lb, rtol=2e-5)
    travel = 2e-3 * 6
    for k in pa:
        assert sa[k][0] == sb[k][0] == 6
        err = (pa[k] - pb[k]).abs()
        assert float((err <= 1e-3 * pb[k].abs() + 0.02 * travel).float().mean()) >= 0.998, k
        assert float(err.max()) <= 0.1 * travel, (k, float(err.max()))
        assert float((sa[k][1] - sb[k][1]).norm()) <= 2e-2 * float(sb[k][1].norm()) + 1e-30, k
