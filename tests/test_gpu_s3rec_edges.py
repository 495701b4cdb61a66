"""The linear pieces of csrc/s3rec.hip and engine.s3rec_param_grads at the ends of their loops: both score forms, the
score gradient and the item gradient through the C ABI, the weight-gradient products and column sums through
``engine.s3rec_param_grads`` — each compared with tests/s3rec_edges_ref64.py (float64) over EVERY element: inside the
bar the reference derives on random inputs, EQUAL to float64 on the certified exact inputs, no agreement quotas.
Outputs live in sentinel-filled buffers with 256-float guard bands (``partial`` too: its bands alone are asserted); the
deterministic pieces run twice and must be bit-equal; rows of the item table without a lookup keep their bits.  The
helper's restatement of the packed layout is tied to the engine's on a workspace the fused kernels left, and the
sequence loop of the three fused kernels takes its second trip at 2^20 + 3 sequences.  tests/
test_s3rec_edges_ref64.py proves without a GPU that every case reaches its loop end and that these checks notice a
lost product, lookup, chunk share, trip, row or partial."""
import types

import numpy as np
import pytest
import torch

import s3rec_edges_ref64 as R
import s3rec_grad_ref64 as gr
import s3rec_ref64 as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
S = R.SENTINEL
G = R.GUARD
WORST = {}
KINDS = pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])


def _ids(cases):
    return [c["id"] for c in cases]


def _note(family, value):
    WORST[family] = max(WORST.get(family, 0.0), float(value))


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _np(t):
    return t.detach().cpu().numpy()


def _lib():
    from yelprecommendation_amd import _lib as L
    return L.load()


def _stream():
    from yelprecommendation_amd import engine
    return engine._stream()


class Guarded:
    """A sentinel-filled flat f32 buffer: G floats, n floats, G floats; ``ptr`` addresses element 0."""

    def __init__(self, n, device, fill=None):
        self.n = n
        self.flat = torch.full((2 * G + n,), S, dtype=torch.float32, device=device)
        self.view = self.flat[G:G + n]
        if fill is not None:
            self.view.copy_(_t(np.asarray(fill, F32).reshape(-1), device))
        self.ptr = self.flat.data_ptr() + 4 * G

    def bands(self, what):
        assert bool((self.flat[:G] == S).all()) and bool((self.flat[G + self.n:] == S).all()), (what, "a guard band was written")

    def read(self, what):
        self.bands(what)
        return _np(self.view)


def _same(got, o, family, q=None):
    """got == the reference: exactly where a certificate quantum is given, inside the bar otherwise."""
    got = np.asarray(got, np.float64).reshape(o.v.shape)
    if q is not None:
        assert R.exact(q, o.s), (family, q)
        bad = np.flatnonzero((got != o.v).reshape(-1))
        assert bad.size == 0, (family, "differs from float64 at", bad[:8], got.reshape(-1)[bad[:8]], o.v.reshape(-1)[bad[:8]])
        return
    r = R.ratio(got, o)
    _note(family, r)
    assert r < 1.0, (family, r)


_TABLES = {}


def _table(E, exact, device):
    if (E, exact) not in _TABLES:
        _TABLES[(E, exact)] = _t(np.array(R.table_of(E, exact)), device)        # a copy: the shared table is read-only
    return _TABLES[(E, exact)]


def _flag(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


# ---- scores ---------------------------------------------------------------------------------------------------------

@KINDS
@pytest.mark.parametrize("case", R.SEQ_CASES, ids=_ids(R.SEQ_CASES))
def test_seq_scores(device, case, exact):
    g = R.gen_seq(case, exact)
    rows, E, N = case["rows"], case["E"], g["num_items"]
    a, b, want = R.scores(g["table"], g["h"], g["pos"], 1, g["neg"], 1, N)
    table, h, pos, neg = _table(E, exact, device), _t(g["h"], device), _t(g["pos"], device), _t(g["neg"], device)
    assert table.shape == (N + 1, E) and h.shape == (rows, E) and pos.numel() == neg.numel() == rows
    oa, ob, flag = Guarded(rows, device), Guarded(rows, device), _flag(device)
    status = _lib().yr_s3rec_seq_scores(table.data_ptr(), h.data_ptr(), pos.data_ptr(), neg.data_ptr(), rows, E, N, oa.ptr,
                                        ob.ptr, flag.data_ptr(), _stream())
    assert status == 0 and int(flag.item()) == want == (R.FLAG_BAD_ITEM if case["bad"] else 0)
    q = R.certificate("scores", g) if exact else None
    _same(oa.read(case["id"]), a, "seq scores", q)
    _same(ob.read(case["id"]), b, "seq scores", q)
    assert (ob.read(case["id"])[~R._ok(g["neg"], N)] == 0).all()


@KINDS
@pytest.mark.parametrize("case", R.CAND_CASES, ids=_ids(R.CAND_CASES))
def test_candidate_scores(device, case, exact):
    g = R.gen_cand(case, exact)
    B, C, E, N = case["B"], case["C"], case["E"], g["num_items"]
    a, b, want = R.scores(g["table"], g["h"], g["pos"], 1, g["cand"], C, N)
    table, h, pos, cand = _table(E, exact, device), _t(g["h"], device), _t(g["pos"], device), _t(g["cand"], device)
    assert table.shape == (N + 1, E) and h.shape == (B, E) and pos.numel() == B and cand.shape == (B, C)
    oa, ob, flag = Guarded(B, device), Guarded(B * C, device), _flag(device)
    status = _lib().yr_s3rec_candidate_scores(table.data_ptr(), h.data_ptr(), pos.data_ptr(), cand.data_ptr(), B, C, E, N,
                                              oa.ptr, ob.ptr, flag.data_ptr(), _stream())
    assert status == 0 and int(flag.item()) == want == (R.FLAG_BAD_ITEM if case["bad"] else 0)
    q = R.certificate("scores", g) if exact else None
    _same(oa.read(case["id"]), a, "candidate scores", q)
    _same(ob.read(case["id"]), b, "candidate scores", q)
    if case["bad"]:
        assert ob.read(case["id"])[-1] == 0


@KINDS
@pytest.mark.parametrize("case", R.SCORE_GRAD_CASES, ids=_ids(R.SCORE_GRAD_CASES))
def test_score_grad(device, case, exact):
    g = R.gen_score_grad(case, exact)
    rows, E, N = case["rows"], case["E"], g["num_items"]
    o, want = R.score_grad(g["table"], g["pos"], g["neg"], g["dpos"], g["dneg"], N)
    table, pos, neg = _table(E, exact, device), _t(g["pos"], device), _t(g["neg"], device)
    dpos, dneg = _t(g["dpos"], device), _t(g["dneg"], device)
    assert table.shape == (N + 1, E) and pos.numel() == neg.numel() == dpos.numel() == dneg.numel() == rows
    out, flag = Guarded(rows * E, device), _flag(device)
    status = _lib().yr_s3rec_score_grad(table.data_ptr(), pos.data_ptr(), neg.data_ptr(), dpos.data_ptr(), dneg.data_ptr(),
                                        rows, E, N, out.ptr, flag.data_ptr(), _stream())
    assert status == 0 and int(flag.item()) == want == (0 if case["bad"] == "none" else R.FLAG_BAD_ITEM)
    _same(out.read(case["id"]), o, "score_grad", R.certificate("score_grad", g) if exact else None)


# ---- the item gradient ----------------------------------------------------------------------------------------------

@KINDS
@pytest.mark.parametrize("case", R.ITEM_CASES, ids=_ids(R.ITEM_CASES))
def test_item_grad(device, case, exact):
    """Onto a non-zero d_item0; the C ABI on the test's own stable sort into guarded buffers, then
    engine.s3rec_item_grad (its own sort and ``partial``): bit-equal."""
    from yelprecommendation_amd import engine
    g = R.gen_item(case, exact)
    rows, E, T, N = case["rows"], case["E"], case["T"], g["num_items"]
    o, touched, want = R.item_grad(g["X"], g["pos"], g["neg"], g["d_emb"], g["h"], g["dpos"], g["dneg"], g["d_item0"], N)
    d = {k: _t(g[k], device) for k in ("X", "pos", "neg", "d_emb", "h", "dpos", "dneg")}
    sorted_ids, order = torch.sort(torch.cat([d["X"], d["pos"], d["neg"]]), stable=True)
    sid, perm = R.sort_lookups(g["X"], g["pos"], g["neg"])
    assert np.array_equal(_np(sorted_ids), sid) and np.array_equal(_np(order), perm)
    assert sorted_ids.numel() == order.numel() == 3 * rows and d["d_emb"].shape == d["h"].shape == (rows, E)
    assert g["d_item0"].shape == (T, E) and N == T - 1 and d["dpos"].numel() == d["dneg"].numel() == rows
    d_item, partial, flag = Guarded(T * E, device, fill=g["d_item0"]), Guarded(3 * rows * E, device), _flag(device)
    status = _lib().yr_s3rec_item_grad(sorted_ids.data_ptr(), order.data_ptr(), d["d_emb"].data_ptr(), d["h"].data_ptr(),
                                       d["dpos"].data_ptr(), d["dneg"].data_ptr(), rows, E, N, partial.ptr, d_item.ptr,
                                       flag.data_ptr(), _stream())
    assert status == 0 and int(flag.item()) == want == (R.FLAG_BAD_ITEM if case["family"] == "bad" else 0)
    partial.bands(case["id"])
    got = d_item.read(case["id"]).reshape(T, E)
    assert np.array_equal(got[~touched], g["d_item0"][~touched]), "a row without a lookup was written"
    assert (~touched).sum() == R.plan_item(sid, N)["absent"]
    _same(got, o, "item_grad", R.certificate("item_grad", g) if exact else None)
    again, flag2 = _t(g["d_item0"], device), _flag(device)
    engine.s3rec_item_grad(d["X"], d["pos"], d["neg"], d["d_emb"], d["h"], d["dpos"], d["dneg"], again, err_flag=flag2)
    assert np.array_equal(_np(again), got) and int(flag2.item()) == want


# ---- the weight gradients -------------------------------------------------------------------------------------------

@KINDS
@pytest.mark.parametrize("case", R.PARAM_CASES, ids=_ids(R.PARAM_CASES))
def test_param_grads(device, case, exact):
    """engine.s3rec_param_grads on a generated workspace into the sentinel-filled packed buffer, twice (bit-equal);
    the cases whose chunk products go to the side streams once more under a non-default current stream, the
    workspace filled on that stream immediately before the call."""
    from yelprecommendation_amd import engine
    B, L, E, heads, blocks = (case[k] for k in ("B", "L", "E", "heads", "blocks"))
    g = R.gen_workspace(case, exact)
    o = R.param_grads(R.workspace_views(g["ws"], B * L, E, heads, blocks), B, L, E, heads, blocks)
    ws = _t(g["ws"], device)
    assert ws.numel() == engine.s3rec_train_workspace_floats(B, L, E, heads, blocks)
    n = blocks * engine.s3rec_block_floats(E, heads)
    out = Guarded(n, device)
    engine.s3rec_param_grads(ws, B, L, E, heads, blocks, out=out.view)
    got = out.read(case["id"])
    _same(got, o, "param_grads", R.certificate("param_grads", g) if exact else None)
    out2 = Guarded(n, device)
    engine.s3rec_param_grads(ws, B, L, E, heads, blocks, out=out2.view)
    assert np.array_equal(out2.read(case["id"]), got)
    if R.plan_param_grads(B, L, heads, blocks)["streams"]:
        st = torch.cuda.Stream(device)
        out3 = Guarded(n, device)
        stale = torch.full_like(ws, float("nan"))
        torch.cuda.synchronize(device)
        with torch.cuda.stream(st):
            stale.copy_(ws, non_blocking=True)              # the producer of the workspace, on the current stream
            engine.s3rec_param_grads(stale, B, L, E, heads, blocks, out=out3.view)
        st.synchronize()
        assert np.array_equal(out3.read(case["id"]), got)


def _cfg(E, L, heads, blocks):
    return types.SimpleNamespace(embed_size=E, max_seq_len=L, num_heads=heads, num_blocks=blocks, dropout_ratio=0.0,
                                 device="cuda")


def _model(params, case, device):
    from yelprecommendation_amd.models.s3rec import S3Rec
    model = S3Rec(_cfg(case["E"], case["L"], case["heads"], case["blocks"]), params["item_embedding.weight"].shape[0] - 1,
                  params["attribute_embedding.weight"].shape[0])
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}, strict=True)
    return model.to(device)


def test_layout_tie(device):
    """The workspace that yr_s3rec_encode_train + yr_s3rec_backward left, read back and passed through the helper's
    param_grads in float64, gives the engine's packed gradient within the closed-form bar: the whole-step tests pin the
    engine's layout against torch, this pins the helper's restatement to the engine's."""
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.loss import BPRLoss
    case = next(c for c in ref.CASES if (c["E"], c["L"], c["heads"], c["blocks"]) == (32, 33, 2, 2))
    E, L, B, heads, blocks = case["E"], case["L"], case["B"], case["heads"], case["blocks"]
    params, batch = gr.case_setup(case)
    t = {k: torch.from_numpy(v).to(device) for k, v in batch.items()}
    model = _model(params, case, device)
    table, pos_enc, packed = model.item_embedding.weight.detach(), model.positional_encoding.detach(), model._params()
    h, ws = engine.s3rec_encode_train(table, pos_enc, packed, t["X"], heads, blocks)
    pos, neg = engine.s3rec_seq_scores(table, h, t["pos_items"], t["neg_items"])
    pos, neg = pos.requires_grad_(), neg.requires_grad_()
    BPRLoss()(pos, neg).backward()
    dh = engine.s3rec_score_grad(table, t["pos_items"], t["neg_items"], pos.grad, neg.grad)
    engine.s3rec_backward(packed, t["X"], dh.view(B, L, E), ws, heads, blocks)
    got = _np(engine.s3rec_param_grads(ws, B, L, E, heads, blocks))
    o = R.param_grads(R.workspace_views(_np(ws), B * L, E, heads, blocks), B, L, E, heads, blocks)
    assert np.abs(o.v).max() > 0
    _same(got, o, "layout tie")


# ---- the sequence loop of the fused kernels -------------------------------------------------------------------------

def test_fused_kernels_second_trip_of_the_sequence_loop(device):
    """B = 2^20 + 3 sequences at L = 1, E = 16, one head, one block, p = 0: the rows on both sides of the grid cap equal
    the same sequences encoded in a batch of four (yr_s3rec_encode, both forms) and alone (yr_s3rec_encode_train,
    yr_s3rec_backward: d_emb), bit for bit; at L = 1 a row is a function of its id alone, so every row is compared with
    the encoding of its id.  The training workspace is 324 floats per row, 1.4 GB: allocated once, freed here."""
    from yelprecommendation_amd import engine
    case = dict(E=16, L=1, heads=1, blocks=1)
    B, E, N = R.FUSED_B, 16, ref.NUM_ITEMS
    assert R.plan_fused(B)["trips"] == 2
    model = _model(ref.make_params(16, 1, 1, 1, seed=3), case, device)
    table, pos_enc, packed = model.item_embedding.weight.detach(), model.positional_encoding.detach(), model._params()
    gen = torch.Generator(device="cpu").manual_seed(11)
    X = torch.randint(0, N + 1, (B, 1), generator=gen).to(device)
    rows = torch.tensor(R.FUSED_ROWS, device=device)
    every_id = torch.arange(N + 1, device=device).view(-1, 1)
    for last_only in (False, True):
        shape = (B, E) if last_only else (B, 1, E)
        buf = Guarded(B * E, device)
        engine.s3rec_encode(table, pos_enc, packed, X, 1, 1, last_only=last_only, out=buf.view.view(shape))
        buf.bands(f"encode last_only={last_only}")
        four = engine.s3rec_encode(table, pos_enc, packed, X[rows].contiguous(), 1, 1, last_only=last_only)
        out = buf.view.view(B, E)
        assert torch.equal(out[rows], four.view(4, E))
        per_id = engine.s3rec_encode(table, pos_enc, packed, every_id, 1, 1, last_only=last_only).view(N + 1, E)
        assert torch.equal(out, per_id[X[:, 0]])
        del buf, out
    n_ws = engine.s3rec_train_workspace_floats(B, 1, E, 1, 1)
    assert n_ws == B * 324
    wbuf = Guarded(n_ws, device)
    hbuf, dbuf = Guarded(B * E, device), Guarded(B * E, device)
    h, d_emb = hbuf.view.view(B, 1, E), dbuf.view.view(B, 1, E)
    engine.s3rec_encode_train(table, pos_enc, packed, X, 1, 1, workspace=wbuf.view, out=h)
    dh = torch.randn((B, 1, E), generator=torch.Generator(device="cpu").manual_seed(12)).to(device)
    engine.s3rec_backward(packed, X, dh, wbuf.view, 1, 1, d_emb=d_emb)
    for b in (wbuf, hbuf, dbuf):
        b.bands("training")
    assert torch.equal(h.view(B, E), per_id[X[:, 0]])
    for r in R.FUSED_ROWS:
        X1 = X[r:r + 1].contiguous()
        h1, ws1 = engine.s3rec_encode_train(table, pos_enc, packed, X1, 1, 1)
        d1 = engine.s3rec_backward(packed, X1, dh[r:r + 1].contiguous(), ws1, 1, 1)
        assert torch.equal(h[r], h1[0]) and torch.equal(d_emb[r], d1[0]), r
    del wbuf, hbuf, dbuf, h, d_emb, dh
    torch.cuda.empty_cache()


def test_zz_report_worst_ratios():
    """Not a check of its own: prints the largest |err| / bar per family seen by the tests above."""
    print("S3Rec edges, max |err| / bar on random inputs:", {k: float("%.3g" % v) for k, v in sorted(WORST.items())})
    assert all(v < 1.0 for v in WORST.values())
