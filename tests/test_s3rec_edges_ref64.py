"""tests/s3rec_edges_ref64.py, the float64 reference of the linear pieces around the fused S3Rec kernels, checked
without a GPU: it equals torch float64 autograd on a small case; its constants are the sources'; every case of
tests/test_gpu_s3rec_edges.py reaches the loop end it is there for (asserted through ``plan_*``, per case and as a
covering set); every "exact" case holds its certificate, computed from the generated arrays; and the bars the helper
states notice what a kernel that mishandles the end of a round, a trip, a run, a chunk or a stream deal would compute
— or, where the any-order bar of a long sum cannot, the exact twin of the same case does (asserted pairing; a short
sum, n <= 136, must cross on the random inputs)."""
import functools

import numpy as np
import pytest
import torch

import s3rec_edges_ref64 as R

F32 = np.float32
SHORT = 136
SMALLEST = {}


def _note(family, value):
    SMALLEST[family] = min(SMALLEST.get(family, np.inf), float(value))


# ---- the helper against autograd ------------------------------------------------------------------------------------

def test_reference_equals_torch_float64_autograd():
    """rows = 40, E = 16, 30 items: with table and h as leaves and loss = sum w_pos pos + w_neg neg + sum table[X] * G,
    table.grad is item_grad (G in the role of d_emb, onto zeros) and h.grad is score_grad."""
    rs = np.random.RandomState(5)
    rows, E, N = 40, 16, 30
    table, h, G = (rs.standard_normal(s) for s in ((N + 1, E), (rows, E), (rows, E)))
    X, pos, neg = (rs.randint(0, N + 1, rows) for _ in range(3))
    wp, wn = rs.standard_normal(rows), rs.standard_normal(rows)
    tt, th = torch.tensor(table, requires_grad=True), torch.tensor(h, requires_grad=True)
    sp, sn = (tt[torch.as_tensor(pos)] * th).sum(1), (tt[torch.as_tensor(neg)] * th).sum(1)
    loss = (torch.tensor(wp) * sp).sum() + (torch.tensor(wn) * sn).sum() + (tt[torch.as_tensor(X)] * torch.tensor(G)).sum()
    loss.backward()
    a, b, flag = R.scores(table, h, pos, 1, neg, 1, N)
    assert flag == 0
    np.testing.assert_allclose(a.v, sp.detach().numpy(), rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(b.v, sn.detach().numpy(), rtol=1e-13, atol=1e-14)
    d_item, touched, flag = R.item_grad(X, pos, neg, G, h, wp, wn, np.zeros((N + 1, E)), N)
    assert flag == 0 and touched.sum() == np.unique(np.r_[X, pos, neg]).size
    np.testing.assert_allclose(d_item.v, tt.grad.numpy(), rtol=1e-13, atol=1e-13)
    assert (d_item.v[~touched] == 0).all()
    dh, flag = R.score_grad(table, pos, neg, wp, wn, N)
    assert flag == 0
    np.testing.assert_allclose(dh.v, th.grad.numpy(), rtol=1e-13, atol=1e-14)
    # the candidate form is the same dot product with h row r // C, and a bad id leaves its lookup out
    C = 7
    cand = rs.randint(0, N + 1, (rows, C))
    _, c, _ = R.scores(table, h, pos, 1, cand, C, N)
    np.testing.assert_allclose(c.v.reshape(rows, C), np.einsum("rce,re->rc", table[cand], h), rtol=1e-13, atol=1e-14)
    X2 = X.copy()
    X2[3] = N + 1
    d2, _, flag = R.item_grad(X2, pos, neg, G, h, wp, wn, np.zeros((N + 1, E)), N)
    G0 = G.copy()
    G0[3] = 0
    d3, _, _ = R.item_grad(X, pos, neg, G0, h, wp, wn, np.zeros((N + 1, E)), N)
    assert flag == R.FLAG_BAD_ITEM and np.allclose(d2.v, d3.v, rtol=1e-13, atol=1e-13)


def test_packed_gradient_equals_autograd_of_the_products():
    """param_grads places d(loss)/d(packed) of loss = sum over blocks of <delta W-products, stash> at the offsets of
    engine.s3rec_param_grads: checked on weights that enter linearly, y = stash W^T + b against the deltas."""
    rs = np.random.RandomState(6)
    B, L, E, H, blocks = 5, 3, 16, 2, 2
    Rr = B * L
    ws = rs.standard_normal(R.workspace_floats(Rr, E, H, blocks))
    views = R.workspace_views(ws, Rr, E, H, blocks)
    got = R.param_grads(views, B, L, E, H, blocks).v
    packed = torch.zeros(blocks * R.block_floats(E, H), dtype=torch.float64, requires_grad=True)
    t = lambda a: torch.tensor(np.ascontiguousarray(a))          # noqa: E731
    loss, at = 0.0, 0

    def take(n):
        nonlocal at
        at += n
        return packed[at - n:at]

    for v in views:
        Wqkv, Wo, bo, g1, b1_ = take(3 * H * E * E).view(3 * H * E, E), take(E * H * E).view(E, H * E), take(E), take(E), take(E)
        W1, b1, W2, b2, g2, b2_ = take(E * E).view(E, E), take(E), take(E * E).view(E, E), take(E), take(E), take(E)
        loss = loss + (t(v["dqkv"]) * (t(v["h_in"]) @ Wqkv.T)).sum() + (t(v["d1m"]) * (t(v["A"]) @ Wo.T + bo)).sum()
        loss = loss + (t(v["gx1"]) * g1).sum() + (t(v["g1"]) * b1_).sum() + (t(v["dz1"]) * (t(v["x1"]) @ W1.T + b1)).sum()
        loss = loss + (t(v["d2m"]) * (t(v["relu"]) @ W2.T + b2)).sum() + (t(v["gx2"]) * g2).sum() + (t(v["g2"]) * b2_).sum()
    assert at == packed.numel()
    loss.backward()
    np.testing.assert_allclose(got, packed.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_geometry_mirrors_the_sources():
    c = R.source_constants()
    assert (c["kItemChunk"], c["kBlock"], c["kWave"], c["YR_LOSS_PARTIALS"], c["LPR"]) == (256, 256, 64, 2048, 16)
    assert (c["S3REC_GRAD_CHUNK_ROWS"], c["S3REC_GRAD_STREAM_JOBS"]) == (2048, 16)
    assert (R.ROUND_ROWS, R.SCORE_SPAN, R.GRAD_SPAN, R.WAVE_SPAN, R.SEQ_GRID) == (16, 32768, 524288, 8192, 1 << 20)
    from yelprecommendation_amd import engine
    assert engine.S3REC_GRAD_CHUNK_ROWS == R.CHUNK_ROWS and engine.S3REC_GRAD_STREAM_JOBS == R.STREAM_JOBS
    assert engine._S3REC_WS_ARRAYS == R.WS_ARRAYS
    assert engine.s3rec_block_floats(32, 2) == R.block_floats(32, 2)


# ---- every case reaches its loop end --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _item_plan(index):
    case = R.ITEM_CASES[index]
    X, pos, neg = R.ids_from_runs(case["runs"], case["rows"], np.random.RandomState(case["seed"]))
    sid, order = R.sort_lookups(X, pos, neg)
    return R.plan_item(sid, case["T"] - 1), sid, order


def test_score_cases_reach_their_loop_ends():
    rows = [c["rows"] for c in R.SEQ_CASES if c["E"] == 16]
    assert rows == [1, 15, 16, 17, 16383, 16384, 16385]
    for E in R.WIDTHS:
        plans = [R.plan_scores(c["rows"], c["rows"]) for c in R.SEQ_CASES if c["E"] == E]
        assert [p["rounds"] for p in plans] == [1, 2, 2, 3, 2048, 2048, 2049]
        assert [p["trips"] for p in plans] == [1, 1, 1, 1, 1, 1, 2]
        assert [p["seam"] for p in plans] == [True, True, False, True, True, False, True]
        assert [p["grid"] for p in plans][-3:] == [2048, 2048, 2048]
    for c in R.SEQ_CASES:                                # the bad ids of a case sit in list b's last rows
        g = R.gen_seq(c, True)
        assert (0 in g["pos"] or 0 in g["neg"]) and g["num_items"] in g["pos"] and g["table"].shape[0] == 40000
        bad = ~R._ok(g["neg"], g["num_items"])
        assert bad.any() == c["bad"] and R._ok(g["pos"], g["num_items"]).all()
        if c["bad"] and c["rows"] >= 16:
            assert set(g["neg"][bad]) == {-1, g["num_items"] + 1, R.BIG}
            p = R.plan_scores(c["rows"], c["rows"])
            assert bad[-1] and 2 * c["rows"] - 1 >= (p["rounds"] - 1) * R.ROUND_ROWS
    assert {(c["B"], c["C"]) for c in R.CAND_CASES} == {(B, C) for B in (1, 3, 17) for C in (1, 2, 15, 16, 17, 99, 100)} | {(331, 99)}
    for c in R.CAND_CASES:
        p = R.plan_scores(c["B"], c["B"] * c["C"])
        assert p["trips"] == (2 if c["B"] == 331 else 1) and p["seam"]
        g = R.gen_cand(c, True)
        assert (g["cand"][-1, -1] == g["num_items"] + 1) == c["bad"]
    assert R.plan_scores(331, 331 * 99)["rows"] == 33100 > R.SCORE_SPAN
    assert {c["E"] for c in R.CAND_CASES} == set(R.WIDTHS)
    # the last round of the candidate cases: full, one row, and in between
    assert {R.plan_scores(c["B"], c["B"] * c["C"])["last_round"] for c in R.CAND_CASES} >= {1, 2, 16}


def test_score_grad_cases_reach_their_loop_ends():
    for E in (16, 128):
        cs = [c for c in R.SCORE_GRAD_CASES if c["E"] == E]
        assert [c["rows"] * E for c in cs] == [E, 524288 - E, 524288, 524288 + E, 2 * 524288 + E]
        assert [R.plan_score_grad(c["rows"], E)["trips"] for c in cs] == [1, 1, 1, 2, 3]
    assert {c["E"] for c in R.SCORE_GRAD_CASES} == set(R.WIDTHS)
    assert {c["bad"] for c in R.SCORE_GRAD_CASES} == {"none", "pos", "neg", "both"}
    for c in R.SCORE_GRAD_CASES:
        g = R.gen_score_grad(c, True)
        okp, okn = R._ok(g["pos"], g["num_items"]).all(), R._ok(g["neg"], g["num_items"]).all()
        assert (not okp, not okn) == (c["bad"] in ("pos", "both"), c["bad"] in ("neg", "both"))


def test_item_cases_reach_their_loop_ends():
    plans = {c["id"]: _item_plan(i)[0] for i, c in enumerate(R.ITEM_CASES)}
    small = [c for c in R.ITEM_CASES if c["family"] not in ("bad", "second-trip")]
    for c in R.ITEM_CASES:
        p = plans[c["id"]]
        assert p["n"] == 3 * c["rows"] and p["chunks"] == -(-p["n"] // 256)
        assert [tuple(r) for r in p["runs"].tolist()] == \
            [(i, lo, lo + k) for (i, k), lo in zip(c["runs"], np.r_[0, np.cumsum([r[1] for r in c["runs"]])[:-1]].tolist())]
        assert p["combine_trips"] == -(-c["T"] // 8192) and p["partial_trips"] == (2 if c["family"] == "second-trip" else 1)
        if c["T"] >= 8191:
            assert p["absent"] >= c["T"] - 5 or c["family"] == "second-trip" and p["absent"] == c["T"] - 3000
    # the covering sets
    assert {c["E"] for c in small} == set(R.WIDTHS) and {c["T"] for c in small} == {1, 4, 5, 8191, 8192, 8193, 8194, 40000}
    assert {c["rows"] for c in small} == {1, 85, 86, 171, 256, 257}
    assert {plans[c["id"]]["n"] for c in small} == {3, 255, 258, 513, 768, 771}
    lengths = set(np.concatenate([plans[c["id"]]["lengths"] for c in small]).tolist())
    assert lengths >= {1, 2, 255, 256, 257, 511, 512, 513, 769}
    used = set(np.concatenate([plans[c["id"]]["runs"][:, 0] for c in R.ITEM_CASES]).tolist())
    assert used >= {0, 8191, 8192, 8193, 39999, -1, 5, 8194, 40000, R.BIG}
    assert {plans[c["id"]]["combine_trips"] for c in small} == {1, 2, 5}
    for E in R.WIDTHS:
        mine = [plans[c["id"]] for c in small if c["E"] == E]
        assert any(p["ends_at_chunk_end"] for p in mine) and any(p["starts_on_chunk_last"] for p in mine)
        assert any(p["whole_middle_chunk"] for p in mine) and any(p["last_chunk"] == 1 for p in mine)
        assert {p["n"] for p in mine if p["one_id"]} == {3, 255, 258, 513, 768, 771}          # every position padded
        assert max(p["runs_per_chunk"].max() for p in mine) >= 3 and max(p["spans"].max() for p in mine) == 4
    # what single layouts are there for
    by = lambda name, E=16: next(plans[c["id"]] for c in R.ITEM_CASES if c["family"] == name and c["E"] == E)      # noqa: E731
    p = by("n771-255+513+3")
    assert p["runs"][1].tolist()[1:] == [255, 768] and p["spans"][1] == 3          # starts on a chunk's last lookup,
    #                                                                              covers chunk 1, ends at a chunk end
    assert by("n513-512+1")["last_chunk"] == 1 and by("n513-512+1")["runs"][1].tolist()[1:] == [512, 513]
    assert by("n513-1+512")["runs"][1].tolist()[1:] == [1, 513]                   # a run that ends in the one-lookup chunk
    assert by("n771-2+769")["spans"].tolist() == [1, 4] and by("n771-769+2")["spans"].tolist() == [4, 1]
    assert by("n258-257+1")["runs"][0].tolist()[1:] == [0, 257]
    for c in R.ITEM_CASES:
        if c["family"] == "bad":
            p = plans[c["id"]]
            assert p["bad_front"] > 0 and p["bad_back"] == 2 and p["runs"][1, 0] == 0 and p["runs"][0, 0] == -1
    big = plans[R.ITEM_CASES[-1]["id"]]
    assert (big["n"], big["chunks"], big["last_chunk"]) == (2097153, 8193, 1) and big["lengths"].max() == 1000001
    assert big["runs"][-1].tolist() == [39999, 2097151, 2097153] and big["spans"][-1] == 2 and big["max_id"] == 39999


def test_param_cases_reach_their_loop_ends():
    plans = {c["id"]: R.plan_param_grads(c["B"], c["L"], c["heads"], c["blocks"]) for c in R.PARAM_CASES}
    first = [c for c in R.PARAM_CASES if (c["E"], c["heads"], c["blocks"]) == (16, 1, 1)]
    assert [(c["B"] * c["L"], c["L"]) for c in first] == [(1, 1), (2047, 23), (2048, 32), (2049, 3), (2049, 1), (4096, 64),
                                                         (4097, 17), (6145, 5)]
    assert [plans[c["id"]]["pieces"] for c in first] == [4, 4, 4, 8, 8, 8, 12, 16]
    assert [plans[c["id"]]["streams"] for c in first] == [False] * 7 + [True]
    assert [plans[c["id"]]["last_chunk"][0] for c in first] == [1, 2047, 2048, 1, 1, 2048, 1, 1]
    rest = [c for c in R.PARAM_CASES if c not in first]
    assert [(c["B"] * c["L"], c["E"], c["heads"], c["blocks"]) for c in rest] == [(100, 32, 2, 3), (100, 32, 2, 4), (2049, 128, 4, 1)]
    assert [(plans[c["id"]]["pieces"], plans[c["id"]]["streams"]) for c in rest] == [(12, False), (16, True), (8, False)]
    assert R.plan_fused(R.FUSED_B) == dict(grid=1 << 20, trips=2) and R.plan_fused(R.SEQ_GRID)["trips"] == 1
    assert [r // R.SEQ_GRID for r in R.FUSED_ROWS] == [0, 0, 1, 1] and R.FUSED_ROWS[-1] == R.FUSED_B - 1


# ---- certificates ---------------------------------------------------------------------------------------------------

def _seq_ref(c, exact, variant=None):
    g = R.gen_seq(c, exact)
    a, b, flag = R.scores(g["table"], g["h"], g["pos"], 1, g["neg"], 1, g["num_items"], variant)
    return g, R.Out(np.r_[a.v, b.v], np.r_[a.n, b.n], np.r_[a.s, b.s]), flag


def _cand_ref(c, exact, variant=None):
    g = R.gen_cand(c, exact)
    a, b, flag = R.scores(g["table"], g["h"], g["pos"], 1, g["cand"], c["C"], g["num_items"], variant)
    return g, R.Out(np.r_[a.v, b.v], np.r_[a.n, b.n], np.r_[a.s, b.s]), flag


def _grad_ref(c, exact, variant=None):
    g = R.gen_score_grad(c, exact)
    o, flag = R.score_grad(g["table"], g["pos"], g["neg"], g["dpos"], g["dneg"], g["num_items"], variant)
    return g, o, flag


@functools.lru_cache(maxsize=2)
def _item_inputs(index, exact):
    return R.gen_item(R.ITEM_CASES[index], exact)


def _item_ref(c, exact, weight=None, variant=None):
    g = _item_inputs(R.ITEM_CASES.index(c), exact)
    o, touched, flag = R.item_grad(g["X"], g["pos"], g["neg"], g["d_emb"], g["h"], g["dpos"], g["dneg"], g["d_item0"],
                                   g["num_items"], weight, variant)
    return g, o, flag


def _param_ref(c, exact, weight=None, swap=None):
    g = R.gen_workspace(c, exact)
    Rr = c["B"] * c["L"]
    views = R.workspace_views(g["ws"], Rr, c["E"], c["heads"], c["blocks"])
    return g, R.param_grads(views, c["B"], c["L"], c["E"], c["heads"], c["blocks"], weight, swap), 0


def test_every_exact_case_holds_its_certificate():
    count, fullest = 0, 0.0
    for kind, cases, ref in (("scores", R.SEQ_CASES, _seq_ref), ("scores", R.CAND_CASES, _cand_ref),
                             ("score_grad", R.SCORE_GRAD_CASES, _grad_ref), ("item_grad", R.ITEM_CASES, _item_ref),
                             ("param_grads", R.PARAM_CASES, _param_ref)):
        for c in cases:
            g, o, _ = ref(c, True)
            q = R.certificate(kind, g)
            assert R.exact(q, o.s), (kind, c["id"], q, o.s.max())
            assert R.quantum(o.v) >= q                      # the float64 value is a multiple of the quantum itself
            assert np.array_equal(o.v.astype(F32).astype(np.float64), o.v)
            fullest = max(fullest, float(o.s.max()) / q)
            count += 1
    print(f"{count} certificates, the fullest uses {fullest:.3g} of the 2^24 = {2 ** 24} quanta")
    assert count == len(R.SEQ_CASES) + len(R.CAND_CASES) + len(R.SCORE_GRAD_CASES) + len(R.ITEM_CASES) + len(R.PARAM_CASES)


# ---- perturbed references -------------------------------------------------------------------------------------------

_KEPT = {}


def _unperturbed(ref, case, exact):
    """The reference of a case, kept while the perturbations of that case are judged."""
    key = (ref.__name__, case["id"], exact)
    if key not in _KEPT:
        for k in [k for k in _KEPT if k[:2] != key[:2]]:
            del _KEPT[k]
        _KEPT[key] = ref(case, exact)[1]
    return _KEPT[key]


def _judge(family, name, ref, case, kwargs):
    """The pairing: the perturbed reference crosses the bar computed from the reference alone on the random inputs, or
    the exact twin of the same case differs; a short sum must cross."""
    o = _unperturbed(ref, case, False)
    _, pert, _ = ref(case, False, **kwargs)
    differs = pert.v != o.v
    assert differs.any(), (family, name, case["id"], "the perturbation changes nothing")
    r = R.ratio(pert.v, o)
    _note(f"{family}: {name}", r)
    if r > 1.0:
        return r
    assert float(o.n[differs].max()) > SHORT, (family, name, case["id"], r, "a short sum must cross on random inputs")
    oe = _unperturbed(ref, case, True)
    _, pe, _ = ref(case, True, **kwargs)
    assert (pe.v != oe.v).any(), (family, name, case["id"], r, "below the bar and not caught by the exact twin")
    return r


def _report(family):
    mine = {k: v for k, v in SMALLEST.items() if k.startswith(family + ":")}
    print("smallest perturbation / bar,", ", ".join(f"{k.split(': ')[1]} {v:.3g}" for k, v in sorted(mine.items())))
    return mine


def test_score_perturbations_cross_the_bar():
    runs = 0
    for c in R.SEQ_CASES:
        for name in ("product_dropped",) + (("seam_h",) if c["rows"] > 1 else ()) + (("bad_clamped",) if c["bad"] else ()):
            assert _judge("scores", name, _seq_ref, c, dict(variant=name)) > 1.0
            runs += 1
    for c in R.CAND_CASES:
        names = ("product_dropped",) + (("h_row_r", "seam_h") if c["B"] > 1 and c["C"] > 1 else ()) + \
            (("seam_h",) if c["B"] > 1 and c["C"] == 1 else ()) + (("bad_clamped",) if c["bad"] else ())
        for name in names:
            assert _judge("scores", name, _cand_ref, c, dict(variant=name)) > 1.0
            runs += 1
    assert len(_report("scores")) == 4 and runs > 100


def test_score_grad_perturbations_cross_the_bar():
    for c in R.SCORE_GRAD_CASES:
        g = R.gen_score_grad(c, False)
        names = (("last_neg_dropped",) if R._ok(g["neg"][-1:], g["num_items"]).all() else ()) + \
            (("second_trip_left",) if R.plan_score_grad(c["rows"], c["E"])["trips"] > 1 else ()) + \
            (("bad_pos_as_last_row",) if c["bad"] in ("pos", "both") else ())
        for name in names:
            assert _judge("score_grad", name, _grad_ref, c, dict(variant=name)) > 1.0
    assert len(_report("score_grad")) == 3


def _item_perturbations(index):
    c = R.ITEM_CASES[index]
    p, sid, order = _item_plan(index)
    n, C = p["n"], R.ITEM_CHUNK
    valid_neg = bool(np.any((order // c["rows"] == 2) & (sid >= 0) & (sid < c["T"])))
    okr = np.flatnonzero(p["ok"])
    t = okr[np.argmax(p["lengths"][okr])]                       # the longest run of a valid id
    lo, hi = int(p["runs"][t, 1]), int(p["runs"][t, 2])

    def w(sl, value):
        a = np.ones(n)
        a[sl] = value
        return dict(weight=a)

    out = {"last_dropped": w(hi - 1, 0.0), "last_twice": w(hi - 1, 2.0), "overwrite": dict(variant="overwrite")}
    if valid_neg:
        out["dpos_for_neg"] = dict(variant="dpos_for_neg")
    if p["spans"][t] >= 3:
        c0 = lo // C + 1
        out["middle_chunk_dropped"] = w(slice(c0 * C, (c0 + 1) * C), 0.0)
    if p["spans"][t] >= 2:
        out["first_chunk_only"] = w(slice((lo // C + 1) * C, hi), 0.0)
    if p["last_chunk"] == 1 and n > 1 and 0 <= sid[-1] < c["T"]:
        out["one_lookup_chunk_dropped"] = w(n - 1, 0.0)
    if p["max_id"] >= R.WAVE_SPAN:
        out["ids_past_first_trip_left"] = dict(variant="ids_past_first_trip_left")
    if p["bad_front"] or p["bad_back"]:
        out["bad_to_last_row"] = dict(variant="bad_to_last_row")
        out["bad_to_row_0"] = dict(variant="bad_to_row_0")
    if c["family"] == "second-trip":                            # seconds per reference over 2.1 M lookups: the four
        keep = ("last_dropped", "middle_chunk_dropped", "one_lookup_chunk_dropped", "ids_past_first_trip_left")
        out = {k: out[k] for k in keep}                         # that are about its seams and trips
    return out


def test_item_grad_perturbations_cross_the_bar_or_meet_the_exact_twin():
    below, total, seen = 0, 0, set()
    for i, c in enumerate(R.ITEM_CASES):
        for name, kwargs in _item_perturbations(i).items():
            below += _judge("item_grad", name, _item_ref, c, kwargs) <= 1.0
            total += 1
            seen.add(name)
    assert seen == {"last_dropped", "last_twice", "dpos_for_neg", "overwrite", "middle_chunk_dropped", "first_chunk_only",
                    "one_lookup_chunk_dropped", "ids_past_first_trip_left", "bad_to_last_row", "bad_to_row_0"}
    print(f"{total} perturbed references, {below} below the bar on random inputs and caught by their exact twins")
    _report("item_grad")


def test_row_sum_perturbations_cross_the_bar_or_meet_the_exact_twin():
    below, total = 0, 0
    for c in R.PARAM_CASES:
        Rr, K = c["B"] * c["L"], R.CHUNK_ROWS

        def w(sl, value):
            a = np.ones(Rr)
            a[sl] = value
            return dict(weight=a)

        perts = {"chunk_last_row_dropped": w(min(K, Rr) - 1, 0.0)}
        if Rr > K:
            perts["chunk_twice"] = w(slice(0, K), 2.0)
            perts["partial_in_other_slot"] = dict(swap=1)
            if Rr % K == 1:
                perts["one_row_chunk_dropped"] = w(Rr - 1, 0.0)
        for name, kwargs in perts.items():
            below += _judge("row_sums", name, _param_ref, c, kwargs) <= 1.0
            total += 1
    print(f"{total} perturbed references, {below} below the bar on random inputs and caught by their exact twins")
    assert len(_report("row_sums")) == 4
