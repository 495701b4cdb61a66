"""The owner passes of csrc/ngcf_owned.hip, each called on its own: the score gradient against the sequential f32 loop of
tests/ngcf_owned_cases.py (np.array_equal: the contract fixes every bit), the ordered weight gradient against
tests/ngcf_ref64.py at the chunk edges (inside the "dw" bar, EQUAL on the exact inputs, twice the same bits, scratch
poisoned with NaN), and the ordered row sets against np.flatnonzero of the flags."""
import numpy as np
import pytest
import torch

import ngcf_owned_cases as O
import ngcf_ref64 as R

pytestmark = pytest.mark.gpu
F32 = np.float32


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---- score backward -------------------------------------------------------------------------------------------------

def _score_bwd(device, c, prefill, workspace=None):
    """(dlayers as numpy, flag) of engine.ngcf_score_backward(deterministic=True) on buffers filled with ``prefill``."""
    from yelprecommendation_amd import engine
    layers = [_t(E, device) for E in c["layers"]]
    dl = [torch.full_like(E, prefill) for E in layers]
    flag = engine.new_error_flag(device)
    neg = c["n"] is not None
    engine.ngcf_score_backward(layers, dl, c["num_users"], _t(c["u"], device), _t(c["p"], device),
                               _t(c["n"], device) if neg else None, _t(c["gpos"], device),
                               _t(c["gneg"], device) if neg else None, err_flag=flag, deterministic=True,
                               workspace=workspace)
    return [d.cpu().numpy() for d in dl], int(flag.item())


def _assert_rows_equal(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            rows = np.flatnonzero((g != w).any(1))
            raise AssertionError((what, "layer", k, "rows", rows[:8], g[rows[0]][:4], w[rows[0]][:4]))


@pytest.mark.parametrize("with_neg", [True, False], ids=["neg", "noneg"])
@pytest.mark.parametrize("layers", O.LAYERS)
@pytest.mark.parametrize("d", O.WIDTHS)
def test_score_backward_equals_the_sequential_loop(device, d, layers, with_neg):
    """B = 0, 1, G - 1, G, G + 1, 257 (G triplets per wave of the default kernel) over 40 users and 50 items, into
    zero-filled buffers and into buffers holding the sentinel: every touched row equals the f32 loop in ascending
    triplet index, every other row keeps its pre-fill; no flag."""
    for B in O.batches(d):
        c = O.score_case(d, layers, B, with_neg)
        for prefill in (0.0, R.SENTINEL):
            got, flag = _score_bwd(device, c, prefill)
            assert flag == 0
            _assert_rows_equal(got, O.expected(c, prefill), (d, layers, B, with_neg, prefill))


@pytest.mark.parametrize("with_neg", [True, False], ids=["neg", "noneg"])
@pytest.mark.parametrize("d,layers", [(16, 3), (64, 1), (128, 3)])
def test_score_backward_mixed_batch(device, d, layers, with_neg):
    """600 triplets: a user with 48 of them, an item in both roles, pos == neg in one triplet, one bad user id and one
    bad item id (flags raised, the two triplets skipped, every other row still exact), rows that no triplet touches;
    a workspace full of 0xFF bytes on entry."""
    from yelprecommendation_amd import engine
    c = O.mixed_case(d, layers, with_neg)
    want_flag = O.flags_expected(c)
    assert want_flag == 3
    n = c["num_users"] + c["num_items"]
    ws = torch.full((engine.ngcf_owned_score_workspace_bytes(n, O.MIXED_B),), 255, dtype=torch.uint8, device=device)
    for prefill in (0.0, R.SENTINEL):
        got, flag = _score_bwd(device, c, prefill, workspace=ws)
        assert flag == want_flag
        want = O.expected(c, prefill)
        _assert_rows_equal(got, want, (d, layers, with_neg, prefill))
        untouched = np.ones(n, bool)
        untouched[list(O.contributions(c, 0))] = False
        assert untouched.sum() >= 20 and (got[0][untouched] == F32(prefill)).all()


def test_score_backward_row_of_a_thousand(device):
    """One user row and one item row with 1,000 contributions each: judged by ngcf_ref64.score_bwd under the "de" bar
    (and equal to the sequential loop, which the contract promises at any length); two calls give the same bits."""
    c = O.long_row_case(64, 3)
    ref = R.score_bwd(c["layers"], c["num_users"], c["u"], c["p"], c["n"], c["gpos"], c["gneg"])
    a, flag = _score_bwd(device, c, 0.0)
    b, _ = _score_bwd(device, c, 0.0)
    assert flag == 0
    for k in range(3):
        r = R.ratio(a[k], ref[k], "de")
        print(f"row of 1000, layer {k}: error / bar = {r:.3g}")
        assert r <= 1.0
        assert np.array_equal(a[k], b[k])
    _assert_rows_equal(a, O.expected(c, 0.0), "row of 1000")


# ---- ordered weight gradient ----------------------------------------------------------------------------------------

def _rowset(n, rows, device, max_rows):
    from yelprecommendation_amd.engine import NGCFRowSet
    rows = np.asarray(rows, np.int32)
    flags = np.zeros(n, np.int32)
    flags[rows] = 1
    spare = np.flatnonzero(flags == 0)
    buf = np.full(n, spare[0] if len(spare) else 0, np.int32)
    buf[:len(rows)] = rows
    s = NGCFRowSet(n, device, max_rows)
    s.flags, s.rows, s.count = _t(flags, device), _t(buf, device), _t(np.array([len(rows)], np.int32), device)
    s.max_rows = int(max_rows)
    return s


def _dw_refs(c, exact, rows=None):
    _, _, dW1, dW2 = R.dense_bwd(c["dEout"], c["Eout"], c["E"], c["Z"], c["W1"], c["W2"], c["dE0"], rows=rows)
    q1 = q2 = None
    if exact:
        A, H = c["Z"].astype(np.float64) + c["E"], c["E"].astype(np.float64) * c["Z"]
        q1 = min(R.quantum(c["dEout"]) * R.quantum(A), R.quantum(c["dW10"]))
        q2 = min(R.quantum(c["dEout"]) * R.quantum(H), R.quantum(c["dW20"]))
    return (dW1.plus(c["dW10"]), q1), (dW2.plus(c["dW20"]), q2)


def _ordered_dw(device, d, c, exact, rows, rowset, what):
    """Two calls of the ordered form into copies of a non-zero dW, the scratch full of NaN bytes before each."""
    from yelprecommendation_amd import engine
    t = {k: _t(v, device) for k, v in c.items() if isinstance(v, np.ndarray)}
    bound = c["n"] if rowset is None else rowset.max_rows
    nbytes = engine.ngcf_owned_dw_workspace_bytes(bound, d)
    runs = []
    for _ in range(2):
        ws = torch.full((max(nbytes, 1),), 255, dtype=torch.uint8, device=device)     # 0xFFFFFFFF: a NaN in every slot
        dE, dW1, dW2 = t["dE0"].clone(), t["dW10"].clone(), t["dW20"].clone()
        engine.ngcf_dense_bwd(t["dEout"], t["Eout"], t["E"], t["Z"], t["W1"], t["W2"], dE, dW1, dW2, rows=rowset,
                              deterministic=True, workspace=ws)
        runs.append((dW1.cpu().numpy(), dW2.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), (what, "two calls differ")
    for got, (ref, q) in zip(runs[0], _dw_refs(c, exact, rows)):
        got = got.astype(np.float64)
        if q is not None:
            assert R.exact(q, ref.s), (what, q)
            assert np.array_equal(got, ref.v), (what, "differs from float64 on the exact inputs")
        else:
            r = R.ratio(got, ref, "dw")
            assert r < 1.0, (what, r)


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("d", R.WIDTHS)
def test_ordered_dw_over_row_chunks(device, d, exact):
    """n = ROWS - 1, ROWS, ROWS + 1, 2 ROWS + 1, 600 ROWS + 5 and 1025 ROWS + 1 (past 512 chunks: several chunks per
    workgroup under the cap of 256 slots), accumulated into a non-zero dW."""
    for n, _ in R.dw_sizes(d):
        c = R.dense_case(d, n, exact)
        _ordered_dw(device, d, c, exact, None, None, (d, n))


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("d", R.WIDTHS)
def test_ordered_dw_row_lists(device, d, exact):
    """The row-list form: one workgroup over four chunks, a grid of two over six — and a list SHORTER than max_rows
    (count = ROWS + 3 under a grid of four): the two workgroups without rows leave their slots as they were (NaN), the
    reducer must not read them; an empty list leaves dW as it was."""
    r = R.wrows(d)
    for j, (n, count, max_rows) in enumerate(R.dw_list_cases(d) + [(5 * r, r + 3, 4 * r), (3 * r, 0, 2 * r)]):
        c = R.dense_case(d, n, exact, seed=j)
        rows = R.row_list(n, count, j)
        _ordered_dw(device, d, c, exact, rows, _rowset(n, rows, device, max_rows), (d, n, count, max_rows))


# ---- ordered row sets -----------------------------------------------------------------------------------------------

def _check_set(s, want_flags, what):
    flags = s.flags.cpu().numpy()
    count = int(s.count.item())
    rows = s.rows.cpu().numpy()[:count]
    assert np.array_equal(flags, want_flags), (what, "flags")
    assert np.array_equal(rows, np.flatnonzero(flags)), (what, "rows not the ascending members")
    assert count == int(want_flags.sum()) and (count < 2 or bool((np.diff(rows) > 0).all())), what


@pytest.mark.parametrize("n", O.FRONTIER_N)
def test_ordered_frontier_mark(device, n):
    """The list is strictly ascending and equals np.flatnonzero(flags), the flags equal the default form's: the empty
    batch, one triplet, a fifth of the nodes, a set that covers all n; n around one scan tile and past four."""
    from yelprecommendation_amd import engine
    for name, (nu, ni, u, p, q) in O.frontier_batches(n).items():
        args = (nu, ni, _t(u, device), _t(p, device), _t(q, device))
        s = engine.ngcf_frontier_mark(*args, ordered=True)
        default = engine.ngcf_frontier_mark(*args)
        want = R.frontier_mark(nu, ni, u, p, q)
        assert torch.equal(s.flags, default.flags) and int(s.count.item()) == int(default.count.item())
        _check_set(s, want, (n, name))
        if name == "all":
            assert want.all()
        if name == "empty":
            assert int(s.count.item()) == 0


def test_ordered_frontier_expand(device):
    """ngcf_ref64.expand_case(): rows of 0 .. 2,051 neighbours, a short and a 2,100-row input list, the input ordered
    or not — the output lists its members ascending and its flags are the default form's."""
    from yelprecommendation_amd import engine
    from yelprecommendation_amd.graph import LaplacianCSR
    c = R.expand_case()
    n = c["n"]
    graph = LaplacianCSR(c["rowptr"], c["col"], np.ones(len(c["col"]), F32), n, device, heavy_threshold=64)
    for name, rows_in in c["lists"].items():
        want = R.frontier_expand(c["rowptr"], c["col"], rows_in)
        for sorted_input in (False, True):
            src = _rowset(n, np.sort(rows_in) if sorted_input else rows_in, device, len(rows_in))
            s = engine.ngcf_frontier_expand(graph, src, ordered=True)
            default = engine.ngcf_frontier_expand(graph, src)
            assert torch.equal(s.flags, default.flags)
            _check_set(s, want, (name, sorted_input))
            assert 0 < int(s.count.item()) < n
