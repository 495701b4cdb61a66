"""The NGCF kernels of csrc/ngcf.hip at the ends of their loops — a pass, a round, the heavy threshold, a 32-row tile,
a staged row chunk, a row list longer than its grid, a batch past the grid cap — each entry point called directly
(through ``engine``, or the C ABI where the wrapper hides an argument) and compared with tests/ngcf_ref64.py
(float64) over every element: inside the bar the reference states on random inputs, EQUAL to float64 on the inputs
whose exactness certificate holds (tests/test_ngcf_ref64.py proves, without a GPU, that these two checks notice a
dropped or doubled entry, pass, wave share, row, chunk, list entry or triplet in every case below).  Buffers whose
rows the contract leaves untouched are pre-filled with a sentinel."""
import numpy as np
import pytest
import torch

import ngcf_ref64 as R

pytestmark = pytest.mark.gpu
F32 = np.float32
KINDS = pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
WORST = {}


def _note(family, value):
    WORST[family] = max(WORST.get(family, 0.0), float(value))


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _same(got, ref, kind, family, q=None, rows=None):
    """got == the reference: exactly where a certificate quantum is given, inside the bar otherwise."""
    got = got.detach().cpu().numpy().astype(np.float64)
    if rows is not None:
        got, ref = got[rows], ref[rows]
    if q is not None:
        assert R.exact(q, ref.s), (family, q)
        bad = np.flatnonzero((got != ref.v).reshape(-1))
        assert bad.size == 0, (family, "differs from float64 at", bad[:8], got.reshape(-1)[bad[:8]], ref.v.reshape(-1)[bad[:8]])
        return
    r = R.ratio(got, ref, kind)
    _note(family, r)
    assert r < 1.0, (family, r)


def _graph(c, device, heavy_threshold=None):
    from yelprecommendation_amd.graph import LaplacianCSR
    return LaplacianCSR(c["rowptr"], c["col"], c["val"], c["n"], device,
                        heavy_threshold=c["heavy_threshold"] if heavy_threshold is None else heavy_threshold)


def _rowset(n, rows, device, max_rows):
    """An NGCFRowSet filled by hand; the list's slots past the count name a valid row outside the set."""
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


def _sent(like):
    return torch.full_like(like, R.SENTINEL)


# ---- SpMM -----------------------------------------------------------------------------------------------------------

def _spmm_quantum(c, exact):
    return min(R.quantum(c["val"]) * R.quantum(c["X"]), R.quantum(c["Y0"])) if exact else None


@KINDS
@pytest.mark.parametrize("kind", R.SPMM_KINDS)
@pytest.mark.parametrize("d", R.WIDTHS)
def test_spmm_every_form_at_the_row_ends(device, d, kind, exact):
    """yr_spmm_csr plain / accumulate with and without the heavy list, yr_spmm_csr_sliced with row_order NULL / by
    falling degree / a random permutation, yr_spmm_csr_subset by flags and by list (bit-identical to the full product
    on the member rows, sentinel elsewhere, heavy rows on both sides, the empty set) — on the graph that carries the
    whole length ladder of its width, on 300 heavy rows (the h += 256 loop) and on n = 1, 3, 4, 5 rows."""
    from yelprecommendation_amd import engine
    c = R.spmm_case(d, kind, exact)
    q = _spmm_quantum(c, exact)
    ref = R.spmm(c["rowptr"], c["col"], c["val"], c["X"])
    refa = ref.plus(c["Y0"])
    graph, light = _graph(c, device), _graph(c, device, heavy_threshold=10 ** 9)
    deg = np.diff(c["rowptr"])
    assert light.n_heavy == 0 and graph.n_heavy == int((deg > R.T(d)).sum())
    if kind == "ladder":
        assert sorted(deg[list(c["marked"].values())]) == sorted(R.ladder(d)) and graph.n_heavy >= 5
        assert deg[0] == 0 and deg[-1] == 8 * R.R(d) + 1
    if kind == "heavy300":
        assert graph.n_heavy == 300 > R.HEAVY_BLOCKS
    X, Y0 = _t(c["X"], device), _t(c["Y0"], device)
    fam = "spmm"
    for g in (graph, light):
        _same(engine.spmm_csr(g, X, form="rows"), ref, "spmm", fam, q)
        _same(engine.spmm_csr(g, X, out=Y0.clone(), accumulate=True, form="rows"), refa, "spmm", fam, q)
    perm = torch.from_numpy(np.random.RandomState(d).permutation(c["n"]).astype(np.int32)).to(device)
    for order in (None, graph.row_order, perm):
        light.row_order = order
        _same(engine.spmm_csr(light, X, form="sliced"), ref, "spmm", "spmm sliced", q)
        _same(engine.spmm_csr(light, X, out=Y0.clone(), accumulate=True, form="sliced"), refa, "spmm", "spmm sliced", q)
    full = engine.spmm_csr(graph, X, form="rows")
    full_acc = engine.spmm_csr(graph, X, out=Y0.clone(), accumulate=True, form="rows")
    rs = np.random.RandomState(7 * d)
    for name, on in R.spmm_subsets(c, rs).items():
        if name == "mixed" and graph.n_heavy >= 2:
            hv = graph.heavy_rows.cpu().numpy()
            assert on[hv].any() and not on[hv].all()
        ton = _t(on, device)
        flags = _t(on.astype(np.int32), device)
        members = rs.permutation(np.flatnonzero(on))
        s = _rowset(c["n"], members, device, len(members))
        for kw in (dict(row_active=flags), dict(rows=s)):
            sub = engine.spmm_csr_subset(graph, X, _sent(X), **kw)
            assert torch.equal(sub[ton], full[ton]) and bool((sub[~ton] == R.SENTINEL).all()), (name, list(kw))
            acc = engine.spmm_csr_subset(graph, X, Y0.clone(), accumulate=True, **kw)
            assert torch.equal(acc[ton], full_acc[ton]) and torch.equal(acc[~ton], Y0[~ton]), (name, list(kw))


@KINDS
def test_spmm_second_trip_of_the_light_rows(device, exact):
    """262,144 + 37 rows of 0 - 2 entries at D = 16: the row-per-wave loop of yr_spmm_csr (65,536 workgroups) takes
    a second trip for the last 37 rows; the flag form of the subset kernel shares the loop."""
    from yelprecommendation_amd import engine
    c = R.spmm_case(16, "big", exact)
    assert c["n"] == 262144 + 37
    q = _spmm_quantum(c, exact)
    graph = _graph(c, device)
    X, Y0 = _t(c["X"], device), _t(c["Y0"], device)
    ref = R.spmm(c["rowptr"], c["col"], c["val"], c["X"])
    full = engine.spmm_csr(graph, X, form="rows")
    _same(full, ref, "spmm", "spmm", q)
    _same(engine.spmm_csr(graph, X, out=Y0.clone(), accumulate=True, form="rows"), ref.plus(c["Y0"]), "spmm", "spmm", q)
    on = np.random.RandomState(3).rand(c["n"]) < 0.5
    on[-37:] = np.arange(37) % 2 == 0
    ton = _t(on, device)
    sub = engine.spmm_csr_subset(graph, X, _sent(X), row_active=_t(on.astype(np.int32), device))
    assert torch.equal(sub[ton], full[ton]) and bool((sub[~ton] == R.SENTINEL).all())


# ---- dense layer ----------------------------------------------------------------------------------------------------

def _dense_refs(c, exact, rows=None):
    """{name: (Out, kind, quantum)} of one dense case."""
    fwd, P = R.dense_fwd(c["E"], c["Z"], c["W1"], c["W2"])
    dZ, dE, dW1, dW2 = R.dense_bwd(c["dEout"], c["Eout"], c["E"], c["Z"], c["W1"], c["W2"], c["dE0"], rows=rows)
    q = dict.fromkeys(("P", "dZ", "dE", "dW1", "dW2"))
    if exact:
        A, H = c["Z"].astype(np.float64) + c["E"], c["E"].astype(np.float64) * c["Z"]
        qd = R.quantum(c["dEout"]) * R.quantum(c["W1"], c["W2"])
        assert not np.any(c["dEout"][c["Eout"] <= 0])
        q = {"P": min(R.quantum(A) * R.quantum(c["W1"]), R.quantum(H) * R.quantum(c["W2"])),
             "dZ": min(qd, qd * R.quantum(c["E"])), "dE": min(qd, qd * R.quantum(c["Z"]), R.quantum(c["dE0"])),
             "dW1": min(R.quantum(c["dEout"]) * R.quantum(A), R.quantum(c["dW10"])),
             "dW2": min(R.quantum(c["dEout"]) * R.quantum(H), R.quantum(c["dW20"]))}
    return {"fwd": (fwd, "fwd", None), "P": (P, "fwd", q["P"]), "dZ": (dZ, "dz", q["dZ"]), "dE": (dE, "de", q["dE"]),
            "dW1": (dW1.plus(c["dW10"]), "dw", q["dW1"]), "dW2": (dW2.plus(c["dW20"]), "dw", q["dW2"])}


def _dev_case(c, device):
    return {k: _t(v, device) for k, v in c.items() if isinstance(v, np.ndarray)}


def _check_fwd(out, refs, exact, fam, rows=None):
    if exact:
        P, _, qP = refs["P"]
        assert R.exact(qP, P.s)
        got, want = out.cpu().numpy(), R.fwd_expected32(P.v)
        if rows is not None:
            got, want = got[rows], want[rows]
        assert np.array_equal(got, want), (fam, "Eout differs from the once-rounded float64 value")
    else:
        _same(out, refs["fwd"][0], "fwd", fam + " Eout", None, rows)


def _run_bwd(t, engine, rows=None, dZ=None):
    dE, dW1, dW2 = t["dE0"].clone(), t["dW10"].clone(), t["dW20"].clone()
    dZ = engine.ngcf_dense_bwd(t["dEout"], t["Eout"], t["E"], t["Z"], t["W1"], t["W2"], dE, dW1, dW2, dZ=dZ, rows=rows)
    return dZ, dE, dW1, dW2


@KINDS
@pytest.mark.parametrize("d", R.WIDTHS)
def test_dense_layer_at_the_tile_edges(device, d, exact):
    """ngcf_dense_fwd / _bwd_data (dE accumulated into) / _bwd_weight (dW accumulated into) at n = 1, 31, 32, 33, 64,
    65, 333: one lane, a tile short of one row, full tiles, a tile of one row."""
    from yelprecommendation_amd import engine
    for n in R.DENSE_N:
        c = R.dense_case(d, n, exact)
        refs, t = _dense_refs(c, exact), _dev_case(c, device)
        _check_fwd(engine.ngcf_dense_fwd(t["E"], t["Z"], t["W1"], t["W2"], out=_sent(t["E"])), refs, exact, "dense")
        got = dict(zip(("dZ", "dE", "dW1", "dW2"), _run_bwd(t, engine, dZ=_sent(t["E"]))))
        for name, g in got.items():
            o, kind, q = refs[name]
            _same(g, o, kind, "dense " + name[:2], q)


@KINDS
@pytest.mark.parametrize("d", R.WIDTHS)
def test_dense_bwd_weight_over_row_chunks(device, d, exact):
    """ngcf_dense_bwd_weight at n = ROWS - 1, ROWS, ROWS + 1, 2 ROWS + 1 (ROWS = 4096 / D rows per staged chunk),
    600 ROWS + 5 (two chunks per workgroup, the last workgroup short) and 1025 ROWS + 1 (three chunks per workgroup,
    a one-row last chunk): the register prefetch of the next chunk and the ragged end, dW accumulated into dW0.
    The long sums are beyond what a bar can judge (tests/test_ngcf_ref64.py): equality on the exact inputs does."""
    from yelprecommendation_amd import engine
    for n, large in R.dw_sizes(d):
        chunks = -(-n // R.wrows(d))
        assert (chunks > 512) == large
        c = R.dense_case(d, n, exact)
        refs, t = _dense_refs(c, exact), _dev_case(c, device)
        got = dict(zip(("dZ", "dE", "dW1", "dW2"), _run_bwd(t, engine)))
        for name, g in got.items():
            o, kind, q = refs[name]
            _same(g, o, kind, ("dW large" if large else "dW") if name[:2] == "dW" else "dense " + name[:2], q)


@KINDS
@pytest.mark.parametrize("d", R.WIDTHS)
def test_dense_row_list_forms(device, d, exact):
    """yr_ngcf_dense_{fwd,bwd_data,bwd_weight}_rows over hand-made lists (random order, row 0 and row n - 1 listed):
    count = 0, 1, 31, 32, 33, 100 with max_rows = count, and count = 100 with max_rows = 1 and 32 — one workgroup
    striding over four tiles with a ragged last one.  Listed rows: bit-identical to the full form, equal to float64
    (exact inputs) or inside the bar; the other rows keep the sentinel; zero_rows (C ABI) clears exactly the listed
    rows."""
    from yelprecommendation_amd import _lib, engine
    lib, n = _lib.load(), R.LIST_N
    for j, (count, max_rows) in enumerate(R.LIST_CASES):
        c = R.dense_case(d, n, exact, seed=j)
        rows = R.row_list(n, count, j)
        assert len(rows) == count and (count < 2 or (0 in rows and n - 1 in rows))
        refs, t = _dense_refs(c, exact, rows=rows), _dev_case(c, device)
        s = _rowset(n, rows, device, max_rows)
        on = s.flags.bool()
        listed = np.sort(rows)
        out_full = engine.ngcf_dense_fwd(t["E"], t["Z"], t["W1"], t["W2"])
        out = engine.ngcf_dense_fwd(t["E"], t["Z"], t["W1"], t["W2"], out=_sent(t["E"]), rows=s)
        assert torch.equal(out[on], out_full[on]) and bool((out[~on] == R.SENTINEL).all()), (count, max_rows)
        if count:
            _check_fwd(out, refs, exact, "dense rows", rows=listed)
        dZ_f, dE_f, _, _ = _run_bwd(t, engine)
        dZ, dE, dW1, dW2 = _run_bwd(t, engine, rows=s, dZ=_sent(t["E"]))
        assert torch.equal(dZ[on], dZ_f[on]) and bool((dZ[~on] == R.SENTINEL).all()), (count, max_rows)
        assert torch.equal(dE[on], dE_f[on]) and torch.equal(dE[~on], t["dE0"][~on]), (count, max_rows)
        if count:
            _same(dZ, refs["dZ"][0], "dz", "dense rows dZ", refs["dZ"][2], rows=listed)
        _same(dE, refs["dE"][0], "de", "dense rows dE", refs["dE"][2])
        _same(dW1, refs["dW1"][0], "dw", "dW rows", refs["dW1"][2])
        _same(dW2, refs["dW2"][0], "dw", "dW rows", refs["dW2"][2])
        # zero_rows: the layer's gradient buffer, cleared on the listed rows by the forward launch
        zr, out2 = _sent(t["E"]), _sent(t["E"])
        f32 = torch.float32
        engine.check(lib.yr_ngcf_dense_fwd_rows(engine._dev(t["E"], f32, "E"), engine._dev(t["Z"], f32, "Z"),
                                                engine._dev(t["W1"], f32, "W1"), engine._dev(t["W2"], f32, "W2"), n, d,
                                                out2.data_ptr(), s.rows.data_ptr(), s.count.data_ptr(), s.max_rows,
                                                zr.data_ptr(), engine._stream()), "yr_ngcf_dense_fwd_rows")
        assert torch.equal(out2, out)
        assert bool((zr[on] == 0.0).all()) and bool((zr[~on] == R.SENTINEL).all()), (count, max_rows)


@KINDS
@pytest.mark.parametrize("d", R.WIDTHS)
def test_dense_bwd_weight_rows_over_chunks(device, d, exact):
    """yr_ngcf_dense_bwd_weight_rows with max_rows = ROWS and count = 3 ROWS + 7 (one workgroup, four chunks, the
    last of seven rows) and max_rows = 2 ROWS, count = 5 ROWS + 1 (two workgroups, three chunks each, a one-row
    chunk); the data kernel over the same lists."""
    from yelprecommendation_amd import engine
    for j, (n, count, max_rows) in enumerate(R.dw_list_cases(d)):
        c = R.dense_case(d, n, exact, seed=j)
        rows = R.row_list(n, count, j)
        refs, t = _dense_refs(c, exact, rows=rows), _dev_case(c, device)
        s = _rowset(n, rows, device, max_rows)
        on = s.flags.bool()
        dZ, dE, dW1, dW2 = _run_bwd(t, engine, rows=s, dZ=_sent(t["E"]))
        assert bool((dZ[~on] == R.SENTINEL).all()) and torch.equal(dE[~on], t["dE0"][~on])
        _same(dZ, refs["dZ"][0], "dz", "dense rows dZ", refs["dZ"][2], rows=np.sort(rows))
        _same(dE, refs["dE"][0], "de", "dense rows dE", refs["dE"][2])
        _same(dW1, refs["dW1"][0], "dw", "dW rows", refs["dW1"][2])
        _same(dW2, refs["dW2"][0], "dw", "dW rows", refs["dW2"][2])


# ---- push and frontier ----------------------------------------------------------------------------------------------

@KINDS
@pytest.mark.parametrize("d", R.WIDTHS)
def test_push_rows_parts_and_long_lists(device, d, exact):
    """yr_spmm_csr_push_rows into a non-zero Y0: listed rows of 0, 1, 15, 16, 17 entries (empty parts among the 16),
    16 * 4 G + 1 (a part's inner loop takes a second trip) and 16 * 8 G + 5; a list of 2,100 rows (33,600 parts
    over the 32,768-workgroup cap: the outer loop strides).  The matrix is not symmetric."""
    from yelprecommendation_amd import engine
    c = R.push_case(d, exact)
    deg = np.diff(c["rowptr"])
    assert list(deg[:len(c["special"])]) == R.push_lengths(d)
    q = _spmm_quantum(c, exact)
    graph = _graph(dict(c, heavy_threshold=256), device)
    X = _t(c["X"], device)
    for which, rows in c["lists"].items():
        assert set(range(len(c["special"]))) <= set(rows.tolist())
        assert (len(rows) * R.PUSH_PARTS > R.PUSH_GRID) == (which == "many")
        s = _rowset(c["n"], rows, device, len(rows))
        Y = engine.spmm_csr_push_rows(graph, X, _t(c["Y0"], device), s)
        _same(Y, R.push_rows(c["rowptr"], c["col"], c["val"], c["X"], c["Y0"], rows), "push", "push", q)


def _mark(lib, engine, device, nu, ni, u, p, n, B=None):
    """yr_ngcf_frontier_mark through the C ABI into guarded buffers: (flags, rows, count) as NumPy arrays."""
    N, pad = nu + ni, 64
    fbuf = torch.full((N + 2 * pad,), 99, dtype=torch.int32, device=device)
    rbuf = torch.full((N + 2 * pad,), -7, dtype=torch.int32, device=device)
    cnt = torch.full((1,), 12345, dtype=torch.int32, device=device)
    tu, tp = _t(u, device), _t(p, device)
    tn = None if n is None else _t(n, device)
    engine.check(lib.yr_ngcf_frontier_mark(tu.data_ptr(), tp.data_ptr(), None if tn is None else tn.data_ptr(),
                                           len(u) if B is None else B, nu, ni, fbuf.data_ptr() + 4 * pad,
                                           rbuf.data_ptr() + 4 * pad, cnt.data_ptr(), 1, engine._stream()),
                 "yr_ngcf_frontier_mark")
    f, r, k = fbuf.cpu().numpy(), rbuf.cpu().numpy(), int(cnt.item())
    assert (f[:pad] == 99).all() and (f[pad + N:] == 99).all(), "a flag written outside the array"
    assert (r[:pad] == -7).all() and (r[pad + k:] == -7).all(), "a row written outside the list"
    return f[pad:pad + N], r[pad:pad + k], k


def test_frontier_mark_batches_and_contention(device):
    """yr_ngcf_frontier_mark at B = 1, 255, 256, 257 (one workgroup short of a lane, full, one lane over) with
    out-of-range ids of every kind (skipped, nothing written outside the arrays), without negatives, and at
    B = 70,000 over 50 users and 40 items (every lane contends for the same flags): the flags equal the NumPy
    definition and the list names every flagged row exactly once."""
    from yelprecommendation_amd import _lib, engine
    lib = _lib.load()
    for B, nu, ni in ((1, 300, 200), (255, 300, 200), (256, 300, 200), (257, 300, 200), (70000, 50, 40)):
        rs = np.random.RandomState(B)
        u, p, n = (rs.randint(0, m, B).astype(np.int64) for m in (nu, ni, ni))
        if B >= 255:
            u[3], u[B - 1], p[5], p[B - 2], n[7], n[B - 1] = -1, nu, ni, -3, ni + 10 ** 9, -1
        for neg in (n, None):
            want = R.frontier_mark(nu, ni, u, p, neg)
            flags, rows, k = _mark(lib, engine, device, nu, ni, u, p, neg)
            np.testing.assert_array_equal(flags, want)
            assert k == int(want.sum()) and sorted(rows.tolist()) == np.flatnonzero(want).tolist(), (B, neg is None)
    flags, rows, k = _mark(lib, engine, device, 30, 20, np.zeros(1, np.int64), np.zeros(1, np.int64), None, B=0)
    assert k == 0 and not flags.any()                                    # an empty batch clears the set


def test_frontier_expand_parts_and_long_lists(device):
    """yr_ngcf_frontier_expand: input rows of 0, 1, 7, 8, 9 entries (empty parts among the 8) and 8 * 256 + 3 (a
    part's loop takes a second trip); 2,100 input rows (16,800 parts over the 16,384-workgroup cap); clear = 0
    through the C ABI onto a set that already has members."""
    from yelprecommendation_amd import _lib, engine
    lib = _lib.load()
    c = R.expand_case()
    assert list(np.diff(c["rowptr"])[:len(R.EXPAND_LENGTHS)]) == R.EXPAND_LENGTHS
    graph = _graph(dict(c, val=np.ones(len(c["col"]), F32), heavy_threshold=256), device)
    for which, rows in c["lists"].items():
        assert (len(rows) * R.EXPAND_PARTS > R.EXPAND_GRID) == (which == "many")
        s_in = _rowset(c["n"], rows, device, len(rows))
        want = R.frontier_expand(c["rowptr"], c["col"], rows)
        assert 0 < want.sum() < c["n"]
        out = engine.ngcf_frontier_expand(graph, s_in)
        np.testing.assert_array_equal(out.flags.cpu().numpy(), want)
        k = int(out.count.item())
        assert k == int(want.sum()) and sorted(out.rows[:k].cpu().tolist()) == np.flatnonzero(want).tolist()
        # clear = 0: the set keeps its members (some of them among the new rows) and lists every row once
        rs = np.random.RandomState(len(rows))
        old = np.unique(np.concatenate([rs.choice(c["n"], 60, replace=False), np.flatnonzero(want)[:9]]))
        s = _rowset(c["n"], old, device, c["n"])
        s.rows[len(old):] = -7
        engine.check(lib.yr_ngcf_frontier_expand(graph.rowptr.data_ptr(), graph.col.data_ptr(), c["n"],
                                                 s_in.rows.data_ptr(), s_in.count.data_ptr(), s_in.max_rows,
                                                 s.flags.data_ptr(), s.rows.data_ptr(), s.count.data_ptr(), 0,
                                                 engine._stream()), "yr_ngcf_frontier_expand")
        f0 = np.zeros(c["n"], np.int32)
        f0[old] = 1
        want2 = R.frontier_expand(c["rowptr"], c["col"], rows, flags0=f0)
        np.testing.assert_array_equal(s.flags.cpu().numpy(), want2)
        k = int(s.count.item())
        got = s.rows.cpu().numpy()
        assert k == int(want2.sum()) and sorted(got[:k].tolist()) == np.flatnonzero(want2).tolist()
        assert got[:len(old)].tolist() == old.tolist() and (got[k:] == -7).all()


# ---- scores ---------------------------------------------------------------------------------------------------------

def _score_check(device, d, layers, B, with_neg, same_user=False, bad_at=None):
    from yelprecommendation_amd import engine
    c = R.score_case(d, layers, B, with_neg, same_user)
    nu = R.SCORE_USERS
    if bad_at is not None:
        c["p"][bad_at] = R.SCORE_ITEMS
    pos, neg = R.score(c["layers"], nu, c["u"], c["p"], c["n"])
    dref = R.score_bwd(c["layers"], nu, c["u"], c["p"], c["n"], c["gpos"], c["gneg"])
    q = R.quantum(*c["layers"])
    qg = q * R.quantum(c["gpos"], *([c["gneg"]] if with_neg else []))
    T = [_t(E, device) for E in c["layers"]]
    tu, tp = _t(c["u"], device), _t(c["p"], device)
    tn = _t(c["n"], device) if with_neg else None
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    res = engine.ngcf_score(T, nu, tu, tp, tn, err_flag=flag)
    _same(res[0] if with_neg else res, pos, None, "score", q * q)
    if with_neg:
        _same(res[1], neg, None, "score", q * q)
    dT = [torch.zeros_like(t) for t in T]
    engine.ngcf_score_backward(T, dT, nu, tu, tp, tn, _t(c["gpos"], device), _t(c["gneg"], device) if with_neg else None,
                               err_flag=flag)
    for got, want in zip(dT, dref):
        _same(got, want, None, "score bwd", qg)
    assert int(flag.item()) == (0 if bad_at is None else engine.FLAG_BAD_ITEM)
    return pos


@pytest.mark.parametrize("d", R.WIDTHS)
def test_scores_equal_float64_at_the_lane_group_edges(device, d):
    """yr_ngcf_score_fwd / _bwd on integer inputs, equality in both directions: B = G - 1, G, G + 1 (a wave's lane
    groups short of one, full, one over) and 4 G + 1 (a second workgroup) with 1 and 8 layers, without negatives,
    every triplet on the same user (all atomics of the user's row contend), and a bad item id inside the last,
    partly filled wave: the flag is raised, its score is 0 and its neighbours' scores are right."""
    g = R.G(d)
    for layers in (1, 8):
        for B in R.score_batches(d):
            if B:
                _score_check(device, d, layers, B, True)
    _score_check(device, d, 2, R.score_batches(d)[-1], False)
    _score_check(device, d, 2, 300, True, same_user=True)
    tail = max(1, g - 1)
    B = R.WAVES * g + tail
    bad = B - 1 - (tail - 1) // 2
    pos = _score_check(device, d, 2, B, True, bad_at=bad)
    assert pos.v[bad] == 0.0 and B - tail <= bad < B          # (the neighbours were compared with the reference above)


def test_scores_past_the_grid_cap(device):
    """B = 65,601 at D = 128 with two layers: 8,201 workgroups' worth of triplets on a grid capped at 8,192 — the
    first workgroups take a second trip, the last one a ragged one."""
    d, layers, B = R.BIG_SCORE
    assert -(-B // (R.WAVES * R.G(d))) > R.SCORE_GRID
    _score_check(device, d, layers, B, True)


def test_zz_report_worst_ratios():
    """Not a check of its own: prints the largest |err| / bar per kernel family seen by the tests above."""
    print("NGCF edges, max |err| / bar on random inputs:", {k: float("%.3g" % v) for k, v in sorted(WORST.items())})
    assert all(v < 1.0 for v in WORST.values())
