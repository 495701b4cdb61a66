"""csrc/cdae.hip at the ends of its loops: the f32 GEMM in both kernels (every K around a 4-vector, a 16-step and a
32-step; every row / column tail; the ragged last split; each of the four tile shapes with the plain and with the
atomic epilogue; bias, the three activations, 1 / count, row sums, accumulate), the dense decoder with the loss in its
epilogue, and the element-wise kernels around the grid cap of 2,048 workgroups — each entry point called through the
C ABI (or ``engine``) and compared with tests/gemm_ref64.py (float64) over EVERY element: inside the bar the reference
derives on random inputs, EQUAL to float64 where the exactness certificate holds.  Outputs live in sentinel-filled
buffers with 256-float guard bands; the sentinel must survive in the bands, in the columns N .. ldc - 1 and in every
row >= M.  Operand rows are padded with NaN: a read past a row's end shows.  tests/test_gemm_ref64.py proves without
a GPU that these checks notice a lost product, K step, split, row, column, bias, alpha or half of the row sums."""
import numpy as np
import pytest
import torch

import gemm_ref64 as R

pytestmark = pytest.mark.gpu
F32 = np.float32
S = R.SENTINEL
G = R.GUARD
WORST = {}
KINDS = pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
LAYOUT = pytest.mark.parametrize("tA,tB", R.LAYOUTS, ids=["nn", "nt", "tn", "tt"])
KERNEL = pytest.mark.parametrize("aligned", [True, False], ids=["tiled", "generic"])


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
    """A sentinel-filled flat f32 buffer: G floats, rows x ld, G floats; ``ptr`` addresses element (0, 0)."""

    def __init__(self, rows, ld, device, fill=None):
        self.rows, self.ld = rows, ld
        self.flat = torch.full((2 * G + rows * ld,), S, dtype=torch.float32, device=device)
        self.view = self.flat[G:G + rows * ld].view(rows, ld)
        if fill is not None:
            self.view[:fill.shape[0], :fill.shape[1]] = _t(np.asarray(fill, F32), device)
        self.ptr = self.flat.data_ptr() + 4 * G

    def read(self, rows, cols, what):
        """The [rows, cols] corner after checking that everything else still holds the sentinel."""
        f = _np(self.flat)
        assert (f[:G] == S).all() and (f[G + self.rows * self.ld:] == S).all(), (what, "a guard band was written")
        b = f[G:G + self.rows * self.ld].reshape(self.rows, self.ld)
        assert (b[rows:] == S).all(), (what, "a row past the count was written")
        assert (b[:, cols:] == S).all(), (what, "a pad column was written")
        return b[:rows, :cols]


def _same(got, ref, family, q=None):
    """got == the reference: exactly where a certificate quantum is given, inside the bar otherwise."""
    got = np.asarray(got, np.float64).reshape(ref.v.shape)
    if q is not None:
        assert R.exact(q, ref.s), (family, q)
        bad = np.flatnonzero((got != ref.v).reshape(-1))
        assert bad.size == 0, (family, "differs from float64 at", bad[:8], got.reshape(-1)[bad[:8]], ref.v.reshape(-1)[bad[:8]])
        return
    r = R.ratio(got, ref)
    _note(family, r)
    assert r < 1.0, (family, r)


def _count(value, device):
    """A spread count holding ``value`` in two of its slots (the readers add the slots up)."""
    c = torch.zeros(R.COUNT_WORDS, dtype=torch.int32, device=device)
    stride = R.COUNT_WORDS // R.COUNT_SLOTS
    c[5 * stride] = value // 2
    c[63 * stride] = value - value // 2
    return c


def _operand(op, trans, aligned, device):
    """op(X) stored (transposed or not) in NaN-padded rows: ld = a multiple of 4 with 8 to spare (the tiled kernel) or
    odd (the generic one).  Returns (tensor, ld)."""
    st = R.stored(np.asarray(op, F32), trans)
    r, c = st.shape
    ld = (c + 3) // 4 * 4 + 8 if aligned else c + 1 + c % 2
    buf = torch.full((max(r, 1), ld), float("nan"), dtype=torch.float32, device=device)
    if r and c:
        buf[:r, :c] = _t(st, device)
    return buf, ld


def _call(tA, tB, M, N, K, A, lda, B, ldb, Cptr, ldc, bias=None, act=0, accumulate=0, split_k=1, count=None, rowsum=None):
    lib = _lib()
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    head = (1 if tA else 0, 1 if tB else 0, M, N, K, p(A), lda, p(B), ldb, Cptr, ldc, p(bias), act, accumulate, split_k)
    if count is None and rowsum is None:
        return lib.yr_gemm_f32(*head, _stream())
    return lib.yr_gemm_f32_ex(*head, p(count), p(rowsum), _stream())


def _run(o, layout, aligned, device, exact, family, bias=False, act=0, count=None, accumulate=False, split_k=1,
         rowsum=False, pad=0, prod=None, zero=False):
    """One launch on the operands ``o`` of R.operands, compared over every element with the reference."""
    tA, tB = layout
    (M, K), N = o["a"].shape, o["b"].shape[1]
    p = R.plan(M, N, K, split_k, aligned, accumulate)
    assert p["kernel"] == ("tiled" if aligned else "generic")
    A, lda = _operand(o["a"], tA, aligned, device)
    B, ldb = _operand(o["b"], tB, aligned, device)
    ldc = N + pad
    C0 = o["C0"] if accumulate else (np.zeros((M, N), F32) if zero else None)
    out = Guarded(M + 2, ldc, device, fill=C0)
    rs = Guarded(1, M + 3, device) if rowsum else None
    alpha = None if count is None else R.alpha_of(count)
    status = _call(tA, tB, M, N, K, A, lda, B, ldb, out.ptr, ldc, bias=_t(o["bias"], device) if bias else None, act=act,
                   accumulate=1 if accumulate else 0, split_k=split_k, count=None if count is None else _count(count, device),
                   rowsum=None if rs is None else rs.ptr)
    assert status == 0, (family, status)
    if prod is None or count is not None:
        prod = R.products(o["a"], o["b"], alpha)
    ref, rows = R.finish(prod, o["bias"] if bias else None, act, C0, p["splits"], certified=exact)
    q = R.gemm_quantum(o["a"], o["b"], o["bias"] if bias else None, alpha, C0) if exact and act != R.ACT_SIGMOID else None
    if exact and act == R.ACT_SIGMOID:
        assert R.exact(R.gemm_quantum(o["a"], o["b"], o["bias"] if bias else None, alpha), R.finish(prod, o["bias"] if bias else None)[0].s)
    _same(out.read(M, N, family), ref, family, q)
    if rs is not None:
        _same(rs.read(1, M, family + " rowsum")[0], rows, family + " rowsum",
              R.gemm_quantum(o["a"], np.ones(1), None, alpha) if exact else None)
    return p


# ---- GEMM -----------------------------------------------------------------------------------------------------------

@KINDS
@KERNEL
@LAYOUT
def test_gemm_k_ladder(device, tA, tB, aligned, exact):
    """M = 70, N = 67 (two tiles each way, tails of 6 and 3), K = 0 ... 49 around a 4-vector, a 16-step and a 32-step:
    a plain store with bias and an activation (K = 0 gives act(bias)), with the row sums and 1 / count on the tiled
    kernel, and accumulate onto a non-zero C0 (K = 0 leaves C0)."""
    for j, K in enumerate(R.K_LADDER):
        o = R.operands(R.KL_M, R.KL_N, K, exact)
        fam = "gemm " + ("tiled" if aligned else "generic")
        _run(o, (tA, tB), aligned, device, exact, fam, bias=True, act=j % 3, pad=5 * (j % 2))
        _run(o, (tA, tB), aligned, device, exact, fam, accumulate=True, pad=5 * ((j + 1) % 2), rowsum=aligned and j % 2 == 0)
        if aligned:
            _run(o, (tA, tB), aligned, device, exact, fam, bias=j % 2 == 0, rowsum=True, count=R.COUNTS[exact][j % 4],
                 pad=5 * (j % 2))


@KINDS
@KERNEL
@LAYOUT
def test_gemm_mn_ladder(device, tA, tB, aligned, exact):
    """K = 20; M = N = 1 ... 129 around the 4-row vector, the 32-row MFMA tile, the 64- and 128-row workgroup tile,
    and the two thin shapes: plain, bias with each activation, accumulate; row sums with the sentinel beyond M."""
    fam = "gemm " + ("tiled" if aligned else "generic")
    for j, (M, N) in enumerate(R.MN_LADDER):
        o = R.operands(M, N, R.MN_K, exact)
        prod = R.products(o["a"], o["b"])
        _run(o, (tA, tB), aligned, device, exact, fam, pad=5 * (j % 2), prod=prod, rowsum=aligned)
        for act in (0, 1, 2):
            _run(o, (tA, tB), aligned, device, exact, fam, bias=True, act=act, pad=5 * ((j + act) % 2), prod=prod)
        _run(o, (tA, tB), aligned, device, exact, fam, accumulate=True, pad=5 * ((j + 1) % 2), prod=prod,
             rowsum=aligned and j % 2 == 1)


@KINDS
@pytest.mark.parametrize("case", R.SPLIT_CASES, ids=[str(c) for c in R.SPLIT_CASES])
def test_gemm_split_k(device, case, exact):
    """Each of the four tile shapes with the atomic epilogue, the ragged last split (19 of 32), split_k beyond K / 32,
    0 and negative: onto zeros, onto a non-zero C0, and with 1 / count for count in {0, 1, 7 or 4, 8} (one count per
    layout).  The K = 4,083 cases on random inputs have a bar wider than one product; their exact twins are compared
    for equality."""
    M, N, K, split_k = case
    o = R.operands(M, N, K, exact)
    prod = R.products(o["a"], o["b"])
    for j, layout in enumerate(R.LAYOUTS):
        p = R.plan(M, N, K, split_k, True)
        fam = "gemm split" + (" long" if K >= R.LONG_K else "")
        assert (p["bm"], p["bn"], p["splits"]) == R.SPLIT_WANT[case]
        _run(o, layout, True, device, exact, fam, split_k=split_k, zero=True, pad=5 * (j % 2), prod=prod)
        _run(o, layout, True, device, exact, fam, split_k=split_k, accumulate=True, pad=5 * ((j + 1) % 2), prod=prod)
        _run(o, layout, True, device, exact, fam, split_k=split_k, zero=True, count=R.COUNTS[exact][j], pad=5 * (j % 2))


@pytest.mark.parametrize("case,tile", R.WIDE_CASES, ids=[str(c) for c, _ in R.WIDE_CASES])
@pytest.mark.parametrize("variant", ["sigmoid", "rowsum"])
def test_gemm_plain_wide_tiles(device, case, tile, variant):
    """At least 2,048 tiles of C, so that the host keeps the 128 x 128, 64 x 128 and 128 x 64 tiles, K = 19: bias +
    sigmoid on random inputs inside the bar, row sums + 1 / 8 on exact inputs equal to float64; the float64 product
    is taken in row blocks."""
    M, N, K, tA, tB = case
    p = R.plan(M, N, K, 1, True)
    assert (p["bm"], p["bn"]) == tile and not p["atomic"] and p["splits"] == 1
    exact = variant == "rowsum"
    o = R.operands(M, N, K, exact, with_c0=False)
    A, lda = _operand(o["a"], tA, True, device)
    B, ldb = _operand(o["b"], tB, True, device)
    ldc = N + 5
    out = Guarded(M + 1, ldc, device)
    rs = Guarded(1, M + 3, device) if exact else None
    status = _call(tA, tB, M, N, K, A, lda, B, ldb, out.ptr, ldc, bias=None if exact else _t(o["bias"], device),
                   act=0 if exact else 1, count=_count(8, device) if exact else None, rowsum=None if rs is None else rs.ptr)
    assert status == 0
    got = out.read(M, N, "wide")
    alpha = 0.125 if exact else None
    fam = "gemm wide %dx%d" % tile
    for r0 in range(0, M, 512):
        sl = slice(r0, min(M, r0 + 512))
        ref, rows = R.finish(R.products(o["a"][sl], o["b"], alpha), None if exact else o["bias"], 0 if exact else 1)
        _same(got[sl], ref, fam, R.gemm_quantum(o["a"], o["b"], None, alpha) if exact else None)
        if exact:
            _same(rs.read(1, M, "wide rowsum")[0][sl], rows, fam + " rowsum", R.gemm_quantum(o["a"], np.ones(1), None, alpha))


def test_gemm_refusals_launch_nothing(device):
    """bias or act with accumulate or more than one split; rowsum with more than one split; alpha_count or rowsum on
    unaligned operands; act = 3; negative sizes: a non-zero status and an untouched output.  M = 0 or N = 0: status 0,
    nothing written."""
    M, N, K = 70, 67, 64
    o = R.operands(M, N, K, False)
    bias, cnt = _t(o["bias"], device), _count(4, device)
    out = Guarded(M + 2, N, device)
    rs = Guarded(1, M + 3, device)

    def refused(aligned, m=M, n=N, k=K, **kw):
        A, lda = _operand(o["a"], False, aligned, device)
        B, ldb = _operand(o["b"], False, aligned, device)
        status = _call(False, False, m, n, k, A, lda, B, ldb, out.ptr, N, **kw)
        torch.cuda.synchronize()
        out.read(0, 0, kw)
        rs.read(0, 0, kw)
        return status

    for aligned in (True, False):
        assert refused(aligned, bias=bias, accumulate=1) != 0
        assert refused(aligned, act=1, accumulate=1) != 0
        assert refused(aligned, bias=bias, split_k=2) != 0
        assert refused(aligned, act=2, split_k=2) != 0
        assert refused(aligned, act=3) != 0
        for neg in ({"m": -1}, {"n": -1}, {"k": -1}):
            assert refused(aligned, **neg) != 0
        assert refused(aligned, m=0) == 0 and refused(aligned, n=0) == 0
    assert refused(True, rowsum=rs.ptr, split_k=2) != 0
    assert refused(False, rowsum=rs.ptr) != 0
    assert refused(False, count=cnt) != 0


# ---- dense decoder --------------------------------------------------------------------------------------------------

def _decode(c, B, I, H, act, pad, with_pred, device):
    lib = _lib()
    ldg = I + pad
    Gb = Guarded(B + 2, ldg, device)
    Pb = Guarded(B + 2, ldg, device) if with_pred else None
    npart = int(lib.yr_cdae_decode_loss_partials(B, I))
    part = Guarded(1, npart + 7, device)
    count = torch.zeros(R.COUNT_WORDS, dtype=torch.int32, device=device)
    dev = {k: (None if c[k] is None else _t(c[k], device)) for k in ("z", "Wo", "bo", "target", "negmask")}
    p = lambda t: None if t is None else t.data_ptr()
    status = lib.yr_cdae_decode_loss(p(dev["z"]), p(dev["Wo"]), p(dev["bo"]), p(dev["target"]), p(dev["negmask"]), B, I, H,
                                     act, Gb.ptr, ldg, None if Pb is None else Pb.ptr, part.ptr, p(count), _stream())
    return status, Gb, Pb, part, npart, count


@pytest.mark.parametrize("case", R.DECODER_CASES, ids=[str(c) for c in R.DECODER_CASES])
def test_dense_decoder(device, case):
    """yr_cdae_decode_loss on its own: B, I around the 64 x 64 tile, H around the 16-step (4, 12, 16, 20, 36, 128),
    both activations, bo / negative_mask / pred NULL or given, ldg = I and I + 5, rows that select nothing and a batch
    that selects nothing: G inside the bar on the selected positions and exactly 0 elsewhere, pred, every loss partial
    at its index, the count exact slot by slot."""
    B, I, H, act, with_bo, with_mask, with_pred, pad, rows = case
    c = R.decoder_case(*case)
    ref = R.decode(c["z"], c["Wo"], c["bo"], c["target"], c["negmask"], act)
    status, Gb, Pb, part, npart, count = _decode(c, B, I, H, act, pad, with_pred, device)
    assert status == 0
    tb, ti = ref["grid"]
    assert npart == tb * ti == ref["partials"].v.size
    g = Gb.read(B, I, "G")
    assert not g[~ref["selected"]].any(), "G of an unselected position is not zero"
    _same(g, ref["G"], "decoder G")
    if with_pred:
        _same(Pb.read(B, I, "pred"), ref["pred"], "decoder pred")
    _same(part.read(1, npart, "partials")[0], ref["partials"], "decoder partials")
    words = _np(count).astype(np.int64)
    stride = R.COUNT_WORDS // R.COUNT_SLOTS
    want = np.zeros(R.COUNT_SLOTS, np.int64)
    T = R.DECODE_TILE
    for jb in range(tb):
        for ji in range(ti):
            want[(ji * tb + jb) % R.COUNT_SLOTS] += int(ref["selected"][jb * T:(jb + 1) * T, ji * T:(ji + 1) * T].sum())
    assert np.array_equal(words[::stride], want) and words.sum() == ref["count"]
    if rows == "none":
        assert ref["count"] == 0 and not g.any() and not part.read(1, npart, "partials").any()


def test_dense_decoder_refusals(device):
    """H % 4 != 0, a z offset by one float, ldg < I: a non-zero status, nothing written."""
    lib = _lib()
    B, I, H = 5, 9, 8
    c = R.decoder_case(B, I, H, 1, True, True, True, 0, "mixed")
    Gb, part = Guarded(B, I, device), Guarded(1, 4, device)
    count = torch.zeros(R.COUNT_WORDS, dtype=torch.int32, device=device)
    z, Wo, bo, t, m = (_t(c[k], device) for k in ("z", "Wo", "bo", "target", "negmask"))
    zoff = torch.zeros(B * H + 4, dtype=torch.float32, device=device)

    def call(zp, h, ldg):
        st = lib.yr_cdae_decode_loss(zp, Wo.data_ptr(), bo.data_ptr(), t.data_ptr(), m.data_ptr(), B, I, h, 1, Gb.ptr, ldg,
                                     None, part.ptr, count.data_ptr(), _stream())
        torch.cuda.synchronize()
        Gb.read(0, 0, "G"), part.read(0, 0, "partials")
        assert not _np(count).any()
        return st
    assert call(z.data_ptr(), 6, I) != 0
    assert call(zoff.data_ptr() + 4, H, I) != 0
    assert call(z.data_ptr(), H, I - 1) != 0


# ---- element-wise kernels -------------------------------------------------------------------------------------------

@KINDS
def test_colsum(device, exact):
    """rows around the 8-row unroll of the four waves (32 rows per pass), cols around the 64-column workgroup; plain and
    accumulated onto a non-zero out."""
    lib = _lib()
    for rows in R.COLSUM_ROWS:
        for cols in R.COLSUM_COLS:
            rs = np.random.RandomState(rows * 131 + cols)
            X, out0 = R.matrix(rs, (rows, cols), exact), R.matrix(rs, (1, cols), exact)
            Xd = _t(X, device) if rows else torch.zeros(1, device=device)
            for acc in (0, 1):
                out = Guarded(1, cols + 3, device, fill=out0 if acc else None)
                assert lib.yr_colsum(Xd.data_ptr(), rows, cols, out.ptr, acc, _stream()) == 0
                ref = R.colsum(X, out0[0] if acc else None)
                _same(out.read(1, cols, "colsum")[0], ref, "colsum", min(R.quantum(X), R.quantum(out0)) if exact else None)


@KINDS
@pytest.mark.parametrize("kind,B,H", R.SCATTER_CASES)
def test_row_scatter_add_and_hidden_init(device, kind, B, H, exact):
    """Every row the same user, all users distinct, out-of-range users skipped (scatter) or flagged with the bias left
    alone (init); B = 2,049 x H = 256 is one row past the grid cap.  The atomics' order is free: exact inputs equal
    float64."""
    lib = _lib()
    c = R.scatter_case(kind, B, H, exact)
    nu, user, Gm, dV0, bias = c["nu"], c["user"], c["G"], c["dV0"], c["bias"]
    ud = _t(user, device)
    dV = Guarded(nu + 1, H, device, fill=dV0)
    assert lib.yr_row_scatter_add(_t(Gm, device).data_ptr(), ud.data_ptr(), B, H, nu, dV.ptr, _stream()) == 0
    _same(dV.read(nu, H, "dV"), R.row_scatter_add(Gm, user, dV0), "row_scatter_add",
          min(R.quantum(Gm), R.quantum(dV0)) if exact else None)
    z = Guarded(B + 1, H, device)
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    assert lib.yr_cdae_hidden_init(z.ptr, _t(bias, device).data_ptr(), _t(dV0, device).data_ptr(), ud.data_ptr(), B, H, nu,
                                   flag.data_ptr(), _stream()) == 0
    ref, want = R.hidden_init(bias, dV0, user)
    got = z.read(B, H, "zpre")
    assert int(flag.item()) == want == (R.FLAG_BAD_USER if kind == "bad" else 0)
    _same(got, ref, "hidden_init", min(R.quantum(bias), R.quantum(dV0)) if exact else None)
    bad = (user < 0) | (user >= nu)
    assert np.array_equal(got[bad], np.broadcast_to(bias, got[bad].shape))


@pytest.mark.parametrize("n", R.EW_N)
def test_elementwise_around_the_grid_cap(device, n):
    """n = 0, 1, 255 ... 257 and one under, at, one over and twice over 2,048 x 256 elements: NS-BCE forward and
    backward with and without a mask, sigmoid, sigmoid backward (in place too) and dropout, in guarded buffers."""
    from yelprecommendation_amd import engine
    lib = _lib()
    rs = np.random.RandomState(n % 9973)
    dv = lambda a: _t(a, device) if n else torch.zeros(1, device=device)
    for with_mask in (True, False):
        p, t, m = R.bce_case(n, with_mask)
        pd, td = dv(p), dv(t)
        md = None if m is None else dv(m)
        if n:
            stats = engine.nsbce_fwd(pd, td, md)
        else:
            ws = torch.zeros(2 * R.MAX_GRID, device=device)
            stats = torch.full((2,), S, device=device)
            assert lib.yr_nsbce_fwd(None, None, None, 0, ws.data_ptr(), stats.data_ptr(), _stream()) == 0
        mean, cnt = R.nsbce_fwd(p, t, m)
        got = _np(stats)
        assert got[1] == cnt
        _same(got[:1], Out1(mean), "nsbce mean")
        if n:
            dp = Guarded(1, n + 3, device)
            gout = torch.full((1,), 0.75, device=device)
            assert lib.yr_nsbce_bwd(pd.data_ptr(), td.data_ptr(), None if md is None else md.data_ptr(), stats.data_ptr(),
                                    gout.data_ptr(), n, dp.ptr, _stream()) == 0
            ref = R.nsbce_bwd(p, t, m, cnt, 0.75)
            g = dp.read(1, n, "dpred")[0]
            assert not g[ref.v == 0].any()
            _same(g, ref, "nsbce bwd")
    x = (6.0 * rs.rand(n) - 3.0).astype(F32)
    y = (0.05 + 0.9 * rs.rand(n)).astype(F32)
    rnd = rs.rand(n).astype(F32)
    xb = Guarded(1, n + 3, device, fill=x[None, :])
    assert lib.yr_sigmoid(xb.ptr, n, _stream()) == 0
    _same(xb.read(1, n, "sigmoid")[0], R.sigmoid(x), "sigmoid")
    gb = Guarded(1, n + 3, device)
    xd, yd, rd = dv(x), dv(y), dv(rnd)
    assert lib.yr_sigmoid_bwd(xd.data_ptr(), yd.data_ptr(), gb.ptr, n, _stream()) == 0
    _same(gb.read(1, n, "sigmoid_bwd")[0], R.sigmoid_bwd(x, y), "sigmoid bwd")
    ib = Guarded(1, n + 3, device, fill=x[None, :])
    assert lib.yr_sigmoid_bwd(ib.ptr, yd.data_ptr(), ib.ptr, n, _stream()) == 0
    assert np.array_equal(ib.read(1, n, "sigmoid_bwd in place"), gb.read(1, n, "sigmoid_bwd"))
    for p_drop in (0.0, 0.3):
        db = Guarded(1, n + 3, device)
        assert lib.yr_dropout(xd.data_ptr(), rd.data_ptr(), p_drop, n, db.ptr, _stream()) == 0
        assert np.array_equal(db.read(1, n, "dropout")[0], R.dropout(x, rnd, p_drop))


def Out1(o):
    return R.Out(np.reshape(o.v, (1,)), np.reshape(o.n, (1,)), np.reshape(o.s, (1,)))


@pytest.mark.parametrize("n", [300, R.GRID_SPAN + 1])
@pytest.mark.parametrize("with_mask", [True, False])
def test_nsbce_clamps_and_empty_selection(device, n, with_mask):
    """pred exactly 0 and 1: the -100 clamp of the logs and the 1e-12 floor of the gradient's denominator, against
    the float64 restatement of the same clamps (every term is 0 or 100: the sum is certified, the mean keeps one
    divide).  No selected position: stats (0, 0) and a zero gradient."""
    from yelprecommendation_amd import engine
    lib = _lib()
    gout = torch.full((1,), 0.75, device=device)
    for kind in ("clamp", "none"):
        if kind == "none" and not with_mask:
            continue
        p, t, m = R.bce_case(n, with_mask, kind)
        pd, td, md = _t(p, device), _t(t, device), None if m is None else _t(m, device)
        stats = engine.nsbce_fwd(pd, td, md)
        mean, cnt = R.nsbce_fwd(p, t, m, certified=True)
        got = _np(stats)
        assert got[1] == cnt
        dp = Guarded(1, n + 3, device)
        assert lib.yr_nsbce_bwd(pd.data_ptr(), td.data_ptr(), None if md is None else md.data_ptr(), stats.data_ptr(),
                                gout.data_ptr(), n, dp.ptr, _stream()) == 0
        g = dp.read(1, n, "dpred")[0]
        if kind == "none":
            assert cnt == 0 and got[0] == 0 and not g.any()
            continue
        assert np.isfinite(got).all() and np.isfinite(g).all()
        _same(got[:1], Out1(mean), "nsbce clamp mean")
        _same(g, R.nsbce_bwd(p, t, m, cnt, 0.75), "nsbce clamp bwd")


@pytest.mark.parametrize("n", R.SEEDED_N)
def test_dropout_seeded_bit_for_bit(device, n):
    """The counter layout of the 10-round generator: float4 group q at the counter (q, 0, 0, 0), the seed split into
    the key's two words, word t for element 4 q + t — around 2,048 x 256 groups, seeds 0, 1234 and 2^32 + 5, p in
    {0, 0.3, 0.6}, against the NumPy restatement bit for bit."""
    lib = _lib()
    rs = np.random.RandomState(n % 9973)
    x = (0.5 + rs.rand(n)).astype(F32)
    xd = _t(x, device)
    cases = [(s, p) for s in R.SEEDS for p in R.DROP_P] if n < 100 else list(zip(R.SEEDS, (0.3, 0.6, 0.3)))
    for seed, p in cases:
        out = Guarded(1, (n + 3) // 4 * 4 + 4, device)
        assert lib.yr_dropout_seeded(xd.data_ptr(), seed, p, n, out.ptr, _stream()) == 0
        got = out.read(1, n, "dropout_seeded")[0]
        want = R.dropout_seeded(x, seed, p)
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (seed, p, bad[:8])
    if n == 5:
        off = torch.zeros(n + 8, dtype=torch.float32, device=device)
        out = Guarded(1, 12, device)
        assert lib.yr_dropout_seeded(off.data_ptr() + 4, 1, 0.3, n, out.ptr, _stream()) != 0
        assert lib.yr_dropout_seeded(xd.data_ptr(), 1, 0.3, n, out.ptr + 4, _stream()) != 0
        torch.cuda.synchronize()
        out.read(0, 0, "refused")


def test_zz_report_worst_ratios():
    """Not a check of its own: prints the largest |err| / bar per family seen by the tests above."""
    print("GEMM edges, max |err| / bar on random inputs:", {k: float("%.3g" % v) for k, v in sorted(WORST.items())})
    assert all(v < 1.0 for v in WORST.values())
