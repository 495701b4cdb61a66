"""tests/ngcf_ref64.py, the float64 reference of the NGCF kernels, checked without a GPU: it equals the oracle that is
pinned to the reference's golden vectors; every "exact" case of tests/test_gpu_ngcf_edges.py holds its certificate
(computed from the generated arrays — no case falls back on the generators' value ranges: the largest, dW over
262,401 rows and the 65,601-triplet score batch, take a few hundred milliseconds in NumPy); and the bars it states
notice what a kernel that mishandles the end of a row, a tile, a chunk or a list would compute."""
import numpy as np
import pytest

import ngcf_ref64 as R
from oracle import bpr_mf as obpr
from oracle import ngcf as ongcf

F32 = np.float32


def _graph(rs, nu, ni):
    u = np.repeat(np.arange(nu), 6)
    i = rs.randint(0, ni, u.shape[0])
    L = ongcf.laplacian_csr(u, i, rs.randint(1, 6, u.shape[0]), nu, ni)
    return L, (L.indptr, L.indices, L.data)


@pytest.mark.parametrize("d", [16, 64])
def test_reference_equals_the_pinned_oracle(d):
    """300 nodes: oracle.ngcf.propagate / propagate_backward stage by stage (each stage of the reference fed the
    oracle's own f32 inputs, inside the bars the reference states for an f32 computation), then the scores and all
    gradients of loss_and_grads against the float64 chain at the project's gradient bar (test_model_probe_...)."""
    rs = np.random.RandomState(d)
    nu, ni = 200, 100
    L, csr = _graph(rs, nu, ni)
    E = (0.5 * rs.standard_normal((nu + ni, d))).astype(F32)
    W1s = [(rs.standard_normal((d, d)) / np.sqrt(d)).astype(F32) for _ in range(2)]
    W2s = [(rs.standard_normal((d, d)) / np.sqrt(d)).astype(F32) for _ in range(2)]
    out, cache = ongcf.propagate(E, W1s[0], W2s[0], L)
    Z = cache[1]
    worst = {"Z": R.ratio(Z, R.spmm(*csr, E), "spmm"), "Eout": R.ratio(out, R.dense_fwd(E, Z, W1s[0], W2s[0])[0], "fwd")}
    dnext = rs.standard_normal(out.shape).astype(F32)
    dE, dW1, dW2 = ongcf.propagate_backward(dnext, cache, W1s[0], W2s[0], L)
    rdZ, rdE, rdW1, rdW2 = R.dense_bwd(dnext, out, E, Z, W1s[0], W2s[0], np.zeros_like(E))
    worst["dW1"], worst["dW2"] = R.ratio(dW1, rdW1, "dw"), R.ratio(dW2, rdW2, "dw")
    back = R.spmm(*csr, rdZ.v.astype(F32))                              # L symmetric: L^T dZ = L dZ
    total = R.Out(rdE.v + back.v, rdE.n + back.n + 1.0, rdE.s + back.s)
    # the oracle's dZ is an f32 computation of its own: its error reaches dE through |L|
    carried = abs(L).astype(np.float64) @ R.bar(rdZ, "dz")
    worst["dE"] = float(R.over(dE - total.v, R.bar(total, "de") + carried).max())
    print("oracle vs ngcf_ref64, max |err| / bar:", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) < 1.0, worst

    B = 64
    u, p, n = rs.randint(0, nu, B), rs.randint(0, ni, B), rs.randint(0, ni, B)
    layers, Zs = [E.astype(np.float64)], []
    for W1, W2 in zip(W1s, W2s):
        Zs.append(R.spmm(*csr, layers[-1]).v)
        layers.append(R.dense_fwd(layers[-1], Zs[-1], W1, W2)[0].v)
    pos, neg = R.score(layers, nu, u, p, n)
    opos, oneg = ongcf.bpr_forward(E, W1s, W2s, L, nu, u, p, n)
    np.testing.assert_allclose(opos, pos.v, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(oneg, neg.v, rtol=1e-4, atol=1e-5)
    loss, odE0, odW1, odW2 = ongcf.loss_and_grads(E, W1s, W2s, L, nu, u, p, n)
    x = pos.v - neg.v
    np.testing.assert_allclose(float(loss), np.mean(np.logaddexp(0.0, -x)), rtol=1e-5)
    g = -1.0 / (1.0 + np.exp(x)) / B
    np.testing.assert_allclose(obpr.bpr_coeff(opos, oneg), g, rtol=1e-4, atol=1e-9)
    d_outs = R.score_bwd(layers, nu, u, p, n, g, -g)
    carry, dWs = d_outs[2].v, {}
    for k in (1, 0):
        dZ, dEk, dWs[("W1", k)], dWs[("W2", k)] = R.dense_bwd(carry, layers[k + 1], layers[k], Zs[k], W1s[k], W2s[k],
                                                              d_outs[k].v)
        carry = dEk.v + R.spmm(*csr, dZ.v).v
    for want, got in [(odE0, carry)] + [(odW1[k], dWs[("W1", k)].v) for k in (0, 1)] + \
                     [(odW2[k], dWs[("W2", k)].v) for k in (0, 1)]:
        np.testing.assert_allclose(want, got, rtol=1e-3, atol=1e-6 + 1e-4 * np.abs(got).max())


def test_quantum_and_certificate():
    assert R.quantum([3.0, -0.375, 0.0]) == 0.125 and R.quantum([0.0]) == np.inf and R.quantum([F32(0.01)]) <= 2.0 ** -29
    assert R.exact(0.125, [2.0 ** 21]) and not R.exact(0.125, [2.0 ** 21 + 0.125]) and not R.exact(0.3, [1.0])
    assert R.exact(np.inf, np.zeros(3))
    # the certificate means what it says: f32 sums of such terms in two opposite orders equal the float64 sum
    rs = np.random.RandomState(0)
    t = (rs.randint(-40, 41, 400000) / 16.0).astype(F32)
    assert R.exact(R.quantum(t), np.abs(t.astype(np.float64)).sum())
    fwd = np.add.reduce(t, dtype=F32)
    acc = F32(0)
    for x in t[::-1][:5000]:
        acc = F32(acc + x)
    assert float(fwd) == t.astype(np.float64).sum() and float(acc) == t[::-1][:5000].astype(np.float64).sum()


# ---- the cases of the GPU file, evaluated by the reference ----------------------------------------------------------

def _spmm_kinds(D):
    return R.SPMM_KINDS + (("big",) if D == 16 else ())


def _dense_certs(c, rows=None):
    """Certified outputs of one exact dense case: [(name, Out, quantum)]."""
    E, Z = c["E"].astype(np.float64), c["Z"].astype(np.float64)
    A, H = Z + E, E * Z
    assert np.array_equal(A.astype(F32), A) and np.array_equal(H.astype(F32), H)     # the kernel's rounding is exact
    _, P = R.dense_fwd(c["E"], c["Z"], c["W1"], c["W2"])
    qP = min(R.quantum(A) * R.quantum(c["W1"]), R.quantum(H) * R.quantum(c["W2"]))
    assert not np.any(c["dEout"][c["Eout"] <= 0])                                     # dP = dEout exactly
    dZ, dE, dW1, dW2 = R.dense_bwd(c["dEout"], c["Eout"], c["E"], c["Z"], c["W1"], c["W2"], c["dE0"], rows=rows)
    qd = R.quantum(c["dEout"]) * R.quantum(c["W1"], c["W2"])
    on = slice(None) if rows is None else np.unique(rows)
    return [("P", P, qP), ("dZ", dZ[on], min(qd, qd * R.quantum(E))), ("dE", dE, min(qd, qd * R.quantum(Z), R.quantum(c["dE0"]))),
            ("dW1", dW1.plus(c["dW10"]), min(R.quantum(c["dEout"]) * R.quantum(A), R.quantum(c["dW10"]))),
            ("dW2", dW2.plus(c["dW20"]), min(R.quantum(c["dEout"]) * R.quantum(H), R.quantum(c["dW20"])))]


def test_every_exact_case_holds_its_certificate():
    """Over the same case lists that tests/test_gpu_ngcf_edges.py iterates, from the generated arrays."""
    checked, top = 0, 0.0

    def hold(name, o, q):
        nonlocal checked, top
        assert R.exact(q, o.s), (name, q, float(np.max(o.s)))
        checked += 1
        top = max(top, float(np.max(o.s, initial=0.0)) / q)

    for D in R.WIDTHS:
        for kind in _spmm_kinds(D):
            c = R.spmm_case(D, kind, True)
            o = R.spmm(c["rowptr"], c["col"], c["val"], c["X"], accumulate_into=c["Y0"])
            hold(("spmm", D, kind), o, min(R.quantum(c["val"]) * R.quantum(c["X"]), R.quantum(c["Y0"])))
        for n in R.DENSE_N + tuple(n for n, _ in R.dw_sizes(D)):
            for name, o, q in _dense_certs(R.dense_case(D, n, True)):
                hold(("dense", D, n, name), o, q)
        for j, (count, _) in enumerate(R.LIST_CASES):
            if count:
                for name, o, q in _dense_certs(R.dense_case(D, R.LIST_N, True, seed=j), R.row_list(R.LIST_N, count, j)):
                    hold(("dense rows", D, count, name), o, q)
        for j, (n, count, _) in enumerate(R.dw_list_cases(D)):
            for name, o, q in _dense_certs(R.dense_case(D, n, True, seed=j), R.row_list(n, count, j)):
                hold(("dW rows", D, count, name), o, q)
        c = R.push_case(D, True)
        for which, rows in c["lists"].items():
            o = R.push_rows(c["rowptr"], c["col"], c["val"], c["X"], c["Y0"], rows)
            hold(("push", D, which), o, min(R.quantum(c["val"]) * R.quantum(c["X"]), R.quantum(c["Y0"])))
        for layers in (1, 8):
            for B in R.score_batches(D):
                _score_certs(hold, D, layers, B, True)
        _score_certs(hold, D, 2, R.score_batches(D)[-1], False)
        _score_certs(hold, D, 2, 300, True, same_user=True)
    _score_certs(hold, *R.BIG_SCORE, True)
    print("certificates held: %d, largest sum |terms| / quantum: %.3g of 2^24 = %.3g" % (checked, top, 2.0 ** 24))
    # the dW sums over 262,401 rows are the largest: 18 n = 4.7 M quanta at the edge of the value ranges, about a tenth
    # of that on the generated arrays (half of dEout is zero)
    assert 4.0e5 <= top <= 4.8e6


def _score_certs(hold, D, layers, B, with_neg, same_user=False):
    c = R.score_case(D, layers, B, with_neg, same_user)
    pos, neg = R.score(c["layers"], R.SCORE_USERS, c["u"], c["p"], c["n"])
    q = R.quantum(*c["layers"]) ** 2
    hold(("score", D, layers, B), pos, q)
    if with_neg:
        hold(("score neg", D, layers, B), neg, q)
    for o in R.score_bwd(c["layers"], R.SCORE_USERS, c["u"], c["p"], c["n"], c["gpos"], c["gneg"]):
        hold(("score bwd", D, layers, B), o, R.quantum(c["gpos"], *([c["gneg"]] if with_neg else [])) * R.quantum(*c["layers"]))


# ---- the bars notice a mishandled end -------------------------------------------------------------------------------

class _Book:
    """Per family: the smallest perturbation / bar on random inputs; a random case below 1 needs its exact twin."""

    def __init__(self):
        self.smallest, self.below, self.count = {}, {}, {}

    def note(self, family, key, random_ratio, exact_differs):
        assert exact_differs, (family, key, "the exact twin does not see it")
        assert random_ratio >= 1.0 or exact_differs, (family, key, random_ratio)
        self.smallest[family] = min(self.smallest.get(family, np.inf), random_ratio)
        self.below[family] = self.below.get(family, 0) + (random_ratio < 1.0)
        self.count[family] = self.count.get(family, 0) + 1


def _both(make):
    """(random ratios, exact differences) of one perturbation family: make(exact_inputs) -> {key: value}."""
    rnd, ex = make(False), make(True)
    assert rnd.keys() == ex.keys() and len(rnd) > 0                      # every random case has its exact twin
    return [(k, rnd[k], ex[k]) for k in rnd]


def _spmm_pert(D, kind, ex):
    c = R.spmm_case(D, kind, ex)
    csr = (c["rowptr"], c["col"], c["val"], c["X"])
    ref = R.spmm(*csr, accumulate_into=c["Y0"])
    b = R.bar(ref, "spmm")
    out = {}
    for key, (r, w) in R.spmm_perturbations(c, D).items():
        d = R.spmm(*csr, accumulate_into=c["Y0"], weight=w).v[r] - ref.v[r]
        out[key] = bool(np.any(d != 0)) if ex else float(R.over(d, b[r]).max())
    return out


def _dense_pert(D, ex):
    """Output row 32 of n = 33 left out: Eout and dZ keep the pre-fill, dE keeps dE0, dW misses the row."""
    c = R.dense_case(D, 33, ex)
    args = (c["dEout"], c["Eout"], c["E"], c["Z"], c["W1"], c["W2"], c["dE0"])
    fwd, _ = R.dense_fwd(c["E"], c["Z"], c["W1"], c["W2"])
    dZ, dE, dW1, dW2 = R.dense_bwd(*args)
    _, pE, pW1, pW2 = R.dense_bwd(*args, rows=np.arange(32))
    pairs = {"Eout": (fwd.v[32] - R.SENTINEL, R.bar(fwd, "fwd")[32]), "dZ": (dZ.v[32] - R.SENTINEL, R.bar(dZ, "dz")[32]),
             "dE": (dE.v[32] - pE.v[32], R.bar(dE, "de")[32]), "dW1": (dW1.v - pW1.v, R.bar(dW1, "dw")),
             "dW2": (dW2.v - pW2.v, R.bar(dW2, "dw"))}
    return {k: bool(np.any(d != 0)) if ex else float(R.over(d, b).max()) for k, (d, b) in pairs.items()}


def _dw_pert(D, n, ex, rows_full, variants, seed=0):
    c = R.dense_case(D, n, ex, seed=seed)
    args = (c["dEout"], c["Eout"], c["E"], c["Z"], c["W1"], c["W2"], c["dE0"])
    _, dE, dW1, dW2 = R.dense_bwd(*args, rows=rows_full)
    refs = (dW1.plus(c["dW10"]), dW2.plus(c["dW20"]))
    out = {}
    for name, rows in variants.items():
        _, pE, pW1, pW2 = R.dense_bwd(*args, rows=rows)
        ds = [(pW1.v - dW1.v, R.bar(refs[0], "dw")), (pW2.v - dW2.v, R.bar(refs[1], "dw")), (pE.v - dE.v, R.bar(dE, "de"))]
        out[name] = (any(bool(np.any(d != 0)) for d, _ in ds[:2]) and bool(np.any(ds[2][0] != 0))) if ex else \
            min(max(float(R.over(d, b).max()) for d, b in ds[:2]), float(R.over(*ds[2]).max()))
    return out


def _push_pert(D, ex):
    c = R.push_case(D, ex)
    csr = (c["rowptr"], c["col"], c["val"], c["X"], c["Y0"])
    out = {}
    for which, rows in c["lists"].items():
        ref = R.push_rows(*csr, rows)
        b = R.bar(ref, "push")
        at = int(np.flatnonzero(np.diff(c["rowptr"])[rows] > 0)[-1])          # the last listed row that has entries
        variants = {"row left out": (np.delete(rows, at), None), "row twice": (np.append(rows, rows[at]), None)}
        for r, k in enumerate(c["special"]):
            if k:
                w = np.ones(len(c["col"]))
                lo = int(c["rowptr"][r])
                w[lo + k * (R.PUSH_PARTS - 1) // R.PUSH_PARTS:lo + k] = 0.0
                variants[("last part dropped", k)] = (rows, w)
        for name, (rr, w) in variants.items():
            d = R.push_rows(*csr, rr, weight=w).v - ref.v
            out[(which, name)] = bool(np.any(d != 0)) if ex else float(R.over(d, b).max())
    return out


def test_every_bar_notices_a_mishandled_end():
    """For every GPU case that has a bar: the bar computed from the reference alone is crossed by each perturbed
    reference, or — where the any-order bound of a long random sum is wider than one term — the exact twin of the
    same case, which is compared for equality, differs.  The exact twin differs for EVERY perturbation."""
    book = _Book()
    for D in R.WIDTHS:
        for kind in ("ladder",):
            for key, rr, ee in _both(lambda ex: _spmm_pert(D, kind, ex)):
                book.note("spmm", (D, kind) + key, rr, ee)
        for key, rr, ee in _both(lambda ex: _dense_pert(D, ex)):
            book.note("dense layer", (D, key), rr, ee)
        rw = R.wrows(D)
        for n, _ in R.dw_sizes(D):
            cut = np.arange((n - 1) // rw * rw)
            for key, rr, ee in _both(lambda ex: {k: v for k, v in _dw_pert(
                    D, n, ex, None, {"last chunk left out": cut}).items()}):
                book.note("dW", (D, n, key), rr, ee)
        for j, (count, _) in enumerate(R.LIST_CASES):
            if count:
                rows = R.row_list(R.LIST_N, count, j)
                var = {"row left out": rows[:-1], "row twice": np.append(rows, rows[0])}
                for key, rr, ee in _both(lambda ex: _dw_pert(D, R.LIST_N, ex, rows, var, seed=j)):
                    book.note("dense rows", (D, count, key), rr, ee)
        for j, (n, count, _) in enumerate(R.dw_list_cases(D)):
            rows = R.row_list(n, count, j)
            var = {"row left out": rows[:-1], "row twice": np.append(rows, rows[0]),
                   "last chunk left out": rows[:(count - 1) // rw * rw]}
            for key, rr, ee in _both(lambda ex: _dw_pert(D, n, ex, rows, var, seed=j)):
                book.note("dW rows", (D, count, key), rr, ee)
        for key, rr, ee in _both(lambda ex: _push_pert(D, ex)):
            book.note("push", (D,) + key, rr, ee)
        # scores have exact cases only: one triplet dropped changes the gradient, its score is one output of its own
        for B in R.score_batches(D):
            c = R.score_case(D, 2, B, True)
            ref = R.score_bwd(c["layers"], R.SCORE_USERS, c["u"], c["p"], c["n"], c["gpos"], c["gneg"])
            w = np.ones(B); w[B - 1] = 0.0
            got = R.score_bwd(c["layers"], R.SCORE_USERS, c["u"], c["p"], c["n"], c["gpos"], c["gneg"], weight=w)
            assert any(np.any(a.v != b.v) for a, b in zip(ref, got)), (D, B)
            pos, _ = R.score(c["layers"], R.SCORE_USERS, c["u"], c["p"], c["n"])
            assert pos.v[B - 1] != 0 or np.any(pos.v != 0)
    print("smallest perturbation / bar on random inputs per family (cases below 1 of all, each caught by its exact twin):")
    for f in book.smallest:
        print("  %-12s %10.3g   (%d of %d below 1)" % (f, book.smallest[f], book.below[f], book.count[f]))
    # short sums are noticed on random inputs as well: every ladder row of at most 129 entries, every tile edge
    for D in R.WIDTHS:
        for key, rr, _ in _both(lambda ex: _spmm_pert(D, "ladder", ex)):
            if key[0] <= 129 and key[1] != "fourth wave's share dropped":
                assert rr >= 1.0, (D, key, rr)
    assert book.below["dense layer"] == 0 and book.below["dense rows"] == 0


def test_csr_builder_lengths_and_symmetric_closure():
    rs = np.random.RandomState(2)
    lengths = np.array([0, 1, 2, 40, 7, 0, 3] + [2] * 33)
    rowptr, col, val = R.csr_with_lengths(rs, lengths, len(lengths), True)
    assert np.array_equal(np.diff(rowptr), lengths)
    assert all(np.all(np.diff(col[a:b]) > 0) for a, b in zip(rowptr[:-1], rowptr[1:]))       # distinct, sorted
    assert R.quantum(val) >= 2.0 ** -4 and np.abs(val).max() <= 0.5
    rp, cc, vv = R.csr_with_lengths(np.random.RandomState(2), lengths, len(lengths), False, symmetric=True)
    M = R._csr(rp, cc, vv, len(lengths))
    assert abs(M - M.T).max() == 0 and M.nnz >= lengths.sum() and np.abs(vv).min() >= 0.5
