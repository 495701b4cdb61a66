"""tests/gemm_ref64.py, the float64 reference of csrc/cdae.hip, checked without a GPU: it equals the oracle that is
pinned to the reference's golden vectors; ``plan`` puts every case of tests/test_gpu_gemm_edges.py on the kernel
variant it is there for; every exact case holds its certificate (from the generated arrays); the bars it states
notice what a kernel that mishandles the end of K, a split, a tile or a grid trip would compute; and the 10-round
Philox of oracle/triplet_sampler.py reproduces the published known answer."""
import numpy as np

import gemm_ref64 as R
from oracle import cdae as ocdae
from oracle import triplet_sampler as ots

F32 = np.float32


def test_helper_equals_the_pinned_oracle():
    """One small model (B = 12, I = 70, H = 8, sigmoid / sigmoid) chained from the helper's pieces — hidden_init, gemm
    with accumulate, sigmoid, decode, nsbce, gemm with 1 / count and row sums, sigmoid_bwd, colsum, row_scatter_add —
    against oracle/cdae.py::loss_and_grads to f32 rounding; the decoder against cdae_ref64.sampled_decode."""
    rs = np.random.RandomState(3)
    B, I, H, nu = 12, 70, 8, 9
    x = (rs.rand(B, I) < 0.2).astype(F32)
    t, m = x.copy(), ((rs.rand(B, I) < 0.3) & (x == 0)).astype(F32)
    Wh, bh = (0.3 * rs.standard_normal((H, I))).astype(F32), (0.1 * rs.standard_normal(H)).astype(F32)
    V = (0.2 * rs.standard_normal((nu, H))).astype(F32)
    Wo, bo = (0.5 * rs.standard_normal((I, H))).astype(F32), (0.1 * rs.standard_normal(I)).astype(F32)
    user = rs.randint(0, nu, B)
    loss, (dWh, dbh, dV, dWo, dbo) = ocdae.loss_and_grads([Wh, bh, V, Wo, bo], user, x, t, m)
    init, flag = R.hidden_init(bh, V, user)
    assert flag == 0
    z = R.sigmoid(R.gemm(x, Wh, tB=True, C0=init.v)[0].v).v
    d = R.decode(z, Wo, bo, t, m, 1)
    cnt = d["count"]
    assert cnt == int(((t + m) != 0).sum()) and not d["G"].v[(t + m) == 0].any()
    np.testing.assert_allclose(d["partials"].v.sum() / cnt, loss, rtol=1e-5)
    mean, c2 = R.nsbce_fwd(d["pred"].v, t, m)
    assert c2 == cnt
    np.testing.assert_allclose(mean.v, loss, rtol=1e-5)
    dy = R.nsbce_bwd(d["pred"].v, t, m, cnt, 1.0).v
    np.testing.assert_allclose(R.sigmoid_bwd(dy, d["pred"].v).v, d["G"].v / cnt, rtol=1e-9, atol=1e-15)
    dWo_r, dbo_r = R.gemm(d["G"].v, z, tA=True, alpha=1.0 / cnt)
    dpre = R.sigmoid_bwd(R.gemm(d["G"].v, Wo, alpha=1.0 / cnt)[0].v, z).v
    dWh_r = R.gemm(dpre, x, tA=True)[0]
    for want, got in ((dWo, dWo_r.v), (dbo, dbo_r.v), (dWh, dWh_r.v), (dbh, R.colsum(dpre).v),
                      (dV, R.row_scatter_add(dpre, user, np.zeros_like(V)).v)):
        np.testing.assert_allclose(want, got, rtol=1e-4, atol=1e-7 + 1e-5 * np.abs(got).max())
    sd = R.sampled_decode(z, Wo, bo, t, m, 1)
    assert sd["count"] == cnt
    np.testing.assert_allclose(sd["loss"].v, d["partials"].v.sum(), rtol=1e-12)
    np.testing.assert_allclose(sd["dz"].v, d["G"].v @ Wo.astype(np.float64), rtol=1e-12, atol=1e-15)
    # identity output and plain BCE: the same arithmetic as sampled_decode on an all-ones mask
    z2, Wo2, bo2 = R.decoder_params(rs, B, H, I, 0, True)
    d2, s2 = R.decode(z2, Wo2, bo2, t, None, 0), R.sampled_decode(z2, Wo2, bo2, t, np.ones_like(t), 0)
    assert d2["count"] == s2["count"] == B * I
    np.testing.assert_allclose(s2["dbo"].v, d2["G"].v.sum(0), rtol=1e-12)


# ---- plan -----------------------------------------------------------------------------------------------------------

def _gpu_launches():
    """(M, N, K, split_k, aligned, accumulate) of every GEMM launch of tests/test_gpu_gemm_edges.py."""
    for aligned in (True, False):
        for acc in (False, True):
            for K in R.K_LADDER:
                yield R.KL_M, R.KL_N, K, 1, aligned, acc
            for M, N in R.MN_LADDER:
                yield M, N, R.MN_K, 1, aligned, acc
    for c in R.SPLIT_CASES:
        for acc in (False, True):
            yield c + (True, acc)
    for (M, N, K, _, _), _ in R.WIDE_CASES:
        yield M, N, K, 1, True, False


def test_plan_mirrors_the_host_and_reaches_every_variant():
    assert (R.GEMM_TILE, R.GEMM_K, R.TK, R.MINB, R.DECODE_TILE) == (64, 32, 16, 2048, 64)
    assert R.MAX_GRID == 2048 and R.GRID_SPAN == 524288 and R.BIG_B * R.BIG_H == R.GRID_SPAN + 256
    tiles, steps, ragged, rows, cols, generic = set(), set(), False, set(), set(), False
    for M, N, K, sk, aligned, acc in _gpu_launches():
        p = R.plan(M, N, K, sk, aligned, acc)
        assert p["splits"] >= 1 and (p["splits"] - 1) * p["kps"] < max(K, 1) and p["kps"] % R.GEMM_K == 0
        assert p["atomic"] == (p["splits"] > 1 or acc)
        if not aligned:
            generic = True
            continue
        tiles.add((p["bm"], p["bn"], p["atomic"]))
        steps.add(R.last_step(p))
        ragged |= p["splits"] > 1 and 0 < p["last"] < p["kps"]
        rows.add(R.last_tile(M, p["bm"]))
        cols.add(R.last_tile(N, p["bn"]))
    assert tiles == {(bm, bn, at) for bm in (64, 128) for bn in (64, 128) for at in (False, True)}
    assert generic and ragged and {1, 2, 3} <= steps and steps & set(range(4, 16))
    assert {1, 3, 4, 5, 31, 32, 33} <= rows and {1, 3, 4, 5, 31, 32, 33} <= cols
    for c in R.SPLIT_CASES:
        p = R.plan(*c, True)
        assert (p["bm"], p["bn"], p["splits"]) == R.SPLIT_WANT[c], c
    assert R.plan(256, 128, 4083, 128, True)["last"] == 19 and R.plan(70, 67, 40, 8, True)["last"] == 8
    for (M, N, K, _, _), tile in R.WIDE_CASES:
        p = R.plan(M, N, K, 1, True)
        assert (p["bm"], p["bn"]) == tile and not p["atomic"] and ((M + tile[0] - 1) // tile[0]) * ((N + tile[1] - 1) // tile[1]) >= R.MINB
    assert R.plan(70, 67, 0, 1, True)["splits"] == 1 and R.last_step(R.plan(70, 67, 0, 1, True)) == 0
    # the decoder cases reach every tile edge of B and I and both sides of the 16-step of H
    Bs, Is, Hs = ({c[k] for c in R.DECODER_CASES} for k in range(3))
    assert Bs == {1, 63, 64, 65, 129} and Is == {1, 63, 64, 65, 130, 193} and Hs == {4, 12, 16, 20, 36, 128}
    for k in range(3, 8):
        assert len({c[k] for c in R.DECODER_CASES}) == 2
    assert {c[8] for c in R.DECODER_CASES} == {"mixed", "none"}
    assert any(R.decode(**_dec(c))["grid"][0] > 1 and R.decode(**_dec(c))["grid"][1] > 2 for c in R.DECODER_CASES[4:5])


def _dec(case):
    c = R.decoder_case(*case)
    return dict(z=c["z"], Wo=c["Wo"], bo=c["bo"], target=c["target"], negmask=c["negmask"], act=case[3])


# ---- certificates ---------------------------------------------------------------------------------------------------

def test_every_exact_case_holds_its_certificate():
    """Over the case lists the GPU file iterates, from the generated arrays (the wide cases in row blocks)."""
    checked, top = 0, 0.0

    def hold(name, q, s):
        nonlocal checked, top
        assert R.exact(q, s), (name, q, float(np.max(s, initial=0.0)))
        checked += 1
        top = max(top, float(np.max(s, initial=0.0)) / q if np.isfinite(q) else 0.0)

    shapes = [(R.KL_M, R.KL_N, K) for K in R.K_LADDER] + [(M, N, R.MN_K) for M, N in R.MN_LADDER] + \
             [c[:3] for c in R.SPLIT_CASES]
    for M, N, K in shapes:
        o = R.operands(M, N, K, True)
        for count in (None,) + R.COUNTS[True]:
            alpha = None if count is None else R.alpha_of(count)
            prod = R.products(o["a"], o["b"], alpha)
            hold(("bias", M, N, K, count), R.gemm_quantum(o["a"], o["b"], o["bias"], alpha), R.finish(prod, o["bias"])[0].s)
            acc, rows = R.finish(prod, None, 0, o["C0"])
            hold(("C0", M, N, K, count), R.gemm_quantum(o["a"], o["b"], None, alpha, o["C0"]), acc.s)
            hold(("rowsum", M, N, K, count), R.gemm_quantum(o["a"], np.ones(1), None, alpha), rows.s)
    for (M, N, K, _, _), _ in R.WIDE_CASES:
        o = R.operands(M, N, K, True, with_c0=False)
        q = R.gemm_quantum(o["a"], o["b"], None, 0.125)
        assert q == 0.125
        for r0 in range(0, M, 1024):
            c, rows = R.finish(R.products(o["a"][r0:r0 + 1024], o["b"], 0.125))
            hold(("wide", M, N, r0), q, c.s)
            hold(("wide rowsum", M, N, r0), q, rows.s)
    for rows in R.COLSUM_ROWS:
        for cols in R.COLSUM_COLS:
            rs = np.random.RandomState(rows * 131 + cols)
            X, out0 = R.matrix(rs, (rows, cols), True), R.matrix(rs, (1, cols), True)
            hold(("colsum", rows, cols), min(R.quantum(X), R.quantum(out0)), R.colsum(X, out0[0]).s)
    for kind, B, H in R.SCATTER_CASES:
        c = R.scatter_case(kind, B, H, True)
        hold(("scatter", kind, B), min(R.quantum(c["G"]), R.quantum(c["dV0"])), R.row_scatter_add(c["G"], c["user"], c["dV0"]).s)
        hold(("init", kind, B), min(R.quantum(c["bias"]), R.quantum(c["dV0"])), R.hidden_init(c["bias"], c["dV0"], c["user"])[0].s)
    for n in (300, R.GRID_SPAN + 1):
        for with_mask in (True, False):
            p, t, m = R.bce_case(n, with_mask, "clamp")
            _, _, sel, term = R._bce_terms(p, t, m)
            assert set(np.unique(term)) <= {0.0, 100.0} and term[sel].any()
            hold(("clamp", n, with_mask), R.quantum(term), np.abs(term).sum())
    print("certificates held: %d, largest sum |terms| / quantum: %.3g of 2^24 = %.3g" % (checked, top, 2.0 ** 24))
    assert top <= 2.0 ** 24


# ---- the bars notice a mishandled end -------------------------------------------------------------------------------

class _Book:
    """Per family: the smallest perturbation / bar on random inputs; a random case below 1 needs its exact twin."""

    def __init__(self):
        self.smallest, self.below, self.count, self.low = {}, {}, {}, []

    def note(self, family, key, random_ratio, exact_differs):
        assert exact_differs, (family, key, "the exact twin does not see it")
        self.smallest[family] = min(self.smallest.get(family, np.inf), random_ratio)
        self.below[family] = self.below.get(family, 0) + (random_ratio < 1.0)
        self.count[family] = self.count.get(family, 0) + 1
        if random_ratio < 1.0:
            self.low.append((family, key))


def _both(make):
    rnd, ex = make(False), make(True)
    assert rnd.keys() == ex.keys() and len(rnd) > 0                      # every random case has its exact twin
    return [(k, rnd[k], ex[k]) for k in rnd]


def _seen(d, b, ex):
    return bool(np.any(np.asarray(d) != 0)) if ex else float(R.over(d, b).max())


def _gemm_pert(M, N, K, split_k, ex, along_k=True):
    """{name: seen} for one shape: the perturbed reference minus the reference, against the bar of the plain store
    with bias (identity), of the accumulate form and of the row sums.  ``along_k``: the perturbations of the K loop
    (the K ladder and the split cases; the M, N ladder has the row, column and bias ones)."""
    o = R.operands(M, N, K, ex)
    a, b = o["a"].astype(np.float64), o["b"].astype(np.float64)
    prod = R.products(a, b)
    out = {}
    for aligned in (True, False):
        p = R.plan(M, N, K, split_k, aligned)
        if p["splits"] > 1:
            refs = [R.finish(prod, None, 0, o["C0"], p["splits"])[0]]
        else:
            refs = [R.finish(prod, o["bias"])[0], R.finish(prod, None, 0, o["C0"])[0]]
        bars = [R.bar(r) for r in refs]
        tag = p["kernel"]

        def add(name, d):
            out[(tag, name)] = all(np.any(d != 0) for _ in bars) if ex else min(float(R.over(d, bb).max()) for bb in bars)
        if K >= 1 and along_k:
            last = a[:, K - 1:K] @ b[K - 1:K]
            add("product K - 1 dropped", -last)
            add("product K - 1 twice", last)
            ks = slice((p["last"] - 1) // p["step"] * p["step"] + (p["splits"] - 1) * p["kps"], K)
            add("last K step dropped", -(a[:, ks] @ b[ks]))
        if p["splits"] > 1:
            for j in (0, p["splits"] - 1):
                ks = slice(j * p["kps"], min(K, (j + 1) * p["kps"]))
                share = a[:, ks] @ b[ks]
                add("split %d dropped" % j, -share)
                add("split %d twice" % j, share)
        else:
            plain, acc = refs
            # the plain store keeps the sentinel in that row; the accumulate form keeps C0 (random inputs: both must
            # cross; a one-column integer product may be zero, so the exact twin is the plain store)
            out[(tag, "last row left out")] = _seen(plain.v[M - 1] - R.SENTINEL, bars[0][M - 1], ex) if ex else \
                min(_seen(plain.v[M - 1] - R.SENTINEL, bars[0][M - 1], ex), _seen(acc.v[M - 1] - o["C0"][M - 1], bars[1][M - 1], ex))
            out[(tag, "last column left out")] = _seen(plain.v[:, N - 1] - R.SENTINEL, bars[0][:, N - 1], ex)
            out[(tag, "bias of column N - 1 left out")] = _seen(np.full(M, float(o["bias"][N - 1])), bars[0][:, N - 1], ex)
        if aligned and p["splits"] == 1 and along_k:
            sc, rows = R.finish(R.products(a, b, 0.125), o["bias"])
            out[(tag, "alpha left out")] = _seen(prod[0] * 0.875, R.bar(sc), ex)
            if K >= 2:
                out[(tag, "odd k left out of the row sums")] = _seen(0.125 * a[:, 1::2].sum(1), R.bar(rows), ex)
    return out


def _wide_rowsum_pert(case, ex):
    """The row sums of the second 32-row tile of the first 128-row workgroup keep the sentinel."""
    M, N, K, _, _ = case
    o = R.operands(M, N, K, ex, with_c0=False)
    rows = R.finish(R.products(o["a"][:128], o["b"][:, :1], 0.125))[1]
    return {"rows 32 .. 63 left out": _seen(rows.v[32:64] - R.SENTINEL, R.bar(rows)[32:64], ex)}


def test_every_bar_notices_a_mishandled_end():
    """Each perturbed reference crosses the bar computed from the reference alone, or — where the any-order bound of a
    long random sum is as wide as one product: the K = 4,083 split cases and (24, 16, 1000, 4), where the largest of
    70 x 67 ... 513 x 512 lost products still crosses by a factor of 1.25 but a typical one does not; the mean of
    524,289 loss terms — the exact twin of the same case, which is compared for equality, differs.  The exact twin differs for EVERY perturbation; every case
    with K <= 136 crosses its bar on the random inputs on its own."""
    book = _Book()
    shapes = [(R.KL_M, R.KL_N, K, 1, True) for K in R.K_LADDER if K] + [(M, N, R.MN_K, 1, False) for M, N in R.MN_LADDER] + \
             [c + (True,) for c in R.SPLIT_CASES]
    for M, N, K, sk, along_k in shapes:
        fam = "gemm" if K <= 136 else "gemm long K"
        for key, rr, ee in _both(lambda ex: _gemm_pert(M, N, K, sk, ex, along_k)):
            book.note(fam, (M, N, K, sk) + key, rr, ee)
            if K <= 136:
                assert rr >= 1.0, ((M, N, K, sk) + key, rr)
    for case, tile in R.WIDE_CASES:
        if tile[0] == 128:
            for key, rr, ee in _both(lambda ex: _wide_rowsum_pert(case, ex)):
                book.note("gemm", case + (key,), rr, ee)
                assert rr >= 1.0
    # the random inputs themselves: one lost product is at least 0.25, the bar of K <= 136 at most 9e-3
    o = R.operands(R.KL_M, R.KL_N, 49, False)
    assert np.abs(o["a"]).min() >= 0.5 and np.abs(o["b"]).min() >= 0.5 and np.abs(o["a"]).max() <= 2.0
    assert 2 * 137 * R.U24 * 544 < 9e-3

    # decoder: a position not counted (the integer count), G of an unselected position (exactly 0 is demanded), one
    # tile's partial at the transposed index (must cross the bar: the partials are floats)
    for case in R.DECODER_CASES:
        kw = _dec(case)
        ref = R.decode(**kw)
        tb, ti = ref["grid"]
        sel = ref["selected"]
        if ref["count"]:
            assert ref["count"] - 1 != ref["count"]
        if not sel.all():
            everywhere = R.decode(**dict(kw, negmask=None, target=np.maximum(kw["target"], 0)))["G"].v
            leak = np.where(sel, 0.0, everywhere)
            book.note("decoder", case + ("unselected G",), float("inf") if leak.any() else 0.0, bool(leak.any()))
        if tb > 1 and ti > 1 and ref["count"]:
            swapped = ref["partials"].v.reshape(ti, tb).T.reshape(-1) if tb == ti else None
            if swapped is None:                      # tb != ti: the partial of tile (jb, ji) stored at jb * ti + ji
                swapped = np.empty(tb * ti)
                for jb in range(tb):
                    for ji in range(ti):
                        swapped[jb * ti + ji] = ref["partials"].v[ji * tb + jb]
            rr = float(R.over(swapped - ref["partials"].v, R.bar(ref["partials"])).max())
            book.note("decoder", case + ("partial transposed",), rr, rr >= 1.0)
            assert rr >= 1.0, (case, rr)
    assert book.count["decoder"] >= 10

    # element-wise: the last row of a column sum, row 32 of 33, the first element of the second grid trip of the loss
    def colsum_pert(ex):
        out = {}
        for rows in R.COLSUM_ROWS[1:]:
            for cols in R.COLSUM_COLS:
                rs = np.random.RandomState(rows * 131 + cols)
                X = R.matrix(rs, (rows, cols), ex)
                if ex:
                    X[rows - 1, 0] = 1.0
                ref = R.colsum(X)
                drops = [rows - 1] + ([32] if rows == 33 else [])
                for r in drops:
                    w = np.ones(rows); w[r] = 0.0
                    out[(rows, cols, r)] = _seen(R.colsum(X, rw=w).v - ref.v, R.bar(ref), ex)
        return out
    for key, rr, ee in _both(colsum_pert):
        book.note("colsum", key, rr, ee)
        assert rr >= 1.0 or key[0] == 1000, (key, rr)

    for n in (R.GRID_SPAN + 1, 2 * R.GRID_SPAN + 1):
        for with_mask in (True, False):
            w = np.ones(n); w[R.GRID_SPAN] = 0.0
            p, t, m = R.bce_case(n, with_mask)
            ref, cnt = R.nsbce_fwd(p, t, m)
            got, cnt2 = R.nsbce_fwd(p, t, m, ew=w)
            rr = float(R.over(got.v - ref.v, R.bar(ref)))
            assert cnt2 == cnt - 1                                           # the count is exact: it notices on its own
            p, t, m = R.bce_case(n if n == R.GRID_SPAN + 1 else 300, with_mask, "clamp")
            if n == R.GRID_SPAN + 1:
                a, b = R.nsbce_fwd(p, t, m, certified=True)[0], R.nsbce_fwd(p, t, m, ew=w, certified=True)[0]
                ee = float(R.over(b.v - a.v, R.bar(a))) >= 1.0
            else:
                ee = True                                                    # the count alone
            book.note("loss", (n, with_mask), rr, ee)

    print("smallest perturbation / bar on random inputs per family (cases below 1 of all, each caught by its exact twin):")
    for f in book.smallest:
        print("  %-12s %10.3g   (%d of %d below 1)" % (f, book.smallest[f], book.below[f], book.count[f]))
    print("  below 1:", sorted({k[:4] for f, k in book.low if f == "gemm long K"}), [k for f, k in book.low if f != "gemm long K"])
    assert book.below["gemm"] == 0 and book.below["decoder"] == 0
    assert {k[:4] for f, k in book.low if f == "gemm long K"} <= {c for c in R.SPLIT_CASES if c[2] >= 1000}


# ---- Philox ---------------------------------------------------------------------------------------------------------

def test_philox_ten_rounds_known_answer_and_seeded_dropout():
    """Philox4x32-10 at counter 0, key 0 gives the published 6627e8d5 e169c58d bc57ac4c 9b00dbd8 (Random123's
    kat_vectors); the 7-round name is the same function at 7 rounds; dropout_seeded uses word t of group q for element
    4 q + t, the seed's halves as the key and u01 of the top 24 bits."""
    w = ots.philox4x32(0, 0, 0, 0, 0, 0, 10)
    assert [int(x) for x in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    w = ots.philox4x32(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 10)
    assert [int(x) for x in w] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    c = np.arange(5, dtype=np.uint64)
    a, b = ots._philox4x32_7(c, c + 1, c * 3, c * 0, 11, 12), ots.philox4x32(c, c + 1, c * 3, c * 0, 11, 12, 7)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[0], ots.philox4x32(c, c + 1, c * 3, c * 0, 11, 12, 10)[0])
    assert float(R.u01([0xFFFFFFFF])[0]) == 1.0 - 2.0 ** -24 and float(R.u01([255])[0]) == 0.0
    x = (1.0 + np.arange(23)).astype(F32)
    seed = 2 ** 32 + 5
    assert np.array_equal(R.dropout_seeded(x, seed, 0.0), x)
    for p in (0.3, 0.6):
        got = R.dropout_seeded(x, seed, p)
        for e in (0, 5, 14, 22):
            q, t = divmod(e, 4)
            word = int(ots.philox4x32(q, 0, 0, 0, 5, 1, 10)[t])
            keep = F32(word >> 8) * F32(2.0 ** -24) >= F32(p)
            assert got[e] == (x[e] * F32(1.0 / (1.0 - p)) if keep else 0.0)
    assert not np.array_equal(R.dropout_seeded(x, 5, 0.3), R.dropout_seeded(x, seed, 0.3))      # the key's high word counts
    big = R.dropout_seeded(np.ones(40000, F32), 1234, 0.3)
    assert abs((big == 0).mean() - 0.3) < 0.01
