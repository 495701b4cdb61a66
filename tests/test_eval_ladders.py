"""The fused evaluation (csrc/eval_topk.hip) against float64 on certified score ladders (tests/eval_ladders.py):
exact list equality, no near-tie escape.  CPU: the builder's certificate holds for every case family, and a NumPy
emulation of the sweep's arithmetic reproduces the lists while weakened emulations do not (the ladders can catch a
degraded kernel).  GPU: every form of the kernel, every threshold source, masks and item bias, == float64."""
import itertools

import numpy as np
import pytest

import eval_ladders as el


# ---- CPU -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_certificate_holds_for_every_family(D):
    """build_case() certifies (asserts) every case; here: every family kind is present and has the property its name
    promises, at every D."""
    for N, n, k, bias in ((33, 40, 1, False), (33, 10, 16, True), (4100, 64, 10, True), (4100, 64, 16, False)):
        case = el.build_case(D, N, n, k, bias=bias, seed=D + k)
        exp = case.expected[el.MASK_VALUE]
        S = case.scores64(mask_value=el.MASK_VALUE)
        A = case.scale64(np.arange(n))
        if N == 4100:
            want = {"plain", "wide", "ties", "cancel+", "cancel0", "cancel-"} | ({"bias"} if bias else set())
            assert set(case.kinds) == want
        for r in range(n):
            kind = case.kinds[case.family[r]]
            kth = exp[r, k - 1]
            if kind.startswith("cancel"):
                s = S[r, kth]
                assert {"cancel+": s > 0, "cancel0": s == 0, "cancel-": s < 0}[kind], (r, kind, s)
                assert abs(s) * 1e3 <= A[r, kth] or case.zero_row[kth]
            if kind == "ties" and k < len(case.ladders[case.family[r]]) and not len(case.masks[r]):
                a, b = case.ladders[case.family[r]][k - 1:k + 1]
                assert np.array_equal(case.I[a], case.I[b]) and kth == min(a, b)   # the tie straddles the k-th place
            if kind == "bias":
                ids = case.ladders[case.family[r]]
                assert all(np.array_equal(case.I[ids[0]], case.I[j]) for j in ids)
        # full-mantissa ladder items: all three bf16 planes non-zero
        lad = np.array([j for f, ids in enumerate(case.ladders) if case.kinds[f] != "bias" for j in ids])
        x1, x2, x3 = el.split3(case.I[lad][:, el.NGATES:])
        assert np.mean(x3 != 0) > 0.9
        # planted items at the edges of tiles, stages and slices, and in the ragged last tile
        planted = {j for ids in case.ladders for j in ids} | set(np.flatnonzero(case.zero_row).tolist())
        awkward = set(el.awkward_positions(n, N, np.random.RandomState(0)))
        assert len(planted & awkward) == min(len(planted), len(awkward))
        assert all(p in planted for p in range(N // 32 * 32, N))


def _emulate(case, rows, mode, rs):
    """f32 scores of the rows as the sweep computes them ("six": the six bf16 partial products of every product, f32
    accumulation in a shuffled order) or as a degraded kernel would ("one": x1 y1 only; "nocross": without the 2^-9
    cross products x1 y2, x2 y1; "perturb": exact f32 scores moved by up to 2^-16 A)."""
    N = case.I.shape[0]
    out = np.empty((len(rows), N), np.float64)
    ip = el.split3(case.I)
    pairs = {"six": ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)), "one": ((0, 0),),
             "nocross": ((0, 0), (1, 1), (0, 2), (2, 0))}
    for q, r in enumerate(rows):
        u = case.U[case.users[r]]
        if mode == "perturb":
            s = case.scores64([r]).astype(np.float32).astype(np.float64)[0]
            out[q] = s + rs.uniform(-1, 1, N) * 2.0 ** -16 * case.scale64([r])[0]
            continue
        up = el.split3(u)
        terms = [ip[b] * up[a][None, :] for a, b in pairs[mode]]       # exact in f32 (bf16 x bf16)
        T = np.concatenate(terms, axis=1).astype(np.float32)
        if case.bias is not None:
            T = np.concatenate([case.bias[:, None], T], axis=1)
        T = T[:, rs.permutation(T.shape[1])]
        acc = np.zeros(N, np.float32)
        for c in range(T.shape[1]):
            acc = (acc + T[:, c]).astype(np.float32)
        out[q] = acc
    for q, r in enumerate(rows):
        out[q, case.masks[r]] = float(np.float32(el.MASK_VALUE))
    return el.order_rows(out, case.k)


def test_ladders_discriminate_degraded_arithmetic():
    """The committed proof that the ladders catch a degraded kernel: the emulated sweep arithmetic reproduces every
    certified list exactly, while one bf16 product, the split without the 2^-9 cross products, and f32 scores
    perturbed by up to 2^-16 A each get a large fraction of the rows wrong."""
    rs = np.random.RandomState(5)
    fails = {m: [] for m in ("one", "nocross", "perturb")}
    for D, bias in ((16, False), (32, True)):
        case = el.build_case(D, 300, 96, 10, bias=bias, seed=11 + D, mask_values=(el.MASK_VALUE,))
        rows = np.arange(96)
        want = case.expected[el.MASK_VALUE]
        assert np.array_equal(_emulate(case, rows, "six", rs), want)
        for m in fails:
            fails[m].append(np.mean((_emulate(case, rows, m, rs) != want).any(axis=1)))
    frac = {m: float(np.mean(v)) for m, v in fails.items()}
    assert frac["one"] >= 0.85, frac
    assert frac["nocross"] >= 0.85, frac
    assert frac["perturb"] >= 0.7, frac


# ---- GPU -------------------------------------------------------------------------------------------------------------

def _cases():
    """(D, N, rows, k, bias): every D with every list length it supports, catalogues of 33 / 4,100 / 16,411 items and
    5 / 300 / 2,100 rows rotated over them, item bias on every other case."""
    pairs = [(33, 300), (4100, 5), (16411, 2100), (16411, 5), (4100, 300), (33, 2100)]
    out = []
    for di, D in enumerate((16, 32, 64, 128)):
        ks = [1, 10, 16] + ([32] if D <= 64 else [])
        for i, k in enumerate(ks):
            N, n = pairs[(i + 2 * di) % len(pairs)]
            out.append((D, N, n, k, (i + di) % 2 == 1))
    out.append((128, 16411, 2100, 10, False))         # the library's two-role rule (D = 128 from 2,048 rows), no bias
    out.append((64, 4100, 2100, 16, True))
    return out


CASES = _cases()
_BUILT = {}


def _case(spec):
    if spec not in _BUILT:
        D, N, n, k, bias = spec
        _BUILT[spec] = el.build_case(D, N, n, k, bias=bias, seed=1000 + 7 * D + N + n + k + bias)
    return _BUILT[spec]


def _two_roles_exist(D, k):
    return (D == 64 and k <= 16) or (D == 128 and k <= 10)


def _check(engine, case, tensors, mv, hint, kw):
    U, I, users, ptr, idx, b = tensors
    run = {key: v for key, v in kw.items() if key != "hint"}
    got = engine.mf_eval_topk(U, I, users, ptr, idx, case.k, mask_value=mv, item_bias=b, hint=hint, **run).cpu().numpy()
    want = case.expected[mv]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (f"{kw} mask={mv}: {len(bad)} of {len(want)} rows differ, first row {bad[0]} "
                           f"({case.kinds[case.family[bad[0]]]}): {got[bad[0]].tolist()} != {want[bad[0]].tolist()}")


@pytest.mark.gpu
@pytest.mark.parametrize("spec", CASES, ids=lambda s: "D{}-N{}-n{}-k{}-{}".format(*s[:4], "bias" if s[4] else "nobias"))
def test_fused_evaluation_equals_float64_on_certified_ladders(device, spec):
    """engine.mf_eval_topk == the certified float64 lists, exactly, in both precisions, both forms of the split sweep,
    prescan off / on, catalogue slices on / off, hint lists (none, the expected lists, the expected lists with the
    k-th entry replaced by the (k+1)-th, junk ids) and every mask value; mf_recommend (fused and unfused) too."""
    import torch
    from yelprecommendation_amd import engine
    D, N, n, k, bias = spec
    case = _case(spec)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    U, I, users = t(case.U), t(case.I), t(case.users)
    b = t(case.bias) if bias else None
    ptr, idx = t(case.mask_ptr), t(case.mask_idx)
    exp_mask = case.expected[el.MASK_VALUE]
    top1 = el.order_rows(case.scores64(mask_value=el.MASK_VALUE), k + 1) if N > k else None
    rs = np.random.RandomState(D + k)
    junk = rs.randint(0, N, (n, k)).astype(np.int64)
    junk[:, 0] = -1
    if k > 1:
        junk[1::2, 1] = N + 7
        junk[2::3, -1] = junk[2::3, 0]
    hints = {"none": None, "expected": exp_mask, "junk": junk}
    if top1 is not None:
        swapped = top1[:, :k].copy()
        swapped[:, k - 1] = top1[:, k]
        hints["kth_swapped"] = swapped
    hint_names = list(hints)
    runs = []
    for precision in ("f32", "bf16x3"):
        forms = [None] if precision == "f32" else (["four_waves", "two_roles"] if _two_roles_exist(D, k) else [None])
        for form, prescan, sliced in itertools.product(forms, (False, True), (True, False)):
            if prescan and not sliced:
                continue                                # (sliced=False implies no prescan)
            runs.append(dict(precision=precision, form=form, prescan=prescan, sliced=sliced))
    for j, kw in enumerate(runs):
        if kw["prescan"]:                               # the library runs the prescan only without a hint (a hint
            combos = [("none", mv) for mv in el.MASK_VALUES]   # gives the bound instead): every mask value
        else:
            combos = [(h, el.MASK_VALUES[(j + (h == "none")) % len(el.MASK_VALUES)])
                      for h in (hint_names[(j + k) % len(hint_names)], hint_names[(j + k + 1) % len(hint_names)])]
        for h, mv in combos:
            hint = case.expected[mv] if h == "expected" else hints[h]
            _check(engine, case, (U, I, users, ptr, idx, b), mv, None if hint is None else t(hint), dict(kw, hint=h))
    if not bias:
        for fused in (False, True) if k <= 16 or D <= 64 else (False,):
            got = engine.mf_recommend(U, I, users, ptr, idx, k, fused=fused).cpu().numpy()
            assert np.array_equal(got, exp_mask), f"mf_recommend(fused={fused})"


# ---- the prescan's bound on cancellation rows --------------------------------------------------------------------------

PRESCAN_CASES = [(64, 16411, 2100, 16, False), (64, 16411, 300, 10, True), (128, 16411, 2100, 10, False),
                 (128, 16411, 300, 16, True), (32, 16411, 300, 32, False)]


def _prescan_case(spec):
    key = ("prescan",) + spec
    if key not in _BUILT:
        D, N, n, k, bias = spec
        _BUILT[key] = el.build_case(D, N, n, k, bias=bias, seed=2000 + 7 * D + n + k + bias, prescan_place=True)
    return _BUILT[key]


def _placed_rows(case):
    """Rows of the families placed in the prescan's tiles whose own top k is unmasked."""
    placed = {f for f, kind in enumerate(case.kinds) if kind.startswith("cancel")} | {case.kinds.index("plain")}
    return [r for r in range(len(case.users)) if case.family[r] in placed and not len(case.masks[r])]


@pytest.mark.parametrize("D,k", [(64, 10), (64, 16), (128, 10), (128, 16)])
def test_prescan_placement_puts_the_top_k_in_distinct_sampled_groups(D, k):
    """prescan_place=True: for the cancellation families and the first plain family, the k best items of every row
    lie in tiles the prescan scores in both precisions, at k different offsets of the tile (k different group
    maxima), so the prescan's bound is the k-th score itself — the floor sits |b| 1e-6 below it."""
    case = el.build_case(D, 16411, 300, k, seed=3, mask_values=(el.MASK_VALUE,), prescan_place=True)
    tiles = set(el.prescan_tiles(16411, D))
    rows = _placed_rows(case)
    kinds = {case.kinds[case.family[r]] for r in rows}
    assert {"cancel+", "cancel0", "cancel-", "plain"} <= kinds
    for r in rows:
        top = case.expected[el.MASK_VALUE][r]
        assert all(j // 32 * 32 in tiles for j in top), r
        assert len({j % 32 for j in top}) == k, r


@pytest.mark.gpu
@pytest.mark.parametrize("spec", PRESCAN_CASES,
                         ids=lambda s: "D{}-N{}-n{}-k{}-{}".format(*s[:4], "bias" if s[4] else "nobias"))
def test_prescan_bound_is_exact_on_cancellation_ladders(device, spec):
    """The prescan's group maxima must equal the sweep's scores bit for bit: its floor is only |b| 1e-6 below the
    k-th largest of them, far less than a rounding of the score when |b| << A.  Ladders whose top k fill k different
    groups of the sampled tiles (cancellation rows with the k-th score positive, 0.0 and negative) make that bound
    the k-th score itself; every form of the sweep, prescan forced and no hint, every mask value == float64."""
    import torch
    from yelprecommendation_amd import engine
    D, N, n, k, bias = spec
    case = _prescan_case(spec)
    assert len(_placed_rows(case)) >= n // 10
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    tensors = (t(case.U), t(case.I), t(case.users), t(case.mask_ptr), t(case.mask_idx), t(case.bias) if bias else None)
    forms = [("f32", None)] + [("bf16x3", f) for f in (["four_waves", "two_roles"] if _two_roles_exist(D, k) else [None])]
    for (precision, form), mv in itertools.product(forms, el.MASK_VALUES):
        for prescan in (True, False):
            _check(engine, case, tensors, mv, None, dict(precision=precision, form=form, prescan=prescan))
