"""Float64 restatement of yr_s3rec_catalogue_rank (include/yelprec_engine.h; csrc/s3rec_rank.hip), the cases its tests
run and the wrong readings they must tell apart.  No fixtures, no GPU.

The contract.  s[n, r] = <H[n], T[r]>; rank[n] counts the columns r in [first_col, R), r != target[n], r not on the
row's exclude list, with s[n, r] > s[n, t] or (s[n, r] == s[n, t] and r < t).

The band.  The scores are computed here from the f32 tables in float64, with A(n, r) = sum_d |H_nd T_rd|.  A correct
f32 kernel is within c_E A of them (tests/eval_ladders.py derives c_E = c_bound(E) for a k-ordered fma chain or the
f32 matrix instruction), so a column is DECIDED when |s(r) - s(t)| > c_E (A(r) + A(t)): every correct kernel puts it
on the same side of the target.  It is also decided when it ties in every arithmetic: its row of T is bit-identical
to the target's row, or both rows are all zero (the kernel's one-arithmetic clause), or the three vectors hold small
integers only — every product and every partial sum is then an integer below 2^24 and exact in f32 in any order, so
the comparison is the exact one.  lo counts the decided-above columns and the decided ties with a smaller id; hi adds
the undecided columns.

Two generators: `random` (H unit normal, T uniform at the Xavier bound of an [R, E] table) and `exact` (entries in
{-2 .. 2}: lo == hi, many exact ties, so the id rule carries weight).
"""
import numpy as np

from eval_ladders import c_bound

F32 = np.float32
FLAG_BAD_USER, FLAG_BAD_ITEM = 1, 2
TILE, WAVE_COLS, CHUNK, GRID_MAX = 32, 512, 2048, 2048      # csrc/s3rec_cb.h: kCbTile, 16 tiles, kCbColChunk, kCbGridMax

VARIANTS = ("last_column_dropped", "tile_dropped", "chunk_dropped", "column_0_counted", "target_counted",
            "ties_to_larger_id", "ge_for_gt", "last_exclude_dropped", "excluded_target_honoured", "excl_rows_ignored")


def workspace_bytes(N, R, E):
    return 4 * N * ((R + CHUNK - 1) // CHUNK)


# ---- cases ----
def _case(id, E, N, R, first_col=1, excl="csr", dup=False, bad_target=False, bad_row=False, seed=0, shift=0,
          sample=None):
    return dict(id=id, E=E, N=N, R=R, first_col=first_col, excl=excl, dup=dup, bad_target=bad_target, bad_row=bad_row,
                seed=seed, shift=shift, sample=sample)


def cases():
    """The smallest shapes at which the kernel can go wrong (a wave's 512 columns and one past, the 2,048-column chunk
    and one past, partial tiles on both sides), every width, both first_col, each exclude form; one case a unit past
    the grid cap and one of full size."""
    out = [
        _case("E16-N1-R2", 16, 1, 2, excl="none"),
        _case("E16-N1-R2-fc0", 16, 1, 2, first_col=0, excl="none", shift=1),
        _case("E16-N33-R33", 16, 33, 33),
        _case("E16-N65-R2049-rows", 16, 65, 2049, excl="rows", dup=True),
        _case("E32-N31-R33-fc0", 32, 31, 33, first_col=0, dup=True),
        _case("E32-N32-R513", 32, 32, 513, excl="rows", bad_row=True),
        _case("E32-N65-R4100-bad", 32, 65, 4100, bad_target=True, dup=True),
        _case("E64-N33-R2048", 64, 33, 2048, dup=True),
        _case("E64-N65-R2049-fc0", 64, 65, 2049, first_col=0, excl="rows", dup=True),
        _case("E64-N65-R4100", 64, 65, 4100, dup=True, bad_target=True, bad_row=True, excl="rows"),
        _case("E64-N32-R513-none", 64, 32, 513, excl="none", dup=True),
        _case("E128-N33-R513", 128, 33, 513, dup=True),
        _case("E128-N65-R4100", 128, 65, 4100, excl="rows"),
        _case("E128-N31-R2049-fc0", 128, 31, 2049, first_col=0, dup=True),
        _case("past-the-grid-cap", 16, 32800, 2049, excl="sparse", dup=True),
        _case("full-size", 64, 31668, 38049, excl="sparse", sample=512),
    ]
    return out


def is_large(case):
    return case["N"] * case["R"] > 1_000_000


def _placements(R, first_col):
    p = [first_col, R - 1, 31, 32, 63, 64, 2047, 2048, R // 2, R // 3]
    p = list(dict.fromkeys(t for t in p if first_col <= t < R))
    if first_col == 1:
        p.insert(2, 0)                                   # "no target"
    return p


def gen(case, exact=False):
    """dict(H, T, target, ptr, idx, rows, K, first_col, exact): the inputs of one case; ``exact`` its integer twin."""
    E, N, R, fc = case["E"], case["N"], case["R"], case["first_col"]
    rs = np.random.RandomState(1000 + case["seed"] + 7919 * sum(map(ord, case["id"])) % 100000)
    if exact:
        H = rs.randint(-2, 3, (N, E)).astype(F32)
        T = rs.randint(-2, 3, (R, E)).astype(F32)
    else:
        H = rs.standard_normal((N, E)).astype(F32)
        bound = np.sqrt(6.0 / (R + E))
        T = rs.uniform(-bound, bound, (R, E)).astype(F32)
    place = _placements(R, fc)
    if N <= 128:
        target = np.array([place[(n + case["shift"]) % len(place)] for n in range(N)], dtype=np.int64)
    else:
        target = rs.randint(fc, R, N).astype(np.int64)
        target[:len(place)] = place
        if fc == 1:
            target[rs.randint(0, N, 8)] = 0
    if case["bad_target"]:
        target[N // 2] = -1
        target[N - 1] = R
    if case["dup"] and R >= 8:
        # a bit-identical copy of the target's row below and above the target id of row 0 (and of every row that
        # shares the target): they tie exactly, the id decides
        t0 = R // 2
        target[0] = t0
        T[fc] = T[t0]
        T[fc + 1] = T[t0]                                # two copies below, one above: the three tie rules differ
        T[R - 1] = T[t0]
        if R > 70:
            T[63] = 0.0                                  # and an all-zero pair: target 64 against column 63
            T[64] = 0.0
    ptr = idx = rows = None
    K = 0
    if case["excl"] == "sparse":
        K = N
        raw = np.sort(rs.randint(0, R, (N, 12)), axis=1)
        keep = np.ones_like(raw, dtype=bool)
        keep[:, 1:] = raw[:, 1:] != raw[:, :-1]
        ptr = np.zeros(N + 1, dtype=np.int64)
        np.cumsum(keep.sum(1), out=ptr[1:])
        idx = raw[keep].astype(np.int64)
    elif case["excl"] in ("csr", "rows"):
        K = N if case["excl"] == "csr" else 7
        lists = []
        for k in range(K):
            kind = (k + k // 6 + case["shift"]) % 6        # no common period with the targets' cycle
            if kind == 0:
                lst = []
            elif kind == 1:
                lst = list(range(R))                     # everything: column 0, the target itself
            elif kind == 2:
                lst = [-3] + sorted({c for c in (0, 31, 32, 63, 64, 511, 512, 2047, 2048, R - 1) if 0 <= c < R}) + [R + 7]
            elif kind == 3:
                lst = np.nonzero(rs.rand(R) < 0.3)[0].tolist()
            elif kind == 4:
                t = int(target[k]) if case["excl"] == "csr" else R // 2
                lst = [t] if 0 <= t < R else []
            else:
                lst = np.nonzero(rs.rand(R) < 0.9)[0].tolist()
            lists.append(lst)
        ptr = np.zeros(K + 1, dtype=np.int64)
        np.cumsum([len(l) for l in lists], out=ptr[1:])
        idx = np.array([c for l in lists for c in l], dtype=np.int64)
        if case["excl"] == "rows":
            rows = np.array([(3 * n + 1) % K for n in range(N)], dtype=np.int64)   # permuted, repeated
            if case["bad_row"]:
                rows[0] = -1
                rows[N - 1] = K
    return dict(H=H, T=T, target=target, ptr=ptr, idx=idx, rows=rows, K=K, first_col=fc, exact=exact, R=R, N=N, E=E)


def expected_flag(g):
    f = 0
    if ((g["target"] < 0) | (g["target"] >= g["R"])).any():
        f |= FLAG_BAD_ITEM
    if g["ptr"] is not None:
        rows = np.arange(g["N"]) if g["rows"] is None else g["rows"]
        if ((rows < 0) | (rows >= g["K"])).any():
            f |= FLAG_BAD_USER
    return f


# ---- the restatement ----
def _excluded(g, n_lo, n_hi, variant=None):
    """bool [n_hi - n_lo, R]: column r is on the exclude list of row n."""
    R = g["R"]
    out = np.zeros((n_hi - n_lo, R), dtype=bool)
    if g["ptr"] is None:
        return out
    for n in range(n_lo, n_hi):
        k = n if (g["rows"] is None or variant == "excl_rows_ignored") else int(g["rows"][n])
        if not 0 <= k < g["K"]:
            continue
        lst = g["idx"][g["ptr"][k]:g["ptr"][k + 1]]
        if variant == "last_exclude_dropped":
            lst = lst[:-1]
        lst = lst[(lst >= 0) & (lst < R)]
        out[n - n_lo, lst] = True
    return out


def _all_small_integers(g):
    H, T = g["H"], g["T"]
    if not ((H == np.round(H)).all() and (T == np.round(T)).all()):
        return False
    return g["E"] * float(np.abs(H).max()) * float(np.abs(T).max()) < 2.0 ** 24


def bands(g, variant=None, rows=None, block=2048, h_err=0.0):
    """dict(lo, hi, rank64, s64, A, has) over ``rows`` (default: all), in row blocks.  rank64 is the float64 rank under
    ``variant`` (None: the contract); lo / hi are the contract's band whatever the variant.  ``h_err``: a bound on
    |H - H'| per element where the kernel's rows H' are not the rows given here (an encoder ran before it): a score
    then moves by at most h_err sum_d |T_rd| more, and the margin of a decision grows by that of both columns."""
    H, T, R, fc, E = g["H"], g["T"], g["R"], g["first_col"], g["E"]
    sel = np.arange(g["N"]) if rows is None else np.asarray(rows)
    c = c_bound(E)
    exact = _all_small_integers(g) and h_err == 0.0
    T64, aT = T.astype(np.float64), np.abs(T.astype(np.float64))
    l1 = aT.sum(1)
    zero_row = ~T.any(axis=1)
    row_id = np.unique(np.ascontiguousarray(T).view(np.uint32), axis=0, return_inverse=True)[1].reshape(-1)
    cols = np.arange(R)
    lo, hi, rk, s64, At = (np.zeros(sel.size, dtype=np.int64), np.zeros(sel.size, dtype=np.int64),
                           np.zeros(sel.size, dtype=np.int64), np.zeros(sel.size), np.zeros(sel.size))
    has_all = np.zeros(sel.size, dtype=bool)
    for b0 in range(0, sel.size, block):
        ns = sel[b0:b0 + block]
        Hb = H[ns].astype(np.float64)
        S = Hb @ T64.T
        A = (np.abs(Hb) + h_err) @ aT.T
        t = g["target"][ns]
        has = (t >= fc) & (t < R)
        tt = np.where(has, t, 0)
        st, at = S[np.arange(ns.size), tt], A[np.arange(ns.size), tt]
        # the exclude lists are contiguous ranges of n only for rows=None; build row by row
        ex = np.zeros((ns.size, R), dtype=bool)
        exv = np.zeros((ns.size, R), dtype=bool)
        if g["ptr"] is not None:
            for i, n in enumerate(ns):
                ex[i] = _excluded(g, n, n + 1)[0]
                exv[i] = _excluded(g, n, n + 1, variant)[0] if variant in ("excl_rows_ignored", "last_exclude_dropped") else ex[i]
        is_t = cols[None, :] == tt[:, None]
        cand = (cols[None, :] >= fc) & ~is_t & ~ex & has[:, None]
        same = row_id[None, :] == row_id[tt][:, None]       # bit-identical rows of T
        same |= zero_row[None, :] & zero_row[tt][:, None]
        diff = S - st[:, None]
        if exact:
            tie = diff == 0
            above = diff > 0
            undecided = np.zeros_like(tie)
        else:
            decided = np.abs(diff) > c * (A + at[:, None]) + h_err * (l1[None, :] + l1[tt][:, None])
            tie = same
            above = decided & (diff > 0) & ~same
            undecided = ~decided & ~same
        below_id = cols[None, :] < tt[:, None]
        l = (cand & (above | (tie & below_id))).sum(1)
        lo[b0:b0 + ns.size] = np.where(has, l, -1)
        hi[b0:b0 + ns.size] = np.where(has, l + (cand & undecided).sum(1), -1)
        # the float64 rank, under the variant
        fcv = 0 if variant == "column_0_counted" else fc
        candv = (cols[None, :] >= fcv) & ~is_t & ~exv & has[:, None]
        if variant == "last_column_dropped":
            candv &= cols[None, :] != R - 1
        if variant == "tile_dropped":
            tile = ((R + TILE - 1) // TILE - 1) // 2
            candv &= ~((cols[None, :] >= tile * TILE) & (cols[None, :] < (tile + 1) * TILE))
        if variant == "chunk_dropped":
            candv &= cols[None, :] < (R - 1) // CHUNK * CHUNK if R > CHUNK else True
        tie64 = (diff == 0) | same
        gt = (diff > 0) & ~same
        if variant == "ties_to_larger_id":
            cnt = candv & (gt | (tie64 & ~below_id))
        elif variant == "ge_for_gt":
            cnt = candv & (gt | tie64)
        else:
            cnt = candv & (gt | (tie64 & below_id))
        r = cnt.sum(1)
        if variant == "target_counted":
            r = r + 1
        r = np.where(has, r, -1)
        if variant == "excluded_target_honoured":
            r = np.where(has & ex[np.arange(ns.size), tt], -1, r)
        rk[b0:b0 + ns.size] = r
        s64[b0:b0 + ns.size] = np.where(has, st, 0.0)
        At[b0:b0 + ns.size] = np.where(has, at, 0.0)
        has_all[b0:b0 + ns.size] = has
    return dict(lo=lo, hi=hi, rank64=rk, s64=s64, A=At, has=has_all, c=c, rows=sel)


def rank_f32(g, rows=None):
    """A plain float32 NumPy evaluation of the contract (its own summation order)."""
    H, T, R, fc = g["H"], g["T"], g["R"], g["first_col"]
    sel = np.arange(g["N"]) if rows is None else np.asarray(rows)
    out = np.full(sel.size, -1, dtype=np.int64)
    cols = np.arange(R)
    for i, n in enumerate(sel):
        t = int(g["target"][n])
        if not fc <= t < R:
            continue
        s = (T * H[n][None, :]).sum(axis=1, dtype=F32)       # one order for every column, the target's included
        cand = (cols >= fc) & (cols != t) & ~_excluded(g, n, n + 1)[0]
        out[i] = int((cand & ((s > s[t]) | ((s == s[t]) & (cols < t)))).sum())
    return out


def sample_rows(case):
    """The rows a large case is judged on."""
    if case["sample"] is None:
        return None
    rs = np.random.RandomState(77)
    rows = np.sort(rs.choice(case["N"], case["sample"], replace=False))
    rows[0], rows[-1] = 0, case["N"] - 1
    return rows


def variant_applies(variant, case, g):
    """Whether the inputs of a case can tell the wrong reading from the contract at all.  The two one-row cases of
    two columns hold at most one candidate column: they check the ends of the loops, not the readings."""
    has = (g["target"] >= g["first_col"]) & (g["target"] < g["R"])
    if not has.any() or g["N"] * g["R"] < 1000:
        return False
    if variant == "chunk_dropped":
        return g["R"] > CHUNK
    if variant == "column_0_counted":
        return g["first_col"] == 1
    if variant in ("last_exclude_dropped", "excluded_target_honoured"):
        return g["ptr"] is not None
    if variant == "excl_rows_ignored":
        return g["rows"] is not None
    if variant in ("ties_to_larger_id", "ge_for_gt"):
        return case["dup"] and g["R"] >= 8
    return True


_MADE = {}


def made(case, exact):
    """(inputs, bands) of a case or of its exact twin, computed once per session and shared by the tests."""
    key = (case["id"], exact)
    if key not in _MADE:
        g = gen(case, exact=exact)
        _MADE[key] = (g, bands(g, rows=sample_rows(case)))
    return _MADE[key]
