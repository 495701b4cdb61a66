"""Float64 restatement of the LINEAR pieces around the fused S3Rec kernels (csrc/s3rec.hip, engine.s3rec_param_grads)
for the tests: both score forms, the score gradient, the item-table gradient, the transposed products and column sums
of the weight gradients and the packed gradient they fill.  Importable helper, no fixtures (like gemm_ref64.py); runs
without a GPU.  The fused encoder and backward kernels keep their own judges (s3rec_ref64.py, s3rec_grad_ref64.py).

Every floating output is an ``Out(v, n, s)`` (the class of cdae_ref64.py): the float64 value, the number of rounded
operations on the way to it and the sum of the magnitudes of its terms.  An f32 kernel that adds n terms in ANY order
is off by at most (n + 1) 2^-24 s to first order; with the factor 2 of margin of cdae_ref64.py

    bar = 2 (n + 1) 2^-24 s                                        (no rtol floor, nothing taken from a kernel)

Scores.  <I[id], h[row]>: the E products are the terms (a lane's FMAs, then the 16-lane shuffle sum: one order among
the any-order ones), n = E.  A bad id scores exactly 0: n = 0, s = 0, bar 0.
Score gradient.  dpos I[p] + dneg I[n]: two terms, each a rounded product where the compiler does not contract, so
each counts twice: n = 4.
Item gradient.  d_item[id] = d_item0[id] + sum over the run of id among the 3 R sorted lookups of (d_emb[r] | dpos[r]
h[r] | dneg[r] h[r]).  The coefficient products are rounded before they are added (counted twice: n = 2 per such
lookup, 1 per d_emb lookup); the sum runs on two levels, a partial per kItemChunk-chunk the run touches (one more term
per partial) and the addition onto d_item0 (one more): n = lookups + products + chunks touched + 1, s = sum |terms| +
|d_item0|.  A row without a lookup is not written: it equals d_item0 bit for bit (``touched`` is False there).
Weight gradients.  out = D^T Xm over R rows: R products on the matrix instruction, cut into S3REC_GRAD_CHUNK_ROWS-row
products and one column sum over the partial products when R exceeds a chunk (one more term per partial): n = R +
chunks.  Column sums over the B sequences, then the L positions: n = B L + L (one more term per position's partial).

Exactness (``quantum`` / ``exact`` of ngcf_ref64.py).  When every term of an output is an integer multiple of one
power of two q and s <= 2^24 q, any order of f32 additions and FMAs gives the float64 value: the "exact" inputs (small
integers, coefficients +-2^-k, d_item0 non-zero integers) are compared for EQUALITY.  The certificate is computed from
the generated arrays (``certificate``), never from value ranges.

``plan_*`` restate the host's geometry from the constants read out of the sources by name (``source_constants``).
"""
import functools
import os
import re

import numpy as np

from cdae_ref64 import Out, over
from ngcf_ref64 import exact, ints, quantum, rand_mag

U24 = 2.0 ** -24
F32 = np.float32
SENTINEL = 7.25
GUARD = 256                                  # floats of sentinel before and after every output
FLAG_BAD_ITEM = 2                            # YR_FLAG_BAD_ITEM
WIDTHS = (16, 32, 64, 128)
TABLE_ROWS = 40000                           # num_items + 1 of the score cases (Yelp2018: 38,049)
BIG = 2 ** 40                                # an id far outside any table
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def source_constants():
    """The constants the geometry follows from, read from the sources by name."""
    pkg = os.path.join(ROOT, "yelprecommendation_amd")
    text = {k: open(p).read() for k, p in (("s3", os.path.join(pkg, "csrc", "s3rec.hip")),
                                           ("common", os.path.join(pkg, "csrc", "common.h")),
                                           ("header", os.path.join(ROOT, "include", "yelprec_engine.h")),
                                           ("engine", os.path.join(pkg, "engine.py")))}

    def find(where, pattern):
        return int(re.search(pattern, text[where]).group(1))

    assert re.search(r"constexpr int kMaxGrid = YR_LOSS_PARTIALS;", text["common"])
    assert re.search(r"constexpr int kWavesPerBlock = kBlock / kWave;", text["common"])
    assert len(re.findall(r"std::min<int64_t>\(p(?:\.enc)?\.B, 1 << 20\)", text["s3"])) == 2
    return dict(kItemChunk=find("s3", r"constexpr int kItemChunk = (\d+);"),
                kBlock=find("common", r"constexpr int kBlock = (\d+);"),
                kWave=find("common", r"constexpr int kWave = (\d+);"),
                YR_LOSS_PARTIALS=find("header", r"#define YR_LOSS_PARTIALS (\d+)"),
                LPR=find("s3", r"constexpr int LPR = (\d+);"),
                S3REC_GRAD_CHUNK_ROWS=find("engine", r"\nS3REC_GRAD_CHUNK_ROWS = (\d+)"),
                S3REC_GRAD_STREAM_JOBS=find("engine", r"\nS3REC_GRAD_STREAM_JOBS = (\d+)"))


_C = source_constants()
ITEM_CHUNK, BLOCK, WAVE, MAX_GRID, LPR = (_C[k] for k in ("kItemChunk", "kBlock", "kWave", "YR_LOSS_PARTIALS", "LPR"))
CHUNK_ROWS, STREAM_JOBS = _C["S3REC_GRAD_CHUNK_ROWS"], _C["S3REC_GRAD_STREAM_JOBS"]
WAVES = BLOCK // WAVE
ROUND_ROWS = BLOCK // LPR                    # rows of one round of the score kernel
SCORE_SPAN = MAX_GRID * ROUND_ROWS           # rows of one grid trip of the score kernel at the cap
GRAD_SPAN = MAX_GRID * BLOCK                 # elements of one trip of s3rec_score_grad_kernel at the cap
WAVE_SPAN = MAX_GRID * WAVES                 # chunks / item ids of one trip of the two item kernels at the cap
SEQ_GRID = 1 << 20                           # the fused kernels' grid cap (asserted against the source above)


def bar(o):
    return 2.0 * (o.n + 1.0) * U24 * o.s


def ratio(got, o):
    """max |got - v| / bar (0 for an empty output); NaN / inf in ``got`` give inf."""
    got = np.asarray(got, np.float64).reshape(o.v.shape)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    return float(over(got - o.v, bar(o)).max())


def _grid_for(work, per_block):
    return int(min(max((work + per_block - 1) // per_block, 1), MAX_GRID))


def _ceil(a, b):
    return (a + b - 1) // b


# ---- geometry -------------------------------------------------------------------------------------------------------

def plan_scores(rows_a, rows_b):
    """Rounds and grid trips of s3rec_scores_kernel; ``seam``: the two lists meet inside a round."""
    rows = rows_a + rows_b
    rounds = _ceil(rows, ROUND_ROWS)
    grid = _grid_for(rows, ROUND_ROWS)
    return dict(rows=rows, rounds=rounds, grid=grid, trips=_ceil(rounds, grid), seam=rows_a % ROUND_ROWS != 0,
                last_round=rows - (rounds - 1) * ROUND_ROWS)


def plan_score_grad(rows, E):
    total = rows * E
    grid = _grid_for(total, BLOCK)
    return dict(total=total, grid=grid, trips=_ceil(total, grid * BLOCK), last=total - (total - 1) // BLOCK * BLOCK)


def plan_item(sorted_ids, num_items):
    """Chunks, runs and trips of the two item kernels for a sorted lookup list: ``runs`` [k, 3] = (id, lo, hi)."""
    sid = np.asarray(sorted_ids, np.int64)
    n = sid.size
    lo = np.flatnonzero(np.r_[True, sid[1:] != sid[:-1]])
    hi = np.r_[lo[1:], n]
    ids = sid[lo]
    ok = (ids >= 0) & (ids <= num_items)
    chunks = _ceil(n, ITEM_CHUNK)
    c0, c1 = lo // ITEM_CHUNK, (hi - 1) // ITEM_CHUNK
    per_chunk = np.zeros(chunks + 1, np.int64)                    # runs touching each chunk
    np.add.at(per_chunk, c0, 1)
    np.add.at(per_chunk, c1 + 1, -1)
    per_chunk = np.cumsum(per_chunk)[:chunks]
    return dict(n=n, chunks=chunks, last_chunk=n - (chunks - 1) * ITEM_CHUNK,
                partial_trips=_ceil(chunks, _grid_for(chunks, WAVES) * WAVES),
                combine_trips=_ceil(num_items + 1, _grid_for(num_items + 1, WAVES) * WAVES),
                runs=np.stack([ids, lo, hi], 1), ok=ok, spans=c1 - c0 + 1, runs_per_chunk=per_chunk,
                lengths=hi - lo, absent=num_items + 1 - int(ok.sum()),
                ends_at_chunk_end=bool(np.any(ok & (hi % ITEM_CHUNK == 0))),
                starts_on_chunk_last=bool(np.any(ok & (lo % ITEM_CHUNK == ITEM_CHUNK - 1) & (hi - lo > 1))),
                whole_middle_chunk=bool(np.any(ok & (c1 - c0 >= 2))), one_id=bool(ids.size == 1),
                bad_front=int((hi - lo)[ids < 0].sum()), bad_back=int((hi - lo)[ids > num_items].sum()),
                max_id=int(ids[ok].max()) if ok.any() else -1)


def plan_rows_products(job_rows):
    """Chunk products of engine._s3rec_rows_products for jobs of the given row counts, and the path they take."""
    pieces = [(_ceil(r, CHUNK_ROWS) if r > CHUNK_ROWS else 1) for r in job_rows]
    last = [r - (p - 1) * CHUNK_ROWS if r > CHUNK_ROWS else r for r, p in zip(job_rows, pieces)]
    return dict(pieces=sum(pieces), per_job=pieces, last_chunk=last, streams=sum(pieces) >= STREAM_JOBS,
                chunked=[r > CHUNK_ROWS for r in job_rows])


def plan_param_grads(B, L, heads, blocks):
    return plan_rows_products([B * L] * (4 * blocks))


def plan_fused(B):
    grid = min(B, SEQ_GRID)
    return dict(grid=grid, trips=_ceil(B, grid))


# ---- the operations -------------------------------------------------------------------------------------------------

def _ok(ids, num_items):
    ids = np.asarray(ids, np.int64)
    return (ids >= 0) & (ids <= num_items)


def _dots(table, h, ids, hrow, num_items, variant=None):
    ok = _ok(ids, num_items)
    E = table.shape[1]
    safe = np.clip(ids, 0, num_items)
    e, hh = table[safe], h[hrow]
    p = e * hh
    if variant == "product_dropped":
        p = p[:, :E - 1]
    keep = ok | (variant == "bad_clamped")
    v = np.where(keep, p.sum(1), 0.0)
    s = np.where(keep, np.abs(p).sum(1), 0.0)
    return Out(v, np.where(ok, float(E), 0.0), s), not ok.all()


def scores(table, h, items_a, per_a, items_b, per_b, num_items, variant=None):
    """(out_a, out_b, flag) of s3rec_scores_kernel: out[r] = <table[items[r]], h[r // per]> per list; a bad id scores
    exactly 0 and sets the flag.  ``variant``: the perturbed references of test_s3rec_edges_ref64.py."""
    table, h = np.asarray(table, np.float64), np.asarray(h, np.float64)
    a, b = np.asarray(items_a, np.int64).reshape(-1), np.asarray(items_b, np.int64).reshape(-1)
    ra, rb = np.arange(a.size) // per_a, np.arange(b.size) // per_b
    if variant == "h_row_r":                           # the candidate form reading h row r, not r / C
        rb = np.minimum(np.arange(b.size), h.shape[0] - 1)
    if variant == "seam_h":                            # the first row of list b against list a's (last) h row
        rb = rb.copy()
        rb[0] = ra[-1]
    oa, fa = _dots(table, h, a, ra, num_items, variant)
    ob, fb = _dots(table, h, b, rb, num_items, variant)
    return oa, ob, FLAG_BAD_ITEM if (fa or fb) else 0


def score_grad(table, pos_items, neg_items, dpos, dneg, num_items, variant=None):
    """(dh_out [rows, E], flag): dpos[r] table[pos[r]] + dneg[r] table[neg[r]]; a bad id contributes nothing."""
    table = np.asarray(table, np.float64)
    p, q = np.asarray(pos_items, np.int64).reshape(-1), np.asarray(neg_items, np.int64).reshape(-1)
    okp, okq = _ok(p, num_items), _ok(q, num_items)
    cp = np.where(okp, np.asarray(dpos, np.float64).reshape(-1), 0.0)
    cq = np.where(okq, np.asarray(dneg, np.float64).reshape(-1), 0.0)
    ip, iq = np.clip(p, 0, num_items), np.clip(q, 0, num_items)
    if variant == "last_neg_dropped":
        cq = cq.copy()
        cq[-1] = 0.0
    if variant == "bad_pos_as_last_row":
        cp = np.asarray(dpos, np.float64).reshape(-1)
        ip = np.where(okp, p, num_items)
    tp, tq = cp[:, None] * table[ip], cq[:, None] * table[iq]
    v = tp + tq
    if variant == "second_trip_left":
        v = v.copy()
        v.reshape(-1)[GRAD_SPAN:] = SENTINEL
    return Out(v, 4.0, np.abs(tp) + np.abs(tq)), FLAG_BAD_ITEM if not (okp.all() and okq.all()) else 0


def sort_lookups(X, pos_items, neg_items):
    """(sorted_ids, order) of the stable sort engine.s3rec_item_grad takes."""
    ids = np.concatenate([np.asarray(a, np.int64).reshape(-1) for a in (X, pos_items, neg_items)])
    order = np.argsort(ids, kind="stable")
    return ids[order], order


def item_grad(X, pos_items, neg_items, d_emb, h, dpos, dneg, d_item0, num_items, weight=None, variant=None):
    """(d_item, touched [num_items + 1], flag): d_item0 plus the three lookups' sums, from a sort and segment sums.
    ``weight`` [3 rows] multiplies the lookups in SORTED order (0: dropped, 2: taken twice); ``variant``: the other
    perturbed references."""
    d0 = np.asarray(d_item0, np.float64)
    E = d0.shape[1]
    sid, order = sort_lookups(X, pos_items, neg_items)
    rows = sid.size // 3
    src, row = order // rows, order % rows
    dp, dn = np.asarray(dpos, np.float64).reshape(-1), np.asarray(dneg, np.float64).reshape(-1)
    if variant == "dpos_for_neg":
        dn = dp
    coeff = np.where(src == 0, 1.0, np.where(src == 1, dp[row], dn[row]))
    if weight is not None:
        coeff = coeff * np.asarray(weight, np.float64)
    if variant == "ids_past_first_trip_left":
        coeff = np.where(sid >= WAVE_SPAN, 0.0, coeff)
    terms = np.where((src == 0)[:, None], np.asarray(d_emb).reshape(rows, E)[row], np.asarray(h).reshape(rows, E)[row])
    terms = terms.astype(np.float64) * coeff[:, None]
    lo = np.flatnonzero(np.r_[True, sid[1:] != sid[:-1]])
    hi = np.r_[lo[1:], sid.size]
    ids = sid[lo]
    ok = (ids >= 0) & (ids <= num_items)
    sums = np.add.reduceat(terms, lo, axis=0)
    np.abs(terms, out=terms)
    mags = np.add.reduceat(terms, lo, axis=0)
    del terms
    products = np.add.reduceat((src != 0).astype(np.float64), lo)
    n_run = (hi - lo) + products + ((hi - 1) // ITEM_CHUNK - lo // ITEM_CHUNK + 1) + 1.0
    v, s, n = d0.copy(), np.abs(d0), np.zeros(d0.shape[0])
    touched = np.zeros(d0.shape[0], bool)
    if variant == "overwrite":
        v[ids[ok]] = 0.0
    v[ids[ok]] += sums[ok]
    s[ids[ok]] += mags[ok]
    n[ids[ok]] = n_run[ok]
    touched[ids[ok]] = True
    if variant in ("bad_to_last_row", "bad_to_row_0") and not ok.all():
        at = num_items if variant == "bad_to_last_row" else 0
        v[at] += sums[~ok].sum(0)
    return Out(v, n[:, None], s), touched, FLAG_BAD_ITEM if not ok.all() else 0


def rows_product(D, Xm, weight=None):
    """D^T Xm over the rows ([M, N] for D [R, M], Xm [R, N]); ``weight`` [R] multiplies the rows."""
    D, Xm = np.asarray(D, np.float64), np.asarray(Xm, np.float64)
    if weight is not None:
        D = D * np.asarray(weight, np.float64)[:, None]
    R = D.shape[0]
    return Out(D.T @ Xm, R + (_ceil(R, CHUNK_ROWS) if R > CHUNK_ROWS else 0.0), np.abs(D).T @ np.abs(Xm))


def rows_sum(D, B, L, weight=None):
    """The column sums of D [B L, width], over the sequences first, then the positions."""
    D = np.asarray(D, np.float64)
    if weight is not None:
        D = D * np.asarray(weight, np.float64)[:, None]
    assert D.shape[0] == B * L
    return Out(D.sum(0), float(B * L + L), np.abs(D).sum(0))


WS_ARRAYS = (("h_in", 1, 0), ("qkv", 0, 3), ("A", 0, 1), ("x1", 1, 0), ("xh1", 1, 0), ("relu", 1, 0), ("xh2", 1, 0),
             ("rstd", None, None), ("g2", 1, 0), ("gx2", 1, 0), ("d2m", 1, 0), ("dz1", 1, 0), ("g1", 1, 0), ("gx1", 1, 0),
             ("d1m", 1, 0), ("dqkv", 0, 3), ("dA", 0, 1))                  # the workspace of csrc/s3rec.hip, per block


def workspace_floats(R, E, heads, blocks):
    return blocks * R * ((12 + 8 * heads) * E + 4)


def block_floats(E, heads):
    return (4 * heads + 2) * E * E + 7 * E


def workspace_views(ws, R, E, heads, blocks):
    """[{name: [R, width] view}] per block of a flat workspace (the layout of s3_layout in csrc/s3rec.hip)."""
    at, out = 0, []
    for _ in range(blocks):
        v = {}
        for name, e, he in WS_ARRAYS:
            width = 4 if e is None else (e + he * heads) * E
            v[name] = ws[at:at + R * width].reshape(R, width)
            at += R * width
        out.append(v)
    assert at == ws.size
    return out


def param_grads(views, B, L, E, heads, blocks, weight=None, swap=None):
    """The packed gradient of engine.s3rec_param_grads from per-block workspace views: which delta meets which stash
    at which offset.  ``weight`` [B L] multiplies the rows of every delta; ``swap`` = k: chunk k's partial product of
    dW_1 lands in dW_2's slot and the other way round (block 0)."""
    assert len(views) == blocks
    v, n, s = [], [], []

    def put(o):
        v.append(o.v.reshape(-1))
        n.append(o.n.reshape(-1))
        s.append(o.s.reshape(-1))

    for blk, w in enumerate(views):
        put(rows_product(w["dqkv"], w["h_in"], weight))          # d(W_q | W_k | W_v) [3 H E][E]
        put(rows_product(w["d1m"], w["A"], weight))              # dW_o [E][H E]
        put(rows_sum(w["d1m"], B, L, weight))                    # b_o
        put(rows_sum(w["gx1"], B, L, weight))                    # ln1 gamma
        put(rows_sum(w["g1"], B, L, weight))                     # ln1 beta
        w1, w2 = rows_product(w["dz1"], w["x1"], weight), rows_product(w["d2m"], w["relu"], weight)
        if swap is not None and blk == 0:
            k = slice(swap * CHUNK_ROWS, (swap + 1) * CHUNK_ROWS)
            delta = rows_product(w["d2m"][k], w["relu"][k]).v - rows_product(w["dz1"][k], w["x1"][k]).v
            w1, w2 = Out(w1.v + delta, w1.n, w1.s), Out(w2.v - delta, w2.n, w2.s)
        put(w1)                                                  # dW_1
        put(rows_sum(w["dz1"], B, L, weight))                    # b_1
        put(w2)                                                  # dW_2
        put(rows_sum(w["d2m"], B, L, weight))                    # b_2
        put(rows_sum(w["gx2"], B, L, weight))                    # ln2 gamma
        put(rows_sum(w["g2"], B, L, weight))                     # ln2 beta
    out = Out(np.concatenate(v), np.concatenate(n), np.concatenate(s))
    assert out.v.size == blocks * block_floats(E, heads)
    return out


# ---- certificates ---------------------------------------------------------------------------------------------------

def certificate(kind, g):
    """The quantum of an exact case's terms, from the generated arrays ``g`` (the dict a generator returns)."""
    if kind == "scores":
        return quantum(g["table"]) * quantum(g["h"])
    if kind == "score_grad":
        return quantum(g["table"]) * quantum(g["dpos"], g["dneg"])
    if kind == "item_grad":
        return min(quantum(g["d_emb"]), quantum(g["h"]) * quantum(g["dpos"], g["dneg"]), quantum(g["d_item0"]))
    if kind == "param_grads":
        q = quantum(g["ws"])
        return min(q, q * q)
    raise KeyError(kind)


# ---- generators -----------------------------------------------------------------------------------------------------

def _values(rs, shape, exact_inputs, hi=2):
    return ints(rs, shape, hi) if exact_inputs else rand_mag(rs, shape)


def _coeffs(rs, rows, exact_inputs, sign, kmax=3):
    """Score gradients: +-2^-k (exact), or at the size of BPR's: -sigmoid(-x) / rows on the positives, + on the
    negatives."""
    if exact_inputs:
        return (rs.choice([-1.0, 1.0], size=rows) * 2.0 ** -rs.randint(0, kmax + 1, size=rows)).astype(F32)
    return (sign * (0.1 + 0.8 * rs.rand(rows)) / rows).astype(F32)


@functools.lru_cache(maxsize=8)
def table_of(E, exact_inputs, rows=TABLE_ROWS):
    t = _values(np.random.RandomState(1000 + E), (rows, E), exact_inputs)
    t.setflags(write=False)
    return t


def _item_ids(rs, shape, num_items):
    return rs.randint(0, num_items + 1, size=shape).astype(np.int64)


def gen_seq(case, exact_inputs):
    """Inputs of yr_s3rec_seq_scores: ids 0 and num_items in both lists, the bad ids in the last round."""
    rows, E = case["rows"], case["E"]
    N = TABLE_ROWS - 1
    rs = np.random.RandomState(case["seed"])
    pos, neg = _item_ids(rs, rows, N), _item_ids(rs, rows, N)
    pos[0], neg[0], pos[-1] = 0, 0, N
    if rows > 1:
        neg[0], neg[1] = N, 0
    if case["bad"]:
        bad = [-1, N + 1, BIG][:max(1, min(3, rows - 2))]
        neg[rows - len(bad):] = bad
    return dict(table=table_of(E, exact_inputs), h=_values(rs, (rows, E), exact_inputs), pos=pos, neg=neg, num_items=N)


def gen_cand(case, exact_inputs):
    B, C, E = case["B"], case["C"], case["E"]
    N = TABLE_ROWS - 1
    rs = np.random.RandomState(case["seed"])
    pos, cand = _item_ids(rs, B, N), _item_ids(rs, (B, C), N)
    pos[0], cand[0, 0] = N, 0
    if case["bad"]:
        cand[-1, -1] = N + 1
    return dict(table=table_of(E, exact_inputs), h=_values(rs, (B, E), exact_inputs), pos=pos, cand=cand, num_items=N)


def gen_score_grad(case, exact_inputs):
    rows, E = case["rows"], case["E"]
    N = TABLE_ROWS - 1
    rs = np.random.RandomState(case["seed"])
    pos, neg = _item_ids(rs, rows, N), _item_ids(rs, rows, N)
    pos[0], neg[0] = 0, N
    at = rows // 2
    if case["bad"] in ("pos", "both"):
        pos[at] = N + 1
    if case["bad"] in ("neg", "both"):
        neg[at] = -1
        neg[0] = BIG if case["bad"] == "both" else neg[0]
    return dict(table=table_of(E, exact_inputs), pos=pos, neg=neg, dpos=_coeffs(rs, rows, exact_inputs, -1.0),
                dneg=_coeffs(rs, rows, exact_inputs, 1.0), num_items=N)


def ids_from_runs(runs, rows, rs):
    """X | pos_items | neg_items from (id, run length) in sorted order: the multiset shuffled over the three sources
    and the rows, so that the stable sort meets every source at every place of a run."""
    ids = np.repeat(np.array([r[0] for r in runs], np.int64), [r[1] for r in runs])
    assert ids.size == 3 * rows and all(a[0] < b[0] for a, b in zip(runs, runs[1:])) and all(r[1] > 0 for r in runs)
    rs.shuffle(ids)
    return ids[:rows].copy(), ids[rows:2 * rows].copy(), ids[2 * rows:].copy()


def gen_item(case, exact_inputs):
    rows, E, T = case["rows"], case["E"], case["T"]
    rs = np.random.RandomState(case["seed"])
    X, pos, neg = ids_from_runs(case["runs"], rows, rs)
    big = 3 * rows > 2 ** 20                   # values in {-1, 0, 1}, coefficients +-1, +-1/2: a run of a million
    hi, kmax = (1, 1) if big else (2, 3)       # lookups stays below 2^24 quanta
    d0 = ints(rs, (T, E), 3, nonzero=True)
    return dict(X=X, pos=pos, neg=neg, d_emb=_values(rs, (rows, E), exact_inputs, hi), h=_values(rs, (rows, E), exact_inputs, hi),
                dpos=_coeffs(rs, rows, exact_inputs, -1.0, kmax), dneg=_coeffs(rs, rows, exact_inputs, 1.0, kmax),
                d_item0=d0 if exact_inputs else (d0 * F32(0.37)).astype(F32), num_items=T - 1)


def gen_workspace(case, exact_inputs):
    B, L, E, heads, blocks = (case[k] for k in ("B", "L", "E", "heads", "blocks"))
    rs = np.random.RandomState(case["seed"])
    return dict(ws=_values(rs, (workspace_floats(B * L, E, heads, blocks),), exact_inputs))


# ---- the case lists of tests/test_gpu_s3rec_edges.py ----------------------------------------------------------------

def _seq_cases():
    out = []
    for E in WIDTHS:
        for rows in (1, 15, 16, 17, SCORE_SPAN // 2 - 1, SCORE_SPAN // 2, SCORE_SPAN // 2 + 1):
            out.append(dict(id=f"E{E}-rows{rows}", E=E, rows=rows, bad=rows not in (1, 16, SCORE_SPAN // 2),
                            seed=len(out) + 11))
    return out


def _cand_cases():
    out = []
    for B in (1, 3, 17):
        for C in (1, 2, 15, 16, 17, 99, 100):
            out.append(dict(id=f"B{B}-C{C}", B=B, C=C, E=WIDTHS[len(out) % 4], bad=len(out) % 2 == 0, seed=len(out) + 101))
    out.append(dict(id="B331-C99", B=331, C=99, E=64, bad=True, seed=131))
    return out


def _score_grad_cases():
    out, kinds = [], ("none", "pos", "neg", "both")
    for E in (16, 128):
        per = GRAD_SPAN // E
        for rows in (1, per - 1, per, per + 1, 2 * per + 1):
            out.append(dict(id=f"E{E}-rows{rows}", E=E, rows=rows, bad=kinds[len(out) % 4], seed=len(out) + 201))
    out.append(dict(id="E32-rows1000", E=32, rows=1000, bad="both", seed=231))
    out.append(dict(id="E64-rows777", E=64, rows=777, bad="pos", seed=232))
    return out


def _pick_ids(k, T, rs):
    """k distinct ascending ids of a T-row table: 0, the two sides of the combine kernel's first trip, the last row,
    the rest at random — most rows stay without a lookup."""
    want = [i for i in (0, T - 1, WAVE_SPAN - 1, WAVE_SPAN) if 0 <= i < T]
    ids = list(dict.fromkeys(want))[:k]
    pool = np.setdiff1d(np.arange(T), ids)
    ids += list(rs.choice(pool, size=k - len(ids), replace=False)) if k > len(ids) else []
    return sorted(int(i) for i in ids)


def _item_cases():
    C = ITEM_CHUNK
    n_of = {1: 3, 85: 255, 86: 258, 171: 513, 256: 768, 257: 771}
    assert (C, 3 * C + 3) == (256, 771)              # the layouts below are written out for a 256-lookup chunk
    # (rows, run lengths in sorted order, rows of the table)
    layouts = [
        ("n3", 1, (1, 2), 4), ("n3-one-id", 1, (3,), 1), ("n255", 85, (1, 2, 252), 5), ("n255-one-id", 85, (255,), 8191),
        ("n258-257+1", 86, (257, 1), 8192), ("n258-255+2+1", 86, (255, 2, 1), 8193), ("n258-one-id", 86, (258,), 40000),
        ("n513-512+1", 171, (512, 1), 8194), ("n513-1+512", 171, (1, 512), 40000), ("n513-one-id", 171, (513,), 8193),
        ("n513-256+257", 171, (256, 257), 5),
        ("n768-256+512", 256, (256, 512), 8192), ("n768-512+256", 256, (512, 256), 8191), ("n768-one-id", 256, (768,), 4),
        ("n768-255+1+511+1", 256, (255, 1, 511, 1), 40000),
        ("n771-255+1+256+257+2", 257, (255, 1, 256, 257, 2), 40000), ("n771-1+511+257+2", 257, (1, 511, 257, 2), 8194),
        ("n771-255+513+3", 257, (255, 513, 3), 8193), ("n771-2+769", 257, (2, 769), 8192),
        ("n771-769+2", 257, (769, 2), 40000), ("n771-one-id", 257, (771,), 1),
    ]
    out = []
    for name, rows, lengths, T in layouts:
        assert sum(lengths) == n_of[rows]
        for E in WIDTHS:
            rs = np.random.RandomState(len(out) + 301)
            ids = [0] if len(lengths) == 1 else _pick_ids(len(lengths), T, rs)
            out.append(dict(id=f"{name}-T{T}-E{E}", E=E, rows=rows, T=T, runs=list(zip(ids, lengths)), seed=len(out) + 301,
                            family=name))
    # bad ids: a run of -1 in front of id 0's run, num_items + 1 and 2^40 at the end
    for E in WIDTHS:
        for T, rows, front, mid in ((8194, 257, 3, (254, 2, 256, 254)), (5, 86, 255, (1,)), (40000, 171, 1, (255, 255))):
            rs = np.random.RandomState(len(out) + 301)
            ids = _pick_ids(len(mid), T, rs)
            runs = [(-1, front)] + list(zip(ids, mid)) + [(T, 1), (BIG, 1)]
            assert sum(r[1] for r in runs) == 3 * rows and ids[0] == 0
            out.append(dict(id=f"bad-T{T}-rows{rows}-E{E}", E=E, rows=rows, T=T, runs=runs, seed=len(out) + 301, family="bad"))
    # the partials' second trip: WAVE_SPAN chunks and one lookup, a run of a million, the last run across the last seam
    n = WAVE_SPAN * C + 1
    assert n % 3 == 0
    rs = np.random.RandomState(7)
    T = 40000
    ids = np.sort(np.r_[[0, WAVE_SPAN - 1, WAVE_SPAN, T - 1], rs.choice(np.setdiff1d(np.arange(1, T - 1), [WAVE_SPAN - 1, WAVE_SPAN]),
                                                                      size=2996, replace=False)])
    rest = n - 1000001 - 2
    cuts = np.sort(rs.choice(np.arange(1, rest), size=ids.size - 3, replace=False))
    lengths = np.r_[1000001, np.diff(np.r_[0, cuts, rest]), 2]
    out.append(dict(id=f"n{n}-T{T}-E16", E=16, rows=n // 3, T=T, runs=list(zip(ids.tolist(), lengths.tolist())), seed=77,
                    family="second-trip"))
    return out


def _param_cases():
    shapes = [(1, 1), (89, 23), (64, 32), (683, 3), (2049, 1), (64, 64), (241, 17), (1229, 5)]
    out = [dict(B=B, L=L, E=16, heads=1, blocks=1) for B, L in shapes]
    out += [dict(B=4, L=25, E=32, heads=2, blocks=3), dict(B=4, L=25, E=32, heads=2, blocks=4),
            dict(B=683, L=3, E=128, heads=4, blocks=1)]
    for i, c in enumerate(out):
        c.update(id=f"R{c['B'] * c['L']}-B{c['B']}-E{c['E']}-h{c['heads']}-b{c['blocks']}", seed=401 + i)
    return out


SEQ_CASES, CAND_CASES, SCORE_GRAD_CASES = _seq_cases(), _cand_cases(), _score_grad_cases()
ITEM_CASES, PARAM_CASES = _item_cases(), _param_cases()
FUSED_B = SEQ_GRID + 3                        # sequences of the fused kernels' second trip
FUSED_ROWS = (0, SEQ_GRID - 1, SEQ_GRID, SEQ_GRID + 2)
