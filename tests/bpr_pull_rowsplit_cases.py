"""Batches for the row split of heavy item buckets in the pull-form BPR step (csrc/bpr_pull.hip, YR_ROWSPLIT), built
on tests/bpr_pull_ref64.py (imported, not edited).  Importable helper, no fixtures; needs the built library (for the
thresholds) but no GPU.

An item bucket that is not shared by tile range and holds at least ``row_min`` records has its ROWS shared by S = 2
or 4 workgroups (4 from ``row_quad`` records on, where the width allows it): part q finishes the local rows r with
(r & (S - 1)) == q.  The thresholds are not copied here: ``rule()`` asks the library (yr_bpr_mf_pull_split_summary
answers that part on the host), and ``expected_parts`` restates the sizing rule on them: -S / 1 / P as the kernel's
``parts`` word reads.

Every case has 65 item buckets (64 and a ragged last one) and tiles of 1,024 triplets, or 1,024 buckets and tiles of
2,048, and (but for rows-crowded) few enough triplets per bucket on average that the compile-time floors set the
thresholds.  Hot buckets receive exact record counts on
chosen local rows, tile by tile; as in bpr_pull_ref64 even rows are positives only and odd rows negatives only, so
at S = 2 the owner part holds the positives of a bucket and the helper its negatives.
"""
import functools

import numpy as np

import bpr_pull_ref64 as P

TILE = 1024
NU = 2000


def rule(B, ni, D, nu=NU):
    from yelprecommendation_amd import engine
    return engine.bpr_mf_pull_split_summary(B, nu, ni, D)


def expected_parts(total, r, T):
    """The ``parts`` word of a bucket of `total` records under the thresholds r (while the pools hold)."""
    if total >= r["split_min"]:
        return max(1, min(-(-total // r["split_target"]), P.MAX_PARTS, T))
    if r["row_split_compiled"] and total >= r["row_min"]:
        return -4 if total >= r["row_quad"] else -2
    return 1


def over_tiles(c, T):
    """counts per local row [R] -> [T, R]: row j's records as evenly over the tiles as it goes, the remainder starting
    at a tile that moves with the row (so that no tile collects every row's remainder)."""
    c = np.asarray(c, np.int64)
    t = np.arange(T)[:, None]
    start = (np.arange(c.shape[0]) * 7) % T
    return c[None, :] // T + (((t - start[None, :]) % T) < (c % T)[None, :])


class RowCase(P.Case):
    pass


def build(name, D, nb, T, hot, order=False, ranges=None, tile=TILE):
    """hot: {bucket: (label, [T, R] counts)}; everything else falls evenly on the rows of the other full buckets."""
    rs = np.random.RandomState(P._seed("rowsplit", name))
    r = P.R(D)
    ni = nb * r - 3
    rows = np.arange(ni)
    fill = rows[~np.isin(rows // r, list(hot) + [nb - 1])]
    parts = []
    for t in range(T):
        ci = np.zeros(ni, np.int64)
        for b, (_, per_tile) in hot.items():
            k = min(r, ni - b * r)
            assert not per_tile[:, k:].any(), (name, b, "records past the table")
            ci[b * r:b * r + k] = per_tile[t, :k]
        # (the filler rows in another order for every tile: what does not divide evenly goes to the first of them)
        parts.append(P.stretch(rs, tile, np.zeros(NU, np.int64), ci, np.arange(NU), fill[rs.permutation(len(fill))]))
    c = RowCase(name, D, NU, ni, parts, order=rs.permutation(nb).astype(np.int32) if order else None, ranges=ranges)
    c.hot = {b: (label, per_tile.sum(0)) for b, (label, per_tile) in hot.items()}
    c.T = T
    c.rule = rule(c.B, ni, D)
    assert c.B == T * tile and c.plan.tile == tile and c.plan.T == T and c.plan.nbI == nb
    return c


def _all_rows(total, D, rows=None):
    r = P.R(D)
    return P.spread(total, np.arange(r) if rows is None else np.asarray(rows), r)


def _main_case(name="rows-64", order=False, ranges=False):
    """D = 64, B = 12,288.  One batch with a bucket at every end of the sizing rule and of the part's loops."""
    D, nb, T = 64, 65, 12
    r = P.R(D)
    q = rule(T * TILE, nb * r - 3, D)
    mn, quad, tmin = q["row_min"], q["row_quad"], q["split_min"]
    # light in the first chunk, heavy in the second: tiles 0..5 bring 170 records each, 4 of them on row 3; tiles
    # 6..11 bring 64 each, 50 of them on row 3.  The first chunk (1,024 records, or the tiles 0..5 in the
    # deterministic mode) holds at most 28 records of row 3, the second at least 296 (> kHeavyRow)
    lh = np.zeros((T, r), np.int64)
    others = np.array([j for j in range(r) if j != 3])
    for t in range(T):
        lh[t] = P.spread(166 if t < 6 else 14, others, r)
        lh[t, 3] = 4 if t < 6 else 50
    hot = {
        2: ("min-1", over_tiles(_all_rows(mn - 1, D), T)),
        5: ("min", over_tiles(_all_rows(mn, D), T)),
        9: ("min+1", over_tiles(_all_rows(mn + 1, D), T)),
        13: ("quad-1", over_tiles(_all_rows(quad - 1, D), T)),
        18: ("quad", over_tiles(_all_rows(quad, D), T)),
        22: ("tile-1", over_tiles(_all_rows(tmin - 1, D), T)),
        27: ("tile", over_tiles(_all_rows(tmin, D), T)),
        31: ("one-row", over_tiles(_all_rows(mn + 10, D, [5]), T)),
        36: ("owner-empty", over_tiles(_all_rows(quad + 8, D, [j for j in range(r) if j & 3]), T)),
        41: ("two-chunks", over_tiles(_all_rows(quad + 100, D), T)),
        47: ("light-heavy", lh),
        nb - 1: ("ragged", over_tiles(_all_rows(quad + 48, D, np.arange(r - 3)), T)),
    }
    rg = [(0, 16 * r), (16 * r, 40 * r), (40 * r, nb * r - 3)] if ranges else None
    return build(name, D, nb, T, hot, order=order, ranges=rg)


def _width_case(D):
    """The other widths: the cap on S (2 at D = 128) and the forms without the deal (D = 16)."""
    nb, T = 65, 12
    r = P.R(D)
    q = rule(T * TILE, nb * r - 3, D)
    mn, tmin = q["row_min"], q["split_min"]
    quad = q["row_quad"] if q["row_max_parts"] >= 4 else 3 * q["row_target"]
    hot = {
        3: ("min", over_tiles(_all_rows(mn, D), T)),
        7: ("quad-1", over_tiles(_all_rows(quad - 1, D), T)),
        11: ("quad", over_tiles(_all_rows(quad, D), T)),
        20: ("tile-1", over_tiles(_all_rows(tmin - 1, D), T)),
        30: ("one-row", over_tiles(_all_rows(mn + 10, D, [r - 1]), T)),
        nb - 1: ("ragged", over_tiles(_all_rows(quad + 48, D, np.arange(r - 3)), T)),
    }
    return build(f"rows-{D}", D, nb, T, hot)


def _overflow_case():
    """172 buckets of row_quad records each want 3 row tasks: 516 against a pool of 512 — nothing is split by row."""
    D, nb, T, tile = 64, 1024, 80, 2048
    r = P.R(D)
    q = rule(T * tile, nb * r - 3, D)
    rs = np.random.RandomState(P._seed("rowsplit-overflow"))
    n_hot = q["row_task_pool"] // 3 + 2
    # (the remainders of the buckets start at different tiles)
    hot = {int(b): ("quad", np.roll(over_tiles(_all_rows(q["row_quad"], D), T), int(b) % T, axis=0))
           for b in np.sort(rs.choice(nb - 1, n_hot, replace=False))}
    return build("rows-overflow", D, nb, T, hot, tile=tile)


def _crowded_case():
    """Row tasks are served by the helper workgroups that the tile-range tasks leave free: 4 buckets of 40,960 records
    take 156 of the 512 (40 parts each), 120 buckets of row_quad records want 360 — each kind inside its own pool,
    516 together: the tile-range parts run, no bucket is split by row.  B = 258,048, tiles of 2,048 triplets."""
    D, nb, T, tile = 64, 1024, 126, 2048
    r = P.R(D)
    q = rule(T * tile, nb * r - 3, D)
    rs = np.random.RandomState(P._seed("rowsplit-crowded"))
    ids = np.sort(rs.choice(nb - 1, 124, replace=False))
    hot = {int(b): ("quad", np.roll(over_tiles(_all_rows(q["row_quad"], D), T), int(b) % T, axis=0)) for b in ids[4:]}
    hot.update({int(b): ("tile", over_tiles(_all_rows(40960, D), T)) for b in ids[:4]})
    return build("rows-crowded", D, nb, T, hot, tile=tile)


@functools.lru_cache(maxsize=None)
def _cases():
    out = {}
    for c in (_main_case(), _main_case("rows-64-ranges", ranges=True), _main_case("rows-64-order", order=True),
              _width_case(16), _width_case(32), _width_case(128), _overflow_case(), _crowded_case()):
        out[c.name] = c
    return out


def case(name):
    return _cases()[name]


def case_names():
    return list(_cases())


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    c = case(name)
    U, I = c.tables(kind)
    return P.step(U, I, c.u, c.p, c.n, c.inv(kind))


def wanted(c):
    """(parts word per item bucket as the sizing wants it, row tasks wanted, rows hold: inside their pool, and
    inside the helper workgroups together with the tile-range tasks that run)"""
    _, ti = c.bucket_totals()
    want = np.array([expected_parts(int(t), c.rule, c.T) for t in ti], np.int64)
    row_tasks = int((-want[want < 0] - 1).sum())
    tasks, slots = int((want[want > 1] - 1).sum()), int(want[want > 1].sum())
    tile_tasks = tasks if (tasks <= P.MAX_TASKS and slots <= P.MAX_SLOTS) else 0
    return want, row_tasks, row_tasks <= c.rule["row_task_pool"] and tile_tasks + row_tasks <= P.MAX_TASKS


def part_rows(c, bucket, S, q):
    """global rows (inside the table) that part q of S finishes in `bucket`"""
    r = P.R(c.D)
    rows = bucket * r + np.arange(r)
    return rows[((np.arange(r) & (S - 1)) == q) & (rows < c.ni)]
