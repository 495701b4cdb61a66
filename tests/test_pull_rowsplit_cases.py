"""CPU: the batches of bpr_pull_rowsplit_cases.py reach the record counts they aim at, and the bars of
bpr_pull_ref64.py notice what a wrong row split would compute: a part dropped, a part applied twice (its records
summed twice, or Adam run twice on its rows), rows filtered by contiguous quarters instead of interleaved."""
import numpy as np
import pytest

import bpr_pull_ref64 as P
import bpr_pull_rowsplit_cases as C


@pytest.mark.parametrize("name", C.case_names())
def test_batches_reach_their_counts(name):
    c = C.case(name)
    q = c.rule
    _, ti = c.bucket_totals()
    want, row_tasks, holds = C.wanted(c)
    r = P.R(c.D)
    if name != "rows-crowded":       # the floors, not the average multiples, set every threshold of these batches
        assert (q["row_min"], q["row_target"], q["split_min"]) == \
            tuple(C.rule(1, c.ni, c.D)[k] for k in ("row_min", "row_target", "split_min"))
    assert q["row_split_compiled"] == 1 and q["row_max_parts"] == (2 if c.D == 128 else 4)
    for b, (label, per_row) in c.hot.items():
        assert ti[b] == per_row.sum(), (name, b, label)
        rows = np.bincount(np.concatenate([c.p, c.n]), minlength=c.ni + r)[b * r:(b + 1) * r]
        assert np.array_equal(rows, per_row), (name, b, label)
    # every other bucket stays whole
    cold = np.setdiff1d(np.arange(c.plan.nbI), list(c.hot))
    assert ti[cold].max() < q["row_min"] and (want[cold] == 1).all()
    by_label = {label: (b, int(want[b]), int(ti[b])) for b, (label, _) in c.hot.items()}
    cap = -q["row_max_parts"]
    if name == "rows-overflow":
        assert set(by_label) == {"quad"} and row_tasks > q["row_task_pool"] and not holds
        assert ti.max() < q["split_min"]
        return
    if name == "rows-crowded":
        tasks = int((want[want > 1] - 1).sum())
        assert row_tasks <= q["row_task_pool"] and tasks <= P.MAX_TASKS and int(want[want > 1].sum()) <= P.MAX_SLOTS
        assert tasks + row_tasks > P.MAX_TASKS and not holds
        return
    assert holds and by_label["min"][1] == -2 and by_label["quad-1"][1] == -2 and by_label["quad"][1] == cap
    assert by_label["min"][2] == q["row_min"] and by_label["tile-1"][2] == q["split_min"] - 1
    assert by_label["tile-1"][1] == cap and by_label["ragged"][1] == cap
    assert by_label["one-row"][1] == -2
    if c.D == 64:
        assert by_label["min-1"][1:] == (1, q["row_min"] - 1) and by_label["min+1"][1:] == (-2, q["row_min"] + 1)
        assert by_label["quad-1"][2] == q["row_quad"] - 1 and by_label["quad"][2] == q["row_quad"]
        assert by_label["tile"][1] == 2 and by_label["tile"][2] == q["split_min"]
        assert by_label["two-chunks"][1] == -4 and by_label["two-chunks"][2] > P.CAP_ITEM
        b, s, _ = by_label["owner-empty"]
        assert s == -4 and not c.hot[b][1][0::4].any() and c.hot[b][1][1::4].all()
        b, s, _ = by_label["one-row"]
        assert np.flatnonzero(c.hot[b][1]).tolist() == [5] and c.hot[b][1][5] > P.HEAVY
        # light, then heavy: row 3 of the bucket, by tiles (a chunk is the first 1,024 records in tile order)
        b, s, _ = by_label["light-heavy"]
        assert s < 0
        per_tile = np.stack([np.bincount(np.concatenate([c.p[t * 1024:(t + 1) * 1024], c.n[t * 1024:(t + 1) * 1024]]),
                                         minlength=c.ni + r)[b * r:(b + 1) * r] for t in range(c.T)])
        first = per_tile[:6].sum()
        assert first <= P.CAP_ITEM < first + per_tile[6].sum() and per_tile[:7, 3].sum() <= P.HEAVY
        assert per_tile[7:, 3].sum() > P.HEAVY
    if c.ranges:
        assert len({sum(lo <= b * r < hi for b in c.hot) for lo, hi in c.ranges} - {0}) >= 1
        assert all(any(lo <= b * r < hi for b in c.hot if want[b] < 0) for lo, hi in c.ranges)
    # the ragged bucket: some parts own rows past the table
    b, s, _ = by_label["ragged"]
    assert b == c.plan.nbI - 1 and any(len(C.part_rows(c, b, -s, k)) < r // -s for k in range(-s))


def _caught(c, kind, gI):
    """Whether an item gradient `gI` in place of the reference's crosses the bar (random) / differs (exact)."""
    ref = C.reference(c.name, kind)
    if kind == "exact":
        return bool(np.any(gI != ref.gI.v))
    return P.ratio(gI, ref.gI.v, P.bar_g(ref.gI, ref.eI)) > 1.0


@pytest.mark.parametrize("name", ["rows-64", "rows-16", "rows-128"])
def test_bars_notice_a_wrong_row_split(name):
    c = C.case(name)
    want, _, _ = C.wanted(c)
    r = P.R(c.D)
    n = 0
    for kind in ("random", "exact"):
        ref = C.reference(name, kind)
        g = ref.gI.v
        for b in np.flatnonzero(want < 0):
            S = int(-want[b])
            for k in range(S):
                rows = C.part_rows(c, b, S, k)
                if not ref.gI.n[rows, 0].any():
                    continue                                  # a part without records (owner-empty, one-row)
                dropped, twice = g.copy(), g.copy()
                dropped[rows] = 0.0
                twice[rows] *= 2.0
                assert _caught(c, kind, dropped) and _caught(c, kind, twice), (name, kind, b, k)
                # Adam run twice on the part's rows: m stays g (beta1 = 0), v and the update do not
                live = rows[ref.gI.n[rows, 0] > 0]
                v2 = P.v_of(g[live]) * (1.0 + P.BETA2)
                o = P.Out(ref.gI.v[live], ref.gI.n[live], ref.gI.s[live])
                assert P.ratio(v2, P.v_of(g[live]), P.bar_v(o, ref.eI[live])) > 1.0, (name, kind, b, k)
                n += 1
            # rows filtered by contiguous quarters, finished interleaved: a row keeps its sum only where both agree
            local = np.arange(r)
            lost = b * r + local[(local & (S - 1)) != local // (r // S)]
            lost = lost[lost < c.ni]
            wrong = g.copy()
            wrong[lost] = 0.0
            if ref.gI.n[lost, 0].any():
                assert _caught(c, kind, wrong), (name, kind, b, "filter")
    assert n >= 8
