"""Heavy item buckets whose ROWS are shared by 2 or 4 workgroups (csrc/bpr_pull.hip, YR_ROWSPLIT), through the C ABI,
against tests/bpr_pull_ref64.py (float64) in the one-step raw-gradient reading of test_gpu_bpr_pull_edges.py: zero
Adam state, beta1 = 0, eps = 1, so m is the gradient itself, and the dense-gradient form gradI_out.  Every element is
compared at that helper's own bars on the random tables and for EQUALITY on the exact twins; rows without a record
come back bit-equal to their input; deterministic runs are made twice and must be bit-equal.

The batches (bpr_pull_rowsplit_cases.py, checked without a GPU by test_pull_rowsplit_cases.py) put exact record
counts on chosen buckets; the thresholds come from yr_bpr_mf_pull_split_summary, and after every run the same query
reads the partition's own words: each test asserts that the split it aims at really ran.

Measured on the MI355X: every exact case equal to float64; max |err| / bar on random inputs: item m / gradI_out 0.011,
user m 0.006, loss 1e-5; U_new and I 0.50 (the rounding of the parameter itself, as in test_gpu_bpr_pull_edges.py).
9 tests, 5 s."""
import functools

import numpy as np
import pytest
import torch

import bpr_pull_ref64 as P
import bpr_pull_rowsplit_cases as C

pytestmark = pytest.mark.gpu

BC2_SQRT = float(np.sqrt(1.0 - P.BETA2))
LOSS_START = 3.5


@functools.lru_cache(maxsize=None)
def _lib():
    from yelprecommendation_amd import _lib as L
    return L.load()


def _upload(device, c, kind):
    U, I = c.tables(kind)
    return dict(U=torch.from_numpy(U.copy()).to(device), I=torch.from_numpy(I.copy()).to(device),
                ids=tuple(torch.from_numpy(a.copy()).to(device) for a in (c.u, c.p, c.n)),
                order=None if c.order is None else torch.from_numpy(c.order.copy()).to(device))


def _run(device, c, kind, inp, det, fused, ranges=None, item_twice=False):
    """One step on a zero state -> (dict of host arrays, the partition's split summary).  item_twice (gradI_out form):
    the item phase runs a second time over the same partition into a freshly pre-filled gradI_out."""
    from yelprecommendation_amd import engine
    lib = _lib()
    U, I = inp["U"], inp["I"].clone()
    U_new = torch.full_like(U, P.SENTINEL)
    mU, vU, mI, vI = torch.zeros_like(U), torch.zeros_like(U), torch.zeros_like(I), torch.zeros_like(I)
    grad = None if fused else torch.full_like(I, P.SENTINEL)
    partials = torch.zeros(engine.LOSS_PARTIALS, dtype=torch.float32, device=device)
    loss_out = torch.full((1,), -1.0, dtype=torch.float32, device=device)
    loss_accum = torch.full((1,), LOSS_START, dtype=torch.float64, device=device)
    flag = engine.new_error_flag(device)
    ws = engine.bpr_mf_pull_workspace(c.B, c.nu, c.ni, c.D, device)
    u, p, n = inp["ids"]
    s = engine._stream()
    adam = (P.LR, P.LR, BC2_SQRT, P.BETA1, P.BETA2, P.EPS, 0.0, engine.OPT_ADAM, 1 if det else 0)
    head = (U.data_ptr(), U_new.data_ptr(), I.data_ptr(), mU.data_ptr(), vU.data_ptr(), mI.data_ptr(), vI.data_ptr(),
            None if grad is None else grad.data_ptr())
    assert lib.yr_bpr_mf_pull_index(u.data_ptr(), p.data_ptr(), n.data_ptr(), c.B, c.D, c.nu, c.ni, ws.data_ptr(),
                                    ws.numel(), flag.data_ptr(), s) == 0

    def apply(phases, lo, hi, with_loss):
        tail = (ws.data_ptr(), ws.numel(), partials.data_ptr(), loss_out.data_ptr() if with_loss else None,
                loss_accum.data_ptr() if with_loss else None, phases, lo, hi)
        if inp["order"] is not None:
            return lib.yr_bpr_mf_pull_apply_ordered(*head, c.B, c.D, c.nu, c.ni, c.inv(kind), *adam, *tail,
                                                    inp["order"].data_ptr(), s)
        return lib.yr_bpr_mf_pull_apply(*head, c.B, c.D, c.nu, c.ni, c.inv(kind), *adam, *tail, s)

    if item_twice:
        assert not fused
        assert apply(engine.PULL_USER_PHASE, 0, 0, False) == 0
        assert apply(engine.PULL_ITEM_PHASE, 0, c.ni, False) == 0
        grad.fill_(P.SENTINEL)
        assert apply(engine.PULL_ITEM_PHASE, 0, c.ni, True) == 0
    elif ranges is None:
        assert apply(engine.PULL_USER_PHASE | engine.PULL_ITEM_PHASE, 0, c.ni, True) == 0
    else:
        assert apply(engine.PULL_USER_PHASE, 0, 0, False) == 0
        for k, (lo, hi) in enumerate(ranges):
            assert apply(engine.PULL_ITEM_PHASE, lo, hi, k == len(ranges) - 1) == 0
    torch.cuda.synchronize()
    summary = engine.bpr_mf_pull_split_summary(c.B, c.nu, c.ni, c.D, ws)
    out = dict(U_new=U_new, mU=mU, vU=vU, I=I, mI=mI, vI=vI, loss=loss_out, accum=loss_accum, flag=flag)
    if grad is not None:
        out["grad"] = grad
    return {k: v.cpu().numpy() for k, v in out.items()}, summary


def _same_bits(a, b):
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def _check_split(c, summary):
    """The partition's own words say what the batch was built for."""
    want, row_tasks, holds = C.wanted(c)
    assert summary["row_tasks"] == row_tasks and summary["row_task_pool"] == c.rule["row_task_pool"]
    assert np.array_equal(summary["parts"], want), np.flatnonzero(summary["parts"] != want)
    assert summary["tasks"] == int((want[want > 1] - 1).sum())


def _check(c, kind, out, fused, tag):
    """Every element of every output of one run against the reference (as test_gpu_bpr_pull_edges._check)."""
    ref = C.reference(c.name, kind)
    U, I = c.tables(kind)
    rnd = kind == "random"
    assert int(out["flag"][0]) == 0
    figures = {}

    def side(name, o, e, p0, m, v, p_new):
        idle = (o.n[:, 0] == 0)
        assert np.array_equal(p_new[idle].view(np.uint32), p0[idle].view(np.uint32)), (tag, name, "idle rows")
        assert not m[idle].any() and not v[idle].any(), (tag, name, "idle moments")
        if rnd:
            figures[f"{name} m"] = P.ratio(m, o.v, P.bar_g(o, e))
        else:
            assert np.array_equal(m.astype(np.float64), o.v), (tag, name, "m on the exact tables",
                                                                 float(np.abs(m - o.v).max()))
        figures[f"{name} v"] = P.ratio(v, P.v_of(o.v), P.bar_v(o, e))
        figures[f"{name} p"] = P.ratio(p_new, P.p_of(p0, o.v), P.bar_p(p0, o, e))

    side("user", ref.gU, ref.eU, U, out["mU"], out["vU"], out["U_new"])
    if fused:
        side("item", ref.gI, ref.eI, I, out["mI"], out["vI"], out["I"])
    else:
        g = out["grad"]
        assert np.array_equal(out["I"].view(np.uint32), I.view(np.uint32)) and not out["mI"].any() and not out["vI"].any()
        assert not g[ref.gI.n[:, 0] == 0].any(), (tag, "gradient rows without a record")
        if rnd:
            figures["item gradI_out"] = P.ratio(g, ref.gI.v, P.bar_g(ref.gI, ref.eI))
        else:
            assert np.array_equal(g.astype(np.float64), ref.gI.v), (tag, "gradI_out on the exact tables")
    loss = float(out["loss"][0])
    if not rnd and P.exact(P.quantum(ref.soft), ref.soft_sum):
        assert loss == float(ref.loss.v), (tag, "loss on the exact tables", loss, float(ref.loss.v))
    else:
        figures["loss"] = abs(loss - float(ref.loss.v)) / P.bar_loss(ref)
    assert float(out["accum"][0]) == LOSS_START + loss, (tag, "loss_accum")
    print(f"RATIO {tag}", {k: float(f"{r:.3g}") for k, r in figures.items()})
    assert all(r < 1.0 for r in figures.values()), (tag, figures)


@pytest.mark.parametrize("name", ["rows-64", "rows-16", "rows-32", "rows-128", "rows-64-order", "rows-overflow",
                                  "rows-crowded"])
def test_row_split_at_its_ends(device, name):
    """rows-64: buckets of min - 1 / min / min + 1 records (whole / split / split), at both sides of S = 2 -> 4, one
    record below the tile-range threshold (rows shared) and at it (tiles shared) in ONE batch, every record on one
    row (a heavy row inside one part, the other part empty), records on the rows of parts 1 .. 3 only (the owner
    keeps nothing and still runs Adam on its rows), 1,500 records (every part filters both chunks), a row that is
    light in the first chunk and heavy in the second, and the ragged last bucket (parts that own rows past the table).
    rows-16 / -32 / -128: the cap on S and the forms with the deal compiled out.  rows-64-order: the same batch with a
    start order.  rows-overflow: a batch that wants 516 row tasks against a pool of 512 — no bucket is split by row.
    rows-crowded: 156 tile-range tasks and 360 row tasks, more together than there are helper workgroups: the tile-range
    parts run, no bucket is split by row.
    Random and exact tables, default and deterministic mode (twice, bit-equal), fused Adam and gradI_out."""
    c = C.case(name)
    for kind in ("random", "exact"):
        inp = _upload(device, c, kind)
        for det in (False, True):
            for fused in (True, False):
                tag = f"{name} {kind} {'det' if det else 'default'} {'fused' if fused else 'gradI_out'}"
                out, summary = _run(device, c, kind, inp, det, fused)
                _check_split(c, summary)
                _check(c, kind, out, fused, tag)
                if det:
                    _same_bits(out, _run(device, c, kind, inp, det, fused)[0])


def test_item_phase_in_three_row_ranges(device):
    """Row-split buckets in each of three item row ranges written into one gradI_out (and one set of Adam rows): the
    row helpers of a call leave the tasks of buckets outside its range alone.  Equal to the one-range call, bit for
    bit in the deterministic mode."""
    c = C.case("rows-64-ranges")
    for kind in ("random", "exact"):
        inp = _upload(device, c, kind)
        for fused in (True, False):
            for det in (True, False):
                out, summary = _run(device, c, kind, inp, det, fused, ranges=c.ranges)
                _check_split(c, summary)
                _check(c, kind, out, fused, f"{c.name} ranges {kind} det={det} fused={fused}")
                if det:
                    _same_bits(out, _run(device, c, kind, inp, det, fused)[0])          # the one-range call


def test_item_phase_twice_over_one_partition(device):
    """Index once, user phase once, the item phase twice in the dense-gradient form: a row part leaves nothing behind
    (no counter, no slot), so the second pass writes every row again — into a gradI_out pre-filled afresh."""
    c = C.case("rows-64")
    for kind in ("random", "exact"):
        inp = _upload(device, c, kind)
        for det in (True, False):
            out, summary = _run(device, c, kind, inp, det, False, item_twice=True)
            _check_split(c, summary)
            _check(c, kind, out, False, f"{c.name} twice {kind} det={det}")
            if det:
                _same_bits(out, _run(device, c, kind, inp, det, False)[0])              # the single pass
