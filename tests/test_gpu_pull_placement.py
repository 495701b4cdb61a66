"""The pull-form BPR step with its owner workgroups placed by XCD class (csrc/pull_placement.h), through the C ABI,
compared as test_gpu_bpr_pull_edges.py compares (its _run; the float64 reference and the bars of bpr_pull_ref64.py).

Placement changes which workgroup takes which bucket and nothing else, so what can go wrong is a bucket nobody takes
(its rows keep the sentinel / their input), a bucket taken twice (Adam applied twice: the update is off by far more
than a bar), and a padded slot that takes a bucket beyond the table.  D = 64 (buckets of 16 rows), B = 3,000 (three
tiles), tables of 16 nb - 5 rows so that the last bucket is ragged and the owner grid ends with empty slots:

  nb = 1, 7, 9, 63, 65, 129 on both sides   the user side in its narrow form (buckets of 4 rows: 3 .. 515 of them, one
                                            to nine rounds of 64 slots), the item side with 1 .. 129 buckets of 16
  nu = 16 * 769 - 5                         the wide user form: 769 buckets on 832 slots
  three item row ranges, no order           40 + 1 + 88 buckets: the map over a range's length behind bucket_begin
  an order from the builder / reversed      the item pass with a start order (the map is not applied)

Every case: random and exact tables, default and deterministic mode (twice, bit-equal), fused Adam and gradI_out."""
import functools

import numpy as np
import pytest
import torch

import bpr_pull_ref64 as P
from test_gpu_bpr_pull_edges import LOSS_START, _lib, _run, _same_bits

pytestmark = pytest.mark.gpu

D, B = 64, 3000
NBS = (1, 7, 9, 63, 65, 129)
WIDE_NB = P.NARROW_BELOW + 1


@functools.lru_cache(maxsize=None)
def _case(nbu, nbi):
    r = P.R(D)
    nu, ni = r * nbu - 5, r * nbi - 5
    rs = np.random.RandomState(P._seed("placement", nbu, nbi))
    q = P._uniform(rs, B, nu, ni)
    # the last row of either table holds records (the ragged last bucket is not idle)
    last_even, last_odd = (ni - 1) - (ni - 1) % 2, (ni - 1) - (ni % 2)
    q[0][:7], q[1][:5], q[2][:5] = nu - 1, last_even, last_odd
    for a in q:
        rs.shuffle(a)
    c = P.Case(f"placement-{nbu}-{nbi}", D, nu, ni, [q])
    assert c.plan.T == 3 and c.plan.nbI == nbi and c.plan.narrow == (nbu < P.NARROW_BELOW)
    assert c.plan.nbU == (-(-nu // P.NARROW_ROWS) if c.plan.narrow else nbu)
    return c


@functools.lru_cache(maxsize=None)
def _reference(nbu, nbi, kind):
    c = _case(nbu, nbi)
    U, I = c.tables(kind)
    return P.step(U, I, c.u, c.p, c.n, c.inv(kind))


def _upload(device, c, kind, order=None):
    U, I = c.tables(kind)
    return dict(U=torch.from_numpy(U.copy()).to(device), I=torch.from_numpy(I.copy()).to(device),
                ids=tuple(torch.from_numpy(a.copy()).to(device) for a in (c.u, c.p, c.n)),
                order=None if order is None else torch.from_numpy(np.ascontiguousarray(order, np.int32)).to(device))


def _check(c, ref, kind, out, fused, tag):
    """test_gpu_bpr_pull_edges._check on a reference passed in: every element of every output."""
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
            assert np.array_equal(m.astype(np.float64), o.v), (tag, name, "m on the exact tables")
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


def _all_forms(device, nbu, nbi, orders=(None,), ranges=None):
    """Both tables, both modes, both item forms, every order: each run against the reference; the deterministic runs
    twice, bit-equal, and bit-equal over the orders and to the one-range call."""
    c = _case(nbu, nbi)
    for kind in ("random", "exact"):
        ref = _reference(nbu, nbi, kind)
        for fused in (True, False):
            for det in (False, True):
                first = None
                for k, order in enumerate(orders):
                    inp = _upload(device, c, kind, order)
                    tag = f"{c.name} {kind} det={det} fused={fused} order={k} ranges={ranges is not None}"
                    out = _run(device, c, kind, inp, det, fused, ranges=ranges)
                    _check(c, ref, kind, out, fused, tag)
                    if det:
                        _same_bits(out, _run(device, c, kind, inp, det, fused))     # again; the one-range call
                        first = first or out
                        _same_bits(out, first)


@pytest.mark.parametrize("nb", NBS)
def test_ragged_tables_with_padded_slots(device, nb):
    _all_forms(device, nb, nb)


def test_wide_user_form_with_padded_slots(device):
    _all_forms(device, WIDE_NB, 9)


def test_item_phase_in_three_row_ranges_without_an_order(device):
    r = P.R(D)
    c = _case(129, 129)
    _all_forms(device, 129, 129, ranges=[(0, 40 * r), (40 * r, 41 * r), (41 * r, c.ni)])


@pytest.mark.parametrize("nb", (65, 129))
def test_item_pass_with_the_builders_order_and_its_reverse(device, nb):
    c = _case(nb, nb)
    _, load = c.bucket_totals()
    load = np.ascontiguousarray(load, np.float64)
    order = np.full(nb, -1, np.int32)
    assert _lib().yr_bpr_mf_pull_item_start_order(load.ctypes.data, nb, order.ctypes.data) == 0
    assert np.array_equal(np.sort(order), np.arange(nb))
    _all_forms(device, nb, nb, orders=(order, order[::-1].copy()))
