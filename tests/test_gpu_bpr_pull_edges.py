"""The pull-form BPR step (csrc/bpr_pull.hip) at the ends of its loops, through the C ABI (yr_bpr_mf_pull_index +
yr_bpr_mf_pull_apply[_ordered], and yr_bpr_mf_pull_step once), against tests/bpr_pull_ref64.py (float64).

ONE call on a zero Adam state with beta1 = 0 and eps = 1 (see the helper's docstring): m is the raw gradient of the
step, v = (1 - beta2) g^2, the update p - lr g / (|g| + 1).  Every element of mU, vU, U_new and of the item side in
both forms (fused Adam: mI, vI, I; dense gradient: gradI_out, with I, mI, vI untouched) is compared — inside the bar
on the random tables, EQUAL to float64 on the certified exact tables (mU, mI, gradI_out, and the loss where its
certificate holds); no agreement quotas.  Rows without a record come back bit-equal to their input (U_new and
gradI_out are pre-filled with a sentinel: a row that was not written shows).  Every case runs in the default and the
deterministic mode; deterministic runs are made twice and must be bit-equal.

The cases, their batches and what each is there for (T, nb, parts, tasks from the kernel's constants) are stated in
bpr_pull_ref64.py and asserted without a GPU by test_bpr_pull_ref64.py.  Measured figures: tests/README.md."""
import functools

import numpy as np
import pytest
import torch

import bpr_pull_ref64 as P

pytestmark = pytest.mark.gpu

BC2_SQRT = float(np.sqrt(1.0 - P.BETA2))
LOSS_START = 3.5                       # loss_accum is added onto a non-zero start


@functools.lru_cache(maxsize=None)
def _lib():
    from yelprecommendation_amd import _lib as L
    return L.load()


def _upload(device, c, kind):
    U, I = c.tables(kind)
    return dict(U=torch.from_numpy(U.copy()).to(device), I=torch.from_numpy(I.copy()).to(device),
                ids=tuple(torch.from_numpy(a.copy()).to(device) for a in (c.u, c.p, c.n)),
                order=None if c.order is None else torch.from_numpy(c.order.copy()).to(device))


def _run(device, c, kind, inp, det, fused, ranges=None, via_step=False):
    """One step on a zero state -> dict of host arrays."""
    from yelprecommendation_amd import engine
    lib = _lib()
    U, I0 = inp["U"], inp["I"]
    I = I0.clone()
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
    gp = None if grad is None else grad.data_ptr()
    adam = (P.LR, P.LR, BC2_SQRT, P.BETA1, P.BETA2, P.EPS, 0.0, engine.OPT_ADAM, 1 if det else 0)
    head = (U.data_ptr(), U_new.data_ptr(), I.data_ptr(), mU.data_ptr(), vU.data_ptr(), mI.data_ptr(), vI.data_ptr(), gp)
    if via_step:
        rc = lib.yr_bpr_mf_pull_step(*head, u.data_ptr(), p.data_ptr(), n.data_ptr(), c.B, c.D, c.nu, c.ni,
                                     c.inv(kind), *adam, ws.data_ptr(), ws.numel(), partials.data_ptr(),
                                     loss_out.data_ptr(), loss_accum.data_ptr(), flag.data_ptr(), s)
        assert rc == 0
    else:
        rc = lib.yr_bpr_mf_pull_index(u.data_ptr(), p.data_ptr(), n.data_ptr(), c.B, c.D, c.nu, c.ni, ws.data_ptr(),
                                      ws.numel(), flag.data_ptr(), s)
        assert rc == 0

        def apply(phases, lo, hi, with_loss):
            tail = (ws.data_ptr(), ws.numel(), partials.data_ptr(), loss_out.data_ptr() if with_loss else None,
                    loss_accum.data_ptr() if with_loss else None, phases, lo, hi)
            if inp["order"] is not None:
                return lib.yr_bpr_mf_pull_apply_ordered(*head, c.B, c.D, c.nu, c.ni, c.inv(kind), *adam, *tail,
                                                        inp["order"].data_ptr(), s)
            return lib.yr_bpr_mf_pull_apply(*head, c.B, c.D, c.nu, c.ni, c.inv(kind), *adam, *tail, s)

        if ranges is None:
            assert apply(engine.PULL_USER_PHASE | engine.PULL_ITEM_PHASE, 0, c.ni, True) == 0
        else:
            assert apply(engine.PULL_USER_PHASE, 0, 0, False) == 0
            for k, (lo, hi) in enumerate(ranges):
                assert apply(engine.PULL_ITEM_PHASE, lo, hi, k == len(ranges) - 1) == 0
    torch.cuda.synchronize()
    out = dict(U_new=U_new, mU=mU, vU=vU, I=I, mI=mI, vI=vI, loss=loss_out, accum=loss_accum, flag=flag)
    if grad is not None:
        out["grad"] = grad
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b):
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def _check(c, kind, out, fused, tag):
    """Every element of every output of one run against the reference."""
    from yelprecommendation_amd import engine
    ref = P.reference(c.name, kind)
    U, I = c.tables(kind)
    rnd = kind == "random"
    assert int(out["flag"][0]) == ref.flags[0] * engine.FLAG_BAD_USER + ref.flags[1] * engine.FLAG_BAD_ITEM
    figures = {}

    def side(name, o, e, p0, m, v, p_new):
        idle = (o.n[:, 0] == 0)
        # rows without a record: bit-equal to their input, zero moments
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


def test_fast_forms_are_exact_where_the_twins_use_them(device):
    """The premise of the exact twins, measured: at x <= -256 v_exp_f32 underflows to 0, v_rcp_f32(1) = 1 and
    v_log_f32(1) = 0, so g = -inv_batch and softplus = -x exactly.  One triplet, U[u] = 1: gradI_out reads g directly."""
    from yelprecommendation_amd import engine
    D = 16
    ids = tuple(torch.tensor([v], dtype=torch.int64, device=device) for v in (0, 0, 1))
    for x in (-258.0, -512.0, -766.0):
        c = P.Case(f"probe{x}", D, 1, 2, [[np.array([0]), np.array([0]), np.array([1])]])
        U = np.ones((1, D), np.float32)
        I = np.zeros((2, D), np.float32)
        I[0, 0], I[1, 0] = x / 2, -x / 2
        inp = dict(U=torch.from_numpy(U).to(device), I=torch.from_numpy(I).to(device), ids=ids, order=None)
        c.inv = lambda kind: P.INV_EXACT
        out = _run(device, c, "exact", inp, det=False, fused=False)
        assert int(out["flag"][0]) == 0
        assert np.all(out["grad"][0] == -P.INV_EXACT) and np.all(out["grad"][1] == P.INV_EXACT), (x, out["grad"])
        assert float(out["loss"][0]) == -x * P.INV_EXACT, (x, float(out["loss"][0]))
        assert np.all(out["mU"][0, 1:] == 0) and out["mU"][0, 0] == -P.INV_EXACT * x
    assert engine.LOSS_PARTIALS == P.USER_GRID


@pytest.mark.parametrize("name", P.case_names())
def test_pull_step_at_its_loop_ends(device, name):
    """Random and exact tables, default and deterministic mode, fused-Adam and gradI_out item forms: twelve runs per
    case (the deterministic ones twice, bit-equal — in the overflow case too: which buckets are shared is a function
    of the batch alone)."""
    c = P.case(name)
    for kind in ("random", "exact"):
        inp = _upload(device, c, kind)
        for det in (False, True):
            for fused in (True, False):
                tag = f"{name} {kind} {'det' if det else 'default'} {'fused' if fused else 'gradI_out'}"
                out = _run(device, c, kind, inp, det, fused)
                _check(c, kind, out, fused, tag)
                if det:
                    _same_bits(out, _run(device, c, kind, inp, det, fused))


def test_item_phase_in_three_row_ranges(device):
    """Two shared buckets, in the first and the third of three item row ranges written into one gradI_out (and one set
    of Adam rows): equal to the one-range call, bit for bit in the deterministic mode, at the bar in the default mode."""
    c = P.case("shared-two-ranges")
    for kind in ("random", "exact"):
        inp = _upload(device, c, kind)
        for fused in (True, False):
            for det in (True, False):
                out = _run(device, c, kind, inp, det, fused, ranges=c.ranges)
                _check(c, kind, out, fused, f"{c.name} ranges {kind} det={det} fused={fused}")
                if det:
                    _same_bits(out, _run(device, c, kind, inp, det, fused))          # the one-range call


@pytest.mark.parametrize("name", ["chunkrows-64", "shared-2049"])
def test_one_call_equals_index_plus_apply(device, name):
    """yr_bpr_mf_pull_step == yr_bpr_mf_pull_index + yr_bpr_mf_pull_apply, bit for bit in the deterministic mode."""
    c = P.case(name)
    inp = _upload(device, c, "random")
    for fused in (True, False):
        _same_bits(_run(device, c, "random", inp, True, fused, via_step=True), _run(device, c, "random", inp, True, fused))
