"""The ordered kernels of csrc/dcn_owned.hip, each called on its own with sentinel-filled outputs and every element
compared.  Head (yr_dcn_head_ordered): pred, loss partials, dh and dx0 torch.equal to yr_dcn_head's on the same inputs,
the weight gradients inside the bar of tests/dcn_ref64.py, twice the same bits, a workspace of 0xFF bytes changes none.
Scatter (yr_dcn_owned_assemble_bwd): np.array_equal to the sequential f32 restatement of tests/dcn_owned_cases.py (the
contract fixes every bit), inside the float64 bar, the default kernel's flags, untouched rows keep the sentinel."""
import numpy as np
import pytest
import torch

import dcn_owned_cases as O
import dcn_ref64 as R

pytestmark = pytest.mark.gpu
F32 = np.float32
S = R.SENTINEL
WEIGHTS = ("dcw", "dcb", "dWo", "dbo")


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---- head -----------------------------------------------------------------------------------------------------------

# (F, H, L, units): units 1, 3, 4, 5 (a lone wave, a workgroup short of one wave, a full one, a second one), 1024 (every
# wave of the 256 workgroups has exactly one unit), 1025 (the first wave's second trip), 2055 (a third trip that ends
# inside the second workgroup); F in {64, 256, 512}, H in {32, 1024}, L in {1, 8} — (512, 1024, 8) is the largest
# accumulator: 4 x 9,729 floats = 155,664 B of LDS
HEAD_CASES = [(64, 32, 1, 1), (256, 1024, 8, 3), (512, 32, 8, 4), (512, 1024, 8, 5), (64, 1024, 1, 5),
              (256, 32, 1, 1024), (64, 1024, 8, 1025), (64, 32, 1, 2055)]


def _head(c, device, deterministic, workspace=None):
    from yelprecommendation_amd import engine
    rows = c["x"].shape[0]
    out = {"pred": torch.full((rows,), S, dtype=torch.float32, device=device),
           "loss": torch.full((R.LOSS_PARTIALS,), S, dtype=torch.float32, device=device),
           "dh": torch.full((rows, c["H"]), S, dtype=torch.float32, device=device),
           "dx0": torch.full((rows, c["F"]), S, dtype=torch.float32, device=device)}
    for k in WEIGHTS:
        out[k] = _t(c["old"][k], device)
    kw = dict(deterministic=True, workspace=workspace) if deterministic else {}
    engine.dcn_head(_t(c["x"], device), _t(c["h"], device), _t(c["cw"], device), _t(c["cb"], device),
                    _t(c["Wo"], device), _t(c["bo"], device), c["bpr"], inv_batch=c["inv_batch"], pred=out["pred"],
                    gpred=None if c["bpr"] else _t(c["gpred"], device),
                    grads=(out["dh"], out["dx0"]) + tuple(out[k] for k in WEIGHTS), loss_partials=out["loss"], **kw)
    return out


@pytest.mark.parametrize("bpr", [True, False], ids=["bpr", "gpred"])
@pytest.mark.parametrize("F,H,L,units", HEAD_CASES)
def test_ordered_head(device, F, H, L, units, bpr):
    from yelprecommendation_amd import engine
    c = R.head_case(F, H, L, units, bpr)
    ref = R.head_ref(c)
    default = _head(c, device, False)
    a = _head(c, device, True)
    b = _head(c, device, True)
    nbytes = engine.dcn_owned_head_workspace_bytes(units, F, H, L)
    assert nbytes >= R.head_grid(units) * ((2 * L + 1) * F + H + 1) * 4
    poisoned = _head(c, device, True, workspace=torch.full((nbytes,), 255, dtype=torch.uint8, device=device))
    for k in ("pred", "loss", "dh", "dx0"):
        assert torch.equal(a[k], default[k]), (k, "differs from yr_dcn_head")
    for k in a:
        assert torch.equal(a[k], b[k]), (k, "two calls differ")
        assert torch.equal(a[k], poisoned[k]), (k, "the workspace's contents reached the result")
    for k in WEIGHTS:
        r = R.ratio(a[k].cpu().numpy(), ref[k].plus(c["old"][k]))
        print(f"ordered head {k}: error / bar = {r:.3g}")
        assert r <= 1.0, (k, r)
    # forward only: no workspace, the default kernel's outputs
    fwd = {"pred": torch.full_like(a["pred"], S), "loss": torch.full_like(a["loss"], S)}
    engine.dcn_head(_t(c["x"], device), _t(c["h"], device), _t(c["cw"], device), _t(c["cb"], device),
                    _t(c["Wo"], device), _t(c["bo"], device), c["bpr"], pred=fwd["pred"],
                    loss_partials=fwd["loss"] if bpr else None, deterministic=True)
    assert torch.equal(fwd["pred"], default["pred"])
    assert torch.equal(fwd["loss"], default["loss"]) if bpr else bool((fwd["loss"] == S).all())


# ---- scatter --------------------------------------------------------------------------------------------------------

def _scatter(c, old, device, deterministic=True, workspace=None, lists=None):
    """(gU, gI, gC, gS as numpy, flag) of engine.dcn_assemble_bwd on copies of ``old``."""
    from yelprecommendation_amd import engine
    t = c["t"]
    attrs = (_t(t["cat"], device), _t(t["sc"], device), t["nc"], t["ns"])
    g = [_t(a, device) for a in old]
    flag = engine.new_error_flag(device)
    kw = dict(deterministic=True, workspace=workspace, lists=lists) if deterministic else {}
    engine.dcn_assemble_bwd(_t(c["dx"], device), attrs, _t(c["u"], device), _t(c["p"], device), _t(c["n"], device),
                            *g, t["nu"], err_flag=flag, **kw)
    return [a.cpu().numpy() for a in g], int(flag.item())


def _assert_tables_equal(got, want, what):
    for name, g, w in zip(("gU", "gI", "gC", "gS"), got, want):
        if not np.array_equal(g, w):
            rows = np.flatnonzero((g != w).any(1))
            raise AssertionError((what, name, "rows", rows[:8], g[rows[0]][:4], w[rows[0]][:4]))


def _in_bar(c, got, old, what):
    t = c["t"]
    ref, flag = R.assemble_bwd(c["dx"], t["cat"], t["sc"], t["nu"], t["ni"], t["nc"], t["ns"], c["u"], c["p"], c["n"])
    for name, g, o, r in zip(("gU", "gI", "gC", "gS"), got, old, ref):
        v = R.ratio(g, r.plus(o))
        assert v <= 1.0, (what, name, v)
    return flag


@pytest.mark.parametrize("B", O.BATCHES)
@pytest.mark.parametrize("D", O.WIDTHS)
def test_ordered_scatter_equals_the_sequential_restatement(device, D, B):
    """40 users, 600 items, 9 categories (Lmax 4), 5 state-cities; B = 1, 5 and 700 — at 700: a user on 48 triplets, an
    item that is pos and neg of one triplet, an item in both roles of different triplets, slots that repeat a category,
    category lists of one chunk, one chunk + 1 and three chunks with more than two chunks' worth of touched items.  Into
    tables of their own numbers and into sentinel-filled ones: every element equals the f32 loops, stays inside the
    float64 bar, untouched rows keep what they held; a workspace of 0xFF bytes and a second call change no bit."""
    from yelprecommendation_amd import engine
    c = O.scatter_case(D, B)
    lists = engine.DCNAttrLists(_t(c["t"]["cat"], device), _t(c["t"]["sc"], device), O.NC, O.NS, device=device)
    nbytes = engine.dcn_owned_scatter_workspace_bytes(O.NU, O.NI, B, D, lists)
    for old in (O.old_tables(D), O.old_tables(D, value=S)):
        want = O.expected(c, old)
        got, flag = _scatter(c, old, device)
        assert flag == want[4] == 0
        _assert_tables_equal(got, want[:4], (D, B))
        assert _in_bar(c, got, old, (D, B)) == 0
        ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=device)
        again, _ = _scatter(c, old, device, workspace=ws, lists=lists)
        _assert_tables_equal(again, got, (D, B, "poisoned workspace"))
    for g, m in zip(got, O.touched(c)):
        assert (~m).any() and (g[~m] == F32(S)).all(), "an untouched row was written"


@pytest.mark.parametrize("D", O.WIDTHS)
def test_ordered_scatter_dyadic_twin_and_lmax_three(device, D):
    """Sixteenths: every sum is exact, so the ordered kernel, the default kernel and float64 agree bit for bit.  The
    twin at Lmax = 3 (the divide rounds) is judged by the float64 bar only."""
    c = O.scatter_case(D, 700, dyadic=True)
    old = O.old_tables(D, dyadic=True)
    got, flag = _scatter(c, old, device)
    default, dflag = _scatter(c, old, device, deterministic=False)
    assert flag == dflag == 0
    _assert_tables_equal(got, O.expected(c, old)[:4], (D, "dyadic"))
    _assert_tables_equal(got, default, (D, "dyadic, default kernel"))
    c3 = O.scatter_case(D, 700, Lmax=3)
    old3 = O.old_tables(D)
    got3, flag3 = _scatter(c3, old3, device)
    assert flag3 == 0 and _in_bar(c3, got3, old3, (D, "Lmax 3")) == 0


def test_ordered_scatter_empty_batch(device):
    c = O.scatter_case(16, 700)
    c = dict(c, u=c["u"][:0], p=c["p"][:0], n=c["n"][:0], dx=c["dx"][:0], B=0)
    old = O.old_tables(16, value=S)
    got, flag = _scatter(c, old, device)
    assert flag == 0
    _assert_tables_equal(got, old, "empty batch")


@pytest.mark.parametrize("kind", R.BAD_IDS)
def test_ordered_scatter_bad_ids(device, kind):
    """The bad-id variants of dcn_ref64.make_bad: a bad user loses its user part only, a bad item its item and
    attribute parts, a slot out of range adds nothing; the flags are the default kernel's and the restatement's."""
    D, B = 16, 700
    c = O.scatter_case(D, B)
    t, (u, p, n, _), flag, _, _ = R.make_bad(c["t"], (c["u"], c["p"], c["n"], None), kind, B)
    c = dict(c, t=t, u=u, p=p, n=n)
    old = O.old_tables(D)
    want = O.expected(c, old)
    got, gflag = _scatter(c, old, device)
    _, dflag = _scatter(c, old, device, deterministic=False)
    assert gflag == dflag == want[4] == flag
    _assert_tables_equal(got, want[:4], kind)
    assert _in_bar(c, got, old, kind) == flag


def test_ordered_scatter_refuses_other_forms(device):
    from yelprecommendation_amd import engine
    c = O.scatter_case(16, 5)
    t = c["t"]
    attrs = (_t(t["cat"], device), _t(t["sc"], device), t["nc"], t["ns"])
    g = [_t(a, device) for a in O.old_tables(16)]
    with pytest.raises(engine.EngineError, match="unsupported"):
        engine.dcn_assemble_bwd(_t(c["dx"][:5], device), attrs, _t(c["u"], device), _t(c["p"], device), None, *g, t["nu"],
                                deterministic=True)
