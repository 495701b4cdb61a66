"""Without a GPU: the cases of dcn_owned_cases.py can tell a wrong summation order (and a moved chunk boundary) from the
contract's, their expected values agree with the float64 restatement of tests/dcn_ref64.py (inside its bar; exactly on
the dyadic twins), the inverted-list builder of the engine equals a brute-force inversion, and the entry points of
csrc/dcn_owned.hip refuse what they must before any launch (error codes, workspace sizes)."""
import ctypes

import numpy as np
import pytest
import torch

import dcn_owned_cases as O
import dcn_ref64 as R

F32 = np.float32


def test_cases_can_see_a_wrong_order():
    """User rows of 48 contributions and item rows of >= 16 at D = 16: summed in reversed and in a random order at
    least one element changes, for at least 9 rows in 10."""
    c = O.order_case()
    users, items, flag = O.entries(c)
    assert flag == 0
    D = c["D"]
    rows = [O.user_terms(c, bs) for bs in users.values()]
    rows += [[c["dx"][r, D:2 * D] for r in rs_] for rs_ in items.values() if len(rs_) >= 16]
    assert len(users) == 40 and len(rows) >= 60 and min(len(t) for t in rows) >= 16
    rs = np.random.RandomState(1)
    zero = np.zeros(D, F32)
    rev = rnd = 0
    for t in rows:
        want = O.chain(zero, t)
        rev += not np.array_equal(want, O.chain(zero, t, range(len(t) - 1, -1, -1)))
        rnd += not np.array_equal(want, O.chain(zero, t, rs.permutation(len(t))))
    assert rev * 10 >= 9 * len(rows) and rnd * 10 >= 9 * len(rows), (rev, rnd, len(rows))


def test_chunk_boundaries_are_visible():
    """Category 3 (600 entries, three chunks, 560 touched items): a boundary moved by one entry, and the row summed as
    one chain, each change at least one element of its gradient; the default is what ``expected`` states."""
    c = O.scatter_case(16, 700)
    old = O.old_tables(16)
    inv = O.invert(c["t"])
    k = O.THREE_CHUNK_CAT
    assert inv["cat_chunk_ptr"][k + 1] - inv["cat_chunk_ptr"][k] == 3
    _, mi, _, _ = O.touched(c)
    assert mi[inv["cat_item"][inv["cat_ptr"][k]:inv["cat_ptr"][k + 1]]].sum() > 2 * O.CHUNK
    want = O.expected(c, old)[2]
    moved = O.expected(c, old, chunk=O.CHUNK - 1)[2]
    chained = O.expected(c, old, one_chain=(k,))[2]
    assert not np.array_equal(want[k], moved[k]) and not np.array_equal(want[k], chained[k])
    rest = [r for r in range(O.NC) if r != k]
    assert np.array_equal(want[rest], chained[rest])


@pytest.mark.parametrize("D,B", [(16, 700), (64, 5), (16, 1)])
def test_expected_agrees_with_float64(D, B):
    """The sequential f32 loops against dcn_ref64.assemble_bwd under its bar; bit for bit on the dyadic twin; rows
    nothing touches keep the sentinel."""
    for dyadic in (False, True):
        c = O.scatter_case(D, B, dyadic=dyadic)
        t = c["t"]
        old = O.old_tables(D, dyadic)
        got = O.expected(c, old)
        ref, flag = R.assemble_bwd(c["dx"], t["cat"], t["sc"], t["nu"], t["ni"], t["nc"], t["ns"], c["u"], c["p"], c["n"])
        assert flag == got[4] == 0
        for g, o, r in zip(got[:4], old, ref):
            r = r.plus(o)
            if dyadic:
                assert R.exact(2.0 ** -6, r.s) and np.array_equal(g.astype(np.float64), r.v)
            else:
                assert R.ratio(g, r) <= 1.0
    c = O.scatter_case(D, B)
    sent = O.expected(c, O.old_tables(D, value=R.SENTINEL))
    for g, m in zip(sent[:4], O.touched(c)):
        assert (~m).any() and (g[~m] == F32(R.SENTINEL)).all() and (g[m] != F32(R.SENTINEL)).any()
    if B == 700:
        users, items, _ = O.entries(c)
        assert len(users[O.HOT_USER]) == O.HOT_TRIPLETS and O.SAME_AT in items[int(c["p"][O.SAME_AT])]
        assert len(items) >= 560 and {3, B + 5} <= set(items[O.BOTH_ITEM])


@pytest.mark.parametrize("kind", R.BAD_IDS)
def test_expected_on_bad_ids(kind):
    """The bad-id variants of dcn_ref64.make_bad: the restatement raises the reference's flag and stays in its bar."""
    c = O.scatter_case(16, 700)
    t, (u, p, n, _), flag, _, _ = R.make_bad(c["t"], (c["u"], c["p"], c["n"], None), kind, 700)
    c = dict(c, t=t, u=u, p=p, n=n)
    old = O.old_tables(16)
    got = O.expected(c, old)
    ref, rflag = R.assemble_bwd(c["dx"], t["cat"], t["sc"], t["nu"], t["ni"], t["nc"], t["ns"], u, p, n)
    assert got[4] == rflag == flag
    for g, o, r in zip(got[:4], old, ref):
        assert R.ratio(g, r.plus(o)) <= 1.0


def test_inverted_lists_equal_brute_force():
    """engine.DCNAttrLists against loops over the table: multiplicity 2, the padding category, an empty category, lists
    of exactly one chunk, one chunk + 1 and three chunks; slots and state-cities out of range are in no list."""
    from yelprecommendation_amd import engine
    assert engine.DCN_OWNED_CHUNK == O.CHUNK
    t = O.tables()
    for bad in (False, True):
        if bad:
            t["cat"][4, 0], t["cat"][9, 1], t["sc"][11], t["sc"][12] = -1, t["nc"], t["ns"], -2
        want = O.invert(t)
        got = engine.DCNAttrLists(torch.from_numpy(t["cat"]), torch.from_numpy(t["sc"]), t["nc"], t["ns"])
        for k in engine.DCNAttrLists.FIELDS:
            g = getattr(got, k).numpy()
            assert g.dtype == np.int32 and np.array_equal(g[:len(want[k])], want[k]), k
        assert got.cat_chunks == want["cat_chunk_ptr"][-1] and got.sc_chunks == want["sc_chunk_ptr"][-1]
    want = O.invert(O.tables())
    n = np.diff(want["cat_ptr"])
    assert n[O.EMPTY_CAT] == 0 and n[O.ONE_CHUNK_CAT] == O.CHUNK and n[O.CHUNK_PLUS_ONE_CAT] == O.CHUNK + 1
    assert np.diff(want["cat_chunk_ptr"])[[O.EMPTY_CAT, O.ONE_CHUNK_CAT, O.CHUNK_PLUS_ONE_CAT]].tolist() == [0, 1, 2]
    k = O.THREE_CHUNK_CAT
    seg = slice(want["cat_ptr"][k], want["cat_ptr"][k + 1])
    twice = want["cat_item"][seg][want["cat_mult"][seg] == 2]
    assert sorted(twice.tolist()) == sorted(O.TWICE_ITEMS) and n[0] > O.CHUNK and want["cat_mult"][:n[0]].max() == 3


def _lib():
    from yelprecommendation_amd import _lib
    return _lib.load(), _lib


def test_new_exports_and_workspace_sizes():
    lib, L = _lib()
    for name in ("yr_dcn_owned_head_workspace_bytes", "yr_dcn_head_ordered", "yr_dcn_owned_scatter_workspace_bytes",
                 "yr_dcn_owned_assemble_bwd"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    head, scat = lib.yr_dcn_owned_head_workspace_bytes, lib.yr_dcn_owned_scatter_workspace_bytes
    assert head(-1, 64, 32, 1) == -2 and head(4, 0, 32, 1) == -2 and head(4, 64, 0, 1) == -2 and head(4, 64, 32, 0) == -2
    assert head(4, 513, 32, 1) == -1 and head(4, 64, 1025, 1) == -1 and head(4, 64, 32, 9) == -1
    nacc = lambda F, H, L_: (2 * L_ + 1) * F + H + 1
    up = lambda x: (x + 255) // 256 * 256
    for units in (0, 1, 3, 4, 5, 1024, 1025, 2055, 1 << 20):
        assert head(units, 256, 1024, 1) == up(R.head_grid(units) * nacc(256, 1024, 1) * 4)
    assert head(1 << 20, 512, 1024, 8) == up(256 * 9729 * 4) and 4 * 9729 * 4 == 155664
    assert scat(0, 10, 1, 64, 1, 1) == -2 and scat(10, 0, 1, 64, 1, 1) == -2 and scat(10, 10, -1, 64, 1, 1) == -2
    assert scat(10, 10, 1, 0, 1, 1) == -2 and scat(10, 10, 1, 64, -1, 1) == -2 and scat(1 << 31, 10, 1, 64, 1, 1) == -2
    assert scat(10, 10, 1, 48, 1, 1) == -1 and scat(10, 10, 1 << 29, 64, 1, 1) == -1
    last = 0
    for B in (0, 1, 32, 4096, 65536):
        s = scat(31668, 38048, B, 64, 2000, 500)
        # counts and segment starts, three int32 per entry three times, T [items, 2 D], the chunks' partials and counts
        assert s % 256 == 0 and s >= max(last, 8 * (31668 + 38048) + 36 * B + 8 * 38048 * 64 + 2500 * (4 * 64 + 4))
        last = s


def test_argument_checks_without_gpu():
    lib, _ = _lib()
    one = ctypes.c_void_p(256)                                        # a non-null, aligned address that is never read
    h = lib.yr_dcn_head_ordered

    def head(units=4, F=64, H=32, L=1, x0=one, bpr=1, loss=one, dx0=one, dh=one, gpred=None, ws=one, wsb=1 << 20):
        return h(x0, F, one, H, units, F, H, L, one, one, one, one, bpr, 0.25, None, gpred, dh, H, dx0, F, one, one,
                 one, one, loss, ws, wsb, None)
    assert head(units=-1) == -2 and head(F=0) == -2 and head(L=0) == -2
    assert head(F=516) == -1 and head(H=1056) == -1 and head(L=9) == -1
    assert head(x0=None) == -2 and head(loss=None) == -2 and head(dh=None) == -2
    assert head(bpr=0, gpred=None) == -2                              # the gpred form without gpred
    assert head(ws=None) == -2 and head(wsb=16) == -2 and head(wsb=-1) == -2
    assert head(ws=ctypes.c_void_p(258)) == -2
    assert head(wsb=lib.yr_dcn_owned_head_workspace_bytes(4, 64, 32, 1) - 256) == -2
    f = lib.yr_dcn_owned_assemble_bwd

    def scatter(B=4, D=64, user=one, a=one, b=one, per_row=0, dx=one, ldx=256, lists=one, ws=one, wsb=1 << 30, nu=40,
                Lmax=4, chunks=3):
        return f(dx, ldx, one, one, Lmax, D, nu, 600, 9, 5, user, a, b, B, per_row, lists, one, one, one, chunks, one, one,
                 one, 1, one, one, one, one, ws, wsb, None, None)
    assert scatter(B=-1) == -2 and scatter(nu=0) == -2 and scatter(Lmax=0) == -2 and scatter(chunks=-1) == -2
    assert scatter(D=48) == -1 and scatter(B=1 << 29) == -1
    assert scatter(user=None) == -1 and scatter(b=None) == -1 and scatter(a=None) == -1 and scatter(per_row=1) == -1
    assert scatter(B=0) == 0 and scatter(B=0, user=None, a=None, b=None, dx=None, ws=None, wsb=0) == 0
    assert scatter(dx=None) == -2 and scatter(lists=None) == -2 and scatter(ws=None) == -2
    assert scatter(ldx=255) == -2 and scatter(ldx=258) == -2 and scatter(dx=ctypes.c_void_p(260)) == -2
    assert scatter(wsb=16) == -2 and scatter(wsb=-1) == -2
    assert scatter(wsb=lib.yr_dcn_owned_scatter_workspace_bytes(40, 600, 4, 64, 3, 1) - 256) == -2


def test_model_flag_defaults_and_refusal_text():
    from yelprecommendation_amd.models.dcn import DCN
    from yelprecommendation_amd.utils import make_config
    m = DCN(make_config("DCN", device="cpu", embed_size=16, hidden_dims=[32], cross_orders=1), 5, 7, [3, 2])
    assert m.deterministic is False
