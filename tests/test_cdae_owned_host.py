"""Without a GPU: the owner-pass entry points (csrc/cdae_owned.hip) refuse what they must before any launch, CDAEStep
accepts deterministic=True where the mode exists and nowhere else, every case of cdae_owned_cases.py reaches the loop
end it is there for, the reference's bars notice one lost or doubled list entry, and the order-sensitive generator
makes an f32 row sum depend on its order."""
import ctypes

import numpy as np
import pytest

import cdae_owned_cases as O
import cdae_ref64 as R


def _lib():
    from yelprecommendation_amd import _lib
    return _lib.load()


# ---- the C ABI ------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_and_sized():
    from yelprecommendation_amd import _lib
    lib = _lib.load()
    for name in ("yr_cdae_owned_workspace_bytes", "yr_cdae_owned_decode", "yr_cdae_owned_hidden_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    size = lib.yr_cdae_owned_workspace_bytes
    for B, I, H in ((0, 1, 16), (1, 1, 16), (33, 33, 32), (65, 9, 256), (256, 38048, 64), (1025, 200, 16), (300, 6001, 1024)):
        assert size(B, I, H) == O.workspace_bytes(B, I, H), (B, I, H)
        assert size(B, I, H) % 16 == 0
    assert [size(-1, 5, 16), size(3, 0, 16), size(3, -2, 16), size(3, 5, 0), size(3, 5, -16)] == [-2] * 5
    assert [size(3, 5, H) for H in (8, 48, 320, 2048)] == [-1] * 4
    assert size(1 << 20, 1 << 20, 16) == -1                           # 32-bit slots


def _decode(lib, B=2, I=8, H=16, act=1, ptr=64, ws=64, ws_bytes=None, **null):
    a = lambda k: None if null.get(k) else ptr
    n = O.workspace_bytes(max(B, 0), max(I, 1), H) if ws_bytes is None and H in (16, 32, 64, 128, 256, 512, 1024) else (ws_bytes or 0)
    return lib.yr_cdae_owned_decode(a("lcols"), a("lvals"), a("lcount"), a("z"), a("Wo"), ptr, B, I, H, act, a("dz"),
                                    a("dWo"), a("dbo"), a("partials"), a("count"), None if null.get("ws") else ws, n, None)


def _hidden(lib, B=2, I=8, H=16, act=1, users=4, n_partials=0, ptr=64, ws=64, ws_bytes=None, **null):
    a = lambda k: None if null.get(k) else ptr
    n = O.workspace_bytes(max(B, 0), max(I, 1), H) if ws_bytes is None and H in (16, 32, 64, 128, 256, 512, 1024) else (ws_bytes or 0)
    return lib.yr_cdae_owned_hidden_bwd(a("cols"), a("vals"), a("count"), a("dz"), a("z"), act, 1, a("pos_count"),
                                        a("user"), B, I, H, users, a("dV"), ptr, a("dbh"), a("dWhT"), a("items"),
                                        a("partials"), n_partials, a("stats"), None, None if null.get("ws") else ws, n, None)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call below returns before a launch: the pointers are the address 64, never dereferenced on the host."""
    lib = _lib()
    for call in (_decode, _hidden):
        assert call(lib, B=-1) == -2 and call(lib, I=0) == -2 and call(lib, I=-3) == -2 and call(lib, H=0) == -2
        assert call(lib, act=2) == -2
        assert [call(lib, H=H) for H in (8, 48, 320, 2048)] == [-1] * 4
        assert [call(lib, B=0, H=H) for H in (16, 32, 64, 128, 256, 512, 1024)] == [0] * 7       # an empty batch
        assert call(lib, B=0, H=48) == -1                                 # the width is judged first
        assert call(lib, ws=True) == -2                                   # no workspace
        assert call(lib, ws=72) == -2                                     # workspace off a 16-byte boundary
        assert call(lib, ws_bytes=O.workspace_bytes(2, 8, 16) - 16) == -2 and call(lib, ws_bytes=-1) == -2
    for k in ("lcols", "lvals", "lcount", "z", "Wo", "dz", "dWo", "dbo", "partials", "count"):
        assert _decode(lib, **{k: True}) == -2, k
    assert _decode(lib, ptr=68) == -2                                     # z / W_o rows off a 16-byte boundary
    for k in ("cols", "vals", "count", "dz", "z", "pos_count", "user", "dV", "dbh", "dWhT", "items"):
        assert _hidden(lib, **{k: True}) == -2, k
    assert _hidden(lib, users=0) == -2 and _hidden(lib, n_partials=-1) == -2
    assert _hidden(lib, n_partials=3, partials=True) == -2 and _hidden(lib, n_partials=3, stats=True) == -2


def test_wrappers_refuse_cpu_tensors_and_shapes():
    import torch
    from yelprecommendation_amd import engine
    f = lambda *s: torch.zeros(*s)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    B, I, H = 2, 8, 16
    n = B * 32 * O.cpp_of(I)
    lists = (i32(n), f(n), i32(B * 32))
    ws = torch.zeros(O.workspace_bytes(B, I, H), dtype=torch.uint8)
    with pytest.raises(engine.EngineError):                               # CPU tensors
        engine.cdae_owned_decode(lists, f(B, H), f(I, H), f(I), 1, f(B, H), f(I, H), f(I), f(B * 8), i32(engine.COUNT_WORDS), ws)
    with pytest.raises(engine.EngineError):                               # dz of another shape
        engine.cdae_owned_decode(lists, f(B, H), f(I, H), f(I), 1, f(B, H + 1), f(I, H), f(I), f(B * 8), i32(engine.COUNT_WORDS), ws)
    with pytest.raises(engine.EngineError):                               # no gradient buffers: the default kernel's job
        engine.cdae_owned_decode(lists, f(B, H), f(I, H), f(I), 1, None, None, None, f(B * 8), i32(engine.COUNT_WORDS), ws)
    with pytest.raises(engine.EngineError):
        engine.cdae_owned_workspace_bytes(4, 8, 320)
    rows = engine.SparseRows.from_buffers(*lists, B, I)
    with pytest.raises(engine.EngineError):
        engine.cdae_owned_hidden_bwd(rows, f(B, H), f(B, H), 1, torch.zeros(B, dtype=torch.int64), i32(engine.COUNT_WORDS),
                                     f(5, H), None, f(H), f(I, H), torch.zeros(I, dtype=torch.uint8), None, 0, None, None, ws)


# ---- CDAEStep -------------------------------------------------------------------------------------------------------

def _step(H, ns=True, **kw):
    from yelprecommendation_amd import cdae_step, optim
    from yelprecommendation_amd.models.cdae import CDAE
    from yelprecommendation_amd.utils import make_config
    model = CDAE(make_config("CDAE", hidden_size=H, device="cpu", lr=1e-3), 40, 6)
    return cdae_step.CDAEStep(model, optim.Adam(model.parameters(), lr=1e-3), ns, transposed_wh=True, **kw)


def test_step_accepts_the_mode_where_it_exists():
    for H in (16, 32, 64, 128, 256, 512, 1024):
        s = _step(H, deterministic=True)
        assert s.deterministic and s.decoder == "sampled" and s.row_marks and s.transposed_wh and not s.catalogue
    for H in (16, 32, 64, 128):
        s = _step(H, ns=False, deterministic=True)
        assert s.deterministic and s.catalogue and s.decoder == "dense"
    for kw in (dict(H=320), dict(H=64, row_marks=False), dict(H=256, ns=False), dict(H=8), dict(H=64, decoder="dense")):
        with pytest.raises(NotImplementedError, match="list batches"):
            _step(deterministic=True, **kw)
    from yelprecommendation_amd import cdae_step, optim
    from yelprecommendation_amd.models.cdae import CDAE
    from yelprecommendation_amd.utils import make_config
    model = CDAE(make_config("CDAE", hidden_size=64, device="cpu", lr=1e-3), 40, 6)
    with pytest.raises(NotImplementedError, match="list batches"):       # no transposed working copy
        cdae_step.CDAEStep(model, optim.Adam(model.parameters(), lr=1e-3), deterministic=True)
    import torch
    with pytest.raises(NotImplementedError, match="list batches"):       # dense batches
        _step(64, deterministic=True).step(torch.zeros(2, dtype=torch.int64), torch.zeros(2, 40))


def test_default_keyword_changes_nothing():
    for H, ns, want in ((128, True, ("sampled", True, True, False)), (512, True, ("sampled", True, True, False)),
                        (320, True, ("dense", False, False, False)), (64, False, ("dense", True, True, True))):
        s = _step(H, ns=ns)
        assert (s.decoder, s.row_marks, s.transposed_wh, s.catalogue) == want and s.deterministic is False
    import inspect
    from yelprecommendation_amd.cdae_step import CDAEStep
    assert list(inspect.signature(CDAEStep.__init__).parameters)[-1] == "deterministic"      # every positional call keeps its meaning


def test_trainer_and_train_refuse_what_the_mode_lacks():
    from yelprecommendation_amd.trainers.cdae_trainer import CDAETrainer
    from yelprecommendation_amd.utils import make_config
    for kw in (dict(optimizer="sgd"), dict(fused_step=False), dict(hidden_size=18)):
        cfg = make_config("CDAE", **{**dict(hidden_size=64, device="cpu", lr=1e-3, loss_name="bce", deterministic=True), **kw})
        with pytest.raises(NotImplementedError, match="list batches"):
            CDAETrainer(cfg, 40, 6).train([])
    cfg = make_config("CDAE", hidden_size=64, device="cpu", lr=1e-3, loss_name="bce", deterministic=True)
    with pytest.raises(NotImplementedError, match="list batches"):       # a loader of dense batches
        CDAETrainer(cfg, 40, 6).train([])


# ---- the cases ------------------------------------------------------------------------------------------------------

CASES = O.kernel_cases()


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_every_case_reaches_its_loop_end(c):
    """col_rows / row_len: at least what the case names; splits, lanes, epl: exactly.  Across the list: every
    column-owner geometry (16 / 32 / 64 lanes, 1 ... 16 floats per lane), 1 / 2 / 7 / 8 splits, a column with more
    rows than a workgroup has threads and one with more than 1,024, rows on both sides of a staging pass, both output
    activations with and without bias."""
    g = O.gen(c)
    got = O.reached(c, g)
    for k, v in c["reach"].items():
        assert (got[k] >= v) if k in ("col_rows", "row_len") else (got[k] == v), (c["id"], k, got[k], v)
    if c["heavy"]:
        hc = g["heavy"]
        I = c["I"]
        assert len(hc) == min(O.N_HEAVY, I) and hc[0] == 0 and hc[-1] == I - 1
        assert I <= O.N_HEAVY or {O.cpp_of(I) - 1, O.cpp_of(I)} <= set(hc.tolist())
        assert (((g["target"] + g["negmask"])[:, hc] != 0).all()) and (g["x"][:, hc] != 0).all()
    if c["long"]:
        assert sorted((g["x"] != 0).sum(1)) == sorted(c["I"] if k < 0 else k for k in R.ENC_COUNTS)
    if c["users"] == "duplicates":
        u = g["user"]
        assert u[0] == u[2] == u[-1] and u[1] == -1 and u[3] == O.NUM_USERS


def test_the_case_list_covers_every_geometry():
    got = {(c["reach"].get("lanes"), c["reach"].get("epl")) for c in CASES}
    assert {(16, 1), (32, 1), (64, 1), (64, 2), (64, 4), (64, 8), (64, 16)} <= got
    assert {1, 2, 7, 8} <= {c["reach"]["splits"] for c in CASES}
    assert max(c["reach"].get("col_rows", 0) for c in CASES) > 1024
    assert {(c["oact"], c["with_bo"]) for c in CASES} == {(0, True), (0, False), (1, True), (1, False)}


def _crossing(ref, other, names, bar_of):
    return max(float(R.over(other[k].v - ref[k].v, bar_of.get(k, R.bar)(ref[k])).max()) for k in names)


def test_bars_notice_one_lost_or_doubled_entry():
    """Each perturbation of ONE entry must move some output past a bar computed from the unperturbed reference alone."""
    bars = {"partials": R.loss_bar}
    # (row, heavy column) of the batch whose column owners walk 300 entries
    c = O.case("column_past_a_workgroup")
    g = O.gen(c)
    dec, hid = O.reference(c, g)
    col, row = int(g["heavy"][7]), 123
    for factor in (0.0, 2.0):
        w = np.ones_like(g["target"], np.float64); w[row, col] = factor
        dec2, _ = O.reference(c, g, weight=w)
        assert _crossing(dec, dec2, ("dWo", "dbo"), bars) >= 1.0, ("decoder entry", factor)
        assert abs(dec2["count"] - dec["count"]) == 1
        x2 = g["x"].copy(); x2[row, col] *= factor
        _, hid2 = O.reference(c, g, x=x2)
        assert float(R.over(hid2["dWh"].v - hid["dWh"].v, R.bar(hid["dWh"])).max()) >= 1.0, ("encoder entry", factor)
    # entry 2,048 of a long row and one split's share, through cdae_ref64.list_weights
    c = O.case("long_rows_H16")
    g = O.gen(c)
    S = O.splits_of(c["B"])
    dec, hid = O.reference(c, g)
    seen = set()
    for r in range(c["B"]):
        for what, wrow in R.list_weights((g["target"][r] + g["negmask"][r]) != 0, S).items():
            if what == "tail dropped":
                continue
            w = np.ones_like(g["target"], np.float64); w[r] = wrow
            dec2, _ = O.reference(c, g, weight=w)
            assert _crossing(dec, dec2, ("dz", "dWo", "dbo", "partials"), bars) >= 1.0, ("loss list", r, what)
            seen.add(what)
        for what, wrow in R.list_weights(g["x"][r] != 0, 1).items():
            if what not in ("entry 2048 dropped", "entry 2048 twice"):
                continue
            _, hid2 = O.reference(c, g, x=g["x"] * np.where(np.arange(c["B"])[:, None] == r, wrow[None, :], 1.0))
            assert float(R.over(hid2["dWh"].v - hid["dWh"].v, R.bar(hid["dWh"])).max()) >= 1.0, ("encoder list", r, what)
    assert seen == {"entry 2048 dropped", "entry 2048 twice", "split share dropped"}


def test_the_order_sensitive_inputs_depend_on_the_order_of_an_f32_sum():
    """dW_o[c, :] = sum_r g(r, c) z[r, :] in f32, rows ascending against a seeded shuffle: more than half of the
    elements of the heavy columns differ — so bit-equal results of two GPU calls are not a matter of course."""
    c = O.case("order_sensitive")
    g = O.gen(c)
    z, Wo = g["z"].astype(np.float64), g["Wo"].astype(np.float64)
    hc = g["heavy"]
    y = 1.0 / (1.0 + np.exp(-(z @ Wo[hc].T + g["bo"][hc])))
    gf = (y - g["target"][:, hc]).astype(np.float32)                   # sigmoid output: g = y - t
    assert np.isfinite(gf).all() and np.isfinite(g["z"]).all()

    def summed(order):
        acc = np.zeros((len(hc), c["H"]), np.float32)
        for r in order:
            acc = (acc + gf[r][:, None] * g["z"][r][None, :]).astype(np.float32)
        return acc

    a = summed(range(c["B"]))
    b = summed(np.random.RandomState(5).permutation(c["B"]))
    differ = float((a != b).mean())
    print(f"order-sensitive dW_o of the heavy columns: {100 * differ:.1f} % of the elements differ between the two orders")
    assert differ > 0.5
