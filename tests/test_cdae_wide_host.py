"""CDAE at the hidden sizes 512 and 1,024 without a GPU: which widths the entry points accept, which configurations
train.py feeds with list batches, and that the bars of tests/test_gpu_cdae_wide.py (computed from the float64
reference alone) notice what a faulty wide kernel would compute."""
import ctypes

import numpy as np
import pytest

import cdae_ref64 as R
import cdae_wide_cases as W
from test_cdae_ref64 import _decode_ratios, _encoder_ratios


def test_entry_points_accept_the_wide_widths_and_no_others():
    """Nothing is launched: every call ends at an argument check (NULL pointers, or an unknown optimizer mode, which
    yr_adam_dense_flat looks at after the tensors' own checks)."""
    from yelprecommendation_amd import _lib
    lib = _lib.load()
    decode = lambda H: lib.yr_cdae_sampled_decode(None, None, None, None, None, None, 8, 8, H, 1, None, None, None,
                                                  None, None, None)
    assert [decode(H) for H in (512, 1024)] == [-2, -2]                 # width accepted, pointers missing
    assert [decode(H) for H in (260, 300, 768, 2048)] == [-1, -1, -1, -1]
    a = 4096                                                            # a fake, 16-byte aligned address

    def flat(rw, n, mode):
        one = (ctypes.c_void_p * 1)(a)
        return lib.yr_adam_dense_flat(one, one, one, one, (ctypes.c_int64 * 1)(n), (ctypes.c_void_p * 1)(a),
                                      (ctypes.c_int * 1)(rw), (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(0), None, 1,
                                      1e-3, 1e-3, 1.0, 0.9, 0.999, 1e-8, 0.0, mode, None)
    unknown = 7
    assert [flat(rw, 3 * rw, unknown) for rw in (768, 2048, 48, 320)] == [-2, -2, -2, -2]     # the width is refused
    assert [flat(rw, 3 * rw, unknown) for rw in (512, 1024, 64, 256)] == [-1, -1, -1, -1]     # past the width check
    assert [flat(rw, 3 * rw + 4, unknown) for rw in (512, 1024)] == [-2, -2]                  # whole rows only
    hidden = lambda H, B: lib.yr_cdae_hidden_bwd_dwh_t(None, None, None, None, None, 1, 1, None, None, B, 8, H, 4,
                                                       None, None, None, None, None, None, 0, None, None, None)
    assert hidden(1024, 0) == 0 and hidden(1024, 2) == -2 and hidden(1028, 0) == -2           # empty batch / NULLs / width


def test_which_configurations_get_list_batches():
    from yelprecommendation_amd.train import cdae_takes_list_batches
    from yelprecommendation_amd.utils import make_config
    cfg = lambda **kw: make_config("CDAE", loss_name="bce", **kw)
    for H in (16, 32, 64, 128, 256, 512, 1024):
        assert cdae_takes_list_batches(cfg(hidden_size=H, top_n=10), 38048) is True
    assert cdae_takes_list_batches(cfg(hidden_size=320, top_n=10), 38048) is False
    assert cdae_takes_list_batches(cfg(hidden_size=512, top_n=20), 38048) is False             # k > 16 from H = 128 up
    assert cdae_takes_list_batches(cfg(hidden_size=64, top_n=20), 38048) is True
    assert cdae_takes_list_batches(cfg(hidden_size=512, top_n=10), 163841) is False
    assert cdae_takes_list_batches(cfg(hidden_size=512, top_n=10, optimizer="sgd"), 38048) is False
    assert cdae_takes_list_batches(cfg(hidden_size=512, top_n=10, negative_sampling=False), 38048) is False
    assert cdae_takes_list_batches(cfg(hidden_size=512, top_n=10, fused_step=False), 38048) is False
    assert cdae_takes_list_batches(cfg(hidden_size=512, top_n=10, list_batches=False), 38048) is False


def test_step_options_at_the_wide_widths():
    """CDAEStep's choices are made before anything touches the device; a stand-in model / optimizer is enough."""
    from yelprecommendation_amd import cdae_step, optim
    from yelprecommendation_amd.models.cdae import CDAE
    from yelprecommendation_amd.utils import make_config

    def options(H, decoder="auto"):
        model = CDAE(make_config("CDAE", hidden_size=H, device="cpu", lr=1e-3), 40, 6)
        try:
            s = cdae_step.CDAEStep(model, optim.Adam(model.parameters(), lr=1e-3), True, decoder=decoder, transposed_wh=True)
        except NotImplementedError:
            return None
        return s.decoder, s.row_marks, s.transposed_wh

    got = {H: options(H) for H in (128, 256, 512, 1024, 260, 300, 320, 768)}
    for H in (128, 256, 512, 1024):
        assert got[H] == ("sampled", True, True), (H, got[H])
    for H in (260, 300, 320, 768):                                     # exactly as before: the dense decoder, no marks
        assert got[H] == ("dense", False, False), (H, got[H])
        assert options(H, "sampled") is None
    assert options(512, "dense") == ("dense", True, True)


# ---- the bars notice a faulty wide kernel ---------------------------------------------------------------------------

def _note(smallest, family, case, ratios, need_float=True):
    kinds = set()
    for (r, what), v in ratios.items():
        val, counted = v if isinstance(v, tuple) else (v, False)
        assert val >= 1.0 or (not need_float and counted), (family, case, r, what, val)
        if val >= 1.0:
            smallest[family] = min(smallest.get(family, np.inf), val)
        kinds.add(what)
    return kinds


def test_every_bar_notices_a_faulty_staging_pass_at_the_wide_widths():
    """As test_cdae_ref64.test_every_bar_notices_a_faulty_staging_pass, for the cases of test_gpu_cdae_wide.py: entry
    2,048 of a long row dropped / counted twice, one split's share of a row dropped, the tail beyond the last full
    pass dropped — each crosses a bar computed from the reference alone (loss only: or changes the exact count)."""
    smallest = {}
    for case in W.ENCODER_CASES:
        kinds = _note(smallest, "encoder", case, _encoder_ratios(case))
        assert kinds == {"entry 2048 dropped", "entry 2048 twice", "tail dropped"}
    for case in W.DECODE_CASES:
        assert W.splits_of(case[0]) == (R.DECODE_SPLITS.get(case[0]) or W.splits_of(case[0]))
        kinds = _note(smallest, "decoder", case, _decode_ratios(*case, settle=False, grads=True))
        assert "split share dropped" in kinds and (not case[5] or len(kinds) == 4)
    for B, I, H, act in W.LOSS_ONLY_CASES:
        kinds = _note(smallest, "loss only", (B, I, H, act), _decode_ratios(B, I, H, act, True, True, True, False),
                      need_float=False)
        assert len(kinds) == 4
    for H, act, scale in W.DWH_CASES:
        for batch in (0, 1):
            c = R.dwh_case(H, batch)
            ref = R.hidden_bwd(c["dz"], c["z"], act, c["user"], 37 if scale else None, c["x"], R.HIDDEN_USERS)
            b = R.bar(ref["dWh"])
            ratios = {}
            for r in range(R.N_LONG):
                for what, w in R.list_weights(c["x"][r] != 0).items():
                    if what != "split share dropped":
                        delta = np.outer(ref["dz"].v[r], c["x"][r] * (w - 1.0))
                        ratios[(r, what)] = float(R.over(delta, b).max())
            assert len(_note(smallest, "dW_h", (H, batch), ratios)) == 3
    print("smallest perturbation / bar per family:", {k: round(v, 2) for k, v in smallest.items()})


@pytest.mark.parametrize("case", [c + (True,) for c in W.PROBE_DECODE_CASES] +
                         [(B, I, H, act, True, True, False) for B, I, H, act in W.PROBE_LOSS_ONLY_CASES] +
                         [c + (True,) for c in W.NARROW_PROBE_DECODE_CASES] +
                         [(B, I, H, act, True, True, False) for B, I, H, act in W.NARROW_PROBE_LOSS_ONLY_CASES])
def test_probe_units_make_a_unit_lost_from_the_dot_product_visible(case):
    """One hidden unit left out of z . W_o[i] (a register slot or a lane of the wave-per-position layout) while the
    unit's own outputs are right: on the probe inputs every probed unit crosses a bar — a loss partial of the row, or
    dz of the row at a probe unit — on every row that has a loss position; with cdae_ref64.decoder_params it does
    not (shown once, at the first case).  The same at H = 100, 128, 132 and 256 for the half-wave-per-position
    instances (tests/test_gpu_cdae_probe_units.py), which share the slot code: cdae_wide_cases.narrow_probe_units."""
    B, I, H, act, with_bo, long, grads = case
    splits = W.splits_of(B)
    c = W.probe_decode_case(B, I, H, act, with_bo, long, settle=not grads)
    pre = c["z"].astype(np.float64) @ c["Wo"].T.astype(np.float64) + (0 if c["bo"] is None else c["bo"])
    assert np.abs(pre).max() <= 3.0 if act == 1 else (pre.min() >= 0.05 and pre.max() <= 0.95)
    ref = R.sampled_decode(c["z"], c["Wo"], c["bo"], c["target"], c["negmask"], act, splits=splits)
    ratios, has = W.unit_dropped(c, act, splits, ref, partials_only=not grads)   # loss only: the partials alone
    assert has.any()
    worst = ratios[:, has].min()
    print(f"probe inputs B={B} I={I} H={H} act={act} grads={grads}: smallest |unit dropped| / bar {worst:.3g} "
          f"over {len(ratios)} units x {int(has.sum())} rows")
    assert worst >= 1.0, [(int(W.probe_units(H)[k]), int(r)) for k, r in zip(*np.nonzero((ratios < 1.0) & has[None, :]))][:10]
    assert float(ratios[:, ~has].max(initial=0.0)) == 0.0
    if case == W.PROBE_DECODE_CASES[0] + (True,):
        plain = R.decode_case(B, I, H, act, with_bo, long)
        pref = R.sampled_decode(plain["z"], plain["Wo"], plain["bo"], plain["target"], plain["negmask"], act, splits=splits)
        pr, phas = W.unit_dropped(plain, act, splits, pref)
        print(f"the same with cdae_ref64.decoder_params: smallest {pr[:, phas].min():.3g}")
        assert pr[:, phas].min() < 1.0


def test_float64_replay_and_its_allowance_against_the_f32_oracle():
    """cdae_wide_cases.replay_steps (what test_wide_list_batches_train_like_dense_batches explains an element beyond
    its tight bar with): three steps of oracle.cdae.CDAEState — f32 NumPy, pinned to the reference's golden vectors —
    end within 2 x allowance of the float64 replay on every parameter element, the allowance is zero where no gradient
    ever arrives and non-zero where one does, and a W_o gradient lost in step 2 is far outside it."""
    from oracle import cdae as ocdae
    rs = np.random.RandomState(21)
    nu, ni, H, B, lr = 30, 301, 32, 12, 1e-3
    Wh, bh, V = R.encoder_params(rs, H, ni, nu, R.input_rows(rs, ni, [40] * B))
    _, Wo, bo = R.decoder_params(rs, B, H, ni, 1, True)
    init = [Wh, bh, V, Wo, bo]
    batches = []
    for _ in range(3):
        user = rs.permutation(nu)[:B].astype(np.int64)
        x_in = R.input_rows(rs, ni, rs.randint(0, 40, B))
        target, negmask = R.loss_rows(rs, ni, rs.randint(1, 60, B))
        batches.append((user, x_in, target, negmask))
    exact, allow = W.replay_steps(init, batches, 1, 1, nu, lr)
    ref = ocdae.CDAEState(init, lr=lr)
    for b in batches:
        ref.train_step(*b)
    hit = np.zeros(ni, bool)
    for _, _, t, m in batches:
        hit |= ((t + m) != 0).any(0)
    store = 3 * R.U24 * np.maximum(np.abs(Wo), np.abs(exact[3]))                 # the f32 storage term alone
    assert float((allow[3] - store)[~hit].max(initial=0.0)) == 0.0 and float((allow[3] - store)[hit].min()) > 0.0
    worst = [float(R.over(ref.params[j] - exact[j], 2.0 * allow[j] + 1e-9).max()) for j in range(5)]
    print("f32 oracle against the float64 replay, max |diff| / (2 x allowance):", [round(v, 3) for v in worst])
    assert max(worst) < 1.0, worst
    lost = ocdae.CDAEState(init, lr=lr)
    for k, b in enumerate(batches):
        if k == 1:
            _, grads = ocdae.loss_and_grads(lost.params, *b, "sigmoid", "sigmoid")
            grads = list(grads); grads[3] = np.zeros_like(grads[3])
            lost.opt.step(grads)
        else:
            lost.train_step(*b)
    touched = ((batches[1][2] + batches[1][3]) != 0).any(0)
    assert float(R.over(lost.params[3] - exact[3], 2.0 * allow[3] + 1e-9)[touched].min()) > 1.0
