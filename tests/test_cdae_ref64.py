"""tests/cdae_ref64.py, the float64 reference of the CDAE list kernels, checked without a GPU: it equals the oracle
that is pinned to the reference's golden vectors, and the bars it states for the cases of
tests/test_gpu_cdae_long_rows.py are tight enough to notice what a faulty staging pass would compute."""
import numpy as np
import pytest

import cdae_ref64 as R
from oracle import cdae as ocdae


@pytest.mark.parametrize("hidden_act,output_act", [(1, 1), (0, 0), (1, 0), (0, 1)])
def test_reference_equals_the_pinned_oracle(hidden_act, output_act):
    """B = 12, I = 301, H = 32: loss and all five gradients of oracle.cdae.loss_and_grads (f32 NumPy, pinned to the
    golden vectors by test_oracle_golden.py) against the chain encode -> sampled_decode -> hidden_bwd, within the
    bars the reference states for an f32 computation."""
    rs = np.random.RandomState(5 + 2 * hidden_act + output_act)
    B, I, H, nu = 12, 301, 32, 20
    name = {1: "sigmoid", 0: "identity"}
    x_in = R.input_rows(rs, I, rs.randint(0, 40, B))
    target, negmask = R.loss_rows(rs, I, rs.randint(1, 60, B))
    user = rs.randint(0, nu, B).astype(np.int64); user[5] = user[1]
    Wh, bh, V = R.encoder_params(rs, H, I, nu, x_in)
    if hidden_act == 0:                               # identity hidden layer: keep z positive for the identity output
        bh, V = np.abs(bh) + np.float32(0.3), np.abs(V)
    _, Wo, bo = R.decoder_params(rs, B, H, I, output_act, True)
    if hidden_act == 0 and output_act == 0:
        Wo = (Wo / np.float32(4.5)).astype(np.float32)               # z up to 3.6: pre-activations stay below 0.95
    z = R.encode(Wh, bh, V, user, x_in, hidden_act)
    assert output_act == 1 or (0.0 < (z.v @ Wo.T.astype(np.float64) + bo).min() and (z.v @ Wo.T.astype(np.float64) + bo).max() < 0.95)
    dec = R.sampled_decode(z.v, Wo, bo, target, negmask, output_act)
    cnt = dec["count"]
    hid = R.hidden_bwd(dec["dz"].v, z.v, hidden_act, user, cnt, x_in, nu)
    loss, (dWh, dbh, dV, dWo, dbo) = ocdae.loss_and_grads([Wh, bh, V, Wo, bo], user, x_in, target, negmask,
                                                          name[hidden_act], name[output_act])
    assert cnt == int(((target + negmask) != 0).sum())
    np.testing.assert_allclose(float(loss), dec["loss"].v / cnt, rtol=1e-5)
    scaled = lambda o: R.Out(o.v / cnt, o.n, o.s / cnt)
    worst = {"dWo": R.ratio(dWo, scaled(dec["dWo"])), "dbo": R.ratio(dbo, scaled(dec["dbo"])),
             "dbh": R.ratio(dbh, hid["dbh"]), "dV": R.ratio(dV, hid["dV"]), "dWh": R.ratio(dWh, hid["dWh"])}
    print("oracle vs cdae_ref64, max |err| / bar:", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) < 1.0, worst


# ---- the bars can notice a faulty staging pass ----------------------------------------------------------------------

def _thinned(rs, x, p):
    """A stand-in for dropout_p(x) with the same law (the GPU test takes the kernel's own Philox mask)."""
    return (x * (rs.rand(*x.shape) >= p) / (1.0 - p)).astype(np.float32)


def _encoder_ratios(case):
    I, H, act, transposed, p = case
    c = R.encoder_case(*case)
    x = _thinned(c["rs"], c["x"], p) if p > 0 else c["x"]
    Wh, bh, V = R.encoder_params(c["rs"], H, I, R.ENCODER_USERS, x)
    ref = R.encode(Wh, bh, V, c["user"], x, act)
    b = R.bar(ref)
    assert np.abs(x.astype(np.float64) @ Wh.T.astype(np.float64)).max() + 0.6 <= 3.0 + 1e-6
    out = {}
    for r in range(len(x)):
        for what, w in R.list_weights(x[r] != 0).items():
            if what == "split share dropped":         # the encoder has no splits
                continue
            got = R.encode(Wh, bh, V, c["user"][r:r + 1], (x[r] * w)[None, :], act)
            out[(r, what)] = float(R.over(got.v[0] - ref.v[r], b[r]).max())
    return out


def _decode_ratios(B, I, H, act, with_bo, long, settle, grads):
    c = R.decode_case(B, I, H, act, with_bo, long, settle)
    splits = R.DECODE_SPLITS.get(B) or max(1, min(8, 512 // B))
    ref = R.sampled_decode(c["z"], c["Wo"], c["bo"], c["target"], c["negmask"], act, splits=splits)
    pre = c["z"].astype(np.float64) @ c["Wo"].T.astype(np.float64) + (0 if c["bo"] is None else c["bo"])
    assert np.abs(pre).max() <= 3.0 if act == 1 else (pre.min() >= 0.05 and pre.max() <= 0.95)
    bars = {k: R.bar(ref[k]) for k in ("dz", "dWo", "dbo")}
    bars["partials"] = R.loss_bar(ref["partials"])
    rows = range(R.N_LONG) if long else (0,)
    out = {}
    for r in rows:
        sel = (c["target"][r] + c["negmask"][r]) != 0
        for what, w in R.list_weights(sel, splits).items():
            d = R.sampled_decode(c["z"][r:r + 1], c["Wo"], c["bo"], c["target"][r:r + 1], c["negmask"][r:r + 1], act,
                                 weight=(w - 1.0)[None, :], splits=splits)           # linear in the weights
            rr = [float(R.over(d["partials"].v[0], bars["partials"][r]).max())]
            if grads:
                rr += [float(R.over(d["dz"].v[0], bars["dz"][r]).max()),
                       float(R.over(d["dWo"].v, bars["dWo"]).max()), float(R.over(d["dbo"].v, bars["dbo"]).max())]
            out[(r, what)] = (max(rr), d["count"] != 0)
    return out


def test_every_bar_notices_a_faulty_staging_pass():
    """For every GPU case: the bar computed from the reference alone is crossed, on at least one float output, by
    each perturbed reference — entry 2048 of a long row dropped / counted twice, one split's share of a row
    dropped, a row's tail beyond its last full pass dropped.  The loss-only decoder has the loss partials and the
    count as its only outputs; there the (exact) count notices what the f32 bound of a 6,001-term partial cannot."""
    smallest = {}

    def note(family, case, ratios, need_float=True):
        kinds = {what for _, what in ratios}
        for (r, what), v in ratios.items():
            val, counted = v if isinstance(v, tuple) else (v, False)
            assert val >= 1.0 or (not need_float and counted), (family, case, r, what, val)
            if val >= 1.0:
                smallest[family] = min(smallest.get(family, np.inf), val)
        return kinds

    for case in R.ENCODER_CASES:
        kinds = note("encoder", case, _encoder_ratios(case))
        assert kinds == {"entry 2048 dropped", "entry 2048 twice", "tail dropped"}
    for case in R.DECODE_CASES:
        kinds = note("decoder", case, _decode_ratios(*case, settle=False, grads=True))
        assert "split share dropped" in kinds and (not case[5] or len(kinds) == 4)
    for B, I, H, act in R.LOSS_ONLY_CASES:
        kinds = note("loss only", (B, I, H, act), _decode_ratios(B, I, H, act, True, True, True, False), need_float=False)
        assert len(kinds) == 4
    for kernel, H, act, scale in R.DWH_CASES:
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
            assert len(note("dW_h", (kernel, H, batch), ratios)) == 3
    for B in R.HIDDEN_B:                               # cdae_hidden_bwd has no lists: its last row dropped
        for H in R.HIDDEN_H:
            c = R.hidden_case(B, H)
            ref = R.hidden_bwd(c["dz"], c["z"], c["act"], c["user"], 37 if c["scale_dz"] else None, None, R.HIDDEN_USERS)
            v = float((np.abs(ref["dz"].v[B - 1]) / R.bar(ref["dbh"])).max())
            note("hidden_bwd", (B, H), {(B - 1, "last row dropped"): v})
    print("smallest perturbation / bar per family:", {k: round(v, 2) for k, v in smallest.items()})
    print("smallest perturbation / bar over all cases: %.2f" % min(smallest.values()))
