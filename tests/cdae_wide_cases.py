"""Cases and float64 helpers for the CDAE list kernels at the wide hidden sizes 512 and 1,024 (tests/test_gpu_cdae_wide.py
runs them on the GPU, tests/test_cdae_wide_host.py shows without one that their bars notice what a faulty kernel would
compute).  Importable helper, no fixtures; the reference, the bars and the input generators are those of cdae_ref64.py.

What only a wide kernel can get wrong: a row of 512 / 1,024 floats is spread over a whole wave, lane l holding floats
l + 64 k (gradient form) or [4 l + 256 k, 4 l + 256 k + 4) (loss-only form) — a register slot or a lane left out of
the dot product z . W_o[i] while that unit's own outputs (dz[:, h], dW_o[:, h]) stay right.  With
cdae_ref64.decoder_params one of 1,024 units carries ~0.1 % of a pre-activation, which the bars cannot see; the
probe inputs below give a few chosen units ~3 % each.

The 32-lane instances of cdae_sampled_decode_kernel (H <= 256) take their slot code from the same kernel text — lane l
holds floats l + 32 k (gradient form) or [NK l, NK l + NK) (loss-only form), NK = 4 up to H = 128 and 8 above — so the
NARROW_* cases put the same net under them, at widths with a masked tail (100, 132) and at both exact ones.
"""
import numpy as np

import cdae_ref64 as R

WIDE = (512, 1024)

# sampled decoder with gradients: (B, I, H, act, with_bo, long rows) — splits 8 / 7 / 2 / 1 / 8 / 8 / 3 / 1
DECODE_CASES = [(1, 301, 1024, 1, True, False), (73, 301, 512, 0, False, False), (256, 301, 1024, 0, True, False),
                (600, 301, 512, 1, True, False), (9, 6001, 512, 1, True, True), (9, 6001, 1024, 0, True, True),
                (170, 6001, 1024, 1, False, True), (300, 6000, 512, 0, True, True)]
# loss only: (B, I, H, act); rows: the long set, the settle() set, short rows
LOSS_ONLY_CASES = [(15, 6001, 512, 1), (15, 6001, 1024, 0), (15, 6001, 1024, 1)]
# encoder: (I, H, act, transposed, p)
ENCODER_CASES = [(6001, 512, 1, True, 0.0), (6001, 1024, 0, True, 0.0), (6001, 1024, 1, False, 0.0)]
# cdae_hidden_bwd_dwh_t on R.dwh_case(H): (H, act, scale_dz)
DWH_CASES = [(512, 1, True), (1024, 0, False), (1024, 1, True)]
# the probe-unit inputs: decoder with gradients (B, I, H, act, with_bo, long) and loss only (B, I, H, act)
PROBE_DECODE_CASES = [(73, 301, 512, 1, True, False), (40, 301, 1024, 0, True, False), (9, 6001, 1024, 1, True, True),
                      (9, 6001, 512, 0, False, True)]
PROBE_LOSS_ONLY_CASES = [(15, 6001, 512, 0), (15, 6001, 1024, 1)]
# the same for the 32-lane instances: NK = 4 (H = 100, 128) and 8 (132, 256); loss only needs H % 4 == 0
NARROW_PROBE_DECODE_CASES = [(73, 301, 100, 1, True, False), (73, 301, 128, 0, False, False),
                             (73, 301, 132, 1, True, False), (73, 301, 256, 0, True, False),
                             (9, 6001, 128, 1, True, True), (9, 6001, 256, 0, False, True)]
NARROW_PROBE_LOSS_ONLY_CASES = [(15, 6001, 100, 1), (15, 6001, 128, 0), (15, 6001, 256, 1)]


def splits_of(B):
    """yr_cdae_sampled_decode_splits."""
    return max(1, min(8, 512 // B))


def narrow_probe_units(H):
    """probe_units for H <= 256: lanes 0 and 31 of the gradient layout, one unit in every slot h // 32 of it (the last
    slot may be partial), one at every place h % NK of the loss-only layout (on lanes spread over the half-wave), and
    the last valid unit H - 1."""
    NK = 4 if H <= 128 else 8
    slots = -(-H // 32)
    units = {0, 31, H - 1}
    for k in range(slots):
        units.add(32 * k + (5 * k + 1) % min(32, H - 32 * k))
    for j in range(NK):
        units.add(NK * ((3 * j + 2) % (H // NK)) + j)
    units = np.array(sorted(units), np.int64)
    assert units.max() == H - 1 and set(units // 32) == set(range(slots))
    assert set(units % NK) == set(range(NK)) and {0, 31} <= set(units % 32)
    return units


def probe_units(H):
    """Hidden units whose loss from the dot product must be noticed: lanes 0 and 63 of the first and the last register
    slot, both sides of the middle of the row, and one unit in every slot of both lane layouts — slot k = h // 64 of
    the gradient form, (h // 256, h % 4) of the loss-only form.  H <= 256: narrow_probe_units."""
    if H not in WIDE:
        return narrow_probe_units(H)
    units = {0, 63, 64, H // 2 - 1, H // 2, H - 64, H - 1}
    for k in range(H // 64):
        units.add(64 * k + (5 * k + 1) % 64)          # (5 k + 1) % 4 runs over 0 .. 3 inside every group of 256
    units = np.array(sorted(units), np.int64)
    assert set(units // 64) == set(range(H // 64))
    assert {(int(h) // 256, int(h) % 4) for h in units} == {(a, b) for a in range(H // 256) for b in range(4)}
    assert {0, 63} <= set(units % 64)
    return units


def probe_decoder_params(rs, B, H, I, act, with_bo):
    """(z, Wo, bo) as cdae_ref64.decoder_params at half the weight, plus the probe units: z[:, h] in [0.7, 0.9] and
    W_o[:, h] positive, every probe unit adding 2 ... 5 % of the range to every pre-activation.  Sigmoid output:
    pre-activations within [-1.6, 3.0]; identity output: within [0.2, 0.95]."""
    z, Wo, bo = R.decoder_params(rs, B, H, I, act, True)
    P = probe_units(H)
    Wo = (Wo * np.float32(0.5)).astype(np.float32)
    z[:, P] = (0.7 + 0.2 * rs.rand(B, len(P))).astype(np.float32)
    total = 1.4 if act == 1 else 0.42                 # what the probe units add at most, all together
    Wo[:, P] = ((0.5 + 0.5 * rs.rand(I, len(P))) * total / (0.9 * len(P))).astype(np.float32)
    return z, Wo, (bo if with_bo else None)


def probe_decode_case(B, I, H, act, with_bo, long, settle=False):
    c = R.decode_case(B, I, H, act, with_bo, long, settle)
    rs = np.random.RandomState(7000 + B + I + 3 * H + act)
    c["z"], c["Wo"], c["bo"] = probe_decoder_params(rs, B, H, I, act, with_bo)
    return c


def unit_dropped(c, act, splits, ref, partials_only=False):
    """For every probe unit h: max over a row's float outputs of |what the kernel would return with unit h left out of
    z . W_o[i] − reference| / bar, on the loss partials of the row and on dz[row, probe units] (the unit's own outputs
    computed from the full rows; ``partials_only``: the loss partials alone, what the loss-only kernel returns).
    Returns (ratios [units, B], rows with a loss position)."""
    z, Wo = c["z"].astype(np.float64), c["Wo"].astype(np.float64)
    t, m = c["target"].astype(np.float64), c["negmask"].astype(np.float64)
    b = np.zeros(Wo.shape[0]) if c["bo"] is None else c["bo"].astype(np.float64)
    sel = (t + m) != 0
    share = np.where(sel, ((np.cumsum(sel, axis=1) - 1) % R.LIST_CAP) % splits, -1)
    of = [share == q for q in range(splits)]
    pre = z @ Wo.T + b
    P = probe_units(z.shape[1])

    def terms(pre):
        y = 1.0 / (1.0 + np.exp(-pre)) if act == 1 else pre
        term = -(t * np.maximum(np.log(y), -100.0) + (1.0 - t) * np.maximum(np.log(1.0 - y), -100.0))
        g = (y - t) / np.maximum((1.0 - y) * y, 1e-12) * (y * (1.0 - y) if act == 1 else 1.0)
        return np.where(sel, term, 0.0), np.where(sel, g, 0.0)

    term0, g0 = terms(pre)
    bar_p, bar_dz = R.loss_bar(ref["partials"]), R.bar(ref["dz"])[:, P]
    out = np.zeros((len(P), len(z)))
    for k, h in enumerate(P):
        term1, g1 = terms(pre - np.outer(z[:, h], Wo[:, h]))
        d_part = np.stack([((term1 - term0) * o).sum(1) for o in of], 1)
        out[k] = R.over(d_part, bar_p).max(1)
        if not partials_only:
            out[k] = np.maximum(out[k], R.over((g1 - g0) @ Wo[:, P], bar_dz).max(1))
    return out, sel.any(1)


# ---- float64 replay of training steps: what two f32 routes of the same steps may differ by -------------------------

def adam64(grads, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """p_final - p_init of Adam (no weight decay) over the gradient sequence ``grads`` (arrays of one shape), float64."""
    m, v, dp = np.zeros_like(grads[0]), np.zeros_like(grads[0]), np.zeros_like(grads[0])
    for t, g in enumerate(grads, 1):
        m = beta1 * m + (1.0 - beta1) * g
        v = beta2 * v + (1.0 - beta2) * g * g
        dp -= lr / (1.0 - beta1 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps)
    return dp


def f32_bound(o, div=1.0):
    """The f32 part of cdae_ref64.bar alone: 2 (n + 1) 2^-24 sum |terms|."""
    return 2.0 * (o.n + 1.0) * R.U24 * o.s / div


def replay_steps(params, batches, hact, oact, num_users, lr):
    """Float64 replay of sampled-decoder training steps from ``params`` = [Wh, bh, V, Wo, bo] over ``batches`` =
    [(user, x_in, target, negmask)].  Returns (final parameters, allowance): per parameter element, how far ONE f32
    evaluation of the same steps may end from the replay — for every step the gradient moved by +- its f32 bound
    (2 (n + 1) 2^-24 sum |terms| of cdae_ref64; the bound of dz carried on into db_h, dV and dW_h), the Adam sequence
    run again with that one step's gradient moved (Adam is element-wise: all elements at once, no linearisation, so a
    gradient that its bound can take through zero gets the whole step), the larger of the two deviations taken and the
    steps' deviations added up; plus 2^-24 |p| per step for the f32 parameter the step is stored into."""
    P = [np.asarray(a, np.float64).copy() for a in params]
    G, D = [[] for _ in P], [[] for _ in P]
    for user, x_in, target, negmask in batches:
        Wh, bh, V, Wo, bo = P
        z = R.encode(Wh, bh, V, user, x_in, hact)
        dec = R.sampled_decode(z.v, Wo, bo, target, negmask, oact)
        cnt = dec["count"]
        hid = R.hidden_bwd(dec["dz"].v, z.v, hact, user, cnt, x_in, num_users)
        ddz = f32_bound(dec["dz"], cnt) * (z.v * (1.0 - z.v) if hact == 1 else 1.0)      # dz's bound after act'
        ok = (np.asarray(user) >= 0) & (np.asarray(user) < num_users)
        dV_in = np.zeros_like(P[2])
        np.add.at(dV_in, np.asarray(user)[ok], ddz[ok])
        g = [hid["dWh"].v, hid["dbh"].v, hid["dV"].v, dec["dWo"].v / cnt, dec["dbo"].v / cnt]
        d = [f32_bound(hid["dWh"]) + ddz.T @ np.abs(np.asarray(x_in, np.float64)), f32_bound(hid["dbh"]) + ddz.sum(0),
             f32_bound(hid["dV"]) + dV_in, f32_bound(dec["dWo"], cnt), f32_bound(dec["dbo"], cnt)]
        for k in range(5):
            G[k].append(g[k]); D[k].append(d[k])
        t = len(G[0])
        for k in range(5):                             # the exact step (Adam from the whole history: same numbers)
            P[k] = np.asarray(params[k], np.float64) + adam64(G[k], lr)
    allow = []
    for k in range(5):
        base = adam64(G[k], lr)
        a = np.zeros_like(base)
        for j in range(len(G[k])):
            dev = np.zeros_like(base)
            for sign in (1.0, -1.0):
                moved = list(G[k]); moved[j] = G[k][j] + sign * D[k][j]
                dev = np.maximum(dev, np.abs(adam64(moved, lr) - base))
            a += dev
        # the parameter itself is stored in f32: half an ulp per step
        allow.append(a + len(G[k]) * R.U24 * np.maximum(np.abs(np.asarray(params[k], np.float64)), np.abs(P[k])))
    return P, allow
