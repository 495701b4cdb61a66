"""Float64 restatement of the DCN kernels (csrc/dcn.hip) for the tests: the input assembly in its row forms with its
scatter backward, the ReLU backward, the fused head (forward, BPR loss, backward; the einsum form of tests/dcn_ref.py
through autograd for the values, the closed form for the magnitudes) and the catalogue scorer exactly as the header
comment of dcn_score_kernel states it.  Importable helper, no fixtures (like ngcf_ref64.py); plain numpy / torch on the
CPU, the engine is not imported.

Every floating output is an ``Out(v, s, n, e)``: the float64 value, the sum of the magnitudes of the terms behind it,
the number n of f32 roundings of relative size 2^-24 that apply to s, and e, the error the output inherits from its
f32 inputs.  With the siblings' factor 2 of margin

    bar = 2 (n 2^-24 s + e)            (no rtol floor, no constant fitted to a GPU)

n and e follow the kernels' f32 operations one by one (u = 2^-24; -ffp-contract=off: no fused multiply-adds):

  * dot product of length K in ANY order (lanes, wave_sum, MFMA): K roundings on sum |a_k b_k|  ->  K u s.
  * beta_l = sum_{j<l} b_j carries l u sum |b_j|; bw_l = beta_l . w_l: (F + l + 1) u s; boc likewise with + |b_o|.
  * product of two inexact numbers: |a| e_b + |b| e_a + e_a e_b + u |a b| (+ 2^-126: an f32 product may underflow).
  * alpha recursion: s_l = alpha_l p_l + bw_l, alpha_{l+1} = alpha_l + s_l, one rounding per operation on its own
    result, the inherited errors through the product rule — e grows with alpha by the same factors (1 + |p_l|), which
    is why the saturated cases (reference init: alpha of 1e8 and more) need no special bar.
  * sigmoid(z) = 1 / (1 + expf(-z)): expf within 3 ulp and the divide within 2.5 ulp (the OpenCL bounds the device
    library is built to; 1 ulp <= 2 u relative), 1 + t one rounding.  An error of z is a shift of the argument and
    the sigmoid is monotone: e = max(sig(z + e_z') - sig(z), sig(z) - sig(z - e_z')) + (1 + 5) u sig(z + e_z') + 2^-126
    with e_z' = e_z + 6 u; expf overflowing to inf at z < -88.7 gives 0 for a value below 2^-126.
  * BPR: d = pred+ - pred- (one rounding), softplus(-d) = max(-d, 0) + log1pf(expf(-|d|)) is 1-Lipschitz and all its
    pieces are below 1.4: e_d + (6 + 4 + 2) u (log1pf within 2 ulp); sigmoid(-d) is 1/4-Lipschitz: e_d / 4 + 12 u.
  * a wave's loss partial: its k units in order, k u s.
  * weight gradients: each row's term into the workgroup's LDS accumulator, each workgroup's sum into global memory,
    both with atomics in arbitrary order.  A sum of m terms in any order is off by at most (m - 1) u s, so the two
    levels give n = (rows of the fullest workgroup) + (workgroups) + 1 (the value already there).
  * assembly: copies are exact (n = 0); the category mean is Lmax - 1 additions and a divide (n = Lmax).  Scatter
    backward: the atomics of one element in any order (n = its number of terms + 1), dx / Lmax one more rounding.

Exactness.  ``exact(q, s)`` of ngcf_ref64.py: every term an integer multiple of the power of two q and s <= 2^24 q.
It can hold for the assembly forward, the scatter backward (tables and gradients on a dyadic grid, Lmax a power of
two: the divide is a shift) and yr_relu_bwd; there the GPU must equal float64 bit for bit.  The head and the scorer
go through expf and are judged by the bar only.
"""
import numpy as np
import torch

import dcn_ref
from ngcf_ref64 import F32, SENTINEL, U24, exact, over, quantum  # noqa: F401  (re-exported to the tests)

# csrc/common.h:10-13 (kWave, kBlock, kWavesPerBlock, kMaxGrid = YR_LOSS_PARTIALS) and csrc/dcn.hip:24-26 (kDcnMaxF /
# kDcnMaxH / kDcnMaxL), :621 (the head's grid: 256 workgroups of 4 waves, one unit per wave and trip), :378 (kSU, kSI,
# kSK, kSN: the scorer's tile of 8 users x 32 items, its K chunk and its H2 slice)
WAVE, BLOCK, WAVES = 64, 256, 4
HEAD_GRID = 256
HEAD_TRIP = HEAD_GRID * WAVES                # units per trip of the head's loop: 1024
MAX_GRID = 2048                              # kMaxGrid: grid_for() of the assembly kernels and yr_relu_bwd
LOSS_PARTIALS = 2048
GRID_ELEMS = MAX_GRID * BLOCK                # elements per trip of the grid-stride loops: 524,288
SU, SI, SK, SN = 8, 32, 32, 128
MAX_F, MAX_H, MAX_L = 512, 1024, 8
MAX_EVAL = SU * 65535                        # gridDim.y of the scorer
FLAG_BAD_USER, FLAG_BAD_ITEM = 1, 2

TINY = 2.0 ** -126
EXP_ULP, LOG1P_ULP, DIV_ULP = 3.0, 2.0, 2.5


class Out:
    __slots__ = ("v", "s", "n", "e")

    def __init__(self, v, s=None, n=0.0, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.s = np.abs(self.v) if s is None else np.broadcast_to(np.asarray(s, np.float64), self.v.shape)
        self.n = np.broadcast_to(np.asarray(n, np.float64), self.v.shape)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    def __getitem__(self, k):
        return Out(self.v[k], self.s[k], self.n[k], self.e[k])

    def plus(self, old):
        """The same sum accumulated into ``old`` (its additions are already counted in n)."""
        old = np.asarray(old, np.float64)
        return Out(self.v + old, self.s + np.abs(old), self.n, self.e)

    def with_values(self, v):
        return Out(np.asarray(v, np.float64).reshape(self.v.shape), self.s, self.n, self.e)


def bar(o):
    return 2.0 * (o.n * U24 * o.s + o.e)


def ratio(got, o):
    """max |got - v| / bar (0 for an empty output); NaN / inf in ``got`` give inf."""
    got = np.asarray(got, np.float64).reshape(o.v.shape)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    return float(over(got - o.v, bar(o)).max())


def f64(a):
    return np.asarray(a, np.float64)


def sig(z):
    t = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + t), t / (1.0 + t))


def _mul(a, ea, b, eb):
    v = a * b
    return v, np.abs(a) * eb + np.abs(b) * ea + ea * eb + U24 * np.abs(v) + TINY


def _sigmoid(z, ez):
    ez = ez + 2.0 * EXP_ULP * U24
    v, lo, hi = sig(z), sig(z - ez), sig(z + ez)
    return v, np.maximum(hi - v, v - lo) + (1.0 + 2.0 * DIV_ULP) * U24 * hi + TINY


# ---- assembly -------------------------------------------------------------------------------------------------------

def _row_ids(rows, B, user, item_a, item_b, num_users, num_items, attr_per_row):
    r = np.arange(rows)
    b = np.where(r < B, r, r - B)
    if item_a is None:
        it = r.copy()
    else:
        it = np.where(r < B, np.asarray(item_a, np.int64)[b], np.asarray(item_b if item_b is not None else item_a, np.int64)[b])
    u = None if user is None else np.asarray(user, np.int64)[b]
    ok_u = np.ones(rows, bool) if u is None else (u >= 0) & (u < num_users)
    ok_i = (it >= 0) & (it < num_items)
    ar = r if attr_per_row else np.where(ok_i, it, 0)
    return u, it, ar, ok_u, ok_i, ok_i | bool(attr_per_row)


def _rows_of(B, item_b):
    return 2 * B if item_b is not None else B


def assemble(U, I, C, S, cat_ids, sc_ids, user, item_a, item_b=None, B=None, attr_per_row=False, skip_slot=None):
    """(Out x [rows, 3 D or 4 D], flag).  Rows [0, B) pair user[b] with item_a[b], rows [B, 2 B) with item_b[b];
    item_a None: item = row; user None: no user segment.  A bad id leaves zeros in its segment (a bad category slot
    adds nothing to the mean, which still divides by Lmax).  ``skip_slot`` (row, slot): that slot is left out."""
    I, C, S = f64(I), f64(C), f64(S)
    cat_ids, sc_ids = np.asarray(cat_ids, np.int64), np.asarray(sc_ids, np.int64)
    D, Lmax = I.shape[1], cat_ids.shape[1]
    if B is None:
        B = len(item_a) if item_a is not None else (cat_ids.shape[0] if attr_per_row else I.shape[0])
    rows = _rows_of(B, item_b)
    nu = 0 if user is None else U.shape[0]
    u, it, ar, ok_u, ok_i, ok_a = _row_ids(rows, B, user, item_a, item_b, nu, I.shape[0], attr_per_row)
    flag = 0
    segs, mags, ns = [], [], []
    if user is not None:
        seg = np.where(ok_u[:, None], f64(U)[np.where(ok_u, u, 0)], 0.0)
        flag |= FLAG_BAD_USER * bool((~ok_u).any())
        segs.append(seg); mags.append(np.abs(seg)); ns.append(np.zeros_like(seg))
    flag |= FLAG_BAD_ITEM * bool((~ok_i).any())
    seg = np.where(ok_i[:, None], I[np.where(ok_i, it, 0)], 0.0)
    segs.append(seg); mags.append(np.abs(seg)); ns.append(np.zeros_like(seg))
    cats = cat_ids[ar]                                                       # [rows, Lmax]
    ok_c = (cats >= 0) & (cats < C.shape[0]) & ok_a[:, None]
    flag |= FLAG_BAD_ITEM * bool(((cats < 0) | (cats >= C.shape[0]))[ok_a].any())
    w = ok_c.astype(np.float64)
    if skip_slot is not None:
        w[skip_slot] = 0.0
    g = C[np.where(ok_c, cats, 0)] * w[:, :, None]                           # [rows, Lmax, D]
    segs.append(g.sum(1) / Lmax); mags.append(np.abs(g).sum(1) / Lmax); ns.append(np.full((rows, D), float(Lmax)))
    sc = sc_ids[ar]
    ok_s = (sc >= 0) & (sc < S.shape[0]) & ok_a
    flag |= FLAG_BAD_ITEM * bool(((sc < 0) | (sc >= S.shape[0]))[ok_a].any())
    seg = np.where(ok_s[:, None], S[np.where(ok_s, sc, 0)], 0.0)
    segs.append(seg); mags.append(np.abs(seg)); ns.append(np.zeros_like(seg))
    return Out(np.concatenate(segs, 1), np.concatenate(mags, 1), np.concatenate(ns, 1)), int(flag)


def assemble_bwd(dx, cat_ids, sc_ids, num_users, num_items, num_cats, num_sc, user, item_a, item_b=None, B=None,
                 attr_per_row=False, skip_slot=None):
    """((gU or None, gI, gC, gS) as Outs of the added sums, flag): the dense scatter-add of the four lookups; the mean
    hands dx / Lmax to every slot, padding included.  Bad ids add nothing."""
    dx = f64(dx)
    cat_ids, sc_ids = np.asarray(cat_ids, np.int64), np.asarray(sc_ids, np.int64)
    Lmax = cat_ids.shape[1]
    D = dx.shape[1] // (4 if user is not None else 3)
    if B is None:
        B = len(item_a) if item_a is not None else dx.shape[0]
    rows = _rows_of(B, item_b)
    u, it, ar, ok_u, ok_i, ok_a = _row_ids(rows, B, user, item_a, item_b, num_users, num_items, attr_per_row)
    dx = dx[:rows]
    flag, off = 0, 0

    def scatter(n_rows, at, ok, g, extra=0.0):
        v, s, c = np.zeros((n_rows, D)), np.zeros((n_rows, D)), np.zeros((n_rows, 1))
        np.add.at(v, at[ok], g[ok]); np.add.at(s, at[ok], np.abs(g[ok])); np.add.at(c, at[ok], 1.0)
        return Out(v, s, c + 1.0 + extra)

    gU = None
    if user is not None:
        gU = scatter(num_users, u, ok_u, dx[:, :D])
        flag |= FLAG_BAD_USER * bool((~ok_u).any())
        off = D
    flag |= FLAG_BAD_ITEM * bool((~ok_i).any())
    gI = scatter(num_items, it, ok_i, dx[:, off:off + D])
    cats = cat_ids[ar]
    ok_c = (cats >= 0) & (cats < num_cats) & ok_a[:, None]
    flag |= FLAG_BAD_ITEM * bool(((cats < 0) | (cats >= num_cats))[ok_a].any())
    if skip_slot is not None:
        ok_c[skip_slot] = False
    gc = np.repeat((dx[:, off + D:off + 2 * D] / Lmax)[:, None, :], Lmax, 1).reshape(rows * Lmax, D)
    gC = scatter(num_cats, cats.reshape(-1), ok_c.reshape(-1), gc, extra=0.0 if Lmax & (Lmax - 1) == 0 else 1.0)
    sc = sc_ids[ar]
    ok_s = (sc >= 0) & (sc < num_sc) & ok_a
    flag |= FLAG_BAD_ITEM * bool(((sc < 0) | (sc >= num_sc))[ok_a].any())
    gS = scatter(num_sc, sc, ok_s, dx[:, off + 2 * D:off + 3 * D])
    return (gU, gI, gC, gS), int(flag)


def relu_bwd(g, y, gate=True):
    g, y = f64(g), f64(y)
    return Out(np.where(y > 0, g, 0.0) if gate else g, n=0.0)


# ---- head -----------------------------------------------------------------------------------------------------------

def head_grid(units):
    return int(min(max(-(-units // WAVES), 1), HEAD_GRID))


def cross_consts(cw, cb, Woc, bo):
    """beta [L + 1, F], sum |b| [L + 1, F], (bw, e_bw) [L], (boc, e_boc)."""
    L, F = cw.shape
    beta = np.vstack([np.zeros((1, F)), np.cumsum(cb, 0)])
    babs = np.vstack([np.zeros((1, F)), np.cumsum(np.abs(cb), 0)])
    bw = (beta[:L] * cw).sum(1)
    ebw = (F + np.arange(L) + 1.0) * U24 * (babs[:L] * np.abs(cw)).sum(1)
    boc = beta[L] @ Woc + bo
    eboc = (F + L + 2.0) * U24 * (babs[L] @ np.abs(Woc) + abs(bo))
    return beta, babs, bw, ebw, boc, eboc


def _alpha(p, ep, bw, ebw):
    """alpha_l [L + 1, R], s_l [L, R] and their inherited errors from p [R, L]."""
    R_, L = p.shape
    al, eal = np.ones((L + 1, R_)), np.zeros((L + 1, R_))
    s, es = np.zeros((L, R_)), np.zeros((L, R_))
    for l in range(L):
        ap, eap = _mul(al[l], eal[l], p[:, l], ep[:, l])
        s[l] = ap + bw[l]
        es[l] = eap + ebw[l] + U24 * np.abs(s[l])
        al[l + 1] = al[l] + s[l]
        eal[l + 1] = eal[l] + es[l] + U24 * np.abs(al[l + 1])
    return al, eal, s, es


def head_closed(x, h, cw, cb, Wo, bo, bpr, inv_batch=0.0, gpred=None, backward=True, unit_weight=None, fmask=None,
                hmask=None, gate=True):
    """The head in the closed form of csrc/dcn.hip:12-18, operation by operation, with the error each value inherits.
    Returns {name: Out}: pred [rows], loss [2048 partials] (bpr), dh, dx0 [rows, .], dcw, dcb [L, F], dWo [H + F],
    dbo [1] (the sums the kernel ADDS).  Mutations for tests/test_dcn_ref64.py: ``unit_weight`` [units] scales a unit's
    share of the loss and of the weight gradients (0: dropped, 2: twice), ``fmask`` [F] / ``hmask`` [H] zero elements
    of the forward dot products, ``gate`` False lets dh through where h == 0."""
    x, h, cw, cb, Wo = f64(x), f64(h), f64(cw), f64(cb), f64(Wo).reshape(-1)
    bo = float(np.asarray(bo).reshape(-1)[0])
    (R_, F), H, L = x.shape, h.shape[1], cw.shape[0]
    units = R_ // 2 if bpr else R_
    Wod, Woc = Wo[:H], Wo[H:]
    beta, babs, bw, ebw, boc, eboc = cross_consts(cw, cb, Woc, bo)
    xm = x if fmask is None else x * f64(fmask)
    hm = h if hmask is None else h * f64(hmask)
    p, ep = xm @ cw.T, F * U24 * (np.abs(xm) @ np.abs(cw).T)
    q, eq = xm @ Woc, F * U24 * (np.abs(xm) @ np.abs(Woc))
    th, eth = hm @ Wod, H * U24 * (np.abs(hm) @ np.abs(Wod))
    al, eal, s, es = _alpha(p, ep, bw, ebw)
    aq, eaq = _mul(al[L], eal[L], q, eq)
    z = th + aq + boc
    ez = eth + eaq + eboc + U24 * (np.abs(th + aq) + np.abs(z))
    pred, epred = _sigmoid(z, ez)
    out = {"pred": Out(pred, e=epred, n=0.0)}
    w_unit = np.ones(units) if unit_weight is None else f64(unit_weight)
    if bpr:
        d = pred[:units] - pred[units:]
        ed = epred[:units] + epred[units:] + U24 * np.abs(d)
        sp = np.logaddexp(0.0, -d) * w_unit
        esp = (ed + (2.0 * EXP_ULP + 2.0 * LOG1P_ULP + 2.0) * U24) * w_unit
        nw = WAVES * head_grid(units)
        slot = np.arange(units) % nw
        out["loss"] = Out(np.bincount(slot, sp, LOSS_PARTIALS), np.bincount(slot, np.abs(sp), LOSS_PARTIALS),
                          np.bincount(slot, None, LOSS_PARTIALS), np.bincount(slot, esp, LOSS_PARTIALS))
        sn = sig(-d)
        esn = ed / 4.0 + (2.0 * EXP_ULP + 1.0 + 2.0 * DIV_ULP) * U24 * sn
        dp = -sn * inv_batch
        edp = esn * abs(inv_batch) + U24 * np.abs(dp)
        dpred, edpred = np.concatenate([dp, -dp]), np.concatenate([edp, edp])
    else:
        dpred = np.zeros(R_) if gpred is None else f64(gpred).reshape(-1)
        edpred = np.zeros(R_)
    if not backward:
        return out
    ab, eab = _mul(dpred, edpred, pred, epred)
    dz, edz = _mul(ab, eab, 1.0 - pred, epred + U24 * np.abs(1.0 - pred))
    open_ = (h > 0) if gate else np.ones_like(h, bool)
    dh = np.where(open_, dz[:, None] * Wod, 0.0)
    out["dh"] = Out(dh, n=1.0, e=np.where(open_, edz[:, None] * np.abs(Wod) + TINY, 0.0))
    wr = np.tile(w_unit, 2 if bpr else 1)[:, None]
    per_wg = -(-units // (WAVES * head_grid(units))) * WAVES * (2 if bpr else 1)
    n_acc = float(per_wg + head_grid(units) + 1)

    def summed(T, eT):
        return Out((wr * T).sum(0), (wr * np.abs(T)).sum(0), n_acc, (wr * eT).sum(0))

    T = dz[:, None] * h
    dWo_h = summed(T, edz[:, None] * np.abs(h) + U24 * np.abs(T) + TINY)
    out["dbo"] = summed(dz[:, None], edz[:, None])
    S, eS = _mul(dz, edz, q, eq)
    c, ec = np.zeros((L, R_)), np.zeros((L, R_))
    for l in range(L - 1, -1, -1):
        c[l], ec[l] = S, eS
        cp, ecp = _mul(c[l], ec[l], p[:, l], ep[:, l])
        S = S + cp
        eS = eS + ecp + U24 * np.abs(S)

    def inner(l):
        ax = al[l][:, None] * x
        v = ax + beta[l]
        return v, eal[l][:, None] * np.abs(x) + U24 * np.abs(ax) + l * U24 * babs[l] + U24 * np.abs(v)

    G = dz[:, None] * Woc
    eG = edz[:, None] * np.abs(Woc) + U24 * np.abs(G) + TINY
    T, eT = _mul(dz[:, None], edz[:, None], *inner(L))
    dWo_c = summed(T, eT)
    out["dWo"] = Out(*(np.concatenate([getattr(dWo_h, k), getattr(dWo_c, k)]) for k in ("v", "s", "n", "e")))
    dx, edx = np.zeros_like(x), np.zeros_like(x)
    dcb, dcw = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        sg, esg = _mul(s[l][:, None], es[l][:, None], G, eG)
        dx = dx + sg
        edx = edx + esg + U24 * np.abs(dx)
        dcb[l] = summed(G, eG)
        t = c[l][:, None] * cw[l]
        G = G + t
        eG = eG + ec[l][:, None] * np.abs(cw[l]) + U24 * np.abs(t) + TINY + U24 * np.abs(G)
    out["dx0"] = Out(dx + G, n=1.0, e=edx + eG)
    for l in range(L):
        T, eT = _mul(c[l][:, None], ec[l][:, None], *inner(l))
        dcw[l] = summed(T, eT)
    for name, parts in (("dcw", dcw), ("dcb", dcb)):
        out[name] = Out(*(np.stack([getattr(o, k) for o in parts]) for k in ("v", "s", "n", "e")))
    return out


EINSUM_ELEMS = 1 << 24                       # rows x F x F x L doubles of one autograd chunk (128 MiB per saved tensor)


def head_einsum(x, h, cw, cb, Wo, bo, bpr, inv_batch=0.0, gpred=None, backward=True):
    """The same values from the einsum form of tests/dcn_ref.py and float64 autograd, in chunks of units whose
    F x F outer products fit: {name: array}.  dh is gated by h > 0 here (autograd hands back dz W_od)."""
    t64 = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    (R_, F), H, L = np.shape(x), np.shape(h)[1], np.shape(cw)[0]
    units = R_ // 2 if bpr else R_
    P = {f"cross_weights.{l}": t64(cw[l]).requires_grad_(backward) for l in range(L)}
    P.update({f"cross_bias.{l}": t64(cb[l]).requires_grad_(backward) for l in range(L)})
    P["output_layer.weight"] = t64(Wo).reshape(1, -1).requires_grad_(backward)
    P["output_layer.bias"] = t64(bo).reshape(1).requires_grad_(backward)
    X, Hh = t64(x), t64(h)
    pred, dx0, dh = np.zeros(R_), np.zeros((R_, F)), np.zeros((R_, H))
    step = max(1, EINSUM_ELEMS // (F * F * L * (2 if bpr else 1)))
    for lo in range(0, units, step):
        u = np.arange(lo, min(units, lo + step))
        r = np.concatenate([u, u + units]) if bpr else u
        xc, hc = X[r].clone().requires_grad_(backward), Hh[r].clone().requires_grad_(backward)
        pr = dcn_ref.head(P, xc, hc)
        pred[r] = pr.detach().numpy()
        if backward:
            if bpr:
                obj = -torch.nn.functional.logsigmoid(pr[:len(u)] - pr[len(u):]).sum() * inv_batch
            else:
                obj = (pr * t64(gpred).reshape(-1)[r]).sum()
            obj.backward()
            dx0[r], dh[r] = xc.grad.numpy(), hc.grad.numpy()
    out = {"pred": pred}
    if bpr:
        slot = np.arange(units) % (WAVES * head_grid(units))
        out["loss"] = np.bincount(slot, np.logaddexp(0.0, -(pred[:units] - pred[units:])), LOSS_PARTIALS)
    if backward:
        out.update(dx0=dx0, dh=dh * (np.asarray(h) > 0),
                   dcw=np.stack([P[f"cross_weights.{l}"].grad.numpy() for l in range(L)]),
                   dcb=np.stack([P[f"cross_bias.{l}"].grad.numpy() for l in range(L)]),
                   dWo=P["output_layer.weight"].grad.numpy().reshape(-1), dbo=P["output_layer.bias"].grad.numpy())
    return out


def head(x, h, cw, cb, Wo, bo, bpr, inv_batch=0.0, gpred=None, backward=True):
    """{name: Out}: the values of the einsum form, the magnitudes and inherited errors of the closed form."""
    closed = head_closed(x, h, cw, cb, Wo, bo, bpr, inv_batch, gpred, backward)
    values = head_einsum(x, h, cw, cb, Wo, bo, bpr, inv_batch, gpred, backward)
    return {k: o.with_values(values[k]) for k, o in closed.items()}


# ---- scorer ---------------------------------------------------------------------------------------------------------

def score(Au, Bi, Pu, Pi, users, W2, b2, Wo, bo, cw, cb, kmask=None, nmask=None, epilogue=None):
    """(Out [n, num_items], flag): sigmoid(deep + alpha_L q + boc) of the header comment of dcn_score_kernel with the
    operands as given; the row of a bad user is NaN (the kernel skips it).  W2 None: one hidden layer.  Mutations:
    ``kmask`` [H1] / ``nmask`` [H2] zero elements of the sums over H1 / H2, ``epilogue`` [H2] is the index at which
    W_od and b2 are read for row n of W2."""
    Au, Bi, Pu, Pi, Wo, cw, cb = (f64(a) for a in (Au, Bi, Pu, Pi, Wo, cw, cb))
    Wo = Wo.reshape(-1)
    bo = float(np.asarray(bo).reshape(-1)[0])
    users = np.asarray(users, np.int64)
    ok = (users >= 0) & (users < Au.shape[0])
    flag = FLAG_BAD_USER * bool((~ok).any())
    ur = np.where(ok, users, 0)
    H1, L = Au.shape[1], cw.shape[0]
    Hd = H1 if W2 is None else np.shape(W2)[0]
    Wod, Woc = Wo[:Hd], Wo[Hd:]
    _, _, bw, ebw, boc, eboc = cross_consts(cw, cb, Woc, bo)
    h1 = np.maximum(Au[ur][:, None, :] + Bi[None, :, :], 0.0)                # [n, ni, H1], one rounding each
    if kmask is not None:
        h1 = h1 * f64(kmask)
    if W2 is None:
        deep = h1 @ Wod
        edeep = (H1 + 1.0) * U24 * (h1 @ np.abs(Wod))
    else:
        W2, b2 = f64(W2), f64(b2)
        at = np.arange(Hd) if epilogue is None else np.asarray(epilogue)
        a = h1 @ W2.T + b2[at]
        ea = (H1 + 1.0) * U24 * (h1 @ np.abs(W2).T) + U24 * np.abs(a)
        wo = Wod[at] if nmask is None else Wod[at] * f64(nmask)
        r = np.maximum(a, 0.0)
        deep = r @ wo
        edeep = ea @ np.abs(wo) + Hd * U24 * (r @ np.abs(wo))
    n, ni = deep.shape
    pp = Pu[ur][:, None, :] + Pi[None, :, :]                                 # [n, ni, L + 1]
    epp = U24 * np.abs(pp)
    al, eal, _, _ = _alpha(pp[:, :, :L].reshape(n * ni, L), epp[:, :, :L].reshape(n * ni, L), bw, ebw)
    aq, eaq = _mul(al[L], eal[L], pp[:, :, L].reshape(-1), epp[:, :, L].reshape(-1))
    deep, edeep = deep.reshape(-1), edeep.reshape(-1)
    z = deep + aq + boc
    ez = edeep + eaq + eboc + U24 * (np.abs(deep + aq) + np.abs(z))
    v, e = _sigmoid(z, ez)
    v = np.where(np.repeat(ok, ni), v, np.nan)
    return Out(v.reshape(n, ni), n=0.0, e=e.reshape(n, ni)), int(flag)


# ---- inputs and the cases of tests/test_gpu_dcn_edges.py (built identically by tests/test_dcn_ref64.py) --------------

def sixteenths(rs, shape):
    return (rs.randint(-16, 17, size=shape) / 16.0).astype(F32)


def normal(rs, shape, scale=1.0):
    return (rs.standard_normal(shape) * scale).astype(F32)


ASM_SIZES = dict(nu=23, ni=37, nc=11, ns=5)
ASM_FORMS = ("triplet", "pair", "items", "per_row")
# (D, Lmax, exact twin)
ASM_SHAPES = [(16, 1, True), (32, 2, True), (64, 3, False), (128, 8, True), (16, 10, False), (32, 8, True),
              (64, 1, True), (128, 3, False)]
# rows x D just under, at and past one trip of the 2048 x 256 grid
ASM_BIG = [(128, GRID_ELEMS // 128 - 1), (128, GRID_ELEMS // 128), (128, GRID_ELEMS // 128 + 1),
           (16, GRID_ELEMS // 16 + 1)]


def asm_tables(D, Lmax, exact_inputs, seed=0, nu=None, ni=None, nc=None, ns=None):
    """U, I, C, S and the item -> attributes table: lists padded with id 0, item 0 all padding."""
    z = ASM_SIZES
    nu, ni, nc, ns = nu or z["nu"], ni or z["ni"], nc or z["nc"], ns or z["ns"]
    rs = np.random.RandomState(1000 * D + 10 * Lmax + int(exact_inputs) + 7 * seed)
    make = (lambda s: sixteenths(rs, s)) if exact_inputs else (lambda s: normal(rs, s))
    U, I, C, S = make((nu, D)), make((ni, D)), make((nc, D)), make((ns, D))
    C[0] = make((D,)) if exact_inputs else normal(rs, (D,)) + F32(0.5)        # the padding row is not zero
    C[0][C[0] == 0] = F32(0.25)
    lens = rs.randint(1, Lmax + 1, ni)
    cat = np.zeros((ni, Lmax), np.int32)
    for i, n in enumerate(lens):
        cat[i, :n] = rs.randint(1, nc, n)
    cat[0] = 0
    cat[1] = rs.randint(1, nc, Lmax)                                         # a full list
    cat[2] = 7                                                               # one category in every slot
    sc = rs.randint(0, ns, ni).astype(np.int32)
    return dict(U=U, I=I, C=C, S=S, cat=cat, sc=sc, nu=nu, ni=ni, nc=nc, ns=ns, D=D, Lmax=Lmax)


def asm_ids(t, form, B, seed=0, same=None):
    """(user, item_a, item_b, per-row (cat, sc) or None) of one row form; ``same``: every row names one user / item."""
    rs = np.random.RandomState(31 * B + seed + ASM_FORMS.index(form))
    u = rs.randint(0, t["nu"], B).astype(np.int64)
    a = rs.randint(0, t["ni"], B).astype(np.int64)
    b = rs.randint(0, t["ni"], B).astype(np.int64)
    a[0] = 0                                                                 # the all-padding item
    if B > 2:
        a[B - 1], u[B - 1] = t["ni"] - 1, t["nu"] - 1
    if same == "user":
        u[:] = 3
    if same == "item":
        a[:], b[:] = 5, 5
    if same == "category":                                                   # items whose lists are all category 7
        a[:], b[:] = 2, 2
    if form == "triplet":
        return u, a, b, None
    if form == "pair":
        return u, a, None, None
    if form == "items":
        return None, None, None, None
    own_cat = rs.randint(0, t["nc"], (B, t["Lmax"])).astype(np.int32)
    own_cat[rs.rand(B, t["Lmax"]) < 0.3] = 0
    return u, a, None, (own_cat, rs.randint(0, t["ns"], B).astype(np.int32))


def asm_dx(rows, width, exact_inputs, seed=0):
    rs = np.random.RandomState(rows + width + seed)
    return sixteenths(rs, (rows, width)) if exact_inputs else normal(rs, (rows, width))


def asm_old(t, exact_inputs):
    rs = np.random.RandomState(t["D"] + 3)
    make = (lambda s: sixteenths(rs, s) + F32(1.0)) if exact_inputs else (lambda s: normal(rs, s) + F32(3.0))
    return [make((t[k], t["D"])) for k in ("nu", "ni", "nc", "ns")]


BAD_IDS = ("user<0", "user>=n", "item<0", "item>=n", "cat<0", "cat>=n", "statecity")


def make_bad(t, ids, kind, B):
    """One bad id of ``kind`` in copies of (tables, ids): (tables, ids, flag, bad rows, segment names they lose)."""
    u, a, b, own = (None if v is None else (tuple(x.copy() for x in v) if isinstance(v, tuple) else v.copy()) for v in ids)
    t = dict(t, cat=t["cat"].copy(), sc=t["sc"].copy())
    at = B // 2
    if kind.startswith("user"):
        u[at] = -1 if kind == "user<0" else t["nu"]
        return t, (u, a, b, own), FLAG_BAD_USER, [at], ("user",)
    if kind.startswith("item"):
        a[at] = -3 if kind == "item<0" else t["ni"]
        return t, (u, a, b, own), FLAG_BAD_ITEM, [at], ("item",) if own is not None else ("item", "cat", "sc")
    item = 4
    if a is None:                                                            # item-only form: row = item
        rows = [item]
    else:
        a[at] = item
        rows = [r for r in range(B) if a[r] == item] + ([B + r for r in range(B) if b[r] == item] if b is not None else [])
    if own is not None:
        rows, tab_c, tab_s, item = [at], own[0], own[1], at
    else:
        tab_c, tab_s = t["cat"], t["sc"]
    if kind == "statecity":
        tab_s[item] = t["ns"]
        return t, (u, a, b, own), FLAG_BAD_ITEM, rows, ("sc",)
    tab_c[item, 0] = -1 if kind == "cat<0" else t["nc"]
    return t, (u, a, b, own), FLAG_BAD_ITEM, rows, ("cat slot",)


RELU_N = (0, 1, 255, 256, 257, GRID_ELEMS + 1)


def relu_case(n):
    rs = np.random.RandomState(n % 9973)
    g = normal(rs, (n,))
    y = np.maximum(normal(rs, (n,)), F32(0))
    y[::7] = F32(0.0)
    y[3::7] = F32(-0.0)
    y[5::11] = -np.abs(normal(rs, y[5::11].shape))                           # not a ReLU output: still gated
    return g, y


# (F, H, L, units): every F, H and L of the list once, the unit counts around one wave, one workgroup and one trip
HEAD_SMALL = [(64, 32, 1, 1), (128, 64, 2, 3), (256, 96, 3, 4), (512, 1024, 8, 5), (20, 1, 4, 5), (65, 63, 5, 4),
              (511, 1023, 6, 3), (64, 65, 7, 5), (128, 96, 8, 4)]
HEAD_LARGE = [(20, 33, 2, HEAD_TRIP), (20, 33, 2, HEAD_TRIP + 1), (64, 32, 3, 2 * HEAD_TRIP + 5)]
HEAD_PITCH = (3, 5, 1, 7)                    # extra floats of ldx, ldh, lddh, lddx in the pitched case


def head_case(F, H, L, units, bpr, kind="random", seed=0):
    """x0, h (post-ReLU: exact zeros), cw, cb, Wo, bo, gpred, the old weight gradients.  kind: "random" (cross weights
    rand * 0.02 as tests/test_gpu_dcn.py; an output layer wide enough that pos and neg rows do not cancel), "init" (the reference's init: torch.rand cross weights and biases, N(0, 1)
    attribute segments, kaiming id segments and output layer), "saturated" (every pred is exactly 0 or 1)."""
    rs = np.random.RandomState(100000 * int(bpr) + 1000 * L + F + H + units % 9973 + 17 * seed)
    R_ = units * (2 if bpr else 1)
    D = max(F // 4, 1)
    x = normal(rs, (R_, F), 0.2)
    h = np.maximum(normal(rs, (R_, H)), F32(0))
    cw, cb = (rs.rand(L, F) * 0.02).astype(F32), (rs.rand(L, F) * 0.02).astype(F32)
    Wo, bo = normal(rs, (H + F,), 0.6), np.array([0.1], F32)
    if kind == "init":
        x[:, :2 * D] = normal(rs, (R_, 2 * D), np.sqrt(2.0 / D))
        x[:, 2 * D:] = normal(rs, (R_, F - 2 * D))
        cw, cb = rs.rand(L, F).astype(F32), rs.rand(L, F).astype(F32)
        Wo, bo = normal(rs, (H + F,), np.sqrt(2.0 / (H + F))), np.zeros(1, F32)
    if kind == "saturated":
        h[:] = F32(240.0 / H)
        h[::2] = F32(0)                                                      # z = -120 and z = +120 alternate
        if bpr:
            h[units:units + 2] = h[:2]                                       # d = 0 as well as d = +-1
        Wo[:H], Wo[H:], bo = F32(1), F32(0), np.array([-120.0], F32)
    gpred = None if bpr else normal(rs, (R_,))
    marked = []
    if units >= HEAD_TRIP and kind == "random":
        # like the ladder rows of ngcf_ref64.py: a unit of the first and the last unit of the last trip carry a
        # gradient that does not vanish (pos row at z = 0, neg row at z = 2.5, so that pos and neg do not cancel; gpred = 4)
        marked = [5, units - 1]
        up, dn = np.maximum(Wo[:H], F32(0)), np.maximum(-Wo[:H], F32(0))

        def aim(row, target):
            p0 = head_closed(x[row:row + 1], np.zeros((1, H)), cw, cb, Wo, bo, False, backward=False)["pred"].v[0]
            need = target - np.log(p0 / (1.0 - p0))
            d = up if need > 0 else dn
            h[row] = d * F32(abs(need) / float(d @ d))
        for m in marked:
            aim(m, 0.0)
            if bpr:
                aim(units + m, 2.5)
            else:
                gpred[m] = F32(4.0)
    old = dict(dcw=normal(rs, (L, F)) + F32(2), dcb=normal(rs, (L, F)) + F32(2), dWo=normal(rs, (H + F,)) + F32(2),
               dbo=np.array([1.5], F32))
    inv = float(F32(1.0 / units)) if bpr else 0.0
    return dict(x=x, h=h, cw=cw, cb=cb, Wo=Wo, bo=bo, gpred=gpred, old=old, inv_batch=inv, bpr=bpr, units=units,
                F=F, H=H, L=L, marked=marked)


def head_ref(c, backward=True, closed=False, **mut):
    f = head_closed if closed or mut else head
    return f(c["x"], c["h"], c["cw"], c["cb"], c["Wo"], c["bo"], c["bpr"], c["inv_batch"],
             c["gpred"] if backward else None, backward, **mut)


SCORE_ONE = (32, 64, 1024)
SCORE_TWO = ((32, 32), (32, 128), (64, 160), (32, 256), (96, 224), (1024, 32), (32, 1024))
SCORE_ITEMS = (1, 31, 32, 33, 77)
SCORE_USERS = {1: [4], 7: [0, 5, 5, 10, 3, 9, 1], 8: [0, 5, 5, 10, 3, 9, 1, 2], 9: [10, 0, 5, 5, 7, 3, 9, 1, 2],
               13: [0, 5, 10, 7, 7, 3, 1, 2, 3, 4, 6, 9, 8]}
SCORE_NU = 11


def score_case(H1, H2, ni, L, seed=0):
    """Synthetic operands of yr_dcn_score: Au, Bi (about half of h1 is cut by the ReLU), Pu, Pi, W2, b2, Wo, bo, cw,
    cb with F = 512 at L = 8 and 64 otherwise."""
    rs = np.random.RandomState(H1 + 3 * (H2 or 0) + 7 * ni + 1000 * L + seed)
    F = 512 if L == 8 else 64
    Hd = H2 or H1
    c = dict(Au=normal(rs, (SCORE_NU, H1), 0.5), Bi=normal(rs, (ni, H1), 0.5), Pu=normal(rs, (SCORE_NU, L + 1), 0.15),
             Pi=normal(rs, (ni, L + 1), 0.15), W2=None, b2=None, Wo=normal(rs, (Hd + F,), 1.0 / np.sqrt(Hd)),
             bo=np.array([0.05], F32), cw=(rs.rand(L, F) * 0.02).astype(F32), cb=(rs.rand(L, F) * 0.02).astype(F32),
             H1=H1, H2=H2, ni=ni, L=L, F=F)
    if H2:
        c["W2"], c["b2"] = normal(rs, (H2, H1), 1.0 / np.sqrt(H1)), normal(rs, (H2,), 0.1)
    return c


def score_ref(c, users, **mut):
    return score(c["Au"], c["Bi"], c["Pu"], c["Pi"], users, c["W2"], c["b2"], c["Wo"], c["bo"], c["cw"], c["cb"], **mut)
