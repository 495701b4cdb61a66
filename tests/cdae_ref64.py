"""Float64 restatement of the CDAE list kernels (csrc/cdae_sparse.hip, cdae_hidden_bwd of csrc/cdae.hip) for the
tests, on dense [B, I] arrays: the encoder, the sampled decoder with its three gradients and the hidden layer's
backward with dW_h.  Importable helper, no fixtures (like eval_ladders.py / dcn_ref.py).

Every output is an ``Out(v, n, s)``: the float64 value, the number of summed terms and the sum of their
magnitudes.  An f32 kernel that adds n terms in ANY order is off by at most (n + 1) 2^-24 sum |terms| to first
order; with the factor 2 of margin of test_gpu_mf_wide._dot_bar the bar of an output is

    bar = max(project bar, 2 (n + 1) 2^-24 s),     project bar = 2e-4 |v| + 1e-7 + 2e-5 max |v|

(the project bar is what test_fused_step_equals_autograd_route applies to the same quantities; the loss: 1e-5 |v|).
Where a term is itself computed from an inner f32 dot product of m terms (the decoder's gradient factor g comes
from z . W_o[i] + b_o[i]), the term's relative error is 2 (m + 1) 2^-24 kappa with kappa the condition of the factor
with respect to the dot product's terms; both are covered by n = n_outer + m and s = sum |term| max(1, kappa).

The input generators keep the bars able to notice ONE lost list entry (tests/test_cdae_ref64.py proves it per case):
list values positive, no cancellation across an encoder row, sigmoid pre-activations within +-3, identity output
pre-activations within [0.05, 0.95] (log and 1 / (y (1 - y)) stay regular: NaN handling is not under test), and the
columns at list index 2047, 2048 and last of every long row carry encoder weights large against the f32 bound of a
6,001-term sum (a 6,001-term sum of equal terms cannot resolve one of them in f32 at all: n^2 2^-23 > 1).
"""
import numpy as np

U24 = 2.0 ** -24
LIST_CAP = 2048                  # kListCap of csrc/cdae_sparse.hip: entries of a row staged per pass
I_LONG = 6001                    # 32 parts of 188 columns: an odd catalogue width (scalar fetch path of the compaction)
# entries per row of the long-row set, encoder list and loss list set independently; row 8: both long
ENC_COUNTS = (0, 1, 2047, 2048, 2049, 4096, 4097, -1, 2049)        # -1: every column
LOSS_COUNTS = (4097, -1, 2049, 0, 1, 4096, 2048, 2047, 2049)
SETTLE_COUNTS = (31, 32, 33, 63, 64, 65)                           # the 32-slot hand-off of the loss-only decoder
N_LONG = len(ENC_COUNTS)


class Out:
    __slots__ = ("v", "n", "s")

    def __init__(self, v, n, s):
        self.v = np.asarray(v, np.float64)
        self.n = np.broadcast_to(np.asarray(n, np.float64), self.v.shape)
        self.s = np.broadcast_to(np.asarray(s, np.float64), self.v.shape)

    def __getitem__(self, k):
        return Out(self.v[k], self.n[k], self.s[k])


def bar(o, rtol=2e-4, atol=1e-7, amax=2e-5):
    top = float(np.abs(o.v).max()) if o.v.size else 0.0
    return np.maximum(rtol * np.abs(o.v) + atol + amax * top, 2.0 * (o.n + 1.0) * U24 * o.s)


def loss_bar(o):
    return np.maximum(1e-5 * np.abs(o.v), 2.0 * (o.n + 1.0) * U24 * o.s)


def over(err, b):
    """|err| / bar element-wise; an exact zero passes a zero bar (an empty sum is exactly 0)."""
    err = np.abs(np.asarray(err, np.float64))
    return np.where(err == 0, 0.0, err / np.maximum(b, 1e-300))


def ratio(got, o, bar_fn=bar):
    """max |got - v| / bar (0 for an empty output); NaN / inf in ``got`` give inf."""
    got = np.asarray(got, np.float64).reshape(o.v.shape)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    return float(over(got - o.v, bar_fn(o)).max())


def _act(pre, act):
    return 1.0 / (1.0 + np.exp(-pre)) if act == 1 else pre


def _dact(y, act):
    return y * (1.0 - y) if act == 1 else np.ones_like(y)


# ---- the three operations -------------------------------------------------------------------------------------------

def encode(Wh, bh, V, user, x_in, act):
    """z = act(x_in . Wh^T + bh + V[user]); Wh [H, I]; an out-of-range user contributes no V row."""
    Wh, bh, V, x = (np.asarray(a, np.float64) for a in (Wh, bh, V, x_in))
    user = np.asarray(user)
    ok = (user >= 0) & (user < V.shape[0])
    Vu = np.where(ok[:, None], V[np.where(ok, user, 0)], 0.0)
    pre = x @ Wh.T + bh + Vu
    spre = np.abs(x) @ np.abs(Wh).T + np.abs(bh) + np.abs(Vu)
    n = (x != 0).sum(1, keepdims=True) + 2.0
    z = _act(pre, act)
    # act'(z) carries the sum's error through the activation; 8 2^-24 |z| for expf and the division
    return Out(z, n, _dact(z, act) * spre + (np.abs(z) * 4.0 / (n + 1.0) if act == 1 else 0.0))


def sampled_decode(z, Wo, bo, target, negmask, act, weight=None, splits=1):
    """The kernel's definition on the positions target + negmask != 0: y = act(z . Wo[i] + bo[i]), BCE term with the
    logs clamped at -100, g = (y - t) / max((1 - y) y, 1e-12) (times y (1 - y) for the sigmoid).  Returns
    dict(loss, partials, count, dz, dWo, dbo), all WITHOUT 1 / count.  ``partials`` [B, splits]: the loss sum of the
    workgroup (row, split), which takes the entries j of every staged pass with j % splits == split.  ``weight``
    [B, I] multiplies every position's contributions (0: the position dropped, 2: counted twice) for the
    sensitivity checks."""
    z, Wo, t, m = (np.asarray(a, np.float64) for a in (z, Wo, target, negmask))
    H = z.shape[1]
    b = np.zeros(Wo.shape[0]) if bo is None else np.asarray(bo, np.float64)
    w = ((t + m) != 0).astype(np.float64)
    if weight is not None:
        w = w * weight
    pre = z @ Wo.T + b
    spre = np.abs(z) @ np.abs(Wo).T + np.abs(b)
    y = _act(pre, act)
    with np.errstate(divide="ignore", invalid="ignore"):
        term = -(t * np.maximum(np.log(y), -100.0) + (1.0 - t) * np.maximum(np.log(1.0 - y), -100.0))
        den = np.maximum((1.0 - y) * y, 1e-12)
        g = (y - t) / den * _dact(y, act)
        dg = _dact(y, act) if act == 1 else np.abs(y * (1.0 - y) - (y - t) * (1.0 - 2.0 * y)) / den ** 2
        k_g = np.maximum(1.0, np.abs(dg) * spre / np.maximum(np.abs(g), 1e-300))
        k_l = np.maximum(1.0, np.abs(g) * spre / np.maximum(np.abs(term), 1e-300))
    term, g, k_g, k_l = (np.where(w != 0, a, 0.0) for a in (term, g, k_g, k_l))
    inner = H + 4.0                                   # the dot product, the bias and the element-wise operations
    per_row = np.abs(w).sum(1)
    per_col = np.abs(w).sum(0)
    gw, agk = g * w, np.abs(g * w) * k_g
    sel = (t + m) != 0
    share = np.where(sel, ((np.cumsum(sel, axis=1) - 1) % LIST_CAP) % splits, -1)
    of = [share == q for q in range(splits)]
    return {
        "loss": Out((term * w).sum(), per_row.max(initial=0.0) + inner, (np.abs(term * w) * k_l).sum()),
        "partials": Out(np.stack([(term * w * o).sum(1) for o in of], 1),
                        np.stack([(np.abs(w) * o).sum(1) for o in of], 1) + inner,
                        np.stack([(np.abs(term * w) * k_l * o).sum(1) for o in of], 1)),
        "count": int(round(w.sum())),
        "dz": Out(gw @ Wo, per_row[:, None] + inner, agk @ np.abs(Wo)),
        "dWo": Out(gw.T @ z, per_col[:, None] + inner, agk.T @ np.abs(z)),
        "dbo": Out(gw.sum(0), per_col + inner, agk.sum(0)),
    }


def hidden_bwd(dz, z, act, user, count, x_in, num_users):
    """dz' = dz (/ count) act'(z), dbh = column sums, dV[user] += dz' (out-of-range users skipped), dWh = dz'^T x_in
    ([H, I]; ``x_in`` None: no dWh) and the user / item marks.  ``count`` None: dz arrives scaled."""
    dz, z = np.asarray(dz, np.float64), np.asarray(z, np.float64)
    user = np.asarray(user)
    B, H = dz.shape
    a = 1.0 if count is None else (1.0 / count if count > 0 else 0.0)
    g = dz * a * _dact(z, act)
    ag = np.abs(g)
    ok = (user >= 0) & (user < num_users)
    dV, sV, nV = np.zeros((num_users, H)), np.zeros((num_users, H)), np.zeros((num_users, 1))
    np.add.at(dV, user[ok], g[ok])
    np.add.at(sV, user[ok], ag[ok])
    np.add.at(nV, user[ok], 1.0)
    res = {"dz": Out(g, 3.0, ag), "dbh": Out(g.sum(0), B + 3.0, ag.sum(0)), "dV": Out(dV, nV + 3.0, sV),
           "user_marks": (nV[:, 0] > 0).astype(np.uint8)}
    if x_in is not None:
        x = np.asarray(x_in, np.float64)
        res["dWh"] = Out(g.T @ x, (x != 0).sum(0)[None, :] + 3.0, ag.T @ np.abs(x))
        res["item_marks"] = (x != 0).any(0).astype(np.uint8)
    return res


# ---- inputs ---------------------------------------------------------------------------------------------------------

def _columns(rs, I, k):
    return np.arange(I) if k < 0 or k >= I else np.sort(rs.choice(I, k, replace=False))


def input_rows(rs, I, counts, binary=False):
    """x [B, I] f32 with exactly counts[r] entries in row r (-1: every column), values in [0.5, 1.5) (or 1)."""
    x = np.zeros((len(counts), I), np.float32)
    for r, k in enumerate(counts):
        c = _columns(rs, I, int(k))
        x[r, c] = 1.0 if binary else (0.5 + rs.rand(len(c))).astype(np.float32)
    return x


def loss_rows(rs, I, counts):
    """(target, negmask) [B, I] f32 0/1 with exactly counts[r] loss positions in row r, about a sixth of them
    positives (neg_times = 5)."""
    t = np.zeros((len(counts), I), np.float32)
    m = np.zeros((len(counts), I), np.float32)
    for r, k in enumerate(counts):
        c = _columns(rs, I, int(k))
        pos = rs.rand(len(c)) < 1.0 / 6.0
        t[r, c[pos]] = 1.0
        m[r, c[~pos]] = 1.0
    return t, m


def long_counts(B, rs, counts, short_hi):
    """The long-row set in rows 0 .. 8 of a batch of B rows; the others are short."""
    assert B >= N_LONG
    return list(counts) + [int(k) for k in rs.randint(0, short_hi, B - N_LONG)]


def probe_columns(x):
    """Columns at list index 2047, 2048 and last of every row with more than LIST_CAP entries."""
    out = set()
    for row in np.asarray(x):
        c = np.flatnonzero(row)
        if len(c) > LIST_CAP:
            out.update((int(c[LIST_CAP - 1]), int(c[LIST_CAP]), int(c[-1])))
    return np.array(sorted(out), np.int64)


def encoder_params(rs, H, I, num_users, x_in):
    """(Wh [H, I], bh, V) f32, all W_h entries positive: the plain columns of the longest row sum to at most 0.6, the
    probe columns to at most 1.8, |bh|, |V| <= 0.3 — pre-activations within [-0.6, 3.0]."""
    x = np.asarray(x_in)
    top = max(1.0, float(np.abs(x).sum(1).max()))
    Wh = ((0.2 + 0.8 * rs.rand(H, I)) * 0.6 / top).astype(np.float32)
    pc = probe_columns(x)
    if len(pc):
        Wh[:, pc] = ((0.5 + 0.5 * rs.rand(H, len(pc))) * 1.8 / (float(np.abs(x).max()) * len(pc))).astype(np.float32)
    bh = ((rs.rand(H) - 0.5) * 0.6).astype(np.float32)
    V = ((rs.rand(num_users, H) - 0.5) * 0.6).astype(np.float32)
    return Wh, bh, V


def decoder_params(rs, B, H, I, act, with_bo):
    """(z [B, H], Wo [I, H], bo or None) f32.  Identity output: every pre-activation within [0.06, 0.94]; sigmoid
    output: within +-3."""
    z = (0.4 + 0.5 * rs.rand(B, H)).astype(np.float32)
    if act == 1:
        Wo = ((2.0 * rs.rand(I, H) - 1.0) * 2.8 / (0.9 * H)).astype(np.float32)
        bo = ((rs.rand(I) - 0.5) * 0.4).astype(np.float32)
    else:
        Wo = ((0.5 + 0.5 * rs.rand(I, H)) / H * (0.3 + 0.7 * rs.rand(I, 1))).astype(np.float32)
        bo = (0.04 * rs.rand(I)).astype(np.float32)
    return z, Wo, (bo if with_bo else None)


def hidden_inputs(rs, B, H, num_users):
    """(dz, z, user) with duplicate users and, for B >= 2, one out-of-range user."""
    dz = (2.0 * rs.rand(B, H) - 1.0).astype(np.float32)
    z = (0.1 + 0.8 * rs.rand(B, H)).astype(np.float32)
    user = rs.randint(0, num_users, B).astype(np.int64)
    if B >= 3:
        user[B - 1] = user[0]
    if B >= 2:
        user[B // 2] = num_users + 5
    return dz, z, user


# ---- the cases of tests/test_gpu_cdae_long_rows.py (built identically by the CPU sensitivity check) -----------------

# a. encoder: (I, H, act, transposed, p)
ENCODER_CASES = [(6001, 4, 1, False, 0.0), (6001, 100, 0, True, 0.0), (6001, 128, 1, True, 0.0),
                 (6001, 256, 0, False, 0.0), (6001, 300, 1, True, 0.0), (6001, 300, 0, False, 0.0),
                 (6001, 4, 0, True, 0.0), (6001, 100, 1, False, 0.0), (6001, 128, 0, False, 0.0),
                 (6001, 256, 1, True, 0.0), (6000, 128, 1, True, 0.0), (6000, 100, 0, False, 0.0),
                 (6001, 128, 1, True, 0.3)]
ENCODER_USERS = 50


def encoder_case(I, H, act, transposed, p):
    rs = np.random.RandomState(1000 + I + 7 * H + act)
    x = input_rows(rs, I, ENC_COUNTS, binary=p > 0)
    user = rs.randint(0, ENCODER_USERS, N_LONG).astype(np.int64)
    user[4] = ENCODER_USERS + 3                                           # out of range: flag, no V row
    return dict(x=x, user=user, seed=int(rs.randint(1, 1 << 40)), rs=rs)


# b. sampled decoder with gradients: (B, I, H, act, with_bo, long rows)
DECODE_SPLITS = {1: 8, 64: 8, 73: 7, 85: 6, 102: 5, 128: 4, 170: 3, 256: 2, 257: 1, 600: 1}
DECODE_CASES = [(1, 301, 32, 1, True, False), (64, 301, 100, 0, True, False), (73, 301, 128, 1, False, False),
                (85, 301, 132, 0, True, False), (102, 301, 256, 1, True, False), (128, 301, 32, 0, False, False),
                (170, 301, 100, 1, True, False), (256, 301, 128, 0, True, False), (257, 301, 132, 1, False, False),
                (600, 301, 256, 0, True, False),
                (9, 6001, 128, 1, True, True), (9, 6001, 256, 0, True, True), (170, 6001, 100, 0, False, True),
                (170, 6001, 128, 1, True, True), (300, 6001, 132, 1, True, True), (300, 6001, 128, 0, True, True),
                (9, 6000, 32, 0, True, True), (300, 6000, 256, 1, False, True)]

# c. loss only: (B, I, H, act); rows: the long set, the settle() set, short rows
LOSS_ONLY_CASES = [(15, 6001, 4, 1), (15, 6001, 100, 0), (15, 6001, 128, 1), (15, 6001, 256, 0), (15, 6001, 130, 1),
                   (300, 6001, 128, 0), (170, 6000, 130, 0)]


def decode_case(B, I, H, act, with_bo, long, settle=False):
    rs = np.random.RandomState(2000 + B + I + 3 * H + act)
    if long:
        head = list(LOSS_COUNTS) + (list(SETTLE_COUNTS) if settle else [])
        counts = head + [int(k) for k in rs.randint(0, 60, B - len(head))]
    else:
        counts = [int(k) for k in rs.randint(0, 40, B)]
        counts[0] = 37
    target, negmask = loss_rows(rs, I, counts)
    z, Wo, bo = decoder_params(rs, B, H, I, act, with_bo)
    return dict(target=target, negmask=negmask, z=z, Wo=Wo, bo=bo, counts=counts)


# d. cdae_hidden_bwd
HIDDEN_B = (1, 15, 16, 17, 127, 128, 129, 300)
HIDDEN_H = (4, 63, 64, 65, 130)
HIDDEN_USERS = 40


def hidden_case(B, H):
    rs = np.random.RandomState(B * 1000 + H)
    dz, z, user = hidden_inputs(rs, B, H, HIDDEN_USERS)
    return dict(dz=dz, z=z, user=user, act=(B + H) % 2, scale_dz=(B + H // 2) % 2 == 0, partials=rs.rand(B * 3).astype(np.float32))


# e. dW_h kernels on the long rows: (kernel, H, act, scale_dz)
DWH_CASES = [("hidden_bwd_dwh_t", 256, 1, True), ("hidden_bwd_dwh_t", 100, 0, False), ("hidden_bwd_dwh_t", 320, 1, True),
             ("sparse_dwh_t", 128, 0, False), ("sparse_dwh", 64, 0, False)]


def dwh_case(H, batch=0):
    rs = np.random.RandomState(3000 + H + 17 * batch)
    counts = ENC_COUNTS if batch == 0 else ENC_COUNTS[::-1]
    x = input_rows(rs, I_LONG, counts)
    dz, z, user = hidden_inputs(rs, N_LONG, H, HIDDEN_USERS)
    return dict(x=x, dz=dz, z=z, user=user)


# ---- perturbed references: what a faulty staging pass would compute -------------------------------------------------

def list_weights(mask_row, splits=1):
    """The four perturbations of one row's list as weight vectors over its columns (None where the row has no such
    entry): entry 2048 dropped, entry 2048 twice, split 0's share of every pass dropped, the tail beyond the last
    full pass dropped."""
    c = np.flatnonzero(mask_row)
    k = len(c)
    one = np.ones(len(mask_row))
    res = {}
    if k > LIST_CAP:
        res["entry 2048 dropped"] = one.copy(); res["entry 2048 dropped"][c[LIST_CAP]] = 0.0
        res["entry 2048 twice"] = one.copy(); res["entry 2048 twice"][c[LIST_CAP]] = 2.0
        if k % LIST_CAP:
            res["tail dropped"] = one.copy(); res["tail dropped"][c[k // LIST_CAP * LIST_CAP:]] = 0.0
    if k:
        j = np.arange(k)
        res["split share dropped"] = one.copy(); res["split share dropped"][c[(j % LIST_CAP) % splits == 0]] = 0.0
    return res
