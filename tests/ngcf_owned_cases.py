"""Cases and the sequential restatement of the owner-pass score gradient of csrc/ngcf_owned.hip.  Importable helper, no
fixtures; runs without a GPU (tests/test_ngcf_owned_host.py) and feeds tests/test_gpu_ngcf_owned_edges.py.

The contract (include/yelprec_engine.h, yr_ngcf_owned_score_bwd): dlayers[k][row] starts from its content on entry and
receives the row's per-triplet contributions in ascending triplet index, each with ONE f32 add; a user row gets
fmaf(gn, E_k[U + neg], gp * E_k[U + pos]) per triplet (gp * E_k[U + pos] without negatives), an item row gp * E_k[user]
as positive, then gn * E_k[user] as negative.  ``expected`` below is that as a plain np.float32 loop.

Inputs that can SEE a wrong order: the layer entries are integers in [-15, 15] and the score gradients
g = +-m 2^-e with m in [1, 2^19), e in [0, 8].  Every product g * entry is then exact in f32 (|m * entry| < 2^23), so
the fused multiply-add of the user row equals float32(float64(gp rp) + float64(gn rn)) — one rounding, computed here in
float64 — while the SUMS of such terms (magnitudes spread over 27 binades) round at nearly every add: another order
gives other bits (checked on the CPU by test_ngcf_owned_host.py).
"""
import numpy as np

F32 = np.float32
USERS, ITEMS = 40, 50
WIDTHS = (16, 64, 128)
LAYERS = (1, 3)


def G(D):
    """Triplets per wave of the default score kernels: lane groups of D / 4 lanes."""
    return 64 // (D // 4)


def batches(D):
    g = G(D)
    return [0, 1, g - 1, g, g + 1, 257]


def _grads(rs, B):
    m = rs.randint(1, 2 ** 19, size=B).astype(np.float64)
    e = rs.randint(0, 9, size=B)
    return (rs.choice([-1.0, 1.0], size=B) * m * 2.0 ** -e).astype(F32)


def _layers(rs, layers, D, users=USERS, items=ITEMS):
    return [rs.randint(-15, 16, size=(users + items, D)).astype(F32) for _ in range(layers)]


def score_case(D, layers, B, with_neg, seed=0):
    rs = np.random.RandomState(4000 + D + 31 * layers + 7 * B + int(with_neg) + 1000 * seed)
    return dict(layers=_layers(rs, layers, D), u=rs.randint(0, USERS, B).astype(np.int64),
                p=rs.randint(0, ITEMS, B).astype(np.int64),
                n=rs.randint(0, ITEMS, B).astype(np.int64) if with_neg else None,
                gpos=_grads(rs, B), gneg=_grads(rs, B) if with_neg else None, num_users=USERS, num_items=ITEMS)


MIXED_B = 600
HOT_USER, BOTH_ITEM, SAME_AT, BAD_USER_AT, BAD_ITEM_AT = 7, 13, 100, 250, 400


def mixed_case(D, layers, with_neg):
    """600 triplets: user 7 takes 48 of them, item 13 occurs as positive and as negative, triplet 100 has pos == neg,
    triplet 250 carries a bad user id and triplet 400 a bad item id; no triplet touches the last ten users and items."""
    c = score_case(D, layers, MIXED_B, with_neg, seed=1)
    rs = np.random.RandomState(17 + D)
    c["u"] %= USERS - 10                                   # the last ten users and items stay untouched
    c["p"] %= ITEMS - 10
    if with_neg:
        c["n"] %= ITEMS - 10
    c["u"][c["u"] == HOT_USER] = HOT_USER + 1
    free = np.setdiff1d(np.arange(MIXED_B), [BAD_USER_AT, BAD_ITEM_AT])
    c["u"][rs.choice(free, 48, replace=False)] = HOT_USER
    c["p"][[3, 77, 301]] = BOTH_ITEM
    if with_neg:
        c["n"][[5, 77 + 1, 500]] = BOTH_ITEM
        c["n"][SAME_AT] = c["p"][SAME_AT]
    c["u"][BAD_USER_AT] = USERS
    c["p"][BAD_ITEM_AT] = -1
    return c


LONG_ROW = 1000


def long_row_case(D, layers):
    """1,000 triplets of one user (and of one negative item): rows with 1,000 contributions."""
    c = score_case(D, layers, LONG_ROW, True, seed=2)
    c["u"][:] = 3
    c["n"][:] = 9
    return c


def valid(c):
    ok = (c["u"] >= 0) & (c["u"] < c["num_users"]) & (c["p"] >= 0) & (c["p"] < c["num_items"])
    if c["n"] is not None:
        ok &= (c["n"] >= 0) & (c["n"] < c["num_items"])
    return ok


def flags_expected(c):
    """YR_FLAG_BAD_USER = 1, YR_FLAG_BAD_ITEM = 2."""
    bad_u = (c["u"] < 0) | (c["u"] >= c["num_users"])
    bad_i = (c["p"] < 0) | (c["p"] >= c["num_items"])
    if c["n"] is not None:
        bad_i |= (c["n"] < 0) | (c["n"] >= c["num_items"])
    return (1 if bad_u.any() else 0) | (2 if bad_i.any() else 0)


def contributions(c, k):
    """{row: [f32 vector, ...]} of layer k in the contract's order."""
    E, U = c["layers"][k], c["num_users"]
    E64 = E.astype(np.float64)
    out = {}
    ok = valid(c)
    for b in np.flatnonzero(ok):
        u, p = int(c["u"][b]), int(c["p"][b])
        gp = float(c["gpos"][b])
        user_term = (gp * E64[U + p]).astype(F32)                       # the product alone is rounded first ...
        if c["n"] is not None:
            n, gn = int(c["n"][b]), float(c["gneg"][b])
            # ... then fmaf(gn, rn, that): one rounding of the exact sum
            user_term = (user_term.astype(np.float64) + gn * E64[U + n]).astype(F32)
        out.setdefault(u, []).append(user_term)
        out.setdefault(U + p, []).append((gp * E64[u]).astype(F32))
        if c["n"] is not None:
            out.setdefault(U + n, []).append((gn * E64[u]).astype(F32))
    return out


def ordered_sum(start, terms, order=None):
    acc = np.array(start, F32)
    for j in (range(len(terms)) if order is None else order):
        acc = (acc + terms[j]).astype(F32)                               # one f32 add per contribution
    return acc


def expected(c, prefill):
    """One [n, D] f32 array per layer: ``prefill`` (a scalar) everywhere, the touched rows summed in the contract's
    order on top of it."""
    out = []
    for k, E in enumerate(c["layers"]):
        d = np.full(E.shape, prefill, F32)
        for row, terms in contributions(c, k).items():
            d[row] = ordered_sum(d[row], terms)
        out.append(d)
    return out


def products_are_exact(c):
    """Every g * entry is an f32 number (the premise of ``contributions``)."""
    ok = True
    for E in c["layers"]:
        for g in (c["gpos"], c["gneg"]):
            if g is None or len(g) == 0:
                continue
            prod = g.astype(np.float64)[:, None] * np.unique(E).astype(np.float64)[None, :]
            ok &= bool((prod.astype(F32).astype(np.float64) == prod).all())
    return ok


def order_case(D=16, rows=40, per_row=24):
    """``rows`` users with ``per_row`` triplets each, one layer: the rows the CPU test re-sums in other orders."""
    B = rows * per_row
    rs = np.random.RandomState(99)
    c = dict(layers=_layers(rs, 1, D, rows, ITEMS), u=np.repeat(np.arange(rows), per_row).astype(np.int64),
             p=rs.randint(0, ITEMS, B).astype(np.int64), n=rs.randint(0, ITEMS, B).astype(np.int64),
             gpos=_grads(rs, B), gneg=_grads(rs, B), num_users=rows, num_items=ITEMS)
    return c


# ---- ordered row sets ------------------------------------------------------------------------------------------------

FRONTIER_N = (1023, 1024, 1025, 4097)                     # around one scan tile (1,024 flags) and past four


def frontier_batches(n):
    """{name: (num_users, num_items, u, p, n)} over a graph of n nodes: empty, one triplet, every node."""
    nu = n // 2
    ni = n - nu
    rs = np.random.RandomState(n)
    B = 3 * n
    full_u = np.concatenate([np.arange(nu), rs.randint(0, nu, B - nu)]).astype(np.int64)
    full_p = np.concatenate([np.arange(ni), rs.randint(0, ni, B - ni)]).astype(np.int64)
    z = np.zeros(0, np.int64)
    some = max(1, n // 5)
    return {"empty": (nu, ni, z, z, z),
            "one": (nu, ni, np.array([nu - 1], np.int64), np.array([0], np.int64), np.array([ni - 1], np.int64)),
            "some": (nu, ni, rs.randint(0, nu, some).astype(np.int64), rs.randint(0, ni, some).astype(np.int64),
                     rs.randint(0, ni, some).astype(np.int64)),
            "all": (nu, ni, rs.permutation(full_u), rs.permutation(full_p), rs.randint(0, ni, B).astype(np.int64))}
