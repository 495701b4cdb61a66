"""Cases and the sequential restatement of the ordered DCN scatter (csrc/dcn_owned.hip, yr_dcn_owned_assemble_bwd).
Importable helper, no fixtures; runs without a GPU (tests/test_dcn_owned_host.py) and feeds
tests/test_gpu_dcn_owned_edges.py.

The contract (include/yelprec_engine.h), with row(b, pos) = b and row(b, neg) = B + b and one f32 add per term:

  level 1   user u:  acc = gU[u];  for its triplets b ascending:  acc += dx[b, 0:D];  acc += dx[B + b, 0:D]
            item i:  acc = gI[i], tc = ts = 0;  for its entries by key 4 b + role (pos 1 before neg 2):
                     acc += dx[row, D:2D];  tc += dx[row, 2D:3D];  ts += dx[row, 3D:4D]
  level 2   the static table inverted (per category its items ascending with the multiplicity m of the category among
            the item's slots; per state-city its items ascending), every list cut into chunks of CHUNK entries:
            q_chunk = 0;  for the chunk's touched items ascending:  q += ts[i]   or   q += (f32(m) * tc[i]) / f32(Lmax)
            dst = old;  for the row's chunks that hold a touched item, ascending:  dst += q_chunk
  a bad user loses its user entry, a bad item its item and attribute parts; a slot out of range is in no list and
  raises the item flag when its item is in the batch; rows nothing touches keep what they held.

``expected`` is that as plain np.float32 loops.  Inputs that can SEE a wrong order: dx = +-m 2^-e with m in [1, 2^19),
e in [0, 8] — magnitudes spread over 27 binades, so sums round at nearly every add and another order gives other bits
(checked by the host test).  Lmax = 4 where bits are compared (the divide is a shift); the twin at Lmax = 3 is judged by
the float64 bar of dcn_ref64.py only.  The dyadic twins (sixteenths) make every sum exact: float64 equals f32 there.
"""
import numpy as np

F32 = np.float32
CHUNK = 256                                   # YR_DCN_OWNED_CHUNK
NU, NI, NC, NS, LMAX = 40, 600, 9, 5, 4
WIDTHS = (16, 64, 128)
BATCHES = (1, 5, 700)
HOT_USER, HOT_TRIPLETS, BOTH_ITEM, SAME_AT = 7, 48, 13, 100
ONE_CHUNK_CAT, CHUNK_PLUS_ONE_CAT, THREE_CHUNK_CAT, EMPTY_CAT = 1, 2, 3, 8
TWICE_ITEMS = (20, 300, 580)                  # items whose list names category 3 in two slots
FLAG_BAD_USER, FLAG_BAD_ITEM = 1, 2


def tables(Lmax=LMAX, seed=0):
    """cat [NI, Lmax] / sc [NI]: category 1 on exactly CHUNK items, category 2 on CHUNK + 1, category 3 on all 600 (three
    chunks: 256 + 256 + 88; twice on three of them), categories 4 .. 7 at random, category 8 on none; the padding
    category 0 fills the rest (a multi-chunk list with multiplicities 1 .. 3).  State-city 0 holds about 300 items (two
    chunks), state-city 4 the last forty."""
    rs = np.random.RandomState(50 + seed)
    cat = np.zeros((NI, Lmax), np.int32)
    i = np.arange(NI)
    cat[:, 0] = THREE_CHUNK_CAT
    if Lmax > 1:
        cat[i < CHUNK, 1] = ONE_CHUNK_CAT
    if Lmax > 2:
        cat[(i >= 100) & (i <= 100 + CHUNK), 2] = CHUNK_PLUS_ONE_CAT
    if Lmax > 3:
        cat[:, 3] = rs.choice([0, 0, 4, 5, 6, 7], NI)
    cat[list(TWICE_ITEMS), Lmax - 1] = THREE_CHUNK_CAT
    sc = rs.randint(1, NS - 1, NI).astype(np.int32)
    sc[rs.permutation(NI)[:300]] = 0
    sc[NI - 40:] = NS - 1                       # the last state-city belongs to the items no case touches
    return dict(cat=cat, sc=sc, nu=NU, ni=NI, nc=NC, ns=NS, Lmax=Lmax)


def _wide(rs, shape):
    m = rs.randint(1, 2 ** 19, size=shape).astype(np.float64)
    e = rs.randint(0, 9, size=shape)
    return (rs.choice([-1.0, 1.0], size=shape) * m * 2.0 ** -e).astype(F32)


def _sixteenths(rs, shape):
    return (rs.randint(-16, 17, size=shape) / 16.0).astype(F32)


def scatter_case(D, B, Lmax=LMAX, dyadic=False, seed=0):
    """Tables, ids and dx [2 B, 4 D] of one triplet batch.  B >= 700: the first 560 triplets name items 0 .. 559 as
    positives (more than two chunks' worth of touched items in category 3), user 7 sits on 48 triplets, item 13 is a
    positive and a negative of different triplets, triplet 100 has pos == neg; the last ten users and the last forty
    items stay untouched."""
    rs = np.random.RandomState(7000 + D + 13 * B + 5 * Lmax + int(dyadic) + 1000 * seed)
    t = tables(Lmax)
    u = rs.randint(0, NU - 10, B).astype(np.int64)
    p = rs.randint(0, NI - 40, B).astype(np.int64)
    n = rs.randint(0, NI - 40, B).astype(np.int64)
    if B >= 700:
        p[:560] = np.arange(560)
        u[u == HOT_USER] = HOT_USER + 1
        u[rs.choice(B, HOT_TRIPLETS, replace=False)] = HOT_USER
        p[3], n[5] = BOTH_ITEM, BOTH_ITEM
        n[SAME_AT] = p[SAME_AT]
    dx = (_sixteenths if dyadic else _wide)(rs, (2 * B, 4 * D))
    return dict(t=t, u=u, p=p, n=n, dx=dx, D=D, B=B)


def old_tables(D, dyadic=False, value=None):
    """What gU / gI / gC / gS hold on entry: ``value`` everywhere, or numbers of their own."""
    if value is not None:
        return [np.full((r, D), value, F32) for r in (NU, NI, NC, NS)]
    rs = np.random.RandomState(D + 3)
    make = (lambda s: _sixteenths(rs, s) + F32(1.0)) if dyadic else (lambda s: _wide(rs, s))
    return [make((r, D)) for r in (NU, NI, NC, NS)]


def order_case(D=16, rows=40, per_row=24):
    """``rows`` users with ``per_row`` triplets each (48 contributions per user row), every item a positive several
    times: the rows the CPU test re-sums in other orders."""
    B = rows * per_row
    rs = np.random.RandomState(99)
    c = scatter_case(D, B, seed=3)
    c["u"] = np.repeat(np.arange(rows), per_row).astype(np.int64)
    c["p"] = rs.randint(0, 30, B).astype(np.int64)
    c["n"] = rs.randint(30, NI, B).astype(np.int64)
    return c


# ---- the static table inverted: brute force ----------------------------------------------------------------------

def invert(t, chunk=CHUNK):
    """dict(cat_ptr, cat_item, cat_mult, cat_chunk_ptr, sc_ptr, sc_item, sc_chunk_ptr) by loops over the table."""
    cat, sc = np.asarray(t["cat"]), np.asarray(t["sc"])
    out = {}
    ptr, item, mult = [0], [], []
    for c in range(t["nc"]):
        for i in range(cat.shape[0]):
            m = int((cat[i] == c).sum())
            if m:
                item.append(i)
                mult.append(m)
        ptr.append(len(item))
    out.update(cat_ptr=np.array(ptr), cat_item=np.array(item, np.int64), cat_mult=np.array(mult, np.int64))
    ptr, item = [0], []
    for s in range(t["ns"]):
        item.extend(i for i in range(len(sc)) if sc[i] == s)
        ptr.append(len(item))
    out.update(sc_ptr=np.array(ptr), sc_item=np.array(item, np.int64))
    for k in ("cat", "sc"):
        out[k + "_chunk_ptr"] = np.concatenate([[0], np.cumsum(-(-np.diff(out[k + "_ptr"]) // chunk))])
    return out


# ---- the order contract ---------------------------------------------------------------------------------------------

def entries(c):
    """{user: [b, ...]}, {item: [row, ...]} in the contract's order, and the flag of the ids."""
    t, B = c["t"], c["B"]
    users, items, flag = {}, {}, 0
    for b in range(B):
        u, p, n = int(c["u"][b]), int(c["p"][b]), int(c["n"][b])
        if 0 <= u < t["nu"]:
            users.setdefault(u, []).append(b)
        else:
            flag |= FLAG_BAD_USER
        for it, row in ((p, b), (n, B + b)):                 # key 4 b + 1 before 4 b + 2
            if 0 <= it < t["ni"]:
                items.setdefault(it, []).append(row)
            else:
                flag |= FLAG_BAD_ITEM
    return users, items, flag


def chain(start, terms, order=None):
    acc = np.array(start, F32)
    for j in (range(len(terms)) if order is None else order):
        acc = (acc + terms[j]).astype(F32)
    return acc


def user_terms(c, bs):
    D, B = c["D"], c["B"]
    out = []
    for b in bs:
        out += [c["dx"][b, :D], c["dx"][B + b, :D]]
    return out


def expected(c, old, chunk=CHUNK, one_chain=()):
    """(gU, gI, gC, gS, flag): copies of ``old`` with every touched row summed in the contract's order.  ``chunk``
    moves the chunk boundaries; the categories in ``one_chain`` are summed as a single chain (both are mutations for
    the host test)."""
    t, D, dx = c["t"], c["D"], c["dx"]
    Lmax = F32(t["Lmax"])
    gU, gI, gC, gS = (a.copy() for a in old)
    users, items, flag = entries(c)
    for u, bs in users.items():
        gU[u] = chain(gU[u], user_terms(c, bs))
    tc, ts = {}, {}
    zero = np.zeros(D, F32)
    for i, rows in items.items():
        gI[i] = chain(gI[i], [dx[r, D:2 * D] for r in rows])
        tc[i] = chain(zero, [dx[r, 2 * D:3 * D] for r in rows])
        ts[i] = chain(zero, [dx[r, 3 * D:4 * D] for r in rows])
        slots = np.asarray(t["cat"][i])
        if ((slots < 0) | (slots >= t["nc"])).any() or not 0 <= int(t["sc"][i]) < t["ns"]:
            flag |= FLAG_BAD_ITEM
    inv = invert(t, chunk)
    for name, dst, terms in (("cat", gC, tc), ("sc", gS, ts)):
        ptr, its = inv[name + "_ptr"], inv[name + "_item"]
        for r in range(len(ptr) - 1):
            acc, any_hit = dst[r].copy(), False
            step = 10 ** 9 if (name == "cat" and r in one_chain) else chunk
            for lo in range(int(ptr[r]), int(ptr[r + 1]), step):
                q, hit = zero.copy(), False
                for e in range(lo, min(lo + step, int(ptr[r + 1]))):
                    i = int(its[e])
                    if i not in terms:
                        continue
                    if name == "cat":
                        q = (q + ((F32(inv["cat_mult"][e]) * terms[i]).astype(F32) / Lmax).astype(F32)).astype(F32)
                    else:
                        q = (q + terms[i]).astype(F32)
                    hit = True
                if hit:
                    acc, any_hit = (acc + q).astype(F32), True
            if any_hit:
                dst[r] = acc
    return gU, gI, gC, gS, flag


def touched(c):
    """Boolean masks (users, items, categories, state-cities) of the rows the batch reaches."""
    t = c["t"]
    users, items, _ = entries(c)
    mu, mi, mc, ms = (np.zeros(k, bool) for k in (t["nu"], t["ni"], t["nc"], t["ns"]))
    mu[list(users)] = True
    mi[list(items)] = True
    for i in items:
        for s in t["cat"][i]:
            if 0 <= s < t["nc"]:
                mc[s] = True
        if 0 <= t["sc"][i] < t["ns"]:
            ms[t["sc"][i]] = True
    return mu, mi, mc, ms
