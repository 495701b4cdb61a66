"""Float64 restatement of ONE pull-form BPR-MF step (csrc/bpr_pull.hip) on a zero Adam state, for the tests.
Importable helper, no fixtures (like ngcf_ref64.py and cdae_ref64.py); runs without a GPU.

    x_b = U[u_b] . (I[p_b] - I[n_b])        softplus_b = log(1 + exp(-x_b))        g_b = -sigmoid(-x_b) * inv_batch
    gradU[r] = sum_{u_b = r} g_b (I[p_b] - I[n_b])
    gradI[i] = sum_{p_b = i} g_b U[u_b] - sum_{n_b = i} g_b U[u_b]
    loss     = inv_batch * sum_b softplus_b

over the triplets whose three ids are valid (the others only raise their flag).  inv_batch is an argument (the
multi-GPU caller passes 1 / global batch), not 1 / B.

How the tests read a gradient through the C ABI.  One call on mU = vU = mI = vI = 0 with beta1 = 0: m = 0 + 1 * (g - 0)
is the gradient itself; the item side is also read from gradI_out.  v = (1 - beta2) g * g.  With eps = 1 at step 1
(step_size = lr, bc2_sqrt = sqrt(1 - beta2)) the update is p - lr g / (|g| + 1), lr-Lipschitz in g.

Bars (derived here, no rtol floor: a floor of 1e-3 |v| is what hides one record dropped from a row of a thousand).
u = 2^-24 is the unit roundoff of f32.  Every gradient element is an ``Out(v, n, s)``: float64 value, number of summed
terms, sum of their magnitudes.

 1. Summation.  n terms added in ANY order (lane groups, shuffles, register totals, chunks, waves of a heavy row,
    parts of a shared bucket; additions of an exact zero do not round) with one rounding per product (an FMA):
    (n + 1) u s to first order.
 2. The user-side difference d = I[p] - I[n] is rounded before it is multiplied: |g| u |d| more per term — the
    product counts twice, as in ngcf_ref64.py.
 3. The coefficient.  The f32 score is D products of a rounded difference, added in some order: with the product
    counted twice, e_x = (2 D + 1) u sum_c |U_c| |d_c|.  sigmoid is 1/4-Lipschitz: inv_batch e_x / 4 on g.
    bpr_terms (csrc/common.h, "about 1 ulp each") computes z = exp2(-|x| * log2e), r = rcp(1 + z) and
    sigmoid(-x) = r or z r.  The argument -|x| * log2e carries the rounded constant and the rounded product, 2 u
    relative, which exp2 turns into 2 u |x| relative on z; exp2 itself 1 ulp = 2 u.  d ln sigmoid / d ln z is at most 1
    in magnitude on either branch, so z passes on at most its own relative error; 1 + z rounds (u), rcp 1 ulp (2 u),
    z r rounds (u), -sigmoid * inv_batch rounds (u):  |g| (2 |x| + 7) u.
        e_g = inv_batch e_x / 4 + |g| (2 |x| + 7) u
    reaches a gradient element through the magnitude of its factor: sum e_g |d_c| (user), sum e_g |U_c| (item).
 4. Loss: softplus = max(-x, 0) + log2(1 + z) * ln2.  1-Lipschitz in x (e_x); 1 + z is off by z (2 |x| + 2) u + u,
    which log passes on at most 1 : 1; log2 1 ulp and the rounded constant and product, 4 u of the log term; the final
    addition u softplus.  The sum over the batch in any order, (n + 1) u s, and the product with inv_batch, u |loss|.

    bar(g element) = 2 [ (n + 1) u s + (2.) + (3.) ]        (the factor 2 of margin of the sibling references, on all)
    bar(v)         = (1 - beta2) (2 |g| bar + bar^2) + 4 u v       twice the relative bar of g, and v's own roundings
    bar(p_new)     = 2^-23 |p| + lr bar(g)
    bar(loss)      = 2 inv_batch [ (n + 1) u s + sum e_softplus ] + 2 u |loss|

Exactness (``quantum`` / ``exact`` as in ngcf_ref64.py, from the arrays).  On the "exact" tables column 0 of every
user row is 16, of every even item -16, of every odd item +16, all other entries are in {-1, 0, 1}; positives are even
items, negatives odd ones.  Then x <= -512 + 2 (D - 1) <= -258: exp2 underflows to 0, rcp(1) = 1, log2(1) = 0, so
g = -inv_batch = -2^-10 and softplus = -x, an integer.  Every gradient term is a multiple of 2^-10, any order of f32
additions and FMAs gives the float64 value, and the GPU tests demand equality (of the loss where sum |x| <= 2^24).  A
probe at the top of the GPU file asserts that the three hardware forms are exact at these arguments.  Every g is equal
there, so a coefficient read from the wrong triplet shows on the random tables only (test_bpr_pull_ref64.py asserts
that it does).

Batches are built from prescribed counts: records per row and per stretch of the batch.  Inside a stretch the batch is
shuffled; which stretch (and so which tile) a record sits in is fixed, because an owner reads its bucket tile by tile.
Even item rows are used as positives only and odd rows as negatives only, so one batch serves both tables.
"""
import functools
import zlib

import numpy as np
import scipy.sparse as sp

from ngcf_ref64 import Out, U24, exact, over, quantum  # noqa: F401  (re-exported: one copy of the certificate)

F32 = np.float32
WIDTHS = (16, 32, 64, 128)
SENTINEL = 7.25                 # pre-fill of U_new and gradI_out: a row the kernel did not write shows
# geometry of csrc/bpr_pull.hip, each under the name it has there
CAP_USER, CAP_ITEM, HEAVY = 768, 1024, 96            # kUserCap, kCap, kHeavyRow
TILE_GROUP = 256                                     # kTileGroup
NARROW_BELOW, NARROW_ROWS = 768, 4                   # kNarrowBelow, kNarrowRows
SPLIT_MIN, SPLIT_TARGET, SPLIT_AVG_MIN, SPLIT_AVG_TARGET = 2048, 1024, 2.5, 1.25
MAX_PARTS, MAX_TASKS, MAX_SLOTS = 64, 512, 1024      # kMaxParts, kMaxTasks, kMaxSlots
USER_GRID, ITEM_GRID = 2048, 4096                    # YR_LOSS_PARTIALS, kMaxOwnerGrid
PART_THREADS, WAVE = 1024, 64                        # kPartThreads, kWave
# the Adam scalars of every call of the GPU file
LR, BETA1, BETA2, EPS = 0.125, 0.0, 0.999, 1.0
ONE_M_B2 = float(F32(1.0 - BETA2))
INV_EXACT = 2.0 ** -10


def R(D):
    return 1024 // D


def GPW(D):
    return 256 // D


def RPW(D):
    return R(D) // 4


def DEAL_BAR(D):
    return R(D) * R(D)


def deals(D, user):
    """Whether the form that deals rows to lane groups by load is compiled: a chunk must be able to hold DEAL_BAR."""
    return DEAL_BAR(D) <= (CAP_USER if user else CAP_ITEM)


def tile_size(B):
    return 1024 if B <= 129024 else 2048 if B <= 258048 else 4096


class Plan:
    """make_plan and the split thresholds of pull_apply_impl."""

    def __init__(self, B, nu, ni, D):
        self.R = R(D)
        self.narrow = -(-nu // self.R) < NARROW_BELOW and self.R > NARROW_ROWS
        self.RU = NARROW_ROWS if self.narrow else self.R
        self.nbU, self.nbI = -(-nu // self.RU), -(-ni // self.R)
        self.tile = tile_size(B)
        self.T = -(-B // self.tile)
        avg = 2.0 * B / self.nbI
        self.split_min = max(SPLIT_MIN, int(SPLIT_AVG_MIN * avg))
        self.split_target = max(SPLIT_TARGET, int(SPLIT_AVG_TARGET * avg))
        self.scan_per = {s: -(-nb // PART_THREADS) for s, nb in (("user", self.nbU), ("item", self.nbI))}
        self.user_trips = -(-self.nbU // USER_GRID)
        self.item_trips = -(-self.nbI // ITEM_GRID)
        self.tile_groups = -(-self.T // TILE_GROUP)


# ---- the step ----------------------------------------------------------------------------------------------------------

def _scatter(rows, idx):
    """W [B, k] -> [rows, k], the sum of the rows of W by idx (a sparse product: no add.at over a million rows)."""
    B = idx.shape[0]
    S = sp.csr_matrix((np.ones(B), idx, np.arange(B + 1)), shape=(B, rows)).T.tocsr()
    return lambda W: np.asarray(S @ W)


class Ref:
    pass


def step(U, I, u, p, n, inv_batch, wu=None, wp=None, wn=None, wl=None, shift=0, keep_bad=False):
    """The reference of one step.  wu / wp / wn / wl: per-triplet weights of the user-side term, the positive and the
    negative item-side term and the loss term (1 everywhere = the step; test_bpr_pull_ref64.py states what a wrong
    kernel would compute with 0, 2 and -1); shift: the item side takes the coefficient of triplet b + shift;
    keep_bad: triplets with a bad id are kept, the id wrapped into the table."""
    U64, I64 = np.asarray(U, np.float64), np.asarray(I, np.float64)
    nu, D = U64.shape
    ni = I64.shape[0]
    u, p, n = (np.asarray(a, np.int64) for a in (u, p, n))
    bad_u = (u < 0) | (u >= nu)
    bad_i = (p < 0) | (p >= ni) | (n < 0) | (n >= ni)
    r = Ref()
    r.flags = (1 if bad_u.any() else 0, 1 if bad_i.any() else 0)
    ok = np.ones(u.shape[0], bool) if keep_bad else ~(bad_u | bad_i)
    r.ok = ok
    ids = np.flatnonzero(ok)
    uu, pp, nn = u[ids] % nu, p[ids] % ni, n[ids] % ni
    w = [np.ones(ids.shape[0]) if a is None else np.asarray(a, np.float64)[ids] for a in (wu, wp, wn, wl)]
    Uu = U64[uu]
    d = I64[pp] - I64[nn]
    x = np.einsum("bd,bd->b", Uu, d)
    g = -inv_batch / (1.0 + np.exp(x))
    soft = np.logaddexp(0.0, -x)
    z = np.exp(-np.abs(x))
    e_x = (2 * D + 1) * U24 * np.einsum("bd,bd->b", np.abs(Uu), np.abs(d))
    e_g = inv_batch * e_x / 4.0 + np.abs(g) * (2.0 * np.abs(x) + 7.0) * U24
    e_soft = e_x + (z * (2.0 * np.abs(x) + 2.0) + 1.0) * U24 + 4.0 * U24 * np.log1p(z) + U24 * soft
    r.ids, r.x, r.g, r.soft = ids, x, g, soft
    gi = np.roll(g, -shift) if shift else g
    ei = np.roll(e_g, -shift) if shift else e_g
    # user side
    gw = (g * w[0])[:, None]
    su = _scatter(nu, uu)
    r.gU = Out(su(gw * d), su(np.abs(w[0])[:, None]), su(np.abs(gw * d)))
    r.eU = su((np.abs(gw) * U24 + (e_g * np.abs(w[0]))[:, None]) * np.abs(d))
    # item side: positives and negatives in one product
    both = np.concatenate([pp, nn])
    gpn = np.concatenate([gi * w[1], -gi * w[2]])[:, None]
    Upn = np.concatenate([Uu, Uu])
    si = _scatter(ni, both)
    r.gI = Out(si(gpn * Upn), si(np.abs(np.concatenate([w[1], w[2]]))[:, None]), si(np.abs(gpn * Upn)))
    r.eI = si(np.concatenate([ei * np.abs(w[1]), ei * np.abs(w[2])])[:, None] * np.abs(Upn))
    r.loss = Out(inv_batch * float((soft * w[3]).sum()), float(np.abs(w[3]).sum()), inv_batch * float(np.abs(soft * w[3]).sum()))
    r.e_loss = inv_batch * float((e_soft * np.abs(w[3])).sum())
    r.soft_sum = float(np.abs(soft * w[3]).sum())
    return r


def bar_g(o, e):
    return 2.0 * ((o.n + 1.0) * U24 * o.s + e)


def bar_v(o, e):
    b = bar_g(o, e)
    return ONE_M_B2 * (2.0 * np.abs(o.v) * b + b * b) + 4.0 * U24 * ONE_M_B2 * o.v * o.v


def bar_p(p0, o, e):
    return 2.0 ** -23 * np.abs(np.asarray(p0, np.float64)) + LR * bar_g(o, e)


def bar_loss(r):
    return 2.0 * ((r.loss.n + 1.0) * U24 * r.loss.s + r.e_loss) + 2.0 * U24 * abs(float(r.loss.v))


def v_of(g):
    return ONE_M_B2 * g * g


def p_of(p0, g):
    return np.asarray(p0, np.float64) - LR * g / (np.abs(g) + 1.0)


def ratio(got, want, b):
    """max |got - want| / bar (0 for an empty output); NaN / inf in ``got`` give inf."""
    got = np.asarray(got, np.float64).reshape(np.shape(want))
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    return float(over(got - want, np.broadcast_to(b, got.shape)).max())


# ---- tables -------------------------------------------------------------------------------------------------------------

def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


@functools.lru_cache(maxsize=4)
def tables(kind, nu, ni, D, seed):
    """(U, I) of a case, read-only."""
    rs = np.random.RandomState(_seed("tables", kind, nu, ni, D, seed))
    if kind == "random":
        U = rs.uniform(0.05, 0.4, (nu, D)) * rs.choice([-1.0, 1.0], (nu, D))
        I = rs.uniform(0.05, 0.4, (ni, D)) * rs.choice([-1.0, 1.0], (ni, D))
    else:
        U = rs.randint(-1, 2, (nu, D)).astype(np.float64)
        I = rs.randint(-1, 2, (ni, D)).astype(np.float64)
        U[:, 0] = 16.0
        I[0::2, 0] = -16.0
        I[1::2, 0] = 16.0
    U, I = U.astype(F32), I.astype(F32)
    U.setflags(write=False)
    I.setflags(write=False)
    return U, I


# ---- batches from prescribed counts -----------------------------------------------------------------------------------

def spread(total, rows, size):
    """`total` records over `rows`, as evenly as it goes -> counts[size]"""
    c = np.zeros(size, np.int64)
    rows = np.asarray(rows)
    if total:
        assert len(rows) and total >= 0
        c[rows] += total // len(rows)
        c[rows[:total % len(rows)]] += 1
    return c


def stretch(rs, length, cu, ci, fill_u, fill_i):
    """`length` consecutive triplets, shuffled: cu[r] records of user row r and ci[i] occurrences of item row i (even
    rows as positives, odd rows as negatives); what is missing to `length` on each of the three id lists goes evenly
    to the filler rows."""
    cu, ci = np.array(cu, np.int64), np.array(ci, np.int64)
    fill_i = np.asarray(fill_i)
    cu += spread(length - int(cu.sum()), fill_u, cu.shape[0])
    cp, cn = ci.copy(), ci.copy()
    cp[1::2] = 0
    cn[0::2] = 0
    cp += spread(length - int(cp.sum()), fill_i[fill_i % 2 == 0], ci.shape[0])
    cn += spread(length - int(cn.sum()), fill_i[fill_i % 2 == 1], ci.shape[0])
    out = []
    for c in (cu, cp, cn):
        assert int(c.sum()) == length and c.min() >= 0
        ids = np.repeat(np.arange(c.shape[0]), c)
        rs.shuffle(ids)
        out.append(ids)
    return out


class Case:
    def __init__(self, name, D, nu, ni, parts, inv_batch=None, order=None, ranges=None, bad=()):
        self.name, self.D, self.nu, self.ni = name, D, nu, ni
        self.u, self.p, self.n = (np.concatenate([q[k] for q in parts]).astype(np.int64) for k in range(3))
        for b, (bu, bp, bn) in bad:                 # bad ids replace what the stretch put there
            self.u[b], self.p[b], self.n[b] = bu if bu is not None else self.u[b], bp if bp is not None else self.p[b], \
                bn if bn is not None else self.n[b]
        self.B = self.u.shape[0]
        self.inv_random = inv_batch if inv_batch is not None else 1.0 / self.B
        self.order, self.ranges = order, ranges
        self.plan = Plan(self.B, nu, ni, D)
        for a in (self.u, self.p, self.n):
            a.setflags(write=False)

    def inv(self, kind):
        return self.inv_random if kind == "random" else INV_EXACT

    def tables(self, kind):
        return tables(kind, self.nu, self.ni, self.D, self.name)

    def valid(self):
        return (self.u >= 0) & (self.u < self.nu) & (self.p >= 0) & (self.p < self.ni) & (self.n >= 0) & (self.n < self.ni)

    def bucket_totals(self):
        """records per user bucket, occurrences per item bucket (valid triplets)"""
        ok, pl = self.valid(), self.plan
        tu = np.bincount(self.u[ok] // pl.RU, minlength=pl.nbU)
        ti = np.bincount(self.p[ok] // pl.R, minlength=pl.nbI) + np.bincount(self.n[ok] // pl.R, minlength=pl.nbI)
        return tu, ti

    def sharing(self):
        """build_splits and the admission rule: (parts per item bucket as wanted, tasks, slots, pools hold)"""
        pl = self.plan
        _, ti = self.bucket_totals()
        want = np.where(ti >= pl.split_min, np.minimum(-(-ti // pl.split_target), min(MAX_PARTS, pl.T)), 1)
        tasks = int((want[want > 1] - 1).sum())
        slots = int(want[want > 1].sum())
        return want, tasks, slots, tasks <= MAX_TASKS and slots <= MAX_SLOTS


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    c = case(name)
    U, I = c.tables(kind)
    return step(U, I, c.u, c.p, c.n, c.inv(kind))


# ---- the cases of test_gpu_bpr_pull_edges.py --------------------------------------------------------------------------

def ladder(D, N):
    g = GPW(D)
    out = []
    for k in (0, 1, g - 1, g, g + 1, 2 * g - 1, 2 * g + 1, HEAVY - 1, HEAVY, HEAVY + 1, 4 * g * N - 1, 4 * g * N + 1,
              8 * g * N + 1):
        if k not in out:
            out.append(k)
    return sorted(out, reverse=True)          # the longest rows on the first wave: unequal loads


def _user_rows(D, form):
    return {"narrow": 3 * R(D) - 1, "wide": NARROW_BELOW * R(D) - 3}[form]


def _ladder_case(D, form):
    """Row-length ladder on both sides: the ladder rows from row 0 on (more values than rows of a bucket go on into
    the next bucket, whose total then lies below DEAL_BAR), a bucket of 0 .. 3 records per row, a bucket without a
    record, and the ragged last bucket (with every row beyond) as filler."""
    rs = np.random.RandomState(_seed("ladder", D, form))
    r = R(D)
    nu = _user_rows(D, form)
    ru = Plan(1, nu, 1, D).RU

    def layout(rows, br, vals):
        c = np.zeros(rows, np.int64)
        c[:len(vals)] = vals
        a = -(-len(vals) // br) * br
        c[a:a + br] = np.resize([1, 2, 0, 3], br)
        return c, np.arange(a + 2 * br, rows)

    ni = (-(-len(ladder(D, 2)) // r) + 3) * r - 3
    cu, fu = layout(nu, ru, ladder(D, 1))
    ci, fi = layout(ni, r, ladder(D, 2))
    B = max(int(cu.sum()), int(ci[0::2].sum()), int(ci[1::2].sum())) + 2 * len(fi) + 5
    return Case(f"ladder-{D}-{form}", D, nu, ni, [stretch(rs, B, cu, ci, fu[:max(1, min(len(fu), 3 * r))], fi)])


def _chunk_totals_case(D, form):
    """Five buckets per side holding CAP - 1, CAP, CAP + 1, 2 CAP and 2 CAP + 1 records, unevenly over their rows."""
    rs = np.random.RandomState(_seed("chunks", D, form))
    r = R(D)
    nu = _user_rows(D, form) if form == "wide" else 7 * NARROW_ROWS - 1
    ru = Plan(1, nu, 1, D).RU
    ni = 7 * r - 3

    def fill(rows, br, cap):
        c = np.zeros(rows, np.int64)
        for k, tot in enumerate((cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1)):
            c[k * br:(k + 1) * br] = rs.multinomial(tot, rs.dirichlet(np.ones(br)))
        return c

    cu, ci = fill(nu, ru, CAP_USER), fill(ni, r, CAP_ITEM)
    B = max(int(cu.sum()), int(ci[0::2].sum()), int(ci[1::2].sum())) + 9
    return Case(f"chunktotals-{D}-{form}", D, nu, ni,
                [stretch(rs, B, cu, ci, np.arange(5 * ru, min(nu, 7 * ru)), np.arange(5 * r, ni))])


def _chunk_rows_case(D):
    """Bucket 0 of either side, tile by tile (tiles of 1,024 triplets): tile 0 brings 60 records on the rows of wave 0
    (a first chunk below DEAL_BAR at D = 64 in the deterministic mode, which cuts the chunk back to the tile boundary,
    and a first chunk favouring other rows than the later ones); tile 1 exactly CAP records, of which 60 on row
    R - 1 and 200 on row R - 2, the rest on the last RPW rows; tile 2 CAP + 1 records (a windowed segment in the
    deterministic mode) evenly; tile 3 again 60 on row R - 1 (light, light, above 96 in total) and 30 on row R - 2
    (heavy, then light); a short last tile."""
    rs = np.random.RandomState(_seed("chunkrows", D))
    r, rpw = R(D), RPW(D)
    nu, ni = _user_rows(D, "wide"), 3 * r - 3

    def tiles(rows, cap):
        out = []
        for t in range(5):
            c = np.zeros(rows, np.int64)
            if t == 0:
                c += spread(60, np.arange(rpw), rows)
            elif t == 1:
                c[r - 1], c[r - 2] = 60, 200
                c += spread(cap - 260, np.arange(r - rpw, r - 2) if rpw > 2 else np.arange(r - 4, r - 2), rows)
            elif t == 2:
                c += spread(cap + 1, np.arange(r), rows)
            elif t == 3:
                c[r - 1], c[r - 2] = 60, 30
            else:
                c[:r] = 1
            out.append(c)
        return out

    tu, ti = tiles(nu, CAP_USER), tiles(ni, CAP_ITEM)
    parts = [stretch(rs, 1024 if t < 4 else 300, tu[t], ti[t], np.arange(r, 3 * r), np.arange(r, ni)) for t in range(5)]
    return Case(f"chunkrows-{D}", D, nu, ni, parts)


def _uniform(rs, length, nu, ni, skip_bucket=None, D=None):
    rows_i = np.arange(ni)
    if skip_bucket is not None:
        rows_i = rows_i[rows_i // R(D) != skip_bucket]
    ev, od = rows_i[rows_i % 2 == 0], rows_i[rows_i % 2 == 1]
    return [rs.randint(0, nu, length), ev[rs.randint(0, len(ev), length)], od[rs.randint(0, len(od), length)]]


def _tile_case(B, D, nu, ni):
    rs = np.random.RandomState(_seed("tiles", B, D))
    return Case(f"tiles-{B}", D, nu, ni, [_uniform(rs, B, nu, ni)])


def _window_case():
    """B = 129,025: the first batch with tiles of 2,048 triplets.  In tile 0 the deterministic mode takes user bucket 0
    in windows of 768 triplet ids — 500 records in the first, none in the second, 300 in the third — and item bucket 0
    in windows of 512 ids: 600 occurrences, none, 500, none.  Segments of 800 > 768 and 1,100 > 1,024 records."""
    D = 64
    rs = np.random.RandomState(_seed("window"))
    r = R(D)
    nu, ni = _user_rows(D, "wide"), 64 * r - 3
    fu, fi = np.arange(r, 40 * r), np.arange(r, ni)
    parts = []
    for length, ku, ki in ((512, 500, 600), (512, 0, 0), (512, 0, 500), (512, 300, 0)):
        parts.append(stretch(rs, length, spread(ku, np.arange(r), nu), spread(ki, np.arange(r), ni), fu, fi))
    parts.append(_uniform(rs, 129025 - 2048, nu, ni))
    return Case("tiles-129025-windows", D, nu, ni, parts)


def _bad_case():
    D = 64
    rs = np.random.RandomState(_seed("bad"))
    nu, ni = 3 * R(D) - 1, 3 * R(D) - 3
    bad = [(2050, (nu, None, None)), (2100, (-1, None, None)), (2200, (None, ni, None)), (2300, (None, None, -5)),
           (2400, (None, 1 << 40, None)), (2499, (nu + 7, None, ni))]
    return Case("tiles-2500-bad", D, nu, ni, [_uniform(rs, 2500, nu, ni)], bad=bad)


def _scan_case(nbU, nbI):
    """D = 128, buckets of 8 rows, 3,000 triplets: the partition's scan with 1 and 2 counters per thread, the owner
    grids at and past their caps.  The last row of either table holds records."""
    D = 128
    rs = np.random.RandomState(_seed("scan", nbU, nbI))
    nu = 4 if nbU == 1 else nbU * 8 - 3
    ni = 5 if nbI == 1 else nbI * 8 - 3
    q = _uniform(rs, 3000, nu, ni)
    q[0][:7] = nu - 1
    last_even, last_odd = (ni - 1) - (ni - 1) % 2, (ni - 1) - (ni % 2)
    q[1][:5], q[2][:5] = last_even, last_odd
    for a in q:
        rs.shuffle(a)
    order = rs.permutation(nbI).astype(np.int32) if nbI == 8193 else None
    c = Case(f"scan-{nbU}-{nbI}", D, nu, ni, [q], order=order)
    assert (c.plan.nbU, c.plan.nbI) == (nbU, nbI)
    return c


SHARED_D, SHARED_NB = 64, 256


def _shared_case(name, B, hot, segs, D=SHARED_D, nbI=SHARED_NB, ranges=None):
    """hot: item buckets; segs: (length, {bucket: (positives, negatives)}) stretches; everything else falls evenly on
    the other buckets."""
    rs = np.random.RandomState(_seed("shared", name))
    r = R(D)
    nu, ni = 3 * r - 1, nbI * r - 3
    rows = np.arange(ni)
    cold = rows[~np.isin(rows // r, hot)]
    cold = cold[rs.permutation(len(cold))[:2048]]
    parts = []
    for length, put in segs:
        ci = np.zeros(ni, np.int64)
        for h, (kp, kn) in put.items():
            mine = rows[rows // r == h]
            ci += spread(kp, mine[mine % 2 == 0], ni) + spread(kn, mine[mine % 2 == 1], ni)
        parts.append(stretch(rs, length, np.zeros(nu, np.int64), ci, np.arange(nu), cold))
    c = Case(name, D, nu, ni, parts, ranges=ranges)
    assert c.B == B
    return c


def _overflow_case():
    """520 hot buckets of 2,100 records at D = 16, nbI = 2,048: each wants ceil(2100 / 1024) = 3 parts — 1,040 tasks
    and 1,560 slots against pools of 512 and 1,024."""
    D, nbI, hot_n, per = 16, 2048, 520, 1050
    rs = np.random.RandomState(_seed("overflow"))
    r = R(D)
    nu, ni = 3 * r - 1, nbI * r - 3
    hot = np.sort(rs.choice(nbI - 1, hot_n, replace=False))
    base = (hot * r)[:, None] + np.arange(0, r, 2)[None, :]             # the even rows of every hot bucket
    p = np.repeat(base.ravel(), -(-per // (r // 2)))
    p = np.concatenate([q[:per] for q in np.split(p, hot_n)])
    n = p + 1
    rs.shuffle(p)
    rs.shuffle(n)
    B = hot_n * per
    return Case("shared-overflow", D, nu, ni, [[rs.randint(0, nu, B), p, n]])


def _build_cases():
    cases = {}

    def add(c):
        cases[c.name] = c

    for D in WIDTHS:
        for form in ("narrow", "wide"):
            add(_ladder_case(D, form))
    for D, form in ((16, "wide"), (32, "narrow"), (64, "wide"), (128, "narrow")):
        add(_chunk_totals_case(D, form))
    for D in WIDTHS:
        add(_chunk_rows_case(D))
    r64, r32 = R(64), R(32)
    for B in (1, 1023, 1024, 1025):
        add(_tile_case(B, 64, 3 * r64 - 1, 3 * r64 - 3))
    for B in (65536, 65537):
        add(_tile_case(B, 32, 3 * r32 - 1, 8 * r32 - 3))
    add(_window_case())
    add(_tile_case(258049, 16, 3 * R(16) - 1, 32 * R(16) - 3))
    for B in (1048576, 1048577):
        add(_tile_case(B, 16, 4096, 4096))
    add(_bad_case())
    for nbU, nbI in ((1, 1), (1023, 1023), (1024, 1024), (1025, 1025), (2049, 2049), (2048, 4096), (4097, 4097),
                     (2049, 8193)):
        add(_scan_case(nbU, nbI))
    h = 100
    for k in (2047, 2048, 2049):
        add(_shared_case(f"shared-{k}", 3072, [h], [(3072, {h: (1024, k - 1024)})]))
    add(_shared_case("shared-4096-T2", 2048, [h], [(2048, {h: (2048, 2048)})]))
    add(_shared_case("shared-2048-T1", 1024, [h], [(1024, {h: (1024, 1024)})]))
    add(_shared_case("shared-65536", 65536, [h], [(65536, {h: (65536, 0)})]))
    add(_shared_case("shared-100000", 100000, [h], [(100000, {h: (100000, 0)})]))
    add(_shared_case("shared-firsthalf", 8192, [h], [(4096, {h: (2048, 2048)}), (4096, {})]))
    add(_shared_case("shared-ragged", 3072, [SHARED_NB - 1], [(3072, {SHARED_NB - 1: (1250, 1250)})]))
    r = R(SHARED_D)
    add(_shared_case("shared-two-ranges", 6144, [10, 200], [(6144, {10: (1250, 1250), 200: (1300, 1200)})],
                     ranges=[(0, 64 * r), (64 * r, 128 * r), (128 * r, SHARED_NB * r - 3)]))
    add(_overflow_case())
    return cases


@functools.lru_cache(maxsize=None)
def _cases():
    return _build_cases()


def case(name):
    return _cases()[name]


def case_names():
    return list(_cases())


# what every case is there for, stated on the arrays: (case, plan / sharing property) -> checked by both test files
def expectations(c):
    """The loop ends a case is meant to reach, computed from the helper's constants (asserted by the CPU file)."""
    pl = c.plan
    want, tasks, slots, holds = c.sharing()
    return dict(T=pl.T, tile=pl.tile, nbU=pl.nbU, nbI=pl.nbI, narrow=pl.narrow, tile_groups=pl.tile_groups,
                scan_per=pl.scan_per, user_trips=pl.user_trips, item_trips=pl.item_trips, parts_max=int(want.max()),
                tasks=tasks, slots=slots, pools_hold=holds)
