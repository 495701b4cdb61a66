"""Float64 restatement of the NGCF kernels (csrc/ngcf.hip) for the tests: the CSR products (pull, row subset, push
from a row list), the layer's dense part with both backward products, the layer-sum scores with their gradient and
the frontier sets.  Importable helper, no fixtures (like cdae_ref64.py); runs without a GPU.

Every floating output is an ``Out(v, n, s)``: the float64 value, the number of summed terms and the sum of their
magnitudes.  An f32 kernel that adds n terms in ANY order is off by at most (n + 1) 2^-24 s to first order; with the
factor 2 of margin of cdae_ref64.py the bar of an output is

    bar = max(project bar, 2 (n + 1) 2^-24 s),      project bar = rtol |v| + atol of PROJECT[kind]

(PROJECT holds the tolerances that tests/test_gpu_ngcf.py applies to the same entry points).  Where a kernel rounds
an operand before the product (A = Z + E, H = E * Z, dP = 0.01f * g) the product counts as two terms.  Leaky ReLU is
1-Lipschitz: the bar of P carries over to the layer's output unchanged.

Exactness.  ``exact(q, s)``: every term of an output is an integer multiple of one power of two q and s <= 2^24 q.
Every partial sum in any order is then a multiple of q below 2^24 q, i.e. an f32 number, and every product is an f32
number too: any order of f32 additions and fused multiply-adds gives the float64 value exactly, and the tests
demand equality.  q comes from the arrays themselves (``quantum``), never from what the generator meant to make.
The bar of a long random sum cannot see one dropped entry (tests/test_ngcf_ref64.py measures from where on); long
rows and long row sums are therefore judged on the exact inputs.
"""
import numpy as np
import scipy.sparse as sp

U24 = 2.0 ** -24
F32 = np.float32
SLOPE = float(F32(0.01))                     # kSlope of csrc/ngcf.hip, as the f32 number the kernels multiply by
WIDTHS = (16, 32, 64, 128)
WAVES = 4                                    # kWavesPerBlock
BLOCK = 256                                  # kBlock
UNROLL = 8                                   # kSpmmUnroll
HEAVY_BLOCKS = 256                           # kSpmmHeavyBlocks
LIGHT_BLOCKS = 65536                         # cap of the light rows' workgroups: 262,144 rows per trip
PUSH_PARTS, EXPAND_PARTS = 16, 8             # kPushParts, kExpandParts
PUSH_GRID, EXPAND_GRID, SCORE_GRID = 32768, 16384, 8192
SENTINEL = 7.25                              # pre-fill of buffers whose rows the contract leaves untouched


def G(D):
    """Neighbours per pass of a wave: lane groups of D / 4 lanes."""
    return 64 // (D // 4)


def R(D):
    """Neighbours per round: UNROLL passes in flight."""
    return UNROLL * G(D)


def T(D):
    """heavy_threshold of the ladder graphs: rows of more than T entries get a workgroup."""
    return 2 * R(D) + 1


def wrows(D):
    """WChunk<D>::ROWS: rows per staged chunk of ngcf_dense_bwd_weight_kernel."""
    return 4096 // D


def ladder(D):
    g, r = G(D), R(D)
    out = []
    for k in (0, 1, g - 1, g, g + 1, r - 1, r, r + 1, 2 * r, 2 * r + 1, T(D), T(D) + 1, 4 * r - 1, 4 * r, 4 * r + 1,
              8 * r + 1):
        if k not in out:
            out.append(k)
    return out


# ---- outputs, bars, certificates ------------------------------------------------------------------------------------

class Out:
    __slots__ = ("v", "n", "s")

    def __init__(self, v, n, s):
        self.v = np.asarray(v, np.float64)
        self.n = np.broadcast_to(np.asarray(n, np.float64), self.v.shape)
        self.s = np.broadcast_to(np.asarray(s, np.float64), self.v.shape)

    def __getitem__(self, k):
        return Out(self.v[k], self.n[k], self.s[k])

    def plus(self, y0):
        """The same sum accumulated into y0 (one more term)."""
        y0 = np.asarray(y0, np.float64)
        return Out(self.v + y0, self.n + 1.0, self.s + np.abs(y0))


# (rtol, atol) of the existing test of each entry point: test_spmm_matches_scipy,
# test_dense_layer_fwd_bwd_matches_oracle, test_frontier_and_subset_kernels (push)
PROJECT = {"spmm": (1e-4, 1e-5), "push": (1e-4, 1e-5), "fwd": (1e-4, 1e-5), "dz": (1e-4, 1e-4), "de": (1e-4, 1e-4),
           "dw": (1e-4, 2e-4)}


def bar(o, kind):
    rtol, atol = PROJECT[kind]
    return np.maximum(rtol * np.abs(o.v) + atol, 2.0 * (o.n + 1.0) * U24 * o.s)


def over(err, b):
    err = np.abs(np.asarray(err, np.float64))
    return np.where(err == 0, 0.0, err / np.maximum(b, 1e-300))


def ratio(got, o, kind):
    """max |got - v| / bar (0 for an empty output); NaN / inf in ``got`` give inf."""
    got = np.asarray(got, np.float64).reshape(o.v.shape)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    return float(over(got - o.v, bar(o, kind)).max())


def quantum(*arrays):
    """The largest power of two of which every entry of every array is an integer multiple (inf: all zero)."""
    q = np.inf
    for a in arrays:
        a = np.asarray(a, np.float64).ravel()
        a = a[a != 0]
        if a.size == 0:
            continue
        assert np.isfinite(a).all()
        m, e = np.frexp(a)
        i = np.round(np.abs(m) * 2.0 ** 53).astype(np.int64)
        q = min(q, float(np.ldexp((i & -i).astype(np.float64), e - 53).min()))
    return q


def exact(terms_quantum, sum_abs):
    """True when sums of integer multiples of ``terms_quantum`` whose magnitudes add up to ``sum_abs`` are exact in
    f32 in any order."""
    sum_abs = np.asarray(sum_abs, np.float64)
    if sum_abs.size == 0 or not np.any(sum_abs):
        return True
    if not np.isfinite(terms_quantum) or terms_quantum <= 0:
        return False
    l2 = np.log2(terms_quantum)
    return bool(l2 == np.round(l2) and sum_abs.max() <= 2.0 ** 24 * terms_quantum)


# ---- the operations -------------------------------------------------------------------------------------------------

def _csr(rowptr, col, val, ncols, weight=None):
    val = np.asarray(val, np.float64)
    if weight is not None:
        val = val * weight
    rowptr = np.asarray(rowptr, np.int64)
    return sp.csr_matrix((val, np.asarray(col, np.int64), rowptr), shape=(len(rowptr) - 1, ncols))


def spmm(rowptr, col, val, X, accumulate_into=None, rows=None, weight=None):
    """Y = L X (+ accumulate_into).  ``rows`` (indices or a boolean mask): only those rows are computed, the others
    keep accumulate_into (NaN without one).  ``weight`` [nnz] multiplies the entries (0: dropped, 2: taken twice)."""
    X = np.asarray(X, np.float64)
    M = _csr(rowptr, col, val, X.shape[0], weight)
    v, s = M @ X, abs(M) @ np.abs(X)
    n = np.diff(np.asarray(rowptr, np.int64)).astype(np.float64)[:, None]
    o = Out(v, n, s)
    if accumulate_into is not None:
        o = o.plus(accumulate_into)
    if rows is not None:
        on = np.zeros(M.shape[0], bool)
        on[np.asarray(rows)] = True
        keep = np.full_like(o.v, np.nan) if accumulate_into is None else np.asarray(accumulate_into, np.float64)
        o = Out(np.where(on[:, None], o.v, keep), o.n, o.s)
    return o


def push_rows(rowptr, col, val, X, Y0, rows, weight=None):
    """Y[j] = Y0[j] + sum over the listed r of L[r, j] X[r] for any CSR (a row listed twice counts twice)."""
    X = np.asarray(X, np.float64)
    M = _csr(rowptr, col, val, X.shape[0], weight)
    mult = np.bincount(np.asarray(rows, np.int64), minlength=M.shape[0]).astype(np.float64)
    Ms = sp.diags(mult) @ M
    n = np.asarray(abs(sp.diags(mult) @ (M != 0).astype(np.float64)).sum(0)).ravel()[:, None]
    return Out(Ms.T @ X, n, abs(Ms).T @ np.abs(X)).plus(Y0)


def dense_fwd(E, Z, W1, W2):
    """(Eout, P): Eout = leaky_relu(P), P = (Z + E) W1^T + (E * Z) W2^T with A and H formed in float64."""
    E, Z, W1, W2 = (np.asarray(a, np.float64) for a in (E, Z, W1, W2))
    A, H = Z + E, E * Z
    P = A @ W1.T + H @ W2.T
    s = np.abs(A) @ np.abs(W1).T + np.abs(H) @ np.abs(W2).T
    n = 4.0 * E.shape[1]                                  # 2 D products, each with an operand the kernel rounded
    return Out(np.where(P > 0, P, SLOPE * P), n, s), Out(P, n, s)


def fwd_expected32(P):
    """What the kernel stores for an exactly computed P: P, or float32(0.01) * float32(P) in one rounding."""
    P32 = np.asarray(P, np.float64).astype(F32)
    return np.where(P32 > 0, P32, F32(0.01) * P32).astype(F32)


def dense_bwd(dEout, Eout, E, Z, W1, W2, dE0, rows=None):
    """(dZ, dE, dW1, dW2).  dP = dEout where the given Eout > 0, else 0.01f dEout; [dA | dH] = dP [W1 | W2];
    dZ = dA + dH E; dE = dE0 + dA + dH Z; dW1 = dP^T (Z + E); dW2 = dP^T (E Z).  ``rows``: the list form — only
    listed rows are summed into dW and updated (a row listed twice counts twice); dZ of the others is NaN."""
    g, Eo, E, Z, W1, W2, dE0 = (np.asarray(a, np.float64) for a in (dEout, Eout, E, Z, W1, W2, dE0))
    nrow, D = E.shape
    mult = np.ones(nrow) if rows is None else np.bincount(np.asarray(rows, np.int64), minlength=nrow).astype(np.float64)
    dP = np.where(Eo > 0, g, SLOPE * g)
    dA, dH = dP @ W1, dP @ W2
    sA, sH = np.abs(dP) @ np.abs(W1), np.abs(dP) @ np.abs(W2)
    m = mult[:, None]
    dZ = Out(np.where(m > 0, dA + dH * E, np.nan), 4.0 * D + 2.0, sA + sH * np.abs(E))
    upd = dA + dH * Z
    dE = Out(dE0 + m * upd, 4.0 * D + 3.0, np.abs(dE0) + m * (sA + sH * np.abs(Z)))
    A, H = Z + E, E * Z
    wP = dP * m
    nw = 2.0 * mult.sum()
    dW1 = Out(wP.T @ A, nw, np.abs(wP).T @ np.abs(A))
    dW2 = Out(wP.T @ H, nw, np.abs(wP).T @ np.abs(H))
    return dZ, dE, dW1, dW2


def _valid(num_users, num_items, u, p, n):
    ok = (u >= 0) & (u < num_users) & (p >= 0) & (p < num_items)
    if n is not None:
        ok &= (n >= 0) & (n < num_items)
    return ok


def score(layers, num_users, u, p, n=None):
    """(pos, neg or None): the dot products of the concatenated layer rows (models/ngcf.py:44-58); a triplet with
    an out-of-range id scores 0."""
    cat = np.concatenate([np.asarray(E, np.float64) for E in layers], axis=1)
    u, p = np.asarray(u, np.int64), np.asarray(p, np.int64)
    n = None if n is None else np.asarray(n, np.int64)
    ok = _valid(num_users, cat.shape[0] - num_users, u, p, n)
    uu = np.where(ok, u, 0)

    def dots(i):
        t = cat[uu] * cat[num_users + np.where(ok, i, 0)] * ok[:, None]
        return Out(t.sum(1), cat.shape[1], np.abs(t).sum(1))
    return dots(p), (None if n is None else dots(n))


def score_bwd(layers, num_users, u, p, n, gpos, gneg, weight=None):
    """One Out per layer: the gradient of the scores with respect to the layer rows, summed over the batch
    (``weight`` [B]: 0 drops a triplet); out-of-range triplets are skipped."""
    cat = np.concatenate([np.asarray(E, np.float64) for E in layers], axis=1)
    u, p = np.asarray(u, np.int64), np.asarray(p, np.int64)
    n = None if n is None else np.asarray(n, np.int64)
    ok = _valid(num_users, cat.shape[0] - num_users, u, p, n)
    w = ok.astype(np.float64) if weight is None else ok * np.asarray(weight, np.float64)
    u, p = u[ok], p[ok]
    gp = (np.asarray(gpos, np.float64) * w)[ok][:, None]
    d, s, c = np.zeros_like(cat), np.zeros_like(cat), np.zeros((cat.shape[0], 1))

    def add(at, g, src):
        nonlocal d, s, c
        S = sp.csr_matrix((np.ones(len(at)), (at, np.arange(len(at)))), shape=(cat.shape[0], len(at)))
        t = g * cat[src]
        d, s, c = d + S @ t, s + S @ np.abs(t), c + np.asarray(S.sum(1))
    add(u, gp, num_users + p); add(num_users + p, gp, u)
    if n is not None:
        n = n[ok]
        gn = (np.asarray(gneg, np.float64) * w)[ok][:, None]
        add(u, gn, num_users + n); add(num_users + n, gn, u)
    D = np.asarray(layers[0]).shape[1]
    return [Out(d[:, k * D:(k + 1) * D], c, s[:, k * D:(k + 1) * D]) for k in range(len(layers))]


def frontier_mark(num_users, num_items, u, p, n=None):
    """int32 flags [num_users + num_items]: the rows a batch's scores read; out-of-range ids are skipped one by one."""
    f = np.zeros(num_users + num_items, np.int32)
    u, p = np.asarray(u, np.int64), np.asarray(p, np.int64)
    f[u[(u >= 0) & (u < num_users)]] = 1
    f[num_users + p[(p >= 0) & (p < num_items)]] = 1
    if n is not None:
        n = np.asarray(n, np.int64)
        f[num_users + n[(n >= 0) & (n < num_items)]] = 1
    return f


def frontier_expand(rowptr, col, rows_in, flags0=None):
    """flags0 (or nothing) + the listed rows + all their neighbours, as int32 flags."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    f = np.zeros(len(rowptr) - 1, np.int32) if flags0 is None else np.array(flags0, np.int32)
    for r in np.asarray(rows_in, np.int64):
        f[r] = 1
        f[col[rowptr[r]:rowptr[r + 1]]] = 1
    return f


# ---- inputs ---------------------------------------------------------------------------------------------------------

def rand_mag(rs, shape):
    """f32 magnitudes in [0.5, 2] with random signs: no term of a sum is negligible."""
    return ((0.5 + 1.5 * rs.rand(*shape)) * rs.choice([-1.0, 1.0], size=shape)).astype(F32)


def ints(rs, shape, hi, nonzero=False):
    a = rs.randint(-hi, hi + 1, size=shape).astype(F32)
    if nonzero:
        a[a == 0] = 1.0
    return a


def eighths(rs, shape):
    return (rs.randint(-8, 9, size=shape) / 8.0).astype(F32)


def csr_values(rs, k, exact_inputs):
    if exact_inputs:
        return (rs.choice([-1.0, 1.0], size=k) * 2.0 ** -rs.randint(1, 5, size=k)).astype(F32)
    return rand_mag(rs, (k,))


def features(rs, shape, exact_inputs):
    return ints(rs, shape, 3) if exact_inputs else rand_mag(rs, shape)


def csr_with_lengths(rs, lengths, ncols, exact_inputs, symmetric=False):
    """(rowptr int64, col int32, val f32) with exactly lengths[r] entries in row r, distinct sorted columns.
    ``symmetric``: the closure L + L^T of the pattern with L[i, j] = L[j, i] (the row lengths then grow)."""
    lengths = np.asarray(lengths, np.int64)
    assert lengths.max(initial=0) <= ncols
    rowptr = np.concatenate([[0], np.cumsum(lengths)])
    col = np.empty(rowptr[-1], np.int32)
    short = lengths <= 2
    # rows of at most two entries (the 262,181-row graph) without a Python loop: c, c + 1 + d mod ncols
    c1 = rs.randint(0, ncols, len(lengths))
    c2 = (c1 + 1 + rs.randint(0, max(ncols - 1, 1), len(lengths))) % ncols
    lo, hi = np.minimum(c1, c2), np.maximum(c1, c2)
    one = short & (lengths == 1)
    two = short & (lengths == 2)
    col[rowptr[:-1][one]] = c1[one]
    col[rowptr[:-1][two]] = lo[two]
    col[rowptr[:-1][two] + 1] = hi[two]
    for r in np.flatnonzero(~short):
        col[rowptr[r]:rowptr[r + 1]] = np.sort(rs.choice(ncols, lengths[r], replace=False))
    val = csr_values(rs, int(rowptr[-1]), exact_inputs)
    if symmetric:
        assert ncols == len(lengths)
        M = sp.csr_matrix((val.astype(np.float64), col, rowptr), shape=(ncols, ncols))
        up, low = sp.triu(M, 1).tocsr(), sp.triu(M.T, 1).tocsr()
        up = up + low - low.multiply(up != 0)                                # the upper entry wins where both exist
        M = (up + up.T + sp.diags(M.diagonal())).tocsr()
        M.sort_indices()
        M.eliminate_zeros()
        return M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data.astype(F32)
    return rowptr, col, val


# ---- cases of tests/test_gpu_ngcf_edges.py (built identically by the CPU checks of tests/test_ngcf_ref64.py) ---------

SPMM_KINDS = ("ladder", "heavy300", "n1", "n3", "n4", "n5")
BIG_ROWS = 4 * LIGHT_BLOCKS + 37                       # one trip of the light rows' loop is 262,144 rows


def spmm_case(D, kind, exact_inputs):
    """dict(rowptr, col, val, X, Y0, heavy_threshold, marked): ``marked`` maps a ladder length to its row."""
    rs = np.random.RandomState(WIDTHS.index(D) * 100 + SPMM_KINDS.index(kind) if kind in SPMM_KINDS else 977)
    marked = {}
    if kind == "ladder":
        lad = ladder(D)
        n = max(lad[-1] + 64, 320 + len(lad))
        lengths = rs.randint(0, 13, n)
        lengths[rs.rand(n) < 0.15] = 0                                       # empty filler rows
        at = np.sort(rs.choice(n, len(lad), replace=False))
        at[0], at[-1] = 0, n - 1                                             # the first and the last row carry one too
        for r, k in zip(at, lad):
            lengths[r] = k
            marked[k] = int(r)
    elif kind == "heavy300":
        n = max(T(D) + 3, 300) + 20
        lengths = rs.randint(0, 9, n)
        at = np.sort(rs.choice(n, 300, replace=False))
        lengths[at] = T(D) + 1 + rs.randint(0, 3, 300)
    elif kind == "big":
        n = BIG_ROWS
        lengths = rs.randint(0, 3, n)
    else:
        n = int(kind[1:])
        lengths = rs.randint(0, n + 1, n)
        lengths[-1] = n                                                      # the last row is full
    rowptr, col, val = csr_with_lengths(rs, lengths, n, exact_inputs)
    return dict(rowptr=rowptr, col=col, val=val, X=features(rs, (n, D), exact_inputs),
                Y0=features(rs, (n, D), exact_inputs), heavy_threshold=T(D), marked=marked, n=n)


def spmm_subsets(case, rs):
    """Row sets for yr_spmm_csr_subset: a mixed one (every second ladder row, so heavy rows fall on both sides, and a
    third of the rest) and the empty one."""
    n = case["n"]
    on = rs.rand(n) < 0.33
    for i, r in enumerate(sorted(case["marked"].values())):
        on[r] = i % 2 == 0
    deg = np.diff(case["rowptr"])
    heavy = np.flatnonzero(deg > case["heavy_threshold"])
    if len(heavy) >= 2:
        on[heavy[::2]], on[heavy[1::2]] = True, False
    return {"mixed": on, "empty": np.zeros(n, bool)}


def spmm_perturbations(case, D):
    """{name: weight vector over the non-zeros} — what a kernel that mishandles a row end would compute."""
    rowptr = case["rowptr"]
    out = {}
    one = np.ones(int(rowptr[-1]))
    g = G(D)
    for k, r in case["marked"].items():
        lo, hi = int(rowptr[r]), int(rowptr[r + 1])
        if k == 0:
            continue
        w = one.copy(); w[hi - 1] = 0.0; out[(k, "last entry dropped")] = (r, w)
        w = one.copy(); w[hi - 1] = 2.0; out[(k, "last entry twice")] = (r, w)
        npass = (k + g - 1) // g
        w = one.copy(); w[lo + (npass - 1) // 2 * g:min(hi, lo + ((npass - 1) // 2 + 1) * g)] = 0.0
        out[(k, "one pass dropped")] = (r, w)
        if k > case["heavy_threshold"]:
            idx = np.arange(k)
            w = one.copy(); w[lo + idx[(idx // g) % WAVES == WAVES - 1]] = 0.0
            out[(k, "fourth wave's share dropped")] = (r, w)
    return out


DENSE_N = (1, 31, 32, 33, 64, 65, 333)


def dw_sizes(D):
    """(n, large) of the ngcf_dense_bwd_weight cases: chunk edges, two chunks per workgroup with a short last
    workgroup, three chunks per workgroup with a one-row last chunk."""
    r = wrows(D)
    return [(r - 1, False), (r, False), (r + 1, False), (2 * r + 1, False), (600 * r + 5, True), (1025 * r + 1, True)]


def dense_case(D, n, exact_inputs, seed=0):
    """E, Z, W1, W2, dEout, dE0, dW10, dW20 and Eout: the f32 array BOTH the kernel and the reference read in the
    backward pass (the reference's forward, rounded), so the leaky-ReLU kink never sits between them."""
    rs = np.random.RandomState(5000 + 7 * D + n % 9973 + 2 * seed + int(exact_inputs))
    if exact_inputs:
        E, Z = ints(rs, (n, D), 3), ints(rs, (n, D), 3)
        W1, W2 = eighths(rs, (D, D)), eighths(rs, (D, D))
        dEout, dE0 = ints(rs, (n, D), 2), ints(rs, (n, D), 3)
        dW10, dW20 = ints(rs, (D, D), 3), ints(rs, (D, D), 3)
    else:
        E, Z = rand_mag(rs, (n, D)), rand_mag(rs, (n, D))
        W1, W2 = (rand_mag(rs, (D, D)) / F32(np.sqrt(D))).astype(F32), (rand_mag(rs, (D, D)) / F32(np.sqrt(D))).astype(F32)
        dEout, dE0 = rand_mag(rs, (n, D)), rand_mag(rs, (n, D))
        dW10, dW20 = rand_mag(rs, (D, D)), rand_mag(rs, (D, D))
    out, P = dense_fwd(E, Z, W1, W2)
    Eout = fwd_expected32(P.v) if exact_inputs else out.v.astype(F32)
    if exact_inputs:
        dEout = np.where(Eout > 0, dEout, F32(0)).astype(F32)        # 0.01f is not dyadic: no gradient on the negative side
    return dict(E=E, Z=Z, W1=W1, W2=W2, dEout=dEout, dE0=dE0, dW10=dW10, dW20=dW20, Eout=Eout, n=n)


LIST_N = 150
# (count, max_rows) of the row-list forms of the dense kernels
LIST_CASES = [(0, 0), (1, 1), (31, 31), (32, 32), (33, 33), (100, 100), (100, 1), (100, 32)]


def row_list(n, count, seed):
    """count distinct rows in random order, row 0 and row n - 1 among them (count >= 2), n - 1 alone (count = 1)."""
    rs = np.random.RandomState(77 + count + 13 * seed)
    if count == 0:
        return np.zeros(0, np.int32)
    if count == 1:
        return np.array([n - 1], np.int32)
    rows = np.concatenate([[0, n - 1], 1 + rs.choice(n - 2, count - 2, replace=False)])
    return rs.permutation(rows).astype(np.int32)


def dw_list_cases(D):
    """(n, count, max_rows) of yr_ngcf_dense_bwd_weight_rows: one workgroup over four chunks; a grid of two."""
    r = wrows(D)
    return [(3 * r + 20, 3 * r + 7, r), (5 * r + 14, 5 * r + 1, 2 * r)]


def push_lengths(D):
    g = G(D)
    return [0, 1, 15, 16, 17, PUSH_PARTS * WAVES * g + 1, PUSH_PARTS * UNROLL * g + 5]


PUSH_N = 2300
LONG_LIST = 2100                                         # more than 32768 / 16 and than 16384 / 8 listed rows


def push_case(D, exact_inputs):
    """A graph whose first rows have push_lengths(D) entries; lists: those rows alone, and 2,100 rows with them."""
    rs = np.random.RandomState(300 + D + int(exact_inputs))
    special = push_lengths(D)
    lengths = rs.randint(0, 21, PUSH_N)
    lengths[:len(special)] = special
    rowptr, col, val = csr_with_lengths(rs, lengths, PUSH_N, exact_inputs)
    X, Y0 = features(rs, (PUSH_N, D), exact_inputs), features(rs, (PUSH_N, D), exact_inputs)
    rs = np.random.RandomState(D)                                            # the same lists for both kinds of input
    few = rs.permutation(len(special) + 3).astype(np.int32)
    many = rs.permutation(np.concatenate([np.arange(len(special)),
                                          len(special) + rs.choice(PUSH_N - len(special), LONG_LIST - len(special),
                                                                   replace=False)])).astype(np.int32)
    return dict(rowptr=rowptr, col=col, val=val, X=X, Y0=Y0, lists={"few": few, "many": many}, special=special,
                n=PUSH_N)


EXPAND_LENGTHS = [0, 1, 7, 8, 9, EXPAND_PARTS * BLOCK + 3]
EXPAND_N = 6000


def expand_case():
    """A sparse pattern whose first rows have EXPAND_LENGTHS entries; the other rows 0 - 2 (so that 2,100 rows and
    their neighbours do not cover the graph)."""
    rs = np.random.RandomState(41)
    lengths = rs.randint(0, 3, EXPAND_N)
    lengths[:len(EXPAND_LENGTHS)] = EXPAND_LENGTHS
    rowptr, col, _ = csr_with_lengths(rs, lengths, EXPAND_N, True)
    k = len(EXPAND_LENGTHS)
    few = rs.permutation(k).astype(np.int32)
    many = rs.permutation(np.concatenate([np.arange(k), k + rs.choice(EXPAND_N - k, LONG_LIST - k, replace=False)]))
    return dict(rowptr=rowptr, col=col, lists={"few": few, "many": many.astype(np.int32)}, n=EXPAND_N)


SCORE_USERS, SCORE_ITEMS = 370, 530


def score_batches(D):
    g = G(D)
    return [g - 1, g, g + 1, WAVES * g + 1]


BIG_SCORE = (128, 2, 65601)                              # D, layers, B: past 8192 workgroups of 4 x 2 triplets


def score_case(D, layers, B, with_neg, same_user=False):
    """Integer layers (|.| <= 3) and integer score gradients (|.| <= 2): every sum is exact."""
    rs = np.random.RandomState(9000 + D + 17 * layers + B % 1009 + int(with_neg) + 2 * int(same_user))
    Es = [ints(rs, (SCORE_USERS + SCORE_ITEMS, D), 3) for _ in range(layers)]
    u = rs.randint(0, SCORE_USERS, B).astype(np.int64)
    if same_user:
        u[:] = 11
    p = rs.randint(0, SCORE_ITEMS, B).astype(np.int64)
    n = rs.randint(0, SCORE_ITEMS, B).astype(np.int64) if with_neg else None
    return dict(layers=Es, u=u, p=p, n=n, gpos=ints(rs, (B,), 2, nonzero=True),
                gneg=ints(rs, (B,), 2, nonzero=True) if with_neg else None)
