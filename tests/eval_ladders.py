"""Evaluation cases whose float64 top-k lists are CERTIFIED: every correct fused evaluation must return them exactly.

Error bound.  For user u and item j let A(u, j) = sum_d |u_d i_jd| + |b_j| (float64, from the f32 tables).  A correct
kernel computes the score s(u, j) = u . i_j + b_j to within

    eps(u, j) = c_D A(u, j),    c_D = gamma_{D+1} + 2^-24 + 2^-34 + 4 u,    u = 2^-24,
    gamma_n = n u / (1 - n u);   c_D = 1.31e-6, 2.27e-6, 4.17e-6, 7.99e-6 at D = 16, 32, 64, 128,

made of:
  * f32 accumulation of the D products and the bias, in any order: gamma_{D+1} A.  The f32 matrix instruction is an
    f32 fma chain (one rounding per product, the bias as the accumulator's start); the bf16 form
    (csrc/eval_topk.hip, SPLIT) adds the exact bf16 x bf16 partial products of a 16-deep block in one matrix
    instruction, six instructions per block: 3 D / 8 accumulator roundings, fewer than D.  The hint rescoring is a
    plain f32 dot product (D / 16 + 4 roundings).  None exceeds D + 1.  ASSUMED, not proven here: round-to-nearest
    at every f32 accumulation, and at most one rounding of the accumulator per bf16 matrix instruction (a one-off
    probe on gfx950 agreed: sixteen products of 2^-25 added to 1.0 gave exactly 1 + 2^-21).  The ladders' gaps
    (1.5 - 4 times eps_a + eps_b) are the headroom left to a kernel whose arithmetic is worse than this model.
  * the bf16x3 split (et_split3): x = x1 + x2 + x3 exactly for normal f32 x (|x2| <= 2^-8 |x|, |x3| <= 2^-17 |x|),
    and the six kept partial products leave out x2 y3, x3 y2 (each below 2^-25 |x y|) and x3 y3 (below 2^-34 |x y|):
    2^-24 + 2^-34 of A at most.
  * 4 u of slack: the float64 reference's own rounding (below D 2^-53 A) and the f32 rounding of a bias-only or
    masked start of the accumulator, with room to spare; it keeps a certified gap a few ulp wide at the smallest A.
Masked items score the mask value (as f32) exactly: eps = 0.

Reference.  Expected lists are the float64 scores ordered by (-score, id); masked items carry float32(mask_value)
and order by ascending id among themselves, as oracle/mf_eval.py and csrc/topk.hip order them.

Certificate.  A case is certified when, in every row, every adjacent pair (a, b) among the first k + 1 expected
entries satisfies s_a - s_b > eps_a + eps_b, and every item j beyond the first k satisfies s_k - eps_k > s_j + eps_j
against the k-th entry — or, in either test, the two scores are equal in EVERY correct kernel: bitwise-identical
item rows with the same bias, items whose score is exact in any arithmetic (all-zero item rows with a zero bias:
0.0; masked items: the mask value), ordered by id.  build_case() asserts the certificate on every case it returns.

Ladders.  Every evaluated row belongs to a family; a family owns k + 8 planted items (fewer when the catalogue is
smaller) whose scores against the family's user descend with gaps rho (eps_a + eps_b), rho mostly in [1.5, 4]
(one family per case at rho ~ 64).  Family directions are orthonormal, the planted items full-mantissa f32 (all three
bf16 planes non-zero), a carrier coordinate sets each score; exact scores are recomputed after the rounding to f32
and certified (every pair of adjacent places among the first k + 1, and every item beyond the list against the k-th
place).  Distractors score far below.  Planted items sit first at awkward catalogue positions: first and last item of
a 32-item tile and of a 64-item stage, catalogue-slice boundaries, the ragged last tile — or, with prescan_place, the
cancellation families and one plain family at k different offsets of tiles the prescan scores (_prescan_slots), so
that the prescan's bound is the k-th score itself.  Family kinds:
  plain / wide   ladders as above;
  ties           duplicate item rows: one pair straddles the k-th place, one at the top;
  cancel+ / cancel0 / cancel-   cancellation: |s| << A (A / |s| >= 1e3 at the k-th place), the k-th score positive,
                 exactly 0.0 (all-zero item rows), negative.  Three gate coordinates (0, 1, 2) push every other item
                 far below for these users;
  bias           the ladder carried by the item bias, all items of the ladder with the same vector (CDAE decoder).
Rows of a family are the family's user times 2^e, e in [-10, 10] (scales 1e-3 .. 1e3: exactly scaled arithmetic;
without item bias),
and mask lists remove ladder members (the best one, the one at the k-th place, several) together with random
distractors across the whole catalogue.
"""
import numpy as np

MASK_VALUE = -3.40282e+38          # yelprecommendation_amd/engine.py MASK_VALUE (the reference's)
MASK_VALUES = (MASK_VALUE, 0.0, -1e30)
U_ROUND = 2.0 ** -24
NGATES = 3                         # gate coordinates of the cancellation families


def c_bound(D):
    n = D + 1
    return n * U_ROUND / (1 - n * U_ROUND) + 2.0 ** -24 + 2.0 ** -34 + 4 * U_ROUND


C_D = {D: c_bound(D) for D in (16, 32, 64, 128)}


# ---- the split arithmetic (csrc/eval_topk.hip et_split3), restated as in test_host_logic.py ----
def bf16(x):
    """f32 -> nearest-even bfloat16, returned as f32."""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7fff + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32)


def split3(x):
    x = np.asarray(x, np.float32)
    x1 = bf16(x)
    r1 = (x - x1).astype(np.float32)
    x2 = bf16(r1)
    x3 = bf16((r1 - x2).astype(np.float32))
    return x1, x2, x3


# ---- slices the library cuts the catalogue into (csrc/eval_topk.hip et_slices / et_pp_slices) ----
def slice_starts(nrows, num_items):
    out = set()
    for users_per_wg, target in ((128, 768), (256, 256)):
        rows = (nrows + users_per_wg - 1) // users_per_wg
        S = max(1, min(target // rows, num_items // 2048, 24))
        per = -(-num_items // S)
        per = -(-per // 32) * 32
        out.update(range(per, num_items, per))
    return sorted(out)


def prescan_tiles(N, D):
    """Starts of the 32-item tiles the prescan scores whole in both precisions (csrc/eval_topk.hip et_launch: every
    stride-th stage of CHP items; CHP = 64 for f32 and for the split form at D <= 32, else 32)."""
    both = None
    for chp in {64, 64 if D <= 32 else 32}:
        chunks = -(-N // chp)
        sample = min(4096, max(chp, N // 8))
        stride = max(1, chunks // max(1, sample // chp))
        items = {c * chp + o for c in range(0, chunks, stride) for o in range(chp)}
        both = items if both is None else both & items
    return [t for t in range(0, N - 31, 32) if all(t + o in both for o in range(32))]


def _prescan_slots(D, N, kinds, L, n_zero):
    """(family, q) / ("zero", z) -> catalogue position: the cancellation families and the first plain one put ladder
    item q at offset q mod 30 of a tile the prescan scores, the zero rows at offsets 30 and 31 — the top k of such a
    family (k <= 30) lie in k different group maxima of the prescan (one per accumulator register and half-wave, that
    is per offset in the tile), so the prescan's bound is the k-th score itself."""
    T = prescan_tiles(N, D)
    placed = [f for f, kind in enumerate(kinds) if kind.startswith("cancel")] + [kinds.index("plain")]
    out, used = {}, set()
    if not T:
        return out
    for z in range(n_zero):
        out[("zero", z)] = T[0] + 30 + z
        used.add(T[0] + 30 + z)
    for i, f in enumerate(placed):
        for q in range(L):
            p = T[(1 + i + (q // 30) * len(placed)) % len(T)] + q % 30
            if p not in used:
                out[(f, q)] = p
                used.add(p)
    return out


def awkward_positions(nrows, num_items, rs):
    """First / last item of every 32-item tile and 64-item stage, the slice boundaries (and their neighbours), the
    ragged last tile — shuffled, the last tile and slice boundaries first."""
    last = list(range(num_items // 32 * 32, num_items)) if num_items % 32 else [num_items - 1]
    sl = [p + o for p in slice_starts(nrows, num_items) for o in (-1, 0)]
    tiles = [p for t in range(0, num_items, 32) for p in (t, t + 31) if p < num_items]
    first = list(dict.fromkeys(last + sl))
    seen = set(first)
    rest = [p for p in tiles if p not in seen]
    rs.shuffle(first)
    rs.shuffle(rest)
    return list(dict.fromkeys(first + rest))


class Case:
    """U [num_users, D], I [N, D], bias [N] or None (f32); users [n]; mask CSR (ascending ids); expected[mv] [n, k]
    for every mask value; score / A helpers in float64 (duplicate item rows take the values of the row they copy,
    rep)."""

    def scores64(self, rows=None, mask_value=None):
        rows = np.arange(len(self.users)) if rows is None else np.asarray(rows)
        U = self.U.astype(np.float64)[self.users[rows]]
        S = (U @ self.I.astype(np.float64).T)[:, self.rep]   # (a matrix product may round equal rows differently)
        if self.bias is not None:
            S += self.bias.astype(np.float64)[None, :]
        if mask_value is not None:
            for r_out, r in enumerate(rows):
                S[r_out, self.masks[r]] = float(np.float32(mask_value))
        return S

    def scale64(self, rows):
        A = (np.abs(self.U.astype(np.float64)[self.users[rows]]) @ np.abs(self.I.astype(np.float64)).T)[:, self.rep]
        if self.bias is not None:
            A += np.abs(self.bias.astype(np.float64))[None, :]
        return A


def order_rows(S, k):
    """Top k of every row of a score matrix: descending score, ascending id among equal scores."""
    n, N = S.shape
    out = np.empty((n, k), np.int64)
    for r in range(n):
        s = S[r]
        kth = np.partition(-s, k - 1)[k - 1]          # -(k-th largest)
        cand = np.flatnonzero(-s <= kth)
        o = np.lexsort((cand, -s[cand]))
        out[r] = cand[o[:k]]
    return out


def _exact_pair(case, r, a, b, masked):
    """Scores equal in every correct kernel: identical rows + bias, or both exact (masked / zero rows, zero bias)."""
    def exact(j):
        return j in masked or (case.zero_row[j] and (case.bias is None or case.bias[j] == 0))
    if exact(a) and exact(b):
        return True
    same = np.array_equal(case.I[a], case.I[b]) and (case.bias is None or case.bias[a] == case.bias[b])
    return same and not (a in masked) and not (b in masked)


def certify(case, mask_value, chunk=512):
    """Expected [n, k] lists for this mask value; asserts the certificate (see the module docstring)."""
    k, c = case.k, C_D[case.D]
    n = len(case.users)
    out = np.empty((n, k), np.int64)
    for r0 in range(0, n, chunk):
        rows = np.arange(r0, min(n, r0 + chunk))
        S = case.scores64(rows, mask_value)
        top = order_rows(S, k + 1)
        out[rows] = top[:, :k]
        A = case.scale64(rows)
        for q, r in enumerate(rows):
            ids = top[q]
            masked = set(case.masks[r].tolist())
            s = S[q, ids]
            eps = np.array([0.0 if j in masked else c * A[q, j] for j in ids])
            for e in range(k):
                a, b = ids[e], ids[e + 1]
                if s[e] == s[e + 1] and _exact_pair(case, r, a, b, masked):
                    assert a < b
                    continue
                assert s[e] - s[e + 1] > eps[e] + eps[e + 1], \
                    f"row {r}: places {e}/{e + 1} (items {a}, {b}) not certified: gap {s[e] - s[e + 1]:.3e}, " \
                    f"eps {eps[e]:.3e} + {eps[e + 1]:.3e}"
            # nothing beyond the list, whatever its A, can overtake the k-th entry
            eps_all = c * A[q]
            eps_all[case.masks[r]] = 0.0
            beyond = np.ones(S.shape[1], bool)
            beyond[ids[:k]] = False
            kth = ids[k - 1]
            for j in np.flatnonzero(beyond & (S[q] + eps_all >= s[k - 1] - eps[k - 1])):
                assert S[q, j] == s[k - 1] and _exact_pair(case, r, kth, j, masked) and kth < j, \
                    f"row {r}: item {j} beyond the list may overtake the k-th entry {kth}"
    return out


def _kinds(k, bias):
    kinds = ["plain", "wide", "ties", "cancel+", "cancel0", "cancel-", "plain"]
    if bias:
        kinds.insert(3, "bias")
    return kinds


def build_case(D, N, nrows, k, bias=False, seed=0, mask_values=MASK_VALUES, rho=(1.5, 4.0), slice_rows=None,
               distractor_scale=0.3, prescan_place=False):
    """A certified evaluation case (see the module docstring).  ``rho``: the range of the ladder gaps' multiples of
    eps_a + eps_b (the "wide" family uses 64).  ``slice_rows``: the number of rows the catalogue slices are cut for
    (default ``nrows``).  ``distractor_scale``: standard deviation of the distractors' free coordinates.
    ``prescan_place``: the cancellation families and the first plain family in the prescan's tiles (_prescan_slots)
    instead of at awkward positions."""
    rs = np.random.RandomState(seed)
    c = C_D[D]
    L = min(k + 8, N)
    kinds = _kinds(k, bias)
    F = max(1, min(len(kinds), (N - 2) // L, D - NGATES))
    kinds = kinds[:F]
    if N < 2 * L:                                      # a tiny catalogue: one plain ladder over nearly all of it
        kinds = ["plain"]
    Dp = D - NGATES
    W = np.linalg.qr(rs.standard_normal((Dp, Dp)))[0][:, :len(kinds)].T * np.sqrt(Dp)   # orthogonal, |w|^2 = Dp
    cancel_gate = {}
    for kind in kinds:
        if kind.startswith("cancel"):
            cancel_gate[kind] = len(cancel_gate)

    I = np.zeros((N, D), np.float64)
    bvec = (rs.standard_normal(N) * 0.05) if bias else None
    zero_row = np.zeros(N, bool)
    rep = np.arange(N)                                # duplicate item rows -> the row they copy
    n_zero = 2 if "cancel0" in kinds else 0
    slots = _prescan_slots(D, N, kinds, L, n_zero) if prescan_place else {}
    taken_slots = set(slots.values())
    pos = [p for p in awkward_positions(slice_rows or nrows, N, rs) if p not in taken_slots]
    pos_set = set(pos) | taken_slots
    rest = [p for p in rs.permutation(N) if p not in pos_set]
    free = iter(pos + rest)
    ladders = []                                      # per family: item ids, descending expected score
    zeros = [slots[("zero", z)] if ("zero", z) in slots else next(free) for z in range(n_zero)]
    for j in zeros:
        zero_row[j] = True
        if bvec is not None:
            bvec[j] = 0.0
    Ug = {}                                           # family -> user vector (float64, f32-representable)
    for f, kind in enumerate(kinds):
        w = W[f]
        u = np.zeros(D)
        u[NGATES:] = w
        if kind.startswith("cancel"):
            u[cancel_gate[kind]] = -(200.0 + rs.rand())
        u = u.astype(np.float32).astype(np.float64)
        Ug[f] = u
        ids = [slots[(f, q)] if (f, q) in slots else next(free) for q in range(L)]
        lo, hi = (64.0, 64.0) if kind == "wide" else ((1.5, 2.0) if kind.startswith("cancel") else rho)
        carrier = NGATES + int(np.argmax(np.abs(u[NGATES:])))
        big = kind.startswith("cancel")
        # item vectors before the carrier is set
        base = np.zeros((L, D))
        for q in range(L):
            if big:
                v = rs.standard_normal(Dp)
                v -= (v @ w) / (w @ w) * w               # orthogonal to w: the score is all carrier, A stays large
                base[q, NGATES:] = v
            else:
                base[q, NGATES:] = 10.0 * w + 0.3 * rs.standard_normal(Dp)
            base[q, :NGATES] = 1.0
            if big:
                base[q, cancel_gate[kind]] = 0.0
        if kind == "bias":
            base[:] = base[0]
        if kind == "ties" and k < L:
            dup = {k: k - 1}                            # the pair straddling the k-th place
            if k >= 3 and L > k + 2:
                dup[1] = 0                              # and one at the top
        else:
            dup = {}
        b_items = bvec[ids].copy() if bvec is not None else np.zeros(L)
        # ladder targets, top first
        A_est = np.abs(u) @ np.abs(base).T + np.abs(b_items)
        if not big:
            A_est += np.abs(u[carrier]) * 0.1 * np.abs(base[:, carrier])
        gaps = rs.uniform(lo, hi, L) * c * 2.0 * A_est.max() * 1.02
        target = np.empty(L)
        if big:
            # the place of the zero rung: npos ladder entries above 0.0 (zero rows, if any, sit at 0.0)
            npos = {"cancel+": k + 4, "cancel0": k - 1, "cancel-": max(0, k - 1 - n_zero)}[kind]
            npos = min(npos, L)
            t = 0.0
            for q in range(npos - 1, -1, -1):
                t += gaps[q]
                target[q] = t
            t = 0.0
            for q in range(npos, L):
                t -= gaps[q]
                target[q] = t
        else:
            if kind == "bias":                          # equal U . I: the bias carries the ladder
                dot = float(u @ base[0].astype(np.float32).astype(np.float64))
                t = dot
            else:
                t = 10.0 * Dp
            for q in range(L):
                if q in dup:
                    target[q] = target[dup[q]]
                    continue
                target[q] = t
                t -= gaps[q]
        for q in range(L):
            j = ids[q]
            if q in dup:
                I[j] = I[ids[dup[q]]]
                rep[j] = rep[ids[dup[q]]]
                if bvec is not None:
                    bvec[j] = bvec[ids[dup[q]]]
                continue
            v = base[q].copy()
            if kind == "bias":
                bvec[j] = target[q] - dot
                v = v.astype(np.float32).astype(np.float64)
            else:
                v[carrier] = 0.0
                v = v.astype(np.float32).astype(np.float64)
                rem = target[q] - (b_items[q] if bvec is not None else 0.0) - u @ v
                v[carrier] = rem / u[carrier]
            I[j] = v.astype(np.float32)
        ladders.append(ids)
    taken = set(zeros) | {j for ids in ladders for j in ids}
    for j in range(N):                                # distractors: small, gated
        if j not in taken:
            I[j, NGATES:] = distractor_scale * rs.standard_normal(Dp)
            I[j, :NGATES] = 1.0 + 0.001 * rs.rand(NGATES)

    case = Case()
    case.D, case.N, case.k, case.kinds, case.ladders = D, N, k, kinds, ladders
    case.I = I.astype(np.float32)
    case.bias = bvec.astype(np.float32) if bvec is not None else None
    case.zero_row, case.rep = zero_row, rep
    # rows: family f = r % F, user = family vector x 2^e
    fam = np.arange(nrows) % len(kinds)
    expo = rs.randint(-10, 11, nrows)
    expo[:len(kinds)] = 0
    if bias:
        expo[:] = 0                                   # (the bias does not scale with the user)
    U = np.stack([Ug[f] * 2.0 ** e for f, e in zip(fam, expo)]).astype(np.float32)
    perm = rs.permutation(nrows + 3)[:nrows]          # user ids: a permutation, with a few unused table rows
    Ut = (rs.standard_normal((nrows + 3, D)) * 0.1).astype(np.float32)
    Ut[perm] = U
    case.U, case.users, case.family, case.expo = Ut, perm.astype(np.int64), fam, expo
    masks = []
    for r in range(nrows):
        ids = ladders[fam[r]]
        v = (r // len(kinds)) % 4
        m = []
        if L > k + 1:
            spare = L - k - 1
            if v == 1:
                m = [ids[0]]
            elif v == 2:
                m = [ids[min(k - 1, L - 1)]]
            elif v == 3:
                m = [ids[0], ids[min(k - 1, L - 1)], ids[min(k, L - 1)]][:spare]
        if v >= 2:
            own = set(ids)
            m += [j for j in rs.choice(N, min(N // 4, 24), replace=False) if j not in own and not zero_row[j]]
        masks.append(np.array(sorted(set(m)), np.int64))
    case.masks = masks
    case.mask_ptr = np.zeros(nrows + 1, np.int64)
    case.mask_ptr[1:] = np.cumsum([len(m) for m in masks])
    case.mask_idx = np.concatenate(masks + [np.zeros(0, np.int64)]).astype(np.int64)
    case.expected = {mv: certify(case, mv) for mv in mask_values}
    return case
