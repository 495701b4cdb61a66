"""Float64 reference for the catalogue rank sweep (engine.catalogue_ranks, csrc/catalogue_rank.hip) and the metrics
taken from ranks (engine.metrics_from_ranks, csrc/metrics.hip), shared by test_catalogue_rank_host.py (CPU) and
test_gpu_catalogue_rank.py (GPU).

List order of a row (the reference's ``pred[mask] = -3.40282e+38`` under the project's tie rule): the unmasked items by
score descending then id ascending, then the masked items by id ascending.  rank = the 0-based place of a target in it:

    unmasked target t:  #{ unmasked i != t : s_i > s_t  or  (s_i == s_t and i < t) }
    masked target t:    #unmasked + #{ masked ids below t }

Error bar.  One f32 accumulator takes all L D products of a score, so tests/eval_ladders.py's rounding model holds with
D replaced by L D: |s32 - s64| <= c_bound(L D) A, A = sum |u_d i_d| (``bar``).  From it the interval of a rank:
lo = the unmasked items DECISIVELY above the target (s_i - e_i > s_t + e_t), hi = those not decisively below.

Exactness certificate (as tests/ngcf_ref64.py): tables of small integers whose products and partial sums are integers
below 2^24 are exact in f32 in ANY order, so a correct kernel's ranks and scores equal float64's (``certify_exact``).

Metrics.  ``metrics_from_ranks`` is oracle/metric.py's loops run on the full order rebuilt from the ranks: place i of
the prediction holds the target whose rank is i, else an id no `actual` list holds — so it shares no closed form with the
kernel.  MRR / AUC: ``mrr_auc_from_scores`` counts pairs from the scores themselves.
"""
from math import log2

import numpy as np

import eval_ladders as el

CAP = 16                    # engine.CATALOGUE_RANK_CAP (asserted equal in test_catalogue_rank_host.py)
TILE = 32                   # engine.SWEEP_TILE
CHUNK = 2048                # engine.SWEEP_COL_CHUNK
GRID_MAX = 2048             # engine.SWEEP_GRID_MAX


def bar(L, D):
    return el.c_bound(L * D)


def scores64(layers_user, layers_item, users):
    """(S, A): float64 scores [len(users), items] and the sums of |products|."""
    S = A = 0.0
    for U, I in zip(layers_user, layers_item):
        u, i = U.astype(np.float64)[users], I.astype(np.float64)
        S = S + u @ i.T
        A = A + np.abs(u) @ np.abs(i).T
    return S, A


def certify_exact(layers_user, layers_item):
    """Small integers whose every partial sum of products is an integer below 2^24: exact in f32 in any order."""
    worst = 0.0
    for U, I in zip(layers_user, layers_item):
        assert np.array_equal(U, np.rint(U)) and np.array_equal(I, np.rint(I))
        worst += np.abs(U).max(initial=0) * np.abs(I).max(initial=0) * U.shape[1]
    assert worst < 2 ** 24, worst


def full_order(s, mask):
    """Item ids of one row in the list order."""
    masked = np.zeros(len(s), bool)
    masked[np.asarray(mask, np.int64)] = True
    ids = np.arange(len(s))
    un = ids[~masked]
    un = un[np.lexsort((un, -s[un]))]
    return np.concatenate([un, ids[masked]])


def ranks_row(s, mask, targets):
    """The place of every target (original order) in full_order(s, mask); -1 for an id outside the catalogue."""
    place = np.empty(len(s), np.int64)
    place[full_order(s, mask)] = np.arange(len(s))
    return np.array([place[t] if 0 <= t < len(s) else -1 for t in targets], np.int64)


def ranks(S, masks, pos):
    """rank [nnz] aligned with the concatenated pos lists."""
    out = [ranks_row(S[r], masks[r], pos[r]) for r in range(len(pos))]
    return np.concatenate(out + [np.zeros(0, np.int64)])


def rank_bounds_row(s, eps, mask, targets):
    """(lo, hi) per target: the unmasked items decisively above / not decisively below; a masked target's rank is
    exact (integers only)."""
    masked = np.zeros(len(s), bool)
    masked[np.asarray(mask, np.int64)] = True
    exact = ranks_row(s, mask, targets)
    lo, hi = [], []
    for t, r in zip(targets, exact):
        if masked[t]:
            lo.append(r)
            hi.append(r)
            continue
        other = ~masked
        other[t] = False
        lo.append(int(np.count_nonzero(other & (s - eps > s[t] + eps[t]))))
        hi.append(int(np.count_nonzero(other & (s + eps >= s[t] - eps[t]))))
    return np.array(lo, np.int64), np.array(hi, np.int64)


def csr(lists):
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    idx = np.array([x for l in lists for x in l], np.int64)
    return ptr, idx


# ---- metrics --------------------------------------------------------------------------------------------------------

def lists_from_ranks(rank_rows, k):
    """(actual, predicted[:k]) with the same hit pattern as the full order: `actual` = markers 0 .. len - 1 in the
    original order, place i of the prediction = the marker whose rank is i, else -1 - i (in no actual list)."""
    actual, predicted = [], []
    for rk in rank_rows:
        pred = [-1 - i for i in range(k)]
        for j, r in enumerate(rk):
            if 0 <= r < k:
                pred[int(r)] = j
        actual.append(list(range(len(rk))))
        predicted.append(pred)
    return actual, predicted


def oracle_four(actual, predicted, k):
    """oracle/metric.py's four loops; imported lazily so that this module loads without the package path."""
    from oracle import metric as om
    return (om.precision_at_k(actual, predicted, k), om.recall_at_k(actual, predicted, k),
            om.map_at_k(actual, predicted, k), om.ndcg_at_k(actual, predicted, k))


def metrics_from_ranks(rank_rows, ks, unmasked=None):
    """{k: (precision, recall, map, ndcg, hr)}, 'mrr', 'auc' from per-row rank lists (original order of actual).
    ``unmasked``: per row, the number of unmasked items (for AUC; None: no AUC)."""
    out = {}
    nonempty = [rk for rk in rank_rows if len(rk)]
    for k in ks:
        actual, predicted = lists_from_ranks(rank_rows, k)
        hr = sum(1.0 for rk in nonempty if any(0 <= r < k for r in rk)) / len(nonempty)
        out[k] = oracle_four(actual, predicted, k) + (hr,)
    out["mrr"] = sum((1.0 / (min(r for r in rk if r >= 0) + 1)) if any(r >= 0 for r in rk) else 0.0
                     for rk in nonempty) / len(nonempty)
    if unmasked is not None:
        total, users = 0.0, 0
        for rk, U in zip(rank_rows, unmasked):
            if not len(rk):
                continue
            valid_unmasked = [r for r in rk if 0 <= r < U]
            negatives = U - len(valid_unmasked)
            if negatives <= 0:
                continue
            right = 0
            for r in valid_unmasked:
                ahead = sum(1 for q in valid_unmasked if q < r)
                right += negatives - (r - ahead)
            total += right / (len(rk) * negatives)
            users += 1
        out["auc"] = total / users if users else float("nan")
    return out


def mrr_auc_from_scores(S, masks, pos):
    """MRR and AUC counted pair by pair from the scores and the list order, no ranks involved."""
    mrr, auc, n_mrr, n_auc = 0.0, 0.0, 0, 0
    for r in range(len(pos)):
        if not len(pos[r]):
            continue
        order = full_order(S[r], masks[r])
        place = {int(j): p for p, j in enumerate(order)}
        n_mrr += 1
        mrr += 1.0 / (min(place[t] for t in pos[r]) + 1)
        masked = set(int(x) for x in masks[r])
        tset = set(int(t) for t in pos[r])
        negatives = [j for j in range(S.shape[1]) if j not in masked and j not in tset]
        if not negatives:
            continue
        right = sum(1 for t in pos[r] if t not in masked for j in negatives if place[int(t)] < place[j])
        auc += right / (len(pos[r]) * len(negatives))
        n_auc += 1
    return mrr / n_mrr, (auc / n_auc if n_auc else float("nan"))


def closed_form_metrics(rank_rows, ks, unmasked=None):
    """The formulas csrc/metrics.hip states (yr_metrics_from_ranks), term by term — checked against the loops above on
    the CPU, so that a GPU mismatch points at the kernel and not at the algebra."""
    out = {}
    n = len(rank_rows)
    nonempty = [list(map(int, rk)) for rk in rank_rows if len(rk)]
    for k in ks:
        p = r = a = d = h = 0.0
        for rk in nonempty:
            ln = len(rk)
            hits = [x for x in rk if 0 <= x < k]
            span = min(ln, k)
            ap = sum(sum(1 for q in rk[:min(x + 1, ln)] if 0 <= q <= x) / (x + 1) for x in hits)
            dcg = sum(1.0 / log2(x + 2) for x in hits if x < span)
            idcg = sum(1.0 / log2(i + 1) for i in range(1, span + 1))
            p += len(hits) / k
            r += len(hits) / ln
            a += ap / ln
            d += dcg / idcg
            h += 1.0 if hits else 0.0
        m = len(nonempty)
        out[k] = (p / n, r / m, a / m, d / m, h / m)
    out["mrr"] = sum(1.0 / (min(x for x in rk if x >= 0) + 1) if any(x >= 0 for x in rk) else 0.0
                     for rk in nonempty) / len(nonempty)
    if unmasked is not None:
        tot, users = 0.0, 0
        for rk, U in zip(rank_rows, unmasked):
            rk = list(map(int, rk))
            if not rk:
                continue
            valid = sum(1 for x in rk if x >= 0)
            n_masked = sum(1 for x in rk if x >= U)
            wrong = sum(x - sum(1 for q in rk if 0 <= q < x) for x in rk if 0 <= x < U)
            negatives = U - (valid - n_masked)
            if negatives > 0:
                tot += ((valid - n_masked) * negatives - wrong) / (len(rk) * negatives)
                users += 1
        out["auc"] = tot / users if users else float("nan")
    return out
