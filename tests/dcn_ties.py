"""Top-k comparison for DCN lists that tolerates float near-ties only (the DCN counterpart of
replay.assert_topk_equal_up_to_near_ties, which recomputes MF dot products).

The sigmoid saturates: many items can score exactly 1.0f, and the reference's argpartition orders ties arbitrarily
while the engine orders them by item id.  Rule: no agreement quota; at every position the two lists may differ only
between items whose float64 scores tie within f32 rounding (|a - b| <= tol), and both lists must be made of items
whose scores are within tol of the exact k-th best score."""
import numpy as np

F32_ULP = 2.0 ** -24


def _tol(s):
    return 4 * F32_ULP * max(1.0, abs(s)) + 1e-6


def masked_rows(scores, mask_ptr, mask_idx):
    s = np.array(scores, dtype=np.float64, copy=True)
    for r in range(s.shape[0]):
        s[r, mask_idx[mask_ptr[r]:mask_ptr[r + 1]]] = 0.0
    return s


def assert_topk_equal_up_to_near_ties(got, want, scores64, k, tol=None):
    """got / want: [n, k] item lists; scores64: [n, num_items] float64 masked scores.  Returns the rows on which no tie
    straddles the k-th place (their metrics must agree exactly)."""
    clean = []
    for r in range(got.shape[0]):
        s = scores64[r]
        order = np.argsort(-s, kind="stable")
        kth = s[order[k - 1]]
        t = tol if tol is not None else _tol(kth)
        for lst, who in ((got[r], "engine"), (want[r], "reference")):
            vals = s[np.asarray(lst, dtype=np.int64)]
            for pos in range(k):
                exact = s[order[pos]]
                tp = tol if tol is not None else _tol(exact)
                assert abs(vals[pos] - exact) <= tp, (
                    f"row {r} position {pos}: {who} item {lst[pos]} scores {vals[pos]!r}, exact rank value {exact!r}")
        straddle = k < len(s) and abs(s[order[k]] - kth) <= t
        if not straddle:
            clean.append(r)
            assert set(np.asarray(got[r]).tolist()) == set(np.asarray(want[r]).tolist()), f"row {r}: lists differ"
    return np.asarray(clean, dtype=np.int64)
