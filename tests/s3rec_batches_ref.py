"""CPU statement (NumPy, integer work only) of the S3Rec batch builder csrc/s3rec_batches.hip (yr_s3rec_batches) —
importable helper of the tests, no fixtures.  The kernel must give the same words bit for bit.

The law of a batch (reference data/datasets/s3rec_data_pipeline.py:13-50, s3rec_dataset.py:21-57), with the
engine's counter-based generator instead of NumPy's stream (``keys`` / ``_draw`` of oracle/triplet_sampler.py: the
Lemire multiply-shift over ``num_items`` from Philox4x32-7 keyed by (seed, epoch), as in csrc/triplets.hip):

* windows — n the length of the user's behaviour row (raw 0-based ids, interaction order, repeats allowed):
  train X = row[0 : max(0, n-3)], Y = row[1 : n-2]; valid X = row[0 : max(0, n-2)], Y = row[2 : n-1];
  test X = row[0 : max(0, n-1)], Y = row[3 : n]; a slice whose start is not below its end is empty.  Of each the last
  L entries, left padded with -1, everything + 1 (0 is the pad, items are 1..num_items).  pos_items = Y; for test
  pos_item = Y[-1].  A behaviour id outside [0, num_items) reads as the pad and sets FLAG_BAD_ITEM.
* train / valid negatives — one per position j < L, pads included: 1 + draw(t, d), t = user L + j, for the first
  d = 0, 1, ... whose value is not in the user's avoid list (values in 1..num_items, ascending, duplicate-free);
  after MAX_DRAWS rejected draws the next free value after the last draw, walking 1..num_items cyclically; no free
  value: 0 and FLAG_BAD_ITEM.
* test negatives — candidates c_d = 1 + draw(user, d), d = 0, 1, ...: the first n_neg that are neither avoided nor
  equal to an earlier accepted one, in stream order; after MAX_DRAWS candidates the rest from an ascending scan of
  1..num_items; what still cannot be filled is 0, with FLAG_BAD_ITEM.
* a user id outside [0, U) sets FLAG_BAD_USER and gives a zero row.

Every loop below is the sequential definition, one user and one candidate at a time: what the wave-per-user kernel
(64 candidates a round, ballot compaction) has to equal.
"""
import numpy as np

from oracle.triplet_sampler import _draw, keys

FLAG_BAD_USER, FLAG_BAD_ITEM = 1, 2
MAX_DRAWS = 4096
MODES = ("train", "valid", "test")
# (X end = n - cut, Y start, Y end = n - cut + 1)
CUT = {"train": 3, "valid": 2, "test": 1}


def windows(row, L, mode, num_items=None):
    """(X, Y, bad) of one behaviour row: int64 [L] each, ids + 1, 0 the pad."""
    row = [int(v) for v in row]
    n, cut = len(row), CUT[mode]
    bad = False
    out = []
    for start, end in ((0, max(0, n - cut)), (4 - cut, n - cut + 1)):
        part = row[start:end] if start < end else []
        part = part[len(part) - L:] if len(part) > L else part
        vals = []
        for v in part:
            if num_items is not None and not 0 <= v < num_items:
                bad = True
                v = -1
            vals.append(v + 1)
        out.append(np.array([0] * (L - len(part)) + vals, dtype=np.int64))
    return out[0], out[1], bad


def _draws(t, first, count, num_items, p0, p1):
    """1 + draw(t, d) for d in [first, first + count)."""
    tt = np.full(count, t, dtype=np.uint64)
    return 1 + _draw(tt, np.arange(first, first + count, dtype=np.uint64), num_items, p0, p1)


def seq_negatives(user, L, avoid, num_items, p0, p1, max_draws=MAX_DRAWS):
    """Train / valid: (neg [L], bad)."""
    avoid = set(int(a) for a in avoid)
    neg, bad = np.zeros(L, dtype=np.int64), False
    for j in range(L):
        t, d, c, found = user * L + j, 0, 0, False
        while d < max_draws and not found:
            for c in _draws(t, d, min(8 if d == 0 else 256, max_draws - d), num_items, p0, p1).tolist():
                d += 1
                if c not in avoid:
                    found = True
                    break
        if not found:                                    # walk 1..num_items cyclically from the last draw
            steps = 0
            while steps < num_items:
                c = 1 if c == num_items else c + 1
                steps += 1
                if c not in avoid:
                    found = True
                    break
        neg[j] = c if found else 0
        bad |= not found
    return neg, bad


def distinct_negatives(user, n_neg, avoid, num_items, p0, p1, max_draws=MAX_DRAWS, info=None):
    """Test: (neg [n_neg], bad).  ``info``, a dict, receives 'candidates' (how many of the stream were looked at) and
    'scanned' (whether the ascending scan was entered)."""
    avoid = set(int(a) for a in avoid)
    acc, d = [], 0
    while len(acc) < n_neg and d < max_draws:
        for c in _draws(user, d, min(256, max_draws - d), num_items, p0, p1).tolist():
            if len(acc) >= n_neg:
                break
            d += 1
            if c not in avoid and c not in acc:
                acc.append(c)
    scanned = len(acc) < n_neg
    if scanned:
        taken = np.fromiter(avoid | set(acc), dtype=np.int64, count=len(avoid | set(acc)))
        free = np.setdiff1d(np.arange(1, num_items + 1, dtype=np.int64), taken)      # ascending
        acc += free[:n_neg - len(acc)].tolist()
    if info is not None:
        info.update(candidates=d, scanned=scanned)
    bad = len(acc) < n_neg
    return np.array(acc + [0] * (n_neg - len(acc)), dtype=np.int64), bad


def batches(beh_ptr, beh_idx, avoid_ptr, avoid_idx, num_items, users, L, mode, seed, epoch, n_neg=None,
            max_draws=MAX_DRAWS):
    """(X [B, L], pos [B, L] or [B], neg [B, n_neg], flag) for the user ids ``users``."""
    assert mode in MODES
    beh_ptr, beh_idx, avoid_ptr, avoid_idx = (np.asarray(a, dtype=np.int64) for a in (beh_ptr, beh_idx, avoid_ptr, avoid_idx))
    U, B = len(beh_ptr) - 1, len(users)
    test = mode == "test"
    n_neg = (99 if test else L) if n_neg is None else n_neg
    assert test or n_neg == L
    _, _, p0, p1 = keys(seed, epoch)
    X = np.zeros((B, L), dtype=np.int64)
    pos = np.zeros(B if test else (B, L), dtype=np.int64)
    neg = np.zeros((B, n_neg), dtype=np.int64)
    flag = 0
    for b, u in enumerate(int(v) for v in users):
        if not 0 <= u < U:
            flag |= FLAG_BAD_USER
            continue
        x, y, bad = windows(beh_idx[beh_ptr[u]:beh_ptr[u + 1]], L, mode, num_items)
        avoid = avoid_idx[avoid_ptr[u]:avoid_ptr[u + 1]]
        assert np.all(np.diff(avoid) > 0), "avoid lists must be ascending and duplicate-free"
        X[b] = x
        if test:
            pos[b] = y[-1]
            neg[b], bad2 = distinct_negatives(u, n_neg, avoid, num_items, p0, p1, max_draws)
        else:
            pos[b] = y
            neg[b], bad2 = seq_negatives(u, L, avoid, num_items, p0, p1, max_draws)
        if bad or bad2:
            flag |= FLAG_BAD_ITEM
    return X, pos, neg, flag
