"""CPU: properties of the CPU statement of the S3Rec batch law (tests/s3rec_batches_ref.py) — the statement the
kernel is held to bit for bit in tests/test_gpu_s3rec_batches.py has to be the law itself."""
import numpy as np
import pytest

import s3rec_batches_ref as ref


def _toy(rs, nu, ni, lo, hi):
    rows = [rs.randint(0, ni, rs.randint(lo, hi + 1)).tolist() for _ in range(nu)]
    avoid = [sorted(set(v for v in r if 1 <= v <= ni)) for r in rows]
    csr = lambda ls: (np.r_[0, np.cumsum([len(l) for l in ls])].astype(np.int64),
                      np.array([v for l in ls for v in l], dtype=np.int64))
    return rows, avoid, csr(rows) + csr(avoid)


@pytest.mark.parametrize("mode", ref.MODES)
def test_negatives_are_never_avoided_and_test_ones_distinct(mode):
    rs = np.random.RandomState(3)
    rows, avoid, csr = _toy(rs, 30, 140, 0, 30)
    L, n_neg = 6, (99 if mode == "test" else 6)
    X, pos, neg, flag = ref.batches(*csr, 140, np.arange(30), L, mode, 2**40 + 3, 2**35 + 1, n_neg=n_neg)
    assert flag == 0 and neg.shape == (30, n_neg) and neg.min() >= 1 and neg.max() <= 140
    for u in range(30):
        assert not set(neg[u].tolist()) & set(avoid[u])
        if mode == "test":
            assert len(set(neg[u].tolist())) == n_neg
            assert pos[u] == (rows[u][-1] + 1 if len(rows[u]) > 3 else 0)


@pytest.mark.parametrize("mode", ref.MODES)
def test_a_slice_of_users_equals_the_rows_of_the_epoch(mode):
    rs = np.random.RandomState(4)
    _, _, csr = _toy(rs, 20, 130, 0, 12)
    n_neg = 70 if mode == "test" else 5
    whole = ref.batches(*csr, 130, np.arange(20), 5, mode, 9, 2, n_neg=n_neg)
    users = np.array([13, 2, 2, 19, 0])
    part = ref.batches(*csr, 130, users, 5, mode, 9, 2, n_neg=n_neg)
    for w, p in zip(whole[:3], part[:3]):
        assert np.array_equal(w[users], p)
    other = ref.batches(*csr, 130, users, 5, mode, 9, 3, n_neg=n_neg)
    assert np.array_equal(other[0], part[0]) and not np.array_equal(other[2], part[2])     # the epoch moves the draws only


def test_fallbacks_and_flags():
    _, _, p0, p1 = ref.keys(5, 1)
    ni = 100
    # train: one free value is found by the walk, none gives 0 and the flag (4 draws, then the walk)
    neg, bad = ref.seq_negatives(0, 4, [v for v in range(1, ni + 1) if v != 37], ni, p0, p1)
    assert neg.tolist() == [37] * 4 and not bad
    neg, bad = ref.seq_negatives(0, 4, range(1, ni + 1), ni, p0, p1)
    assert neg.tolist() == [0] * 4 and bad
    # the walk goes on from the last draw, cyclically: with 51..100 free and every draw below 51 refused the first
    # free value after a refused draw is 51
    neg, bad = ref.seq_negatives(3, 50, range(1, 51), ni, p0, p1, max_draws=1)
    assert not bad and set(neg.tolist()) <= set(range(51, 101)) and (neg == 51).sum() > 10
    # test: exactly 99 free out of 100 — the stream alone finds them (0.99^4096 ~ 1e-18), the scan is not entered
    info = {}
    neg, bad = ref.distinct_negatives(0, 99, [50], ni, p0, p1, info=info)
    assert not bad and sorted(neg.tolist()) == [v for v in range(1, 101) if v != 50] and not info["scanned"]
    # 50 free values, 99 wanted: 50 distinct ones, 49 zeros, the flag
    neg, bad = ref.distinct_negatives(0, 99, range(1, 51), ni, p0, p1, info=info)
    assert bad and info["scanned"] and sorted(neg[:50].tolist()) == list(range(51, 101)) and not neg[50:].any()
    # the scan fills in ascending order what the stream did not find
    neg, bad = ref.distinct_negatives(0, 8, [], ni, p0, p1, max_draws=3, info=info)
    rest = [v for v in range(1, 101) if v not in neg[:3].tolist()]
    assert not bad and info["candidates"] == 3 and neg[3:].tolist() == rest[:5]


def test_bad_ids_are_flagged():
    ptr, idx = np.array([0, 3, 8]), np.array([1, 2, 3, 4, 99, -1, 5, 6])
    aptr, aidx = np.array([0, 0, 0]), np.array([], dtype=np.int64)
    X, pos, neg, flag = ref.batches(ptr, idx, aptr, aidx, 10, [0, 2, -1, 1], 4, "test", 1, 0, n_neg=3)
    assert flag == ref.FLAG_BAD_USER | ref.FLAG_BAD_ITEM
    assert not X[1].any() and not X[2].any() and not neg[1].any() and pos[1] == 0 and pos[2] == 0
    assert X[3].tolist() == [5, 0, 0, 6] and pos[3] == 7 and X[0].tolist() == [0, 0, 2, 3]
