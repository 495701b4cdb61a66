"""CPU statement (NumPy, vectorised integer arithmetic) of the device-side BPR triplet stream
(yelprecommendation_amd/csrc/triplets.hip) — test infrastructure only: imported by tests/, never by
the product.

What it restates: the LAW of the reference's producer — ``DataLoader(MFDataset, shuffle=True)``
(train.py:76-77): one permutation of the rows per epoch; ``MFDataset._negative_sampling``
(data/datasets/mf_dataset.py:18-22): ``neg = np.random.randint(num_items)`` redrawn while
``neg in pos_items`` — with the engine's own counter-based generator, so that position t of epoch e
is a pure function of (seed, e, t).  The reference's NumPy/torch RNG streams are NOT reproduced
(parity runs replay recorded streams instead: ``RecordedStream`` in data/triplets.py); what IS pinned
is (a) this file == the kernel, word for word (integer work, bit-exact), and (b) the law: a
permutation per epoch, never a positive, uniform over the non-positives (tests/test_gpu_triplets.py,
tests/test_triplet_sampler_oracle.py).
"""
import numpy as np

U32 = np.uint64(0xFFFFFFFF)


def _fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & U32
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x85EBCA6B)) & U32
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE35)) & U32
    h ^= h >> np.uint64(16)
    return h


def _feistel(x, half_bits, k0, k1):
    mask = np.uint64((1 << half_bits) - 1) if half_bits < 32 else U32
    hb = np.uint64(half_bits)
    L, R = (x >> hb) & mask, x & mask
    for r in range(4):
        k = k1 if r & 1 else k0
        f = _fmix32(R ^ k ^ np.uint64((0x9E3779B9 * (r + 1)) & 0xFFFFFFFF)) & mask
        L, R = R, L ^ f
    return (L << hb) | R


def philox4x32(c0, c1, c2, c3, k0, k1, rounds):
    """Philox4x32 with ``rounds`` rounds (csrc/philox.h): 10 is the standard generator (dropout masks), 7 the
    sampler's.  Counter words as arrays (or scalars), key words scalars; returns four uint64 arrays below 2^32."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(rounds):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & U32, p1 >> np.uint64(32), p1 & U32
        c0, c1, c2, c3 = (hi1 ^ c1 ^ k0) & U32, lo1, (hi0 ^ c3 ^ k1) & U32, lo0
        k0 = (k0 + np.uint64(0x9E3779B9)) & U32
        k1 = (k1 + np.uint64(0xBB67AE85)) & U32
    return c0, c1, c2, c3


def _philox4x32_7(c0, c1, c2, c3, k0, k1):
    return philox4x32(c0, c1, c2, c3, k0, k1, 7)


def half_bits_for(n_rows):
    h = 1
    while h < 32 and (1 << (2 * h)) < n_rows:
        h += 1
    return h


def keys(seed, epoch):
    seed, epoch = int(seed) & (2**64 - 1), int(epoch) & (2**64 - 1)
    k0 = int(_fmix32((seed & 0xFFFFFFFF) ^ 0x243F6A88)) ^ (epoch & 0xFFFFFFFF)
    k1 = int(_fmix32((seed >> 32) ^ 0x85A308D3)) ^ (epoch >> 32) ^ int(_fmix32(epoch & 0xFFFFFFFF))
    p0 = (seed & 0xFFFFFFFF) ^ (((epoch * 0x9E3779B97F4A7C15) & (2**64 - 1)) >> 32)
    p1 = (seed >> 32) ^ (epoch & 0xFFFFFFFF)
    return np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF), p0 & 0xFFFFFFFF, p1 & 0xFFFFFFFF


def permutation(n_rows, seed, epoch, first=0, count=None):
    """P(t) for t in [first, first + count): the keyed bijection of [0, n_rows)."""
    count = n_rows - first if count is None else count
    k0, k1, _, _ = keys(seed, epoch)
    hb = half_bits_for(n_rows)
    r = np.arange(first, first + count, dtype=np.uint64)
    todo = np.ones(count, dtype=bool)
    while todo.any():
        r[todo] = _feistel(r[todo], hb, k0, k1)
        todo &= r >= np.uint64(n_rows)
    return r.astype(np.int64)


def _draw(t, d, num_items, p0, p1):
    w = _philox4x32_7(t & U32, t >> np.uint64(32), d, np.zeros_like(t), p0, p1)
    n = np.uint64(num_items)
    m = w[0] * n
    thr = np.uint64(((1 << 32) - num_items) % num_items)
    for alt in w[1:]:
        again = ((m & U32) < n) & ((m & U32) < thr)
        m = np.where(again, alt * n, m)
    return (m >> np.uint64(32)).astype(np.int64)


def sample(row_user, row_item, avoid_ptr, avoid_idx, num_items, seed, epoch, shuffle=True, first=0, count=None,
           max_draws=4096):
    """(user, pos, neg) for the stream positions [first, first + count) of one epoch."""
    n_rows = len(row_user)
    count = n_rows - first if count is None else count
    rows = permutation(n_rows, seed, epoch, first, count) if shuffle else np.arange(first, first + count)
    u, p = np.asarray(row_user)[rows], np.asarray(row_item)[rows]
    _, _, p0, p1 = keys(seed, epoch)
    t = np.arange(first, first + count, dtype=np.uint64)
    neg = np.zeros(count, dtype=np.int64)
    todo = np.ones(count, dtype=bool)
    avoid_ptr, avoid_idx = np.asarray(avoid_ptr), np.asarray(avoid_idx)
    # membership through one sorted key array (user * num_items + item)
    owner = np.repeat(np.arange(len(avoid_ptr) - 1), np.diff(avoid_ptr))
    key = owner * num_items + avoid_idx
    assert np.all(np.diff(key) > 0), "avoid lists must be ascending and duplicate-free"
    d = 0
    while todo.any():
        idx = np.flatnonzero(todo)
        cand = _draw(t[idx], np.full(idx.size, d, dtype=np.uint64), num_items, p0, p1)
        k = u[idx] * num_items + cand
        pos = np.searchsorted(key, k)
        taken = (pos < key.size) & (key[np.minimum(pos, key.size - 1)] == k)
        neg[idx] = cand
        todo[idx[~taken]] = False
        d += 1
        if d >= max_draws and todo.any():
            for j in np.flatnonzero(todo):           # next free item after the last draw (kernel's fallback)
                lst = set(avoid_idx[avoid_ptr[u[j]]:avoid_ptr[u[j] + 1]].tolist())
                c, steps = int(neg[j]), 0
                while steps < num_items:
                    c = 0 if c + 1 == num_items else c + 1
                    steps += 1
                    if c not in lst:
                        break
                neg[j] = c if steps < num_items else 0
            break
    return u.astype(np.int64), p.astype(np.int64), neg
