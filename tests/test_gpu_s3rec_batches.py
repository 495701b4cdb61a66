"""GPU: the S3Rec batch builder (csrc/s3rec_batches.hip through the C ABI) against its CPU statement
tests/s3rec_batches_ref.py — integer work: bit for bit, in all three modes, at the smallest shapes where the kernel can
go wrong (the ends of a 64-candidate round, duplicates inside a round, the fallbacks) — plus the law's size-independent
properties, the loader, and train.py end to end on both loaders."""
import os

import numpy as np
import pytest
import torch

import s3rec_batches_ref as ref

pytestmark = pytest.mark.gpu

BIG = ((0, 0), (12345, 3), (2**63 + 11, 2**33 + 5))          # (seed, epoch), bits set above 2^32


def _csr(lists):
    return (np.r_[0, np.cumsum([len(l) for l in lists])].astype(np.int64),
            np.array([v for l in lists for v in l], dtype=np.int64))


def _dev(device, *arrs):
    return [torch.from_numpy(np.ascontiguousarray(a).astype(np.int64)).to(device) for a in arrs]


def _rows_for(rs, L, ni):
    """Row lengths 0..5 and L + cut - 1, L + cut, L + cut + 1 for every mode's cut (3, 2, 1), raw ids with repeats."""
    lengths = sorted(set(range(6)) | {L + c + d for c in (1, 2, 3) for d in (-1, 0, 1)}) + [2 * L + 3]
    return [rs.randint(0, ni, n).tolist() for n in lengths]


def _default_avoid(rows, ni):
    return [sorted(set(v for v in r if 1 <= v <= ni)) for r in rows]


def _both(device, rows, avoid, ni, users, L, mode, seed, epoch, n_neg=None, flag=None):
    from yelprecommendation_amd import engine
    csr = _csr(rows) + _csr(avoid)
    want = ref.batches(*csr, ni, users, L, mode, seed, epoch, n_neg=n_neg)
    got = engine.s3rec_batches(*_dev(device, *csr), ni, _dev(device, users)[0], L, mode, seed, epoch, n_neg=n_neg,
                               err_flag=flag)
    return want, [g.cpu().numpy() for g in got]


@pytest.mark.parametrize("L", [1, 6, 50, 64])
@pytest.mark.parametrize("mode", ref.MODES)
def test_kernel_equals_cpu_statement_bit_for_bit(device, L, mode):
    from yelprecommendation_amd import engine
    rs = np.random.RandomState(L)
    ni = 300
    rows = _rows_for(rs, L, ni)
    avoid = _default_avoid(rows, ni)
    flag = engine.new_error_flag(device)
    for (seed, epoch), B in zip(BIG, (1, 5, 257)):               # 257: more than one workgroup, no multiple of its waves
        users = np.r_[rs.permutation(len(rows)), rs.randint(0, len(rows), 257)][:B] if B > 5 else rs.permutation(len(rows))[:B]
        want, got = _both(device, rows, avoid, ni, users, L, mode, seed, epoch, flag=flag)
        for w, g in zip(want[:3], got):
            assert w.shape == g.shape and np.array_equal(w, g)
    assert int(flag.item()) == 0


@pytest.mark.parametrize("n_neg", [1, 63, 64, 65, 99, 128])
def test_test_mode_at_the_ends_of_a_round(device, n_neg):
    """257 users (not a multiple of the waves per workgroup), a 130-item catalogue (160 for n_neg = 128) with 20 avoided
    values: every round of 64 candidates holds duplicates of itself and of the accepted list."""
    from yelprecommendation_amd import engine
    rs = np.random.RandomState(n_neg)
    ni, nu, L = (130 if n_neg <= 99 else 160), 257, 6           # 110 free values; 140 where 128 are wanted
    rows = [rs.randint(0, ni, rs.randint(0, 12)).tolist() for _ in range(nu)]
    avoid = [sorted(rs.choice(np.arange(1, ni + 1), 20, replace=False).tolist()) for _ in range(nu)]
    flag = engine.new_error_flag(device)
    seed, epoch = BIG[2]
    want, got = _both(device, rows, avoid, ni, np.arange(nu), L, "test", seed, epoch, n_neg=n_neg, flag=flag)
    for w, g in zip(want[:3], got):
        assert np.array_equal(w, g)
    assert want[3] == 0 and int(flag.item()) == 0
    neg = got[2]
    assert all(len(set(r.tolist())) == n_neg and not set(r.tolist()) & set(a) for r, a in zip(neg, avoid))


def test_tight_catalogue_is_filled_by_the_stream(device):
    """num_items = 100 with exactly 99 free: 4,096 candidates miss a given free value with probability
    0.99^4096 ~ 1e-18, so the stream alone finds all 99 — on the CPU statement the scan is not entered."""
    from yelprecommendation_amd import engine
    ni, nu = 100, 5
    avoid = [[7 * u + 1] for u in range(nu)]
    rows = [[a[0]] * 4 for a in avoid]
    _, _, p0, p1 = ref.keys(*BIG[1])
    for u in range(nu):
        info = {}
        ref.distinct_negatives(u, 99, avoid[u], ni, p0, p1, info=info)
        assert not info["scanned"] and info["candidates"] > 99
    flag = engine.new_error_flag(device)
    want, got = _both(device, rows, avoid, ni, np.arange(nu), 6, "test", *BIG[1], n_neg=99, flag=flag)
    assert np.array_equal(want[2], got[2]) and int(flag.item()) == 0
    assert all(sorted(r.tolist()) == [v for v in range(1, 101) if v != a[0]] for r, a in zip(got[2], avoid))


def test_fallbacks(device):
    from yelprecommendation_amd import engine
    flag = engine.new_error_flag(device)
    # one user of a 2^20-item catalogue with all but 120 values avoided: the ascending scan fills the list, no flag
    ni = 1 << 20
    rs = np.random.RandomState(9)
    free = np.sort(rs.choice(np.arange(1, ni + 1), 120, replace=False))
    avoid = [np.setdiff1d(np.arange(1, ni + 1), free).tolist()]
    want, got = _both(device, [[5, 6, 7, 8, 9]], avoid, ni, [0], 6, "test", 3, 1, n_neg=99, flag=flag)
    assert np.array_equal(want[2], got[2]) and int(flag.item()) == 0 and want[3] == 0
    assert set(got[2][0].tolist()) <= set(free.tolist()) and len(set(got[2][0].tolist())) == 99
    # 50 free values, 99 wanted: 50 distinct values, 49 zeros and FLAG_BAD_ITEM
    want, got = _both(device, [[1, 2, 3, 4]], [list(range(1, 51))], 100, [0], 6, "test", 3, 1, n_neg=99, flag=flag)
    assert np.array_equal(want[2], got[2]) and want[3] == ref.FLAG_BAD_ITEM
    assert int(flag.item()) == engine.FLAG_BAD_ITEM
    assert sorted(got[2][0][:50].tolist()) == list(range(51, 101)) and not got[2][0][50:].any()
    flag.zero_()
    # train mode with one free value (found by the walk) and with none (0 and the flag)
    one = [[v for v in range(1, 91) if v != 37]]
    want, got = _both(device, [[1, 2, 3, 4, 5, 6, 7]], one, 90, [0], 6, "train", 3, 0, flag=flag)
    assert np.array_equal(want[2], got[2]) and (got[2] == 37).all() and int(flag.item()) == 0
    want, got = _both(device, [[1, 2, 3, 4, 5, 6, 7]], [list(range(1, 91))], 90, [0], 6, "valid", 3, 0, flag=flag)
    assert np.array_equal(want[2], got[2]) and not got[2].any() and np.array_equal(want[0], got[0])
    assert int(flag.item()) == engine.FLAG_BAD_ITEM and want[3] == ref.FLAG_BAD_ITEM


@pytest.mark.parametrize("mode", ref.MODES)
def test_bad_ids_and_batches_of_the_epoch(device, mode):
    from yelprecommendation_amd import engine
    rs = np.random.RandomState(21)
    ni, nu, L = 200, 40, 6
    rows = [rs.randint(0, ni, rs.randint(0, 15)).tolist() for _ in range(nu)]
    avoid = _default_avoid(rows, ni)
    n_neg = 99 if mode == "test" else None
    flag = engine.new_error_flag(device)
    whole_want, whole = _both(device, rows, avoid, ni, np.arange(nu), L, mode, 8, 4, n_neg=n_neg, flag=flag)
    users = np.array([31, 2, 2, 39, 0, 17, 8])
    _, part = _both(device, rows, avoid, ni, users, L, mode, 8, 4, n_neg=n_neg, flag=flag)
    for w, p, ww in zip(whole, part, whole_want[:3]):
        assert np.array_equal(w, ww) and np.array_equal(w[users], p)          # any batch = the rows of the epoch
    assert int(flag.item()) == 0
    # bad user ids are flagged and give zero rows; nothing is dereferenced
    users = np.array([3, nu, -1, 2**40, 5])
    want, got = _both(device, rows, avoid, ni, users, L, mode, 8, 4, n_neg=n_neg, flag=flag)
    for w, g in zip(want[:3], got):
        assert np.array_equal(w, g) and not g[1:4].any()
    assert got[2][0].all() and got[2][4].all() and int(flag.item()) == engine.FLAG_BAD_USER == want[3]
    flag.zero_()
    # a behaviour id outside [0, num_items) reads as the pad and is flagged
    rows2 = [[1, 2, ni, 4, -3, 6, 7, 8]]
    want, got = _both(device, rows2, [[1, 2]], ni, [0], L, mode, 8, 4, n_neg=n_neg, flag=flag)
    for w, g in zip(want[:3], got):
        assert np.array_equal(w, g)
    assert int(flag.item()) == engine.FLAG_BAD_ITEM == want[3]


def test_uniform_law_over_the_free_values(device):
    """One user, 50 items, 6 avoided: every free value equally often (chi-square below df + 5 sqrt(2 df), 43 degrees of
    freedom) — in train mode over ~200,000 positions (the user repeated, epochs 0..) and for the first test negative over
    many epochs."""
    from yelprecommendation_amd import engine
    ni, L = 50, 64
    avoided = [1, 8, 9, 22, 31, 50]
    free = np.setdiff1d(np.arange(1, ni + 1), avoided)
    d = _dev(device, [0, 5], [0, 7, 8, 21, 30], [0, 6], avoided)
    bar = 43 + 5 * np.sqrt(2 * 43)
    users = torch.zeros(1, dtype=torch.int64, device=device)
    negs = torch.cat([engine.s3rec_batches(*d, ni, users, L, "train", 2024, e)[2].reshape(-1) for e in range(3200)])
    cnt = torch.bincount(negs, minlength=ni + 1).cpu().numpy().astype(np.float64)
    assert negs.numel() == 204_800 and cnt[avoided].sum() == 0 and cnt[0] == 0
    exp = negs.numel() / len(free)
    chi2 = ((cnt[free] - exp) ** 2 / exp).sum()
    assert chi2 < bar, chi2
    first = torch.cat([engine.s3rec_batches(*d, ni, users, 6, "test", 7, e, n_neg=3)[2][:, 0] for e in range(4400)])
    cnt = torch.bincount(first, minlength=ni + 1).cpu().numpy().astype(np.float64)
    exp = first.numel() / len(free)
    assert cnt[avoided].sum() == 0 and ((cnt[free] - exp) ** 2 / exp).sum() < bar


def test_loader_epochs(device):
    from yelprecommendation_amd.data.s3rec_batches import S3RecBatchLoader, S3RecSequences
    rs = np.random.RandomState(2)
    nu, ni, L = 150, 400, 12
    counts = rs.randint(1, 30, nu)
    u = torch.from_numpy(np.repeat(np.arange(nu), counts)).to(device)
    i = torch.from_numpy(rs.randint(0, ni, int(counts.sum()))).to(device)
    store = S3RecSequences(u, i, nu, ni, L, seed=3)
    loader = S3RecBatchLoader(store, "train", 64, shuffle=True, seed=11)
    assert len(loader) == 3
    e0, e1 = list(loader), list(loader)
    assert [b["X"].shape[0] for b in e0] == [64, 64, 22] and sorted(e0[0]) == ["X", "neg_items", "pos_items", "user_id"]
    for ep in (e0, e1):
        assert torch.equal(torch.sort(torch.cat([b["user_id"] for b in ep])).values, torch.arange(nu, device=device))
    cat = lambda ep, k: torch.cat([b[k] for b in ep])
    assert not torch.equal(cat(e0, "user_id"), cat(e1, "user_id")) and not torch.equal(cat(e0, "neg_items"), cat(e1, "neg_items"))
    again = list(S3RecBatchLoader(store, "train", 64, shuffle=True, seed=11))                 # reproducible per seed
    assert all(torch.equal(cat(e0, k), cat(again, k)) for k in ("user_id", "X", "pos_items", "neg_items"))
    other = list(S3RecBatchLoader(store, "train", 64, shuffle=True, seed=12))
    assert not torch.equal(cat(e0, "neg_items"), cat(other, "neg_items"))
    # a batch is the rows of the whole-epoch draw of its users
    X, pos, neg = store.draw("train", 0, seed=11)
    b = e0[1]
    assert torch.equal(X[b["user_id"]], b["X"]) and torch.equal(pos[b["user_id"]], b["pos_items"]) \
        and torch.equal(neg[b["user_id"]], b["neg_items"])
    test = list(S3RecBatchLoader(store, "test", 64, shuffle=True, seed=0))                     # never shuffled
    assert torch.equal(cat(test, "user_id"), torch.arange(nu, device=device)) and test[0]["neg_items"].shape == (64, 99)
    assert sorted(test[0]) == ["X", "neg_items", "pos_item", "user_id"] and test[0]["pos_item"].shape == (64,)
    # the default avoid values are the raw ids (the reference's off-by-one); shifted=True avoids the items themselves
    shifted = S3RecSequences(u, i, nu, ni, L, seed=3, shifted=True)
    a0 = store.avoid_idx[store.avoid_ptr[0]:store.avoid_ptr[1]].cpu().tolist()
    a1 = shifted.avoid_idx[shifted.avoid_ptr[0]:shifted.avoid_ptr[1]].cpu().tolist()
    raw = i[:counts[0]].cpu().tolist()
    assert a0 == sorted(set(v for v in raw if v >= 1)) and a1 == sorted(set(v + 1 for v in raw))
    store.check()


def _losses(caplog):
    import re
    return [float(m.group(1)) for r in caplog.records for m in [re.search(r"train loss: ([0-9.eE+-]+)", r.getMessage())] if m]


def test_train_main_device_loader(device, tmp_path, caplog):
    """python -m yelprecommendation_amd.train model_name=S3Rec ... fast_loader=true: four finite metrics in [0, 1],
    best_model.pt, and the summed training loss of epoch 2 below that of epoch 1 (dropout 0, lr 1e-3, seed 42: measured
    3.1563 then 2.6369 over the five batches of an epoch on one MI355X)."""
    import logging
    from yelprecommendation_amd import train
    with caplog.at_level(logging.INFO, logger="yelprecommendation_amd"):
        metrics = train.main(["model_name=S3Rec", "synthetic=300x200x12", "fast_loader=true", "epochs=2", "batch_size=64",
                              "embed_size=32", "max_seq_len=12", "dropout_ratio=0", "lr=0.001", "seed=42",
                              "load_pretrain=false", f"model_dir={tmp_path}"])
    assert len(metrics) == 4 and all(np.isfinite(m) and 0.0 <= m <= 1.0 for m in metrics)
    assert os.path.exists(os.path.join(str(tmp_path), "best_model.pt"))
    losses = _losses(caplog)
    print("S3Rec device loader, summed training loss per epoch:", losses, "test metrics:", metrics)
    assert len(losses) == 2 and losses[1] < losses[0]


def test_train_main_host_loader(device, tmp_path, caplog):
    """The same run through DataLoader(S3RecDataset) on a smaller frame: the host path trains through the same trainer."""
    import logging
    from yelprecommendation_amd import train
    with caplog.at_level(logging.INFO, logger="yelprecommendation_amd"):
        metrics = train.main(["model_name=S3Rec", "synthetic=60x150x10", "fast_loader=false", "epochs=2", "batch_size=32",
                              "embed_size=32", "max_seq_len=12", "dropout_ratio=0", "lr=0.001", "seed=42",
                              "load_pretrain=false", f"model_dir={tmp_path}"])
    assert len(metrics) == 4 and all(np.isfinite(m) and 0.0 <= m <= 1.0 for m in metrics)
    assert os.path.exists(os.path.join(str(tmp_path), "best_model.pt"))
    losses = _losses(caplog)
    print("S3Rec host loader, summed training loss per epoch:", losses)
    assert len(losses) == 2 and all(np.isfinite(losses))
