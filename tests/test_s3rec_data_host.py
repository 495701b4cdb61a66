"""CPU: the S3Rec host data path (data/datasets/s3rec_data_pipeline.py, s3rec_dataset.py) against what the reference
recorded (tests/golden/s3rec_data_small.npz, made by tests/golden/make_golden_s3rec_data.py), the config block, the
train.py dispatch and the argument checks of yr_s3rec_batches — nothing here needs a GPU."""
import os

import numpy as np
import pandas as pd
import pytest

import s3rec_batches_ref as ref

MODES = ("train", "valid", "test")


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "s3rec_data_small.npz"))
    cfg = dict(zip(g["cfg_names"].tolist(), g["cfg_values"].tolist()))
    rows = [g["beh_idx"][a:b].tolist() for a, b in zip(g["beh_ptr"][:-1], g["beh_ptr"][1:])]
    return g, cfg, rows


def _split(rows, L):
    from yelprecommendation_amd.data.datasets.s3rec_data_pipeline import S3RecDataPipeline
    from yelprecommendation_amd.utils import make_config
    pipe = S3RecDataPipeline(make_config("S3Rec", max_seq_len=L))
    return dict(zip(MODES, pipe.split(pd.DataFrame({"behaviors": rows}))))


def test_split_reproduces_the_reference_windows(golden):
    g, cfg, rows = golden
    assert sorted(len(r) for r in rows)[:5] == [1, 2, 3, 4, 5]            # the short rows are in the fixture
    parts = _split(rows, cfg["max_seq_len"])
    for mode in MODES:
        assert np.array_equal(np.array(parts[mode]["X"].tolist()), g[f"{mode}_X"])
        assert np.array_equal(np.array(parts[mode]["Y"].tolist()), g[f"{mode}_Y"])


def test_dataset_replays_the_reference_stream(golden):
    """Same np.random calls in the same order: the seeded host run gives the recorded negatives."""
    from yelprecommendation_amd.data.datasets.s3rec_dataset import S3RecDataset
    g, cfg, rows = golden
    parts = _split(rows, cfg["max_seq_len"])
    np.random.seed(cfg["seed"])
    for mode in MODES:
        ds = S3RecDataset(parts[mode], None, None, num_items=cfg["num_items"], train=mode != "test")
        items = [ds[u] for u in range(len(ds))]
        assert np.array_equal(np.array([it["neg_items"] for it in items]), g[f"{mode}_neg_items"])
        assert np.array_equal(np.array([it["X"] for it in items]), g[f"{mode}_X"])
        if mode == "test":
            assert sorted(items[0]) == ["X", "neg_items", "pos_item", "user_id"]
            assert np.array_equal(np.array([it["pos_item"] for it in items]), g["test_pos_item"])
        else:
            assert sorted(items[0]) == ["X", "neg_items", "pos_items", "user_id"]
            assert np.array_equal(np.array([it["pos_items"] for it in items]), g[f"{mode}_Y"])


def test_cpu_statement_windows_equal_the_pipeline(golden):
    """The explicit-end window arithmetic of tests/s3rec_batches_ref.py against the reference's negative indices."""
    g, cfg, rows = golden
    for L in (1, cfg["max_seq_len"], 50):
        parts = _split(rows, L) if L != cfg["max_seq_len"] else None
        for mode in MODES:
            for u, row in enumerate(rows):
                x, y, bad = ref.windows(row, L, mode, cfg["num_items"])
                want_x = g[f"{mode}_X"][u] if parts is None else np.array(parts[mode]["X"].iloc[u])
                want_y = g[f"{mode}_Y"][u] if parts is None else np.array(parts[mode]["Y"].iloc[u])
                assert not bad and np.array_equal(x, want_x) and np.array_equal(y, want_y), (L, mode, u)
    assert np.array_equal(g["test_pos_item"], g["test_Y"][:, -1])


def test_make_config_carries_the_s3rec_block():
    from yelprecommendation_amd.utils import make_config
    cfg = make_config("S3Rec")
    want = dict(embed_size=64, max_seq_len=50, num_heads=2, num_blocks=2, pretrain=False, load_pretrain=True,
                pretrain_epochs=100, mask_portion=0.2, dropout_ratio=0.1)
    assert {k: cfg[k] for k in want} == want and cfg.model_name == "S3Rec" and "model" not in cfg


def test_build_dispatches_s3rec(tmp_path):
    from yelprecommendation_amd import train
    from yelprecommendation_amd.data.datasets.s3rec_dataset import S3RecDataset
    from yelprecommendation_amd.utils import make_config
    cfg = make_config("S3Rec", synthetic="40x60x9", device="cpu", max_seq_len=6, model_dir=str(tmp_path))
    args = train.build(cfg)
    assert args.model_info == {"num_items": 60, "num_users": 40}
    assert all(isinstance(d, S3RecDataset) and len(d) == 40 for d in (args.train_dataset, args.valid_dataset, args.test_dataset))
    assert not args.test_dataset.train
    for ds in (args.train_dataset, args.valid_dataset):
        first = ds[0]
        assert sorted(first) == ["X", "neg_items", "pos_items", "user_id"]
        assert first["X"].shape == first["pos_items"].shape == first["neg_items"].shape == (6,)
        assert first["X"].dtype == np.int64 and 1 <= first["neg_items"].min() and first["neg_items"].max() <= 60
    # the attributes in the schema _load_attributes reads: {item + 1: {'categories': [...]}} and the pad's empty entry
    attrs = args.data_pipeline.item2attributes
    assert sorted(attrs) == list(range(61)) and attrs[0] == {"categories": []} and args.data_pipeline.attributes_count > 0
    unknown = make_config("MF", model_dir=str(tmp_path))
    unknown["model_name"] = "nope"
    with pytest.raises(ValueError, match="S3Rec"):                       # the message lists the models on the path
        train.build(unknown)


def test_pretrain_is_refused(tmp_path):
    from yelprecommendation_amd import train
    from yelprecommendation_amd.utils import make_config
    cfg = make_config("S3Rec", synthetic="40x60x9", device="cpu", max_seq_len=6, model_dir=str(tmp_path), pretrain=True)
    with pytest.raises(NotImplementedError, match="pre-training"):
        train.train(cfg, train.build(cfg))


def test_store_refuses_cpu_tensors():
    import torch
    from yelprecommendation_amd._lib import EngineError
    from yelprecommendation_amd.data.s3rec_batches import S3RecSequences
    with pytest.raises(EngineError):
        S3RecSequences(torch.zeros(4, dtype=torch.int64), torch.arange(4), 1, 10, 6)
    with pytest.raises(EngineError):
        S3RecSequences.from_frame(pd.DataFrame({"behaviors": [[1, 2, 3]]}), 10, 6, "cpu")


def test_s3rec_batches_argument_codes():
    """Checked before any launch: -1, -2 and 0 without a GPU (fake aligned addresses, never dereferenced)."""
    from yelprecommendation_amd import _lib
    lib = _lib.load()
    a = 4096
    call = lambda num_items=100, B=4, L=6, mode=2, n_neg=99, ptrs=(a,) * 4, users=a, X=a, pos=a, neg=a: \
        lib.yr_s3rec_batches(*ptrs, 10, num_items, users, B, L, mode, n_neg, 1, 2, X, pos, neg, None, None)
    assert call(n_neg=129) == -1 and call(n_neg=129, B=0) == -1
    assert call(num_items=2**32 - 1, B=0) == 0 and call(num_items=2**32) == -1
    assert call(mode=3) == -1 and call(mode=-1) == -1
    assert call(B=-1) == -2 and call(L=0) == -2 and call(n_neg=-1) == -2 and call(num_items=0) == -2
    assert call(mode=0, n_neg=5, L=6) == -2                              # a negative per position: n_neg == L
    assert call(B=0) == 0 and call(B=0, mode=0, n_neg=6) == 0 and call(B=0, ptrs=(None,) * 4, users=None, X=None) == 0
    for missing in ("users", "X", "pos", "neg"):
        assert call(**{missing: None}) == -2
    for k in range(4):
        assert call(ptrs=tuple(None if j == k else a for j in range(4))) == -2
