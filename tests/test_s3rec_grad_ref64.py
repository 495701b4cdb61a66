"""CPU: the torch restatement of S3Rec fine-tuning (tests/s3rec_grad_ref64.py) against the NumPy restatement of the
forward (tests/s3rec_ref64.py) and against the gradients the reference recorded (tests/golden/
s3rec_train_small.npz), the dropout masks, and what the gradient bar still catches."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import s3rec_grad_ref64 as gr
import s3rec_ref64 as ref

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = gr.configs()
IDS = [gr.config_id(c, p) for c, p in CONFIGS]


@functools.lru_cache(maxsize=None)
def _baseline(index, p):
    case = ref.CASES[index]
    params, batch = gr.case_setup(case)
    hb = (case["heads"], case["blocks"])
    r64 = gr.loss_and_grads(params, batch, *hb, dtype=torch.float64, p_drop=p)
    r32 = gr.loss_and_grads(params, batch, *hb, dtype=torch.float32, p_drop=p)
    return params, batch, r64, gr.bars(r32["grads"], r64["grads"])


def test_configurations_are_the_issue_s():
    assert [c["id"] for c, p in CONFIGS if p == 0] == [c["id"] for c in ref.CASES]
    assert sorted({c["id"] for c, p in CONFIGS if p > 0}) == sorted(gr.DROPOUT_CASES)
    assert sorted({p for _, p in CONFIGS}) == [0.0, 0.1, 0.5]
    assert {c["B"] for c, p in CONFIGS if p > 0} >= {3, 257}


@pytest.mark.parametrize("case", ref.CASES, ids=[c["id"] for c in ref.CASES])
def test_forward_equals_the_numpy_restatement(case):
    params, batch, r64, _ = _baseline(case["index"], 0.0)
    hb = (case["heads"], case["blocks"])
    h = ref.encode(params, batch["X"], *hb)
    pos, neg = ref.finetune(params, batch["X"], batch["pos_items"], batch["neg_items"], *hb, h=h)
    assert r64["h"].dtype == np.float64
    for got, want in ((r64["h"], h), (r64["pos"], pos), (r64["neg"], neg)):
        assert float(np.max(np.abs(got - want))) <= 1e-12


@pytest.fixture(scope="module")
def record():
    g = np.load(os.path.join(HERE, "golden", "s3rec_small.npz"))
    t = np.load(os.path.join(HERE, "golden", "s3rec_train_small.npz"))
    cfg = dict(zip(g["cfg_names"].tolist(), g["cfg_values"].tolist()))
    state = {k[5:]: g[k] for k in g.files if k.startswith("pert:")}
    batch = {k: g[f"valid0_{k}"] for k in ("X", "pos_items", "neg_items")}
    hb = (cfg["num_heads"], cfg["num_blocks"])
    r64 = gr.loss_and_grads(state, batch, *hb, dtype=torch.float64)
    r32 = gr.loss_and_grads(state, batch, *hb, dtype=torch.float32)
    return t, r64, r32


def test_float64_gradients_equal_the_reference_s(record):
    t, r64, _ = record
    assert abs(r64["loss"] - float(t["grad64_loss"])) <= 1e-12
    took_part = [k for k, v in r64["grads"].items() if v is not None]
    assert len(took_part) == 34 and sorted(f"grad64:{k}" for k in took_part) == \
        sorted(k for k in t.files if k.startswith("grad64:"))
    for name in took_part:
        assert float(np.max(np.abs(r64["grads"][name] - t[f"grad64:{name}"]))) <= 1e-10, name


def test_the_none_set_matches_the_record(record):
    t, r64, r32 = record
    want = sorted(t["grad_none"].tolist())
    assert want == sorted(["attribute_embedding.weight", "aap_weight.weight", "mip_weight.weight", "map_weight.weight",
                           "sp_weight.weight"])
    for r in (r64, r32):
        assert sorted(k for k, v in r["grads"].items() if v is None) == want


def test_the_reference_s_float32_record_lies_inside_the_bar(record):
    t, r64, r32 = record
    bars = gr.bars(r32["grads"], r64["grads"])
    for name, bar in bars.items():
        err = float(np.max(np.abs(t[f"grad32:{name}"].astype(np.float64) - r64["grads"][name])))
        assert err <= bar, (name, err, bar)


@pytest.mark.parametrize("case,p", CONFIGS, ids=IDS)
def test_every_wrong_reading_moves_a_gradient_past_its_bar(case, p):
    """Smallest max_tensor(|grad_variant - grad| / bar) over the configurations each reading applies to (every one
    must exceed 1; measured with this file, printed by the test):
        residual_to_x1 4.2e+05, key_mask_not_in_dK 8.3e+04, scale_not_in_dS 5.0e+05, padding_out_of_mean 4.9e+05,
        dropout_unscaled 1.3e+05."""
    params, batch, r64, bars = _baseline(case["index"], p)
    hb = (case["heads"], case["blocks"])
    for variant in gr.VARIANTS:
        if not gr.applies(variant, case, p):
            continue
        v = gr.loss_and_grads(params, batch, *hb, dtype=torch.float64, p_drop=p, variant=variant)
        ratio = max((float(np.max(np.abs(v["grads"][k] - r64["grads"][k]))) / bar if bar > 0 else
                     (math.inf if np.any(v["grads"][k] != r64["grads"][k]) else 0.0)) for k, bar in bars.items())
        print(f"{gr.config_id(case, p)} {variant}: ratio {ratio:.3e}")
        assert ratio > 1, (variant, ratio)


def test_exact_zeros_have_a_zero_bar():
    """A batch with no padded key: every K row is masked to zero, so dW_k (through the mask) and dW_q (dQ = dS K) are
    exactly zero in both restatements, and the bar asks the kernel for exactly zero."""
    case = next(c for c in ref.CASES if (c["E"], c["L"], c["B"]) == (16, 7, 3))
    params, batch = gr.case_setup(case)
    batch = dict(batch, X=np.maximum(batch["X"], 1))
    hb = (case["heads"], case["blocks"])
    r64 = gr.loss_and_grads(params, batch, *hb, dtype=torch.float64)
    r32 = gr.loss_and_grads(params, batch, *hb, dtype=torch.float32)
    bars = gr.bars(r32["grads"], r64["grads"])
    for name, bar in bars.items():
        assert (bar == 0) == ("k_weights" in name or "q_weights" in name), name


def test_dropout_masks():
    B, L, E, blocks = 25, 25, 64, 2                                   # 40,000 elements per site
    n = B * L * E
    for p in (0.1, 0.5):
        m = gr.dropout_masks(gr.DROPOUT_SEED, p, B, L, E, blocks)
        assert m.shape == (2 * blocks, B, L, E) and m.dtype == bool
        sigma = math.sqrt(p * (1 - p) / n)
        for site in range(2 * blocks):
            assert abs(m[site].mean() - (1 - p)) <= 4 * sigma, (p, site)
            for other in range(site):
                assert not np.array_equal(m[site], m[other])
        assert not np.array_equal(m, gr.dropout_masks(gr.DROPOUT_SEED + 1, p, B, L, E, blocks))
        assert np.array_equal(m, gr.dropout_masks(gr.DROPOUT_SEED, p, B, L, E, blocks))
    assert gr.dropout_masks(7, 0.0, 2, 3, 16, 1).all()


def test_dropout_masks_are_yr_dropout_seeded_at_site_0():
    """Site 0 draws at the counter (q lo, q hi, 0, 0): the mask yr_dropout_seeded applies."""
    from gemm_ref64 import dropout_seeded
    x = np.ones(3 * 7 * 16, np.float32)
    m = gr.dropout_masks(99, 0.3, 3, 7, 16, 1)
    assert np.array_equal(m[0].reshape(-1), dropout_seeded(x, 99, 0.3) != 0)
