"""S3Rec pre-training without a GPU: tests/s3rec_pretrain_ref64.py against the record of the reference
(tests/golden/s3rec_pretrain_small.npz), its wrong readings, the loop ends the GPU cases reach, the argument checks of
the catalogue-BCE entry points (no launch), the device-free part of the masking law and the CPU refusals."""
import os

import numpy as np
import pytest
import torch

import s3rec_pretrain_ref64 as R

F32 = np.float32
HEADS, BLOCKS = 2, 2


@pytest.fixture(scope="module")
def rec(golden_dir):
    g = np.load(os.path.join(golden_dir, "s3rec_pretrain_small.npz"))
    small = np.load(os.path.join(golden_dir, "s3rec_small.npz"))
    state = {k[5:]: small[k] for k in small.files if k.startswith("pert:")}
    batches = [dict(X=g[f"b{i}_X"], masks=g[f"b{i}_masks"], seg=g[f"b{i}_seg"], pos=g[f"b{i}_pos"], neg=g[f"b{i}_neg"])
               for i in range(3)]
    return dict(g=g, state=state, batches=batches, ptr=g["attr_ptr"], idx=g["attr_idx"])


@pytest.fixture(scope="module")
def both(rec):
    """The restatement of the first batch in float64 and float32, computed once."""
    args = (rec["state"], rec["batches"][0], rec["ptr"], rec["idx"], HEADS, BLOCKS)
    return R.step_and_grads(*args, dtype=torch.float64), R.step_and_grads(*args, dtype=torch.float32)


def test_the_record_holds_every_branch(rec):
    g, L = rec["g"], 12
    X, m = g["b0_X"], g["b0_masks"]
    pad = X == 0
    assert (pad & m).any() and (pad & ~m).any()                      # a masked and an unmasked padded position
    lens = R.check_segments(X, g["b0_seg"], g["b0_pos"], g["b0_neg"], L)
    assert ((lens >= 2) & (lens <= L // 2 - 1)).all()
    assert g["grad_none"].tolist() == ["map_weight.weight"]
    assert os.path.getsize(os.path.join(R.ROOT, "tests", "golden", "s3rec_pretrain_small.npz")) < 2 ** 20


def test_the_restatement_is_the_reference_in_float64(rec, both):
    g, (r64, r32) = rec["g"], both
    for k in R.OUTPUTS:
        np.testing.assert_allclose(r64[k], g[f"out64:{k}"], rtol=0, atol=1e-10)
    np.testing.assert_allclose([r64[k] for k in R.LOSSES[:4]], g["loss64"], rtol=0, atol=1e-10)
    none = sorted(k for k, v in r64["grads"].items() if v is None)
    assert none == sorted(g["grad_none"].tolist()) == sorted(k for k, v in r32["grads"].items() if v is None)
    for k, v in r64["grads"].items():
        if v is not None:
            np.testing.assert_allclose(v, g[f"grad64:{k}"], rtol=0, atol=1e-10)


def test_the_float32_record_is_inside_the_bar(rec, both):
    g, (r64, r32) = rec["g"], both
    for k in R.OUTPUTS:
        bar = R.bar_of(r32[k], r64[k])
        assert np.abs(g[f"out32:{k}"].astype(np.float64) - r64[k]).max() <= bar, k
    bars = R.loss_bars(rec["state"], rec["batches"], rec["ptr"], rec["idx"], HEADS, BLOCKS)
    for i, k in enumerate(R.LOSSES[:4]):
        assert abs(float(g["loss32"][i]) - r64[k]) <= bars[k], (k, abs(float(g["loss32"][i]) - r64[k]), bars[k])
    for k, v in r64["grads"].items():
        if v is not None:
            assert np.abs(g[f"grad32:{k}"].astype(np.float64) - v).max() <= R.bar_of(r32["grads"][k], v), k


def test_the_restated_epochs_are_the_recorded_ones(rec):
    losses, _ = R.train(rec["state"], rec["batches"], rec["ptr"], rec["idx"], HEADS, BLOCKS, 2, 1e-3, torch.float64)
    np.testing.assert_allclose([sum(e) for e in losses], rec["g"]["train_losses64"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("variant", R.STEP_VARIANTS)
def test_a_wrong_reading_of_the_step_crosses_a_bar(rec, both, variant):
    """On every recorded batch: some loss or some gradient leaves its bar (the smallest ratios are in DESIGN 4.10, Pre-training)."""
    worst = np.inf
    lbars = R.loss_bars(rec["state"], rec["batches"], rec["ptr"], rec["idx"], HEADS, BLOCKS)
    for i, b in enumerate(rec["batches"]):
        args = (rec["state"], b, rec["ptr"], rec["idx"], HEADS, BLOCKS)
        fbars = R.fused_loss_bars(*args)                              # the widest bar a GPU test puts on a loss
        r64, r32 = both if i == 0 else (R.step_and_grads(*args, dtype=torch.float64),
                                        R.step_and_grads(*args, dtype=torch.float32))
        bad = R.step_and_grads(*args, dtype=torch.float64, variant=variant)
        ratios = [abs(bad[k] - r64[k]) / max(lbars[k] + fbars[k], 1e-300) for k in R.LOSSES[:4]]
        for k, v in r64["grads"].items():
            w = bad["grads"][k]
            if (v is None) != (w is None):
                ratios.append(np.inf)                                 # the None set moved
            elif v is not None:
                ratios.append(np.abs(w - v).max() / max(R.bar_of(r32["grads"][k], v), 1e-300))
        worst = min(worst, max(ratios))
    print(f"{variant}: smallest (over the batches) largest ratio {worst:.3g}")
    assert worst > 1.0, (variant, worst)


KERNEL_CASES = R.kernel_cases()


def _applies(variant, case, g):
    if variant == "row_last_target_dropped":
        # needs a row whose list holds a column, whose targets count (yscale set) and whose logits do (zscale set:
        # at z = 0 the term -z y is 0 whatever y is, and g carries zscale)
        hit = R.dense_targets(g["key"], g["ptr"], g["idx"], g["K"], case["R"])
        return bool((hit.any(1) & (g["ys"] != 0) & (g["zs"] != 0)).any())
    if variant == "zscale_on_targets":
        return bool((g["zs"] == 0).any()) and not case["exact"]
    return True


@pytest.mark.parametrize("variant", R.KERNEL_VARIANTS)
def test_a_wrong_reading_of_the_kernel_crosses_a_bar(variant):
    worst = np.inf
    for case in KERNEL_CASES:
        if case["N"] * case["R"] > 300000:                            # the large cases repeat the small ones' law
            continue
        g = R.gen(case)
        if not _applies(variant, case, g):
            continue
        a = (g["F"], g["T"], g["zs"], g["ys"], g["key"], g["ptr"], g["idx"], g["K"])
        want, bad = R.catalogue_bce(*a), R.catalogue_bce(*a, variant=variant)
        if case["exact"]:                                             # the exact twin: any difference is caught
            assert any((np.asarray(bad[k].v, F32) != np.asarray(want[k].v, F32)).any() for k in ("row_loss", "dF", "dT")), \
                (variant, case["id"])
            continue
        r = max(R.ratio(bad[k].v, want[k], want[e]) for k, e in (("loss", "e_loss"), ("row_loss", "e_row"),
                                                                 ("dF", "e_dF"), ("dT", "e_dT")))
        worst = min(worst, r)
        assert r > 1.0, (variant, case["id"], r)
    print(f"{variant}: smallest ratio over the cases {worst:.3g}")


def test_every_gpu_case_reaches_its_loop_end():
    c = R.constants()
    t, chunk, grid, waves = c["kCbTile"], c["kCbColChunk"], c["kCbGridMax"], c["kWavesPerBlock"]
    by = {k["id"]: k for k in KERNEL_CASES}
    assert len(by) == len(KERNEL_CASES)
    shapes = {(k["N"], k["R"]) for k in KERNEL_CASES}
    for n in (1, t - 1, t, t + 1, 2 * t + 1):
        assert any(N == n for N, _ in shapes) and any(Rr == n for _, Rr in shapes)
    assert {33, 810, 38049} <= {Rr for _, Rr in shapes} and (33, 38049) in shapes and by["R38049-mip"]["E"] == 64
    assert {k["E"] for k in KERNEL_CASES} == {16, 32, 64, 128}
    assert {k["csr"] for k in KERNEL_CASES} == {True, False}
    assert all(k["N"] * k["R"] <= 3_000_000 for k in KERNEL_CASES)
    # partial tiles on both sides, a wave's range and a chunk at their ends and one past, the second trips
    assert R.plan_rows(t + 1, t + 1)["partial_row_tile"] and R.plan_rows(t + 1, t + 1)["partial_col_tile"]
    wave_cols = c["kCbTilesPerWave"] * t
    assert R.plan_rows(t + 1, wave_cols)["waves_last_chunk"] == 1 and R.plan_rows(t + 1, wave_cols + 1)["waves_last_chunk"] == 2
    assert (t + 1, wave_cols) in shapes and (t + 1, wave_cols + 1) in shapes
    assert R.plan_rows(t + 1, chunk)["chunks"] == 1 and R.plan_rows(t + 1, chunk + 1)["chunks"] == 2
    assert (t + 1, chunk) in shapes and (t + 1, chunk + 1) in shapes
    assert R.plan_rows(t + 1, chunk)["waves_last_chunk"] == waves
    k = by["rows-grid-second-trip"]
    assert R.plan_rows(k["N"], k["R"])["trips"] == 2 and R.plan_rows(k["N"] - t, k["R"])["trips"] == 1
    k = by["cols-grid-second-trip"]
    assert R.plan_cols(k["N"], k["R"])["trips"] == 2 and R.plan_cols(k["N"], k["R"] - t)["trips"] == 1
    k = by["cols-wave-second-trip"]
    assert R.plan_cols(k["N"], k["R"])["wave_trips"] == 2 and R.plan_cols(k["N"] - 1, k["R"])["wave_trips"] == 1
    assert R.plan_rows(33, 38049)["chunks"] > 2 and grid * t * 3 <= 3_000_000
    # what the CSR cases hold: no target, one, column 0, column R - 1, the longest list and the next shorter,
    # the last partial column tile; the bad keys first and last
    g = R.gen(by["E32-csr"])
    lens = np.diff(g["ptr"])
    Rr = by["E32-csr"]["R"]
    assert lens[0] == 0 and lens[1] == 1 and lens[3] == Rr and lens[4] == Rr - 1
    assert g["idx"][g["ptr"][1]] == 0 and g["idx"][g["ptr"][2]] == Rr - 1 and Rr % t != 0
    assert (g["idx"][g["ptr"][5]:g["ptr"][6]] >= Rr // t * t).all()
    assert set(range(6)) <= set(g["key"].tolist())
    g = R.gen(by["bad-first-last-csr"])
    assert g["key"][0] == -1 and g["key"][-1] == g["K"]
    g = R.gen(by["all-zscale-0"])
    assert (g["zs"] == 0).all()
    g = R.gen(by["alternating"])
    assert set(g["zs"].tolist()) == {0.0, 1.0}
    g = R.gen(by["R33-csr-aap"])
    assert (g["zs"] != g["ys"]).any()
    assert by["loss-only"]["loss_only"]


def test_the_rows_with_zscale_0_have_a_zero_bar():
    case = next(k for k in KERNEL_CASES if k["id"] == "alternating")
    g = R.gen(case)
    want = R.catalogue_bce(g["F"], g["T"], g["zs"], g["ys"], g["key"], g["ptr"], g["idx"], g["K"])
    off = g["zs"] == 0
    assert (want["dF"].v[off] == 0).all() and (want["e_dF"][off] == 0).all()
    np.testing.assert_allclose(want["row_loss"].v[off], case["R"] * np.log(2.0), rtol=1e-15)


def test_the_entry_points_are_exported_and_check_their_arguments():
    """-2, -1 and 0 before any launch (fake aligned addresses, never dereferenced: no GPU here)."""
    from yelprecommendation_amd import _lib
    lib = _lib.load()
    assert "yr_s3rec_catalogue_bce" in _lib.SIGNATURES and "yr_s3rec_catalogue_bce_workspace_floats" in _lib.SIGNATURES
    a = 4096
    ws = lib.yr_s3rec_catalogue_bce_workspace_floats
    assert ws(33, 810, 64) == R.workspace_floats(33, 810, 64) == 33 * (1 + 65)
    assert ws(33, 38049, 64) == R.workspace_floats(33, 38049, 64) and ws(0, 5, 16) == 0
    assert ws(-1, 5, 16) == -2 and ws(5, -1, 16) == -2 and ws(5, 5, 0) == -2 and ws(5, 5, 48) == -1

    def call(N=4, Rr=5, K=5, E=16, F=a, T=a, zs=a, ys=a, key=a, ptr=a, idx=a, loss=a, row=a, dF=a, dT=a, wsp=a, nws=None):
        nws = max(0, ws(max(N, 0), max(Rr, 0), E if E in (16, 32, 64, 128) else 16)) if nws is None else nws
        return lib.yr_s3rec_catalogue_bce(F, T, zs, ys, key, ptr, idx, N, Rr, K, E, loss, row, dF, dT, wsp, nws, None, None)

    assert call(N=-1) == -2 and call(Rr=-1) == -2 and call(K=-1) == -2 and call(E=0) == -2
    assert call(E=48) == -1 and call(E=256) == -1
    assert call(N=-1, E=48) == -2                                     # BADARG before UNSUPPORTED
    assert call(N=0) == 0 and call(Rr=0) == 0                         # empty: nothing to do, nothing dereferenced
    assert call(N=0, F=None, loss=None) == 0                          # empty before the null pointers
    assert call(N=0, E=48) == -1                                      # UNSUPPORTED before empty
    for name in ("F", "T", "zs", "ys", "key", "loss", "wsp"):
        assert call(**{name: None}) == -2, name
    assert call(ptr=None) == -2 and call(idx=None) == -2              # one half of the CSR without the other
    assert call(F=a + 4) == -2 and call(T=a + 8) == -2                # 16-byte alignment
    assert call(nws=ws(4, 5, 16) - 1) == -2                           # a workspace too small


def _cfg(tmp_path, **over):
    from yelprecommendation_amd.utils import make_config
    return make_config("S3Rec", **{**dict(device="cpu", max_seq_len=12, embed_size=32, model_dir=str(tmp_path)), **over})


def _attrs(n, count):
    out = {k: {"categories": [k % count, (3 * k + 1) % count]} for k in range(1, n + 1)}
    out[0] = {"categories": []}
    return out


def test_the_pretrainer_constructs_on_the_cpu_and_refuses_to_train(tmp_path):
    from yelprecommendation_amd.trainers.s3rec_trainer import S3RecPreTrainer, attribute_csr
    trainer = S3RecPreTrainer(_cfg(tmp_path), 100, _attrs(100, 7), 7)
    for fn in (trainer.train, trainer.pretrain):
        with pytest.raises(NotImplementedError, match="pre-training"):
            fn([])
    assert trainer.model.map_weight.weight.grad is None
    ptr, idx = attribute_csr(_attrs(100, 7), 100, 7)
    assert ptr.shape == (102,) and ptr[1] == 0 and (np.diff(ptr)[1:] >= 1).all()
    for k in range(1, 101):
        assert idx[ptr[k]:ptr[k + 1]].tolist() == sorted({k % 7, (3 * k + 1) % 7})
    with pytest.raises(ValueError, match="attribute id"):
        S3RecPreTrainer(_cfg(tmp_path), 100, _attrs(100, 7), 6)
    with pytest.raises(ValueError, match="sp_negative"):
        S3RecPreTrainer(_cfg(tmp_path), 100, _attrs(100, 7), 7, sp_negative="any")


@pytest.mark.parametrize("sp_negative", ["same_row", "other_row"])
def test_the_masking_law_on_the_host(tmp_path, sp_negative):
    from yelprecommendation_amd.trainers.s3rec_trainer import S3RecPreTrainer
    L = 12
    X = torch.from_numpy(np.random.RandomState(3).randint(1, 101, (64, L)))      # no pad: every segment is unambiguous
    runs = []
    for _ in range(2):                                                # the same seed, the same masks
        trainer = S3RecPreTrainer(_cfg(tmp_path, seed=11, mask_portion=0.3), 100, _attrs(100, 7), 7, sp_negative=sp_negative)
        masks, item_masked = trainer.item_level_masking(X)
        runs.append((masks, item_masked) + tuple(trainer.segment_masking(X)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    masks, item_masked, seg, pos, neg = runs[0]
    assert masks.dtype == torch.bool and torch.equal(item_masked, masks * X) and 0.15 < masks.float().mean() < 0.45
    lens = R.check_segments(X.numpy(), seg.numpy(), pos.numpy(), neg.numpy(), L)
    assert lens.min() >= 2 and lens.max() <= L // 2 - 1 and len(set(lens.tolist())) > 1
    Xn, negn = X.numpy(), neg.numpy()
    for b in range(X.shape[0]):                                       # the negative: a window of its source row, right-aligned
        n = int(lens[b])
        rows = [b] if sp_negative == "same_row" else [r for r in range(X.shape[0]) if r != b]
        assert (negn[b, :L - n] == 0).all()
        assert any((negn[b, L - n:] == Xn[r, s:s + n]).all() for r in rows for s in range(L - n)), b
    small = S3RecPreTrainer(_cfg(tmp_path, max_seq_len=5), 100, _attrs(100, 7), 7)
    with pytest.raises(ValueError, match="max_seq_len"):
        small.segment_masking(torch.zeros((2, 5), dtype=torch.int64))
    if sp_negative == "other_row":
        with pytest.raises(ValueError, match="two rows"):
            trainer.segment_masking(X[:1])


def test_the_model_refuses_cpu_tensors(tmp_path):
    from yelprecommendation_amd.models.s3rec import S3Rec
    model = S3Rec(_cfg(tmp_path), 100, 7)
    X = torch.zeros((2, 12), dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="pre-training"):
        model.pretrain_loss(X, X > 0, X, X, X, None, None)
    with pytest.raises(NotImplementedError, match="pre-training"):
        model.pretrain(X, X, X, X)
