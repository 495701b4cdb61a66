"""Without a GPU: the cases of ngcf_owned_cases.py can tell a wrong summation order from the contract's, their expected
values agree with the float64 restatement of tests/ngcf_ref64.py, and the entry points of csrc/ngcf_owned.hip and the
ordered step refuse what they must before any launch (error codes, workspace sizes)."""
import ctypes

import numpy as np
import pytest

import ngcf_owned_cases as O
import ngcf_ref64 as R


def test_cases_can_see_a_wrong_order():
    """Rows of 24 contributions at D = 16: summed in reversed (and in a random) order at least one element of the row
    changes, for at least 9 rows in 10 — an owner pass that walked its segment by arrival slot would be caught."""
    c = O.order_case()
    assert O.products_are_exact(c)
    contrib = O.contributions(c, 0)
    rows = [r for r, t in contrib.items() if r < c["num_users"] and len(t) >= 16]
    assert len(rows) == 40
    rs = np.random.RandomState(1)
    differ_rev = differ_rnd = 0
    for r in rows:
        t = contrib[r]
        zero = np.zeros(16, np.float32)
        want = O.ordered_sum(zero, t)
        differ_rev += not np.array_equal(want, O.ordered_sum(zero, t, range(len(t) - 1, -1, -1)))
        differ_rnd += not np.array_equal(want, O.ordered_sum(zero, t, rs.permutation(len(t))))
    assert differ_rev * 10 >= 9 * len(rows) and differ_rnd * 10 >= 9 * len(rows), (differ_rev, differ_rnd)


@pytest.mark.parametrize("with_neg", [True, False])
def test_expected_agrees_with_float64(with_neg):
    """The sequential f32 loop against ngcf_ref64.score_bwd (float64) under the project's "de" bar, on the mixed batch
    (bad ids skipped, pos == neg, an item in both roles); the premise of the loop — exact products — holds for every
    case the GPU test uses."""
    c = O.mixed_case(16, 3, with_neg)
    assert O.products_are_exact(c) and O.flags_expected(c) == 3
    got = O.expected(c, 0.0)
    ref = R.score_bwd(c["layers"], c["num_users"], c["u"], c["p"], c["n"], c["gpos"], c["gneg"])
    for k in range(3):
        assert R.ratio(got[k], ref[k], "de") <= 1.0
    u = c["u"][O.valid(c)]
    assert (u == O.HOT_USER).sum() == 48
    for D in O.WIDTHS:
        for B in O.batches(D):
            assert O.products_are_exact(O.score_case(D, 3, B, with_neg))
    assert O.products_are_exact(O.long_row_case(16, 1))
    # untouched rows keep the pre-fill
    sent = O.expected(c, R.SENTINEL)[0]
    touched = np.zeros(len(sent), bool)
    touched[list(O.contributions(c, 0))] = True
    assert (~touched).any() and (sent[~touched] == np.float32(R.SENTINEL)).all()


def _lib():
    from yelprecommendation_amd import _lib
    return _lib.load(), _lib


def test_new_exports_and_workspace_sizes():
    lib, L = _lib()
    for name in ("yr_ngcf_owned_score_workspace_bytes", "yr_ngcf_owned_score_bwd", "yr_ngcf_owned_dw_workspace_bytes",
                 "yr_ngcf_owned_dense_bwd_weight", "yr_ngcf_frontier_order", "yr_ngcf_step_ordered_workspace_bytes",
                 "yr_ngcf_bpr_step_ordered"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.yr_engine_version() == 36
    score, dw, step = (lib.yr_ngcf_owned_score_workspace_bytes, lib.yr_ngcf_owned_dw_workspace_bytes,
                       lib.yr_ngcf_step_ordered_workspace_bytes)
    assert score(0, 10) == -2 and score(10, -1) == -2 and score(1 << 31, 10) == -2
    assert score(100, 1 << 29) == -1                                  # 4 B + role no longer fits an int32
    assert score(100, (1 << 29) - 1) > 0
    assert dw(-1, 64) == -2 and dw(10, 48) == -1 and dw(0, 64) == 0
    assert step(0, 64, 3, 10) == -2 and step(100, 48, 3, 10) == -1 and step(100, 64, 8, 10) == -2
    assert step(100, 64, 3, 1 << 29) == -1
    n = 31668 + 38048
    last = last_step = 0
    for B in (0, 1, 32, 4096, 65536, 1 << 20):
        assert score(n, B) >= max(last, 36 * B) and score(n, B) % 256 == 0
        last = score(n, B)
        s = step(n, 64, 3, B)
        # the ordered step holds what the default step holds, the counting sort and the slots of the weight gradient
        assert s >= last_step and s >= lib.yr_ngcf_step_workspace_bytes(n, 64, 3, B) + last + dw(n, 64)
        last_step = s
    # the slots: one per workgroup, at most 256 of 2 D^2 floats; a size for `rows` serves every smaller row count
    for D in R.WIDTHS:
        sizes = [dw(r, D) for r in (1, R.wrows(D), R.wrows(D) + 1, 255 * R.wrows(D), 256 * R.wrows(D), 257 * R.wrows(D), n)]
        assert sizes == sorted(sizes) and sizes[0] == 2 * D * D * 4 and sizes[-1] == 256 * 2 * D * D * 4
    assert dw(n, 128) == 256 * 2 * 128 * 128 * 4                      # 33.5 MB at D = 128 (DESIGN's memory table)


def test_argument_checks_without_gpu():
    lib, _ = _lib()
    arr = (ctypes.c_void_p * 2)(0, 0)
    one = ctypes.c_void_p(256)                                        # a non-null, aligned address that is never read
    # score backward: sizes first, then the empty batch, then pointers
    f = lib.yr_ngcf_owned_score_bwd
    assert f(arr, arr, 2, None, None, None, None, None, -1, 64, 40, 50, None, 0, None, None) == -2
    assert f(arr, arr, 0, None, None, None, None, None, 1, 64, 40, 50, None, 0, None, None) == -2
    assert f(arr, arr, 9, None, None, None, None, None, 1, 64, 40, 50, None, 0, None, None) == -2
    assert f(arr, arr, 2, None, None, None, None, None, 1, 48, 40, 50, None, 0, None, None) == -1
    assert f(arr, arr, 2, None, None, None, None, None, 1 << 29, 64, 40, 50, None, 0, None, None) == -1
    assert f(arr, arr, 2, None, None, None, None, None, 0, 64, 40, 50, None, 0, None, None) == 0
    assert f(arr, arr, 2, None, None, None, None, None, 1, 64, 40, 50, None, 0, None, None) == -2        # null ids
    assert f(arr, arr, 2, one, one, one, one, None, 1, 64, 40, 50, one, 1 << 20, None, None) == -2       # neg without gneg
    assert f(arr, arr, 2, one, one, one, one, one, 1, 64, 40, 50, one, 16, None, None) == -2             # workspace too small
    assert f(arr, arr, 2, one, one, one, one, one, 1, 64, 40, 50, ctypes.c_void_p(260), 1 << 20, None, None) == -2
    assert f(arr, arr, 2, one, one, one, one, one, 1, 64, 40, 50, one, 1 << 20, None, None) == -2        # null layers
    # ordered weight gradient
    g = lib.yr_ngcf_owned_dense_bwd_weight
    assert g(None, None, None, None, -1, 64, None, None, None, None, 0, None, 0, None) == -2
    assert g(None, None, None, None, 10, 48, None, None, None, None, 0, None, 0, None) == -1
    assert g(None, None, None, None, 0, 64, None, None, None, None, 0, None, 0, None) == 0
    assert g(None, None, None, None, 10, 64, None, None, one, one, 0, None, 0, None) == 0                # max_rows = 0
    assert g(None, None, None, None, 10, 64, None, None, one, None, 5, None, 0, None) == -2              # list without count
    assert g(None, None, None, None, 10, 64, None, None, None, one, 0, None, 0, None) == -2              # count without list
    assert g(None, None, None, None, 10, 64, None, None, one, one, 11, None, 0, None) == -2              # max_rows > n
    assert g(one, one, one, one, 10, 64, one, one, None, None, 0, None, 1 << 20, None) == -2             # no workspace
    assert g(one, one, one, one, 10, 64, one, one, None, None, 0, one, 16, None) == -2                   # too small
    assert g(one, one, one, one, 10, 64, ctypes.c_void_p(260), one, None, None, 0, one, 1 << 20, None) == -2
    # ordered row list
    h = lib.yr_ngcf_frontier_order
    assert h(None, -1, None, None, None) == -2 and h(None, 10, None, None, None) == -2
    assert h(None, 10, one, one, None) == -2 and h(one, 10, one, one, None) == -2                        # in place
    assert h(ctypes.c_void_p(260), 10, one, one, None) == -2                                             # misaligned flags
    # the ordered step refuses what the default step refuses, before any launch
    s = lib.yr_ngcf_bpr_step_ordered
    args = lambda n, D, mode: (None, None, None, n, 10, None, 0, 0, 5, None, None, None, 2, D, None, None, None, 0,
                               1e-3, 1e-3, 1.0, 0.9, 0.999, 1e-8, 0.0, mode, 0.5, None, 0, None, None, None, None)
    assert s(*args(0, 64, 0)) == -2 and s(*args(10, 48, 0)) == -1 and s(*args(10, 64, 7)) == -1
    assert s(*args(10, 64, 0)) == -2 and lib.yr_ngcf_bpr_step(*args(10, 64, 0)) == -2                    # null graph


def test_deterministic_needs_the_fused_adam_step():
    from yelprecommendation_amd.ngcf_step import DETERMINISTIC_NEEDS, deterministic_available
    assert deterministic_available({"optimizer": "adam"}) and deterministic_available({"optimizer": "AdamW"})
    assert not deterministic_available({"optimizer": "sgd"})
    assert not deterministic_available({"optimizer": "adam", "fused_step": False})
    assert "fused" in DETERMINISTIC_NEEDS and "adam" in DETERMINISTIC_NEEDS and "sgd" in DETERMINISTIC_NEEDS
