"""CPU: the certified cases of NGCF's layered evaluation sweep (tests/ngcf_eval_cases.py) build, their column split
reproduces the float64 scores, and yr_ngcf_eval_topk / yr_ngcf_eval_topk_workspace_bytes check their arguments before
any pointer is read."""
import numpy as np
import pytest

import ngcf_eval_cases as nc


@pytest.mark.parametrize("spec", nc.SPECS, ids=nc.spec_id)
def test_spec_certifies_and_the_layer_split_keeps_the_scores(spec):
    D, layers, N, rows, k = spec
    case = nc.build(spec)                                   # build_case asserts the certificate
    assert case.D == D * layers and case.I.shape == (N, D * layers) and len(case.users) == rows
    tables, num_users = nc.layer_tables(case, D, layers)
    assert len(tables) == layers and all(t.shape == (num_users + N, D) and t.dtype == np.float32 for t in tables)
    S = np.zeros((rows, N))
    for E in tables:
        E = E.astype(np.float64)
        S += E[case.users] @ E[num_users:].T
    want = case.scores64()
    assert np.allclose(S[:, case.rep], want, rtol=1e-13)
    # ... and to what two float64 summation orders of W products can differ by: W 2^-53 A each (cancellation rows have
    # |score| << A, so a bound relative to the score itself would not hold for them)
    A = case.scale64(np.arange(rows))
    assert np.all(np.abs(S[:, case.rep] - want) <= 2 * D * layers * 2.0 ** -53 * A)


def test_argument_checks_without_gpu():
    """Range checks first (n_layers, k, sizes: BADARG; width, k > 16: UNSUPPORTED), an empty batch is 0, and only then
    the null pointers are refused — as yr_mf_eval_topk_bias in test_host_logic.py."""
    from yelprecommendation_amd import _lib
    lib = _lib.load()

    def call(n_layers=3, D=64, nrows=4, num_users=10, num_items=10, k=10):
        return lib.yr_ngcf_eval_topk(None, n_layers, D, None, nrows, num_users, num_items, None, None, 0.0, k, None,
                                     None, 0, None, None, None)
    assert call(n_layers=0) == -2 and call(n_layers=9) == -2
    assert call(k=0) == -2 and call(nrows=-1) == -2 and call(num_items=0x7ffffff1) == -2 and call(num_users=0) == -2
    assert call(D=48) == -1
    assert call(k=17) == -1
    assert call(n_layers=9, D=48) == -2                     # the range checks come first
    assert call(nrows=0) == 0
    assert call() == -2                                     # everything in range: now the null pointers
    ws = lib.yr_ngcf_eval_topk_workspace_bytes
    assert ws(4, 10, 0, 64, 10) == -2 and ws(4, 10, 9, 64, 10) == -2 and ws(-1, 10, 3, 64, 10) == -2
    assert ws(4, 10, 3, 48, 10) == -1 and ws(4, 10, 3, 64, 17) == -1
    assert ws(0, 10, 3, 64, 10) == 0
    assert ws(128, 1000, 3, 64, 10) == 512                  # one slice: the row thresholds only
    assert ws(130, 4100, 3, 64, 10) == 768 + 130 * 2 * 10 * 8   # two slices of partial lists
    # the slice rule (et_slices) at the full shape (248 row blocks -> 3 slices) and for a small batch (8 slices)
    assert ws(31668, 38048, 3, 64, 10) == (31668 * 4 + 255) // 256 * 256 + 31668 * 3 * 10 * 8
    assert ws(300, 16411, 3, 64, 16) == 1280 + 300 * 8 * 16 * 8
