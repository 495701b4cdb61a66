"""yr_cdae_catalogue_bce (csrc/cdae_catalogue.hip) at the ends of its loops, through the C ABI into sentinel-filled
buffers with guard bands (workspace included), EVERY element of row_loss, dz, dW_o and db_o against
tests/cdae_catalogue_ref64.py (float64) inside the bar the helper derives.  The case list is
``cdae_catalogue_ref64.kernel_cases()``; tests/test_cdae_catalogue_ref64.py proves without a GPU that every case
reaches the loop end it is there for.  Two calls must agree bit for bit, a row alone must give the bits it gives
inside a larger batch (row_loss, dz), and on saturated pre-activations the sweep must say what the dense decoder
(yr_cdae_decode_loss and the two gradient products) says — where BCE-with-logits would not."""
import numpy as np
import pytest
import torch

import cdae_catalogue_ref64 as R

pytestmark = pytest.mark.gpu
F32 = np.float32
S, G = R.SENTINEL, R.GUARD
CASES = R.kernel_cases()
NAMES = ("row_loss", "dz", "dWo", "dbo")


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


class Guarded:
    """A sentinel-filled flat f32 buffer: G floats, n floats, G floats; ``ptr`` addresses element 0."""

    def __init__(self, n, device):
        self.n = n
        self.flat = torch.full((2 * G + n,), float(S), dtype=torch.float32, device=device)
        self.ptr = self.flat.data_ptr() + 4 * G

    def read(self, what):
        assert bool((self.flat[:G] == S).all()) and bool((self.flat[G + self.n:] == S).all()), (what, "a guard band was written")
        return self.flat[G:G + self.n].cpu().numpy()


def run(g, device, loss_only=False, rows=None):
    """One call; returns dict(row_loss, dz, dWo, dbo as f32 arrays, flag, status).  ``rows``: a slice of the batch."""
    from yelprecommendation_amd import _lib, engine
    lib = _lib.load()
    sl = slice(None) if rows is None else rows
    z, Wo, bo, user = _t(g["z"][sl], device), _t(g["Wo"], device), _t(g["bo"], device), _t(g["user"][sl], device)
    ptr, idx = _t(g["ptr"], device), _t(np.concatenate([g["idx"], [0]]), device)           # never empty storage
    (B, H), I = z.shape, Wo.shape[0]
    nws = lib.yr_cdae_catalogue_bce_workspace_floats(B, I, H)
    assert nws == R.workspace_floats(B, I, H)
    if loss_only:
        nws //= 1 + H                                                   # what the call without dz needs
    row, dz, dWo, dbo = Guarded(B, device), Guarded(B * H, device), Guarded(I * H, device), Guarded(I, device)
    ws = Guarded(nws, device)
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    status = lib.yr_cdae_catalogue_bce(z.data_ptr(), Wo.data_ptr(), bo.data_ptr(), user.data_ptr(), ptr.data_ptr(),
                                       idx.data_ptr(), B, I, g["K"], H, g["act"], row.ptr,
                                       None if loss_only else dz.ptr, None if loss_only else dWo.ptr,
                                       None if loss_only else dbo.ptr, ws.ptr, nws, flag.data_ptr(), engine._stream())
    torch.cuda.synchronize()
    ws.read("workspace")
    return dict(status=status, flag=int(flag.item()), row_loss=row.read("row_loss"), dz=dz.read("dz").reshape(B, H),
                dWo=dWo.read("dWo").reshape(I, H), dbo=dbo.read("dbo"))


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_catalogue_bce(device, case):
    g = R.gen(case)
    want = R.reference(case, g)
    got = run(g, device, loss_only=case["loss_only"])
    assert got["status"] == 0 and got["flag"] == want["flag"] == (R.FLAG_BAD_ITEM if case["keys"] == "bad" else 0)
    again = run(g, device, loss_only=case["loss_only"])
    for k in NAMES:                                                     # two calls, one answer
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), (case["id"], k)
    if case["loss_only"]:
        assert all((got[k] == S).all() for k in ("dz", "dWo", "dbo")), case["id"]
    for k, bar_fn in R.BARS:
        if case["loss_only"] and k != "row_loss":
            continue
        r = R.ratio(got[k], want[k], bar_fn)
        print(f"{case['id']}: {k} max err / bar = {r:.4f}")
        assert r < 1.0, (case["id"], k, r)


def test_a_row_alone_is_the_row_in_a_larger_batch(device):
    """row_loss and dz of a row do not depend on B: the column chunks are a constant of the kernel."""
    n_all = 64                    # a power of two: 1 / (B I) of the row alone is 64 times that of the batch, exactly
    g = R.gen(R._case("row-alone", n_all, R.constants()["chunk"] + 1, 32, 1))
    whole = run(g, device)
    for n in (0, 31, 32, n_all - 1):
        alone = run(g, device, rows=slice(n, n + 1))
        assert np.array_equal(alone["row_loss"].view(np.uint32), whole["row_loss"][n:n + 1].view(np.uint32)), n
        v = np.abs(whole["dz"][n])
        assert (v[v > 0] > 2.0 ** -100).all()                           # no underflow: the scaling below is exact
        # 1 / (64 I) and 1 / I as f32: the first is the second times 2^-6 exactly, and g (1 / (B I)) scales with it
        assert np.array_equal(alone["dz"][0].view(np.uint32), (whole["dz"][n] * F32(n_all)).view(np.uint32)), n


def test_saturated_pre_activations_say_what_the_dense_decoder_says(device):
    """Pre-activations of exactly +-30 and +-120 against both target values, sigmoid output: the expected values are the
    parent's dense route on the same inputs — yr_cdae_decode_loss (negative_mask = None), then the two gradient
    products as CDAEStep runs them — and the sweep must lie within the helper's bars of them.  BCE-with-logits would
    give 30 (not 100) and a gradient of 1 (not 0) at pre = 30, t = 0."""
    from yelprecommendation_amd import engine
    g = R.saturation_case()
    want = R.catalogue_bce(g["z"], g["Wo"], g["bo"], g["user"], g["ptr"], g["idx"], g["K"], g["act"])
    got = run(g, device)
    assert got["status"] == 0 and got["flag"] == 0
    z, Wo, bo = _t(g["z"], device), _t(g["Wo"], device), _t(g["bo"], device)
    x = _t(want["target"].astype(F32), device)
    (B, H), I = z.shape, Wo.shape[0]
    Gm = torch.empty(B, I, dtype=torch.float32, device=device)
    partials = torch.zeros(engine.cdae_decode_loss_partials(B, I), dtype=torch.float32, device=device)
    count = torch.zeros(engine.COUNT_WORDS, dtype=torch.int32, device=device)
    engine.cdae_decode_loss(z, Wo, bo, x, None, g["act"], Gm, partials, count)
    assert int(count.sum().item()) == B * I
    dWo, dbo = torch.empty_like(Wo), torch.empty_like(bo)
    dz = torch.zeros_like(z)
    engine.gemm_f32(Gm, z, transA=True, out=dWo, alpha_count=count, rowsum=dbo)
    engine.gemm_f32(Gm, Wo, out=dz, accumulate=True, split_k=1, alpha_count=count)
    dense = dict(dz=dz.cpu().numpy(), dWo=dWo.cpu().numpy(), dbo=dbo.cpu().numpy())
    dense_loss = float(partials.double().sum().item())
    # the saturation is in the expected values: the term at (30, t = 0) is 100 and its gradient exactly 0
    Gh, t = Gm.cpu().numpy(), want["target"]
    pre = g["z"].astype(np.float64) @ g["Wo"].astype(np.float64).T
    assert (Gh[(pre == 30.0) & (t == 0)] == 0).all() and (Gh[(pre == -120.0) & (t == 1)] == 0).all()
    n_100 = int((((pre >= 30.0) & (t == 0)) | ((pre == -120.0) & (t == 1))).sum())
    n_30 = int(((pre == -30.0) & (t == 1)).sum())
    assert abs(dense_loss - (100.0 * n_100 + 30.0 * n_30)) < 1e-3 * dense_loss
    total = R.Out(dense_loss, want["loss"].n, want["loss"].s)
    err = abs(float(got["row_loss"].astype(np.float64).sum()) - dense_loss)
    print(f"saturation: loss {got['row_loss'].astype(np.float64).sum():.6f} dense {dense_loss:.6f} "
          f"bar {float(R.loss_bar(total)):.3e}")
    assert err <= float(R.loss_bar(total))
    for k in ("dz", "dWo", "dbo"):
        o = R.Out(dense[k].astype(np.float64), want[k].n, want[k].s)
        r = R.ratio(got[k], o, R.bar)
        print(f"saturation: {k} max err / bar = {r:.4f}")
        assert r < 1.0, (k, r)
    # and each row's loss is the exact sum the dense terms give: 100 and 30 are exact in f32
    row_terms = np.where(((pre >= 30.0) & (t == 0)) | ((pre == -120.0) & (t == 1)), 100.0,
                         np.where((pre == -30.0) & (t == 1), 30.0, 0.0)).sum(1)
    assert np.abs(got["row_loss"] - row_terms).max() < 1e-3


def test_the_engine_wrapper_is_the_c_call(device):
    from yelprecommendation_amd import engine
    case = next(c for c in CASES if c["id"] == "B33-I2048-H32-sig")
    g = R.gen(case)
    raw = run(g, device)
    args = (_t(g["z"], device), _t(g["Wo"], device), _t(g["bo"], device), _t(g["user"], device), _t(g["ptr"], device),
            _t(g["idx"], device), g["act"])
    out = engine.cdae_catalogue_bce(*args)
    for a, k in zip(out, NAMES):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), raw[k].view(np.uint32)), k
    row2, dz2, dWo2, dbo2 = engine.cdae_catalogue_bce(*args, grads=False)
    assert dz2 is dWo2 is dbo2 is None and torch.equal(row2, out[0])
