"""yr_s3rec_catalogue_bce (csrc/s3rec_pretrain.hip) at the ends of its loops, through the C ABI into sentinel-filled
buffers with guard bands, EVERY element of loss, row_loss, dF and dT against tests/s3rec_pretrain_ref64.py (float64):
inside the closed-form bar the helper derives, EQUAL to float64 on the exact twins, exactly zero where zscale is 0.
The case list is ``s3rec_pretrain_ref64.kernel_cases()``; tests/test_s3rec_pretrain_ref64.py proves without a GPU
that every case reaches the loop end it is there for.  Two calls must agree bit for bit, and a row alone must give the
bits it gives inside a larger N (row_loss, dF)."""
import numpy as np
import pytest
import torch

import s3rec_pretrain_ref64 as R

pytestmark = pytest.mark.gpu
F32 = np.float32
S, G = R.SENTINEL, R.GUARD
CASES = R.kernel_cases()
WORST = {}


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _lib():
    from yelprecommendation_amd import _lib as L
    return L.load()


def _stream():
    from yelprecommendation_amd import engine
    return engine._stream()


class Guarded:
    """A sentinel-filled flat f32 buffer: G floats, n floats, G floats; ``ptr`` addresses element 0."""

    def __init__(self, n, device):
        self.n = n
        self.flat = torch.full((2 * G + n,), S, dtype=torch.float32, device=device)
        self.ptr = self.flat.data_ptr() + 4 * G

    def read(self, what):
        assert bool((self.flat[:G] == S).all()) and bool((self.flat[G + self.n:] == S).all()), (what, "a guard band was written")
        return self.flat[G:G + self.n].cpu().numpy()


def run(g, device, loss_only=False, rows=None):
    """One call; returns dict(loss, row_loss, dF, dT as f32 arrays, flag, status).  ``rows``: a slice of the rows of F."""
    sl = slice(None) if rows is None else rows
    F, T = _t(g["F"][sl], device), _t(g["T"], device)
    zs, ys, key = _t(g["zs"][sl], device), _t(g["ys"][sl], device), _t(g["key"][sl], device)
    (N, E), Rr = F.shape, T.shape[0]
    ptr = idx = None
    if g["ptr"] is not None:
        ptr, idx = _t(g["ptr"], device), _t(np.concatenate([g["idx"], [0]]), device)    # never empty storage
    lib = _lib()
    nws = lib.yr_s3rec_catalogue_bce_workspace_floats(N, Rr, E)
    assert nws == R.workspace_floats(N, Rr, E)
    loss, row = Guarded(1, device), Guarded(N, device)
    dF, dT, ws = Guarded(N * E, device), Guarded(Rr * E, device), Guarded(nws, device)
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    status = lib.yr_s3rec_catalogue_bce(F.data_ptr(), T.data_ptr(), zs.data_ptr(), ys.data_ptr(), key.data_ptr(),
                                        None if ptr is None else ptr.data_ptr(), None if idx is None else idx.data_ptr(),
                                        N, Rr, g["K"], E, loss.ptr, row.ptr, None if loss_only else dF.ptr,
                                        None if loss_only else dT.ptr, ws.ptr, nws, flag.data_ptr(), _stream())
    torch.cuda.synchronize()
    ws.read("workspace")
    out = dict(status=status, flag=int(flag.item()), loss=loss.read("loss"), row_loss=row.read("row_loss"),
               dF=dF.read("dF").reshape(N, E), dT=dT.read("dT").reshape(Rr, E))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_catalogue_bce(device, case):
    g = R.gen(case)
    want = R.catalogue_bce(g["F"], g["T"], g["zs"], g["ys"], g["key"], g["ptr"], g["idx"], g["K"])
    got = run(g, device, loss_only=case["loss_only"])
    assert got["status"] == 0 and got["flag"] == want["flag"] == (R.FLAG_BAD_ITEM if case["keys"] == "bad" else 0)
    again = run(g, device, loss_only=case["loss_only"])
    for k in ("loss", "row_loss", "dF", "dT"):                        # two calls, one answer
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), (case["id"], k)
    names = ("loss", "row_loss") if case["loss_only"] else ("loss", "row_loss", "dF", "dT")
    if case["loss_only"]:
        assert (got["dF"] == S).all() and (got["dT"] == S).all()
    if case["exact"]:
        ok_g, ok_l = R.certificate(g, want)
        assert ok_g and ok_l, case["id"]
        for k in names:
            # float64 keeps sigmoid(-129) = 1e-56 and log1p(exp(-129)) where f32 has 0: its value ROUNDED to f32 is
            # the exact multiple the certificate speaks of
            v = want[k].v.reshape(got[k].shape).astype(F32)
            bad = np.flatnonzero((got[k] != v).reshape(-1))
            assert bad.size == 0, (case["id"], k, "differs from float64 at", bad[:8])
        return
    for k, bar in (("loss", "e_loss"), ("row_loss", "e_row"), ("dF", "e_dF"), ("dT", "e_dT")):
        if k not in names:
            continue
        r = R.ratio(got[k], want[k], want[bar])
        print(f"{case['id']}: {k} max err / bar = {r:.4f}")
        WORST[k] = max(WORST.get(k, 0.0), r)
        assert r < 1.0, (case["id"], k, r)
    off = g["zs"] == 0
    if off.any():
        # exactly zero gradient, and R log 2 (as the f32 the kernel adds) to the row's bar
        if not case["loss_only"]:
            assert (got["dF"][off] == 0).all(), case["id"]
        Rr = case["R"]
        assert (np.abs(got["row_loss"][off].astype(np.float64) - Rr * R.LOG2_F32) <= want["e_row"][off]).all()
    if off.all() and not case["loss_only"]:
        assert (got["dT"] == 0).all(), case["id"]


def test_a_row_alone_is_the_row_in_a_larger_batch(device):
    """row_loss and dF of a row do not depend on N: the column chunks are a constant of the kernel."""
    n_all = 64                    # a power of two: 1 / (N R) of the row alone is 64 times that of the batch, exactly
    g = R.gen(R._case("row-alone", n_all, R.constants()["kCbColChunk"] + 1, 32, csr=True))
    whole = run(g, device)
    for n in (0, 31, 32, n_all - 1):
        alone = run(g, device, rows=slice(n, n + 1))
        assert np.array_equal(alone["row_loss"].view(np.uint32), whole["row_loss"][n:n + 1].view(np.uint32)), n
        v = np.abs(whole["dF"][n])
        assert (v[v > 0] > 2.0 ** -100).all()                         # no underflow: the scaling below is exact
        assert np.array_equal(alone["dF"][0].view(np.uint32), (whole["dF"][n] * F32(n_all)).view(np.uint32)), n


def test_the_engine_wrapper_is_the_c_call(device):
    from yelprecommendation_amd import engine
    case = next(c for c in CASES if c["id"] == "E64-csr")
    g = R.gen(case)
    raw = run(g, device)
    loss, row, dF, dT = engine.s3rec_catalogue_bce(_t(g["F"], device), _t(g["T"], device), _t(g["zs"], device),
                                                   _t(g["ys"], device), _t(g["key"], device), _t(g["ptr"], device),
                                                   _t(g["idx"], device))
    for a, b in ((loss, raw["loss"]), (row, raw["row_loss"]), (dF, raw["dF"]), (dT, raw["dT"])):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32))
    loss2, _, dF2, dT2 = engine.s3rec_catalogue_bce(_t(g["F"], device), _t(g["T"], device), _t(g["zs"], device),
                                                    _t(g["ys"], device), _t(g["key"], device), _t(g["ptr"], device),
                                                    _t(g["idx"], device), grads=False)
    assert dF2 is None and dT2 is None and float(loss2) == float(loss)
