"""GPU parity of the balanced owner passes (csrc/bpr_pull.hip): rows are dealt to the lane groups of an owner
workgroup by load (a binding fixed by the first chunk of a bucket that holds a record), oversize item buckets are
shared between workgroups.  Every case is compared with the NumPy oracle over four Adam steps at the bars of
test_gpu_pull_step.test_pull_step_matches_oracle; the tables are a few buckets large — the smallest shapes at which
the binding can go wrong: a deal that differs from index order, a deal that is the identity, a heavy row next to
dealt rows, a ragged last bucket, a row without a record, buckets of several chunks whose later chunks favour other
rows than the first.

A bucket is R = 1024 / D rows, wave w of its workgroup finishes RPW = R / 4 of them (rows [w RPW, (w + 1) RPW) under
index order).  The wide user form (R rows per bucket, the one that deals) is taken from 768 user buckets up, below
that a user bucket is 4 rows with one row per wave (nothing to deal): both are run.

A bucket's rows are dealt when its first chunk holds at least R * R records (the deal is R serial steps: a short walk
cannot win them back), and the deal is compiled only into the forms whose chunks can hold that many: both sides at
D = 128 and D = 64, the item side at D = 32 (a full chunk of 1,024: reached by the several-chunk case).  The D = 16
forms and the D = 32 user side keep the index-order binding at compile time; their cases here check that they still
do what they did."""
import functools

import numpy as np
import pytest
import torch

from oracle import bpr_mf as obpr

pytestmark = pytest.mark.gpu

WIDTHS = [16, 32, 64, 128]
STEPS = 4
LR = 5e-3
WIDE_USER_BUCKETS = 768          # kNarrowBelow of bpr_pull.hip: fewer 1024/D-row buckets take the one-row-per-wave form


def _spread(rs, counts, rows, total):
    """add what is missing to `total` to counts[rows], as evenly as it goes"""
    rest = total - int(counts.sum())
    assert rest >= 0
    add = np.full(len(rows), rest // len(rows))
    add[:rest % len(rows)] += 1
    counts[rows] += add
    return counts


def _ids(rs, counts):
    ids = np.repeat(np.arange(len(counts)), counts)
    rs.shuffle(ids)
    return ids.astype(np.int64)


def _pattern(rs, R, rows, heavy_rows, lo, hi, per_wave):
    """Records per row of a table of `rows` rows whose first three buckets are:
    bucket 0: the rows of wave 0 under index order carry lo..hi records each, the others 0..3 — the deal must move
              them to other waves; bucket 1: per_wave records on the first row of every wave, 0..3 elsewhere — the deal
              is the identity (up to the sprinkled rows); bucket 2: 0..3 records, its row 1 none at all.
    heavy_rows: (row, records) pairs added on top."""
    rpw = R // 4
    c = rs.randint(0, 4, size=rows)
    c[3 * R:] = 0
    c[:rpw] = rs.randint(lo, hi + 1, size=rpw)
    c[R:2 * R:rpw] = per_wave
    c[2 * R + 1] = 0
    for r, k in heavy_rows:
        c[r] = k
    return c


def _dealt_batches(d, nu, heavy):
    """Cases 1 and 2.  ni = 2.5 buckets.  Per item row, positives and negatives each bring half of the records
    (35..45 + 35..45 on the long rows: 70..90 records, the upper part of the 40..90 band, so that bucket 0 holds the
    256 records from which a bucket's rows are dealt at D = 64; 64 at D = 128); what the user pattern needs beyond the item pattern goes, spread evenly, to
    the rows of the ragged last bucket (row 1 of it stays empty) — the batch size follows from the counts (a few
    hundred to 1,500 triplets: with only 2.5 R item rows a batch of 2,000 would make every row heavy and leave
    nothing to deal).  heavy: one row of 300 records (the threshold is 96) in bucket 0 next to the long light rows
    (row RPW, wave 1's under index order), one in the ragged bucket; likewise on the user side."""
    rs = np.random.RandomState(1000 * d + nu + int(heavy))
    R = 1024 // d
    rpw = R // 4
    ni = 2 * R + R // 2
    hu = [(rpw, 300), (2 * R + 2, 300)] if heavy else []
    hi = [(rpw, 150), (2 * R + 2, 150)] if heavy else []
    batches = []
    for _ in range(2):
        cu = _pattern(rs, R, nu, hu, 70, 90, 40)
        cp = _pattern(rs, R, ni, hi, 35, 45, 20)
        cn = _pattern(rs, R, ni, hi, 35, 45, 20)
        B = max(int(cu.sum()), int(cp.sum()), int(cn.sum()))
        ragged = np.array([r for r in range(2 * R, ni) if r != 2 * R + 1])
        cp, cn = _spread(rs, cp, ragged, B), _spread(rs, cn, ragged, B)
        cu = _spread(rs, cu, np.arange(2 * R, min(nu, 8 * R)), B)
        assert cp[2 * R + 1] == 0 and cn[2 * R + 1] == 0
        batches.append((_ids(rs, cu), _ids(rs, cp), _ids(rs, cn)))
    return ni, batches


def _chunked_batches(d, nu):
    """Case 3.  Two item buckets in all (ni = 2 R; 32 at D = 64) and B = 6,000: every bucket takes about six chunks of
    1,024 records.  An owner reads its bucket's records tile by tile (tiles of 1,024 triplets here), so the first
    1,024 triplets are the first chunk: their positives favour the rows of wave 0 (weight 2.2 against 1: about 85
    records per favoured row at D = 64, below the heavy threshold), the later ones the rows of wave 3.  Users the
    same, on the first two buckets of the user table."""
    rs = np.random.RandomState(77 * d + nu)
    R = 1024 // d
    rpw = R // 4
    ni, B, first = 2 * R, 6000, 1024

    def draw(count, fav_lo):
        w = np.ones(R)
        w[fav_lo:fav_lo + rpw] = 2.2
        return rs.randint(0, 2, size=count) * R + rs.choice(R, size=count, p=w / w.sum())

    batches = []
    for _ in range(2):
        p = np.concatenate([draw(first, 0), draw(B - first, R - rpw)])
        u = np.concatenate([draw(first, 0), draw(B - first, R - rpw)])
        n = rs.randint(0, ni, size=B)
        batches.append((u.astype(np.int64), p.astype(np.int64), n.astype(np.int64)))
    return ni, batches


def _user_rows(d, form):
    R = 1024 // d
    return {"narrow3": 3 * R, "narrow2": 2 * R, "wide": WIDE_USER_BUCKETS * R}[form]


@functools.lru_cache(maxsize=None)
def _case(kind, d, form):
    """(U0, I0, batches, oracle state after STEPS steps, oracle loss sum): computed once, shared, never written to"""
    nu = _user_rows(d, form)
    if kind == "chunks":
        ni, batches = _chunked_batches(d, nu)
    else:
        ni, batches = _dealt_batches(d, nu, kind == "heavy")
    rs = np.random.RandomState(d + len(kind))
    U = (rs.standard_normal((nu, d)) * 0.2).astype(np.float32)
    I = (rs.standard_normal((ni, d)) * 0.2).astype(np.float32)
    ref = obpr.MFState(U, I, "adam", lr=LR)
    total = 0.0
    for k in range(STEPS):
        total += float(ref.train_step(*batches[k % len(batches)]))
    want = tuple(np.array(x, copy=True) for x in (ref.U, ref.I, ref.opt.m[0], ref.opt.v[0], ref.opt.m[1], ref.opt.v[1]))
    for x in (U, I) + want + tuple(a for b in batches for a in b):
        x.setflags(write=False)
    return U, I, batches, want, total


def _run(device, U, I, batches, **kw):
    from yelprecommendation_amd.bpr_step import BPRMFStep
    st = BPRMFStep(torch.from_numpy(U.copy()).to(device), torch.from_numpy(I.copy()).to(device), lr=LR, impl="pull", **kw)
    dev_batches = [tuple(torch.from_numpy(a.copy()).to(device) for a in b) for b in batches]
    for k in range(STEPS):
        st.step(*dev_batches[k % len(dev_batches)])
    loss = st.epoch_loss()
    st.check()
    return tuple(x.clone() for x in (st.U, st.I, st.mU, st.vU, st.mI, st.vI)), loss


def _assert_matches_oracle(got, loss, want, total):
    np.testing.assert_allclose(loss, total, rtol=2e-5)
    for g, w, atol in zip(got, want, (1e-5, 1e-5, 1e-8, 1e-11, 1e-8, 1e-11)):
        np.testing.assert_allclose(g.cpu().numpy(), w, rtol=1e-3, atol=atol)


CASES = ([("dealt", d, f) for d in WIDTHS for f in ("narrow3", "wide")] +
         [("heavy", d, f) for d in WIDTHS for f in ("narrow3", "wide")] +
         [("chunks", d, f) for d in WIDTHS for f in ("narrow2", "wide")])


@pytest.mark.parametrize("kind,d,form", CASES)
def test_dealt_rows_match_oracle(device, kind, d, form):
    """Cases 1-3 of the module docstring in the default mode."""
    U, I, batches, want, total = _case(kind, d, form)
    got, loss = _run(device, U, I, batches)
    _assert_matches_oracle(got, loss, want, total)


@pytest.mark.parametrize("kind,d,form", CASES)
def test_dealt_rows_deterministic_mode(device, kind, d, form):
    """The deal is a pure function of a chunk's counts and every row is still summed in triplet order: two
    deterministic runs are bit-identical in all six state tensors and the loss, and match the oracle (and so the
    default mode) at the same bars."""
    U, I, batches, want, total = _case(kind, d, form)
    a, la = _run(device, U, I, batches, deterministic=True)
    b, lb = _run(device, U, I, batches, deterministic=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert la == lb
    _assert_matches_oracle(a, la, want, total)
    c, lc = _run(device, U, I, batches)
    for x, y, atol in zip(a, c, (1e-5, 1e-5, 1e-8, 1e-11, 1e-8, 1e-11)):
        torch.testing.assert_close(x, y, rtol=1e-3, atol=atol)
    np.testing.assert_allclose(la, lc, rtol=2e-5)


def _skewed_batch(device, B, seed):
    """Yelp2018 shape, 8 % of the positives on ONE bucket of 16 items (as test_gpu_pull_step's shared-bucket test)"""
    g = torch.Generator(device=device).manual_seed(seed)
    nu, ni = 31668, 38048
    u = torch.randint(0, nu, (B,), generator=g, device=device)
    p = torch.randint(0, ni, (B,), generator=g, device=device)
    r = torch.rand(B, generator=g, device=device)
    p = torch.where(r < 0.08, torch.randint(4000, 4016, (B,), generator=g, device=device), p).contiguous()
    n = torch.randint(0, ni, (B,), generator=g, device=device)
    return nu, ni, u, p, n


SHARED_B = 28672


def test_shared_bucket_of_dealt_parts_matches_atomic_form(device):
    """Shared item buckets at the thresholds in force (swept on dealt rows and kept: YR_SPLIT_MIN = 2048,
    YR_SPLIT_AVG_MIN = 2.5, YR_SPLIT_TARGET = 1024, YR_SPLIT_AVG_TARGET = 1.25).  A bucket is shared from
    max(2048, 2.5 x 2B / 2378) records up; at Yelp2018 shape (2,378 item buckets) the second term passes 2,048 only
    beyond 970,000 triplets, so below that a bucket needs 2,048 records.  With 8 % of the positives on ONE bucket it
    receives 0.08 B + 2 B / 2378 records on average: 2,048 at B = 25,334.  The smallest batch that shares it for sure
    is a little above that — B = 28,672 gives 2,318 expected records with a standard deviation of 46 (asserted below on
    the batches themselves) — and the bucket is cut into ceil(2318 / 1024) = 3 parts of about 770 records.  Every part
    holds more than the 256 records from which rows are dealt and deals by its OWN counts, so the parts' bindings
    differ and their sums meet in the scratch slot by true row.  As for
    test_gpu_pull_step.test_oversize_item_buckets_are_shared_between_workgroups: the result equals the atomic form's
    at that test's bars, two deterministic runs are bit-identical, the loss is the same in all forms."""
    from yelprecommendation_amd.bpr_step import BPRMFStep
    d = 64
    batches = []
    for seed in (11, 12):
        nu, ni, u, p, n = _skewed_batch(device, SHARED_B, seed)
        in_bucket = int(((p >> 4) == 250).sum() + ((n >> 4) == 250).sum())
        assert in_bucket >= 2048 and in_bucket >= 2.5 * 2 * SHARED_B / ((ni + 15) // 16)
        batches.append((u, p, n))
    g = torch.Generator(device=device).manual_seed(13)
    U = (torch.rand(nu, d, generator=g, device=device) - 0.5) * 0.2
    I = (torch.rand(ni, d, generator=g, device=device) - 0.5) * 0.2
    out = {}
    for name, kw in (("pull", dict(impl="pull")), ("det", dict(impl="pull", deterministic=True)),
                     ("det2", dict(impl="pull", deterministic=True)), ("atomic", dict(impl="atomic"))):
        st = BPRMFStep(U.clone(), I.clone(), lr=1e-3, **kw)
        for k in range(4):
            st.step(*batches[k % 2])
        st.check()
        out[name] = [x.clone() for x in (st.U, st.I, st.mI, st.vI)] + [st.epoch_loss()]
    for a, b in zip(out["det"], out["det2"]):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    for other in ("pull", "det"):
        for a, b, tol in zip(out[other][:4], out["atomic"][:4], (2e-5, 2e-5, 2e-6, 1e-8)):
            torch.testing.assert_close(a, b, rtol=2e-3, atol=tol)
        assert abs(out[other][4] - out["atomic"][4]) <= 1e-5 * abs(out["atomic"][4])


def test_item_phase_twice_over_one_partition(device):
    """Through the C ABI: index once, user phase once, then the item phase alone TWICE in the dense-gradient form
    (gradI_out given: the call writes the gradient rows and nothing else, so it can be repeated; deterministic order,
    so that the two results can be compared bit for bit).  The partition has
    a shared bucket: rows 4000..4015 receive 8 % of 65,536 positives, 5,200 records against a threshold of at most
    2,048.  The last part to arrive must leave the bucket's arrival counter at zero — otherwise the second call never
    sees a last arriver and the bucket's rows are not written."""
    from yelprecommendation_amd import _lib, engine
    lib = _lib.load()
    B, d = 1 << 16, 64
    nu, ni, u, p, n = _skewed_batch(device, B, 5)
    g = torch.Generator(device=device).manual_seed(6)
    U = (torch.rand(nu, d, generator=g, device=device) - 0.5) * 0.2
    I = (torch.rand(ni, d, generator=g, device=device) - 0.5) * 0.2
    U_new, mU, vU = torch.empty_like(U), torch.zeros_like(U), torch.zeros_like(U)
    partials = torch.zeros(engine.LOSS_PARTIALS, dtype=torch.float32, device=device)
    flag = engine.new_error_flag(device)
    ws = engine.bpr_mf_pull_workspace(B, nu, ni, d, device)
    rc = lib.yr_bpr_mf_pull_index(u.data_ptr(), p.data_ptr(), n.data_ptr(), B, d, nu, ni, ws.data_ptr(), ws.numel(),
                                  flag.data_ptr(), engine._stream())
    assert rc == 0
    step_size, bc2_sqrt = engine.adam_scalars(1, 1e-3, 0.9, 0.999)

    def apply(phases, grad):
        rc = lib.yr_bpr_mf_pull_apply(U.data_ptr(), U_new.data_ptr(), I.data_ptr(), mU.data_ptr(), vU.data_ptr(), None,
                                      None, grad.data_ptr(), B, d, nu, ni, 1.0 / B, 1e-3, step_size, bc2_sqrt, 0.9,
                                      0.999, 1e-8, 0.0, engine.OPT_ADAM, 1, ws.data_ptr(), ws.numel(),
                                      partials.data_ptr(), None, None, phases, 0, ni, engine._stream())
        assert rc == 0

    g1, g2 = torch.full_like(I, float("nan")), torch.full_like(I, float("nan"))
    apply(engine.PULL_USER_PHASE, g1)              # no item launch: g1 is not touched
    apply(engine.PULL_ITEM_PHASE, g1)
    apply(engine.PULL_ITEM_PHASE, g2)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all()      # every row written, by both calls
    assert (g1[4000:4016].abs().sum(1) > 0).all() and (g2[4000:4016].abs().sum(1) > 0).all()
    assert torch.equal(g1, g2)                     # deterministic order: the same call twice, the same bits
