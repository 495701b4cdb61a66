"""Restatements of S3Rec pre-training for the tests.  Importable helper, no tests and no fixtures in it; runs without
a GPU.

1. ``step`` — reference models/s3rec.py:120-181 + trainers/s3rec_trainer.py:118-167 in torch on the CPU with a
   ``dtype`` argument, every loss in DENSE form ([B, L, R] logits against a dense target array), the encoder delegated
   to ``s3rec_grad_ref64.encode`` with ``encode(X)`` = what ``finetune`` runs before its prediction layer.  float64 is
   the judge, float32 the measure of what f32 arithmetic costs on a case: per tensor
       bar = 8 * max |f32 - f64|          of this restatement alone, never of a kernel,
   exactly zero where both are exactly zero (the project's rule: s3rec_ref64 / s3rec_grad_ref64).

2. ``catalogue_bce`` — the contract of yr_s3rec_catalogue_bce (include/yelprec_engine.h) in NumPy float64, every
   output with its own closed-form bar: the kernel takes F and T as inputs, so nothing upstream enters.
       z[n, r] = zs[n] <F[n], T[r]>        y[n, r] = ys[n] [r in targets(key[n])]
       term = max(z, 0) - z y + log1p(exp(-|z|))     row_loss[n] = sum_r term     loss = sum / (N R)
       g = zs (sigmoid(z) - y) / (N R)               dF = g T                      dT = g^T F

   Bars (u = 2^-24, the unit roundoff of f32; no rtol floor — a floor of 1e-4 |v| is what hides one column lost from
   a row of 38,049).  Three parts, in the style of gemm_ref64.py / bpr_pull_ref64.py:
    a. Sums and dot products.  n terms added in ANY order (matrix-instruction steps, register totals, waves, chunks;
       an added exact zero does not round), one rounding per product: 2 (n + 1) u sum |terms| — the margin factor 2 of
       the sibling references included.  For the logit: e_d = 2 (E + 1) u sum_k |F_k T_k|, and z = zs d rounds once
       more: e_z = |zs| e_d + u |z|.
    b. The logit error carried through.  softplus(z) = max(z, 0) + log1p(exp(-|z|)) is 1-Lipschitz and -z y is
       |y|-Lipschitz: (1 + |y|) e_z on a term.  sigmoid is 1/4-Lipschitz: e_z / 4 on sigmoid.
    c. The device exp / log / rcp (csrc/common.h fast_exp, fast_log, fast_rcp, "about 1 ulp each"), with the
       allowances bpr_pull_ref64.py derives for the same three instructions: with w = exp(-|z|),
         log term: (w (2 |z| + 2) + 1) u + 4 u log1p(w);   sigmoid: (2 |z| + 7) u sigmoid  (relative).
       The term's own roundings (the product z y, one subtraction, one addition): u (|z y| + 2 (max(z, 0) + |z y| +
       log1p(w))).  g = zs ((sigmoid - y) inv): the subtraction, two products and the rounded inv: 4 u |g|.
         e_term = (1 + |y|) e_z + (c, log) + (own roundings)
         e_g    = |zs| inv (e_z / 4 + (2 |z| + 7) u sigmoid) + 4 u |g|
       bar(row_loss[n]) = sum_r e_term + 2 (R + 1) u sum_r |term|
       bar(loss)        = sum_n bar(row_loss[n]) / (N R)          (the final sum runs in double on the device)
       bar(dF[n, e])    = sum_r e_g |T[r, e]| + 2 (R + 1) u sum_r |g T[r, e]|
       bar(dT[r, e])    = sum_n e_g |F[n, e]| + 2 (N + 1) u sum_n |g F[n, e]|
   Rows with zs = 0: g is exactly 0, so dF's row and the row's share of dT are exactly 0 and the bar is 0 there (the
   kernel's value must be exactly 0 too); z = 0 gives term = log1p(1), so row_loss = R log 2 to its bar.

   Exactness (``quantum`` / ``exact`` of ngcf_ref64, from the arrays).  On the "exact" inputs column 0 of every row of
   F is 16 and of T is -16, every other entry is in {-1, 0, 1}, zs is 1 and N R is a power of two.  Then
   z <= -256 + (E - 1) <= -129: exp2 underflows to 0, rcp(1) = 1, log2(1) = 0, so sigmoid = 0 and g = -y / (N R), a
   power of two or zero; term = -z y, an integer.  Every gradient term is a multiple of 1 / (N R) and every loss term
   an integer: any order of f32 additions gives the float64 value, and the GPU tests demand equality.

VARIANTS are wrong readings; tests/test_s3rec_pretrain_ref64.py checks that each crosses a bar on every case it
applies to.  The tile sizes and trip lengths of csrc/s3rec_pretrain.hip are read from the source BY NAME
(``constants``), and ``plan_rows`` / ``plan_cols`` say which loop ends a shape reaches.
"""
import functools
import math
import os
import re

import numpy as np
import torch

import s3rec_grad_ref64 as gr
from ngcf_ref64 import Out, U24, exact, over, quantum  # noqa: F401  (re-exported: one copy of the certificate)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yelprecommendation_amd", "csrc")
F32 = np.float32
BAR_FACTOR = 8.0
SENTINEL = 7.25
GUARD = 256
FLAG_BAD_ITEM = 2
LOG2_F32 = float(F32(math.log(2.0)))

VARIANTS = {
    # readings of the step (the dense restatement)
    "map_through_map_weight": "MAP projects with map_weight (the documented intent), not aap_weight",
    "mip_mask_not_inverted": "MIP multiplies logits and targets by masks, not by their negation",
    "aap_logits_masked": "AAP multiplies its logits by masks as well as its targets",
    "mip_without_column_0": "MIP leaves column 0 (the pad's one-hot target) out of the targets",
    "mean_over_unmasked_rows": "each catalogue loss is a mean over the rows whose factor is set only",
    "sp_targets_swapped": "SP labels the positive pair 0 and the negative pair 1",
    "sp_at_L_minus_2": "SP reads the encodings at position L - 2",
    # readings of the kernel contract
    "last_table_row_dropped": "the sweep stops one table row short",
    "row_last_target_dropped": "a key's last target is not a target",
    "zscale_on_targets": "zscale multiplies the targets, the logits stay unscaled",
}
STEP_VARIANTS = tuple(v for v in VARIANTS if v not in ("last_table_row_dropped", "row_last_target_dropped",
                                                       "zscale_on_targets"))
KERNEL_VARIANTS = ("last_table_row_dropped", "row_last_target_dropped", "zscale_on_targets")


# ---- the kernels' constants, by name ----------------------------------------------------------------------------------

@functools.lru_cache(None)
def constants():
    """{name: value} of the named tile sizes and trip lengths of csrc/s3rec_pretrain.hip (and kWavesPerBlock)."""
    text = open(os.path.join(CSRC, "s3rec_pretrain.hip")).read()
    common = open(os.path.join(CSRC, "common.h")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", common).group(1))
    wave = int(re.search(r"constexpr int kWave = (\d+);", common).group(1))
    out = {"kWavesPerBlock": block // wave}
    for name in ("kCbTile", "kCbTilesPerWave", "kCbGridMax", "kCbLossBlock"):
        out[name] = int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))
    assert re.search(r"constexpr int kCbColChunk = kWavesPerBlock \* kCbTilesPerWave \* kCbTile;", text)
    out["kCbColChunk"] = out["kWavesPerBlock"] * out["kCbTilesPerWave"] * out["kCbTile"]
    return out


def _cdiv(a, b):
    return -(-a // b)


def plan_rows(N, R):
    """The ROWS pass (loss, dF) on an [N, R] problem: tiles, chunks, launch units and what its loops reach."""
    c = constants()
    tile, chunk = c["kCbTile"], c["kCbColChunk"]
    row_tiles, col_tiles, chunks = _cdiv(N, tile), _cdiv(R, tile), _cdiv(R, chunk)
    units = row_tiles * chunks
    last_cols = R - (chunks - 1) * chunk                      # columns of the last chunk
    return dict(row_tiles=row_tiles, col_tiles=col_tiles, chunks=chunks, units=units,
                trips=_cdiv(units, c["kCbGridMax"]), partial_row_tile=N % tile != 0, partial_col_tile=R % tile != 0,
                waves_last_chunk=min(c["kWavesPerBlock"], _cdiv(_cdiv(last_cols, tile), c["kCbTilesPerWave"])))


def plan_cols(N, R):
    """The COLS pass (dT): a workgroup per column tile, wave w takes the row tiles w, w + waves, ..."""
    c = constants()
    tile = c["kCbTile"]
    row_tiles, col_tiles = _cdiv(N, tile), _cdiv(R, tile)
    return dict(units=col_tiles, trips=_cdiv(col_tiles, c["kCbGridMax"]), row_tiles=row_tiles,
                wave_trips=_cdiv(row_tiles, c["kWavesPerBlock"]), waves_used=min(row_tiles, c["kWavesPerBlock"]))


def workspace_floats(N, R, E):
    return N * (1 + _cdiv(R, constants()["kCbColChunk"]) * (1 + E))


# ---- the contract of yr_s3rec_catalogue_bce ------------------------------------------------------------------------

def dense_targets(key, ptr, idx, K, R, variant=None):
    """bool [N, R]: r in targets(key[n]); a key outside [0, K) has none.  ``ptr`` None: the key is the column."""
    key = np.asarray(key, np.int64)
    Y = np.zeros((key.shape[0], R), bool)
    for n, k in enumerate(key):
        if not 0 <= k < K:
            continue
        cols = np.array([k]) if ptr is None else np.asarray(idx[ptr[k]:ptr[k + 1]], np.int64)
        if variant == "row_last_target_dropped":
            cols = cols[:-1]
        cols = cols[(cols >= 0) & (cols < R)]
        Y[n, cols] = True
    return Y


def catalogue_bce(F, T, zs, ys, key, ptr=None, idx=None, K=None, variant=None):
    """dict(loss, row_loss, dF, dT: Out; e_loss, e_row, e_dF, e_dT: bars; flag)."""
    F64, T64 = np.asarray(F, np.float64), np.asarray(T, np.float64)
    zs, ys = np.asarray(zs, np.float64), np.asarray(ys, np.float64)
    (N, E), R = F64.shape, T64.shape[0]
    K = R if K is None else K
    key = np.asarray(key, np.int64)
    flag = FLAG_BAD_ITEM if ((key < 0) | (key >= K)).any() else 0
    hit = dense_targets(key, ptr, idx, K, R, variant)
    live = np.ones(R)
    if variant == "last_table_row_dropped":
        live[-1] = 0.0
    inv = 1.0 / (N * R)
    d = F64 @ T64.T
    if variant == "zscale_on_targets":
        z, y = d, hit * (zs * ys)[:, None]
        zfac = np.ones(N)
    else:
        z, y = zs[:, None] * d, hit * ys[:, None]
        zfac = zs
    w = np.exp(-np.abs(z))
    lg = np.log1p(w)
    term = (np.maximum(z, 0.0) - z * y + lg) * live
    sig = 1.0 / (1.0 + np.exp(-z))
    g = zfac[:, None] * (sig - y) * inv * live
    e_d = 2.0 * (E + 1) * U24 * (np.abs(F64) @ np.abs(T64).T)
    e_z = np.abs(zfac)[:, None] * e_d + U24 * np.abs(z)
    e_term = (1.0 + np.abs(y)) * e_z + (w * (2.0 * np.abs(z) + 2.0) + 1.0) * U24 + 4.0 * U24 * lg \
        + U24 * (np.abs(z * y) + 2.0 * (np.maximum(z, 0.0) + np.abs(z * y) + lg))
    e_g = np.abs(zfac)[:, None] * inv * (e_z / 4.0 + (2.0 * np.abs(z) + 7.0) * U24 * sig) + 4.0 * U24 * np.abs(g)
    row = Out(term.sum(1), R, np.abs(term).sum(1))
    e_row = e_term.sum(1) + 2.0 * (R + 1) * U24 * row.s
    loss = Out(term.sum() * inv, N * R, np.abs(term).sum() * inv)
    aT, aF = np.abs(T64), np.abs(F64)
    dF = Out(g @ T64, R, np.abs(g) @ aT)
    dT = Out(g.T @ F64, N, np.abs(g).T @ aF)
    e_dF = e_g @ aT + 2.0 * (R + 1) * U24 * dF.s
    e_dT = e_g.T @ aF + 2.0 * (N + 1) * U24 * dT.s
    return dict(loss=loss, row_loss=row, dF=dF, dT=dT, e_loss=np.asarray(e_row.sum() * inv), e_row=e_row, e_dF=e_dF,
                e_dT=e_dT, flag=flag, z=z, g=g, term=term)


def ratio(got, o, bar):
    """max |got - v| / bar; 0 where the error is 0 (a zero bar demands equality); NaN / inf in ``got`` give inf."""
    got = np.asarray(got, np.float64).reshape(o.v.shape)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    return float(over(got - o.v, np.broadcast_to(bar, o.v.shape)).max())


# ---- the kernel's cases ------------------------------------------------------------------------------------------------

def _case(id, N, R, E, csr, pattern="mixed", keys="cycle", exact=False, loss_only=False):
    return dict(id=id, N=N, R=R, E=E, csr=csr, pattern=pattern, keys=keys, exact=exact, loss_only=loss_only)


def kernel_cases():
    c = constants()
    t, wave_cols, chunk, grid = c["kCbTile"], c["kCbTilesPerWave"] * c["kCbTile"], c["kCbColChunk"], c["kCbGridMax"]
    ends = (1, t - 1, t, t + 1, 2 * t + 1)
    out = []
    for k, n in enumerate(ends):                                      # N at the ends of the row tile
        out.append(_case(f"N{n}-R{t + 1}", n, t + 1, 32, csr=bool(k & 1)))
    for k, r in enumerate(ends):                                      # R at the ends of the column tile
        if r != t + 1:                                                # (t + 1, t + 1) is in the list already
            out.append(_case(f"N{t + 1}-R{r}", t + 1, r, 32, csr=not (k & 1)))
    out.append(_case("N1-R1-csr", 1, 1, 16, csr=True))
    for E in (16, 32, 64, 128):                                       # every width, both forms
        out.append(_case(f"E{E}-mip", 40, 70, E, csr=False))
        out.append(_case(f"E{E}-csr", 40, 70, E, csr=True))
    out.append(_case("R33-csr-aap", 65, 33, 64, csr=True, pattern="aap"))
    out.append(_case("R810-csr-aap", 65, 810, 64, csr=True, pattern="aap"))
    out.append(_case("R810-csr-map", 65, 810, 64, csr=True, pattern="mip"))
    out.append(_case("R38049-mip", 33, 38049, 64, csr=False, pattern="mip"))
    out.append(_case("all-zscale-0", 40, 70, 32, csr=True, pattern="zero"))
    out.append(_case("alternating", 40, 70, 32, csr=False, pattern="alternate"))
    out.append(_case("bad-first-last-csr", 40, 70, 32, csr=True, keys="bad"))
    out.append(_case("bad-first-last-mip", 40, 70, 32, csr=False, keys="bad"))
    out.append(_case("loss-only", 40, 70, 32, csr=True, loss_only=True))
    # a wave's column range, a chunk, and one trip of each grid loop, each at its end and one past it
    out.append(_case(f"R{wave_cols}", t + 1, wave_cols, 16, csr=True))
    out.append(_case(f"R{wave_cols + 1}", t + 1, wave_cols + 1, 16, csr=False))
    out.append(_case(f"R{chunk}", t + 1, chunk, 16, csr=False))
    out.append(_case(f"R{chunk + 1}", t + 1, chunk + 1, 16, csr=True))
    out.append(_case("cols-wave-second-trip", c["kWavesPerBlock"] * t + 1, t + 1, 32, csr=True))
    out.append(_case("rows-grid-second-trip", grid * t + 3, 3, 16, csr=True))
    out.append(_case("cols-grid-second-trip", 3, grid * t + 3, 16, csr=False))
    # the exact twins: N R a power of two
    out.append(_case("exact-32x32-mip", 32, 32, 32, csr=False, exact=True))
    out.append(_case("exact-32x32-csr", 32, 32, 16, csr=True, exact=True))
    out.append(_case("exact-64x4096-csr", 64, 4096, 64, csr=True, exact=True))
    out.append(_case("exact-128x64-mip", 128, 64, 128, csr=False, exact=True))
    out.append(_case("exact-256x16-csr", 256, 16, 64, csr=True, exact=True))
    return out


def gen(case):
    """The arrays of a case (f32 / int64), a pure function of the case."""
    N, R, E = case["N"], case["R"], case["E"]
    rs = np.random.RandomState(zlib_seed(case["id"]))
    if case["exact"]:
        F = rs.randint(-1, 2, (N, E)).astype(F32)
        T = rs.randint(-1, 2, (R, E)).astype(F32)
        F[:, 0], T[:, 0] = 16.0, -16.0
    else:
        F = (rs.standard_normal((N, E)) * 0.6).astype(F32)
        T = (rs.standard_normal((R, E)) * 0.6).astype(F32)
    mask = rs.rand(N) < 0.4
    pattern = "ones" if case["exact"] else case["pattern"]
    if pattern == "aap":                      # logits unscaled, targets where the mask is set
        zs, ys = np.ones(N), mask.astype(np.float64)
    elif pattern == "mip":                    # both multiplied by the negated mask
        zs = ys = (~mask).astype(np.float64)
    elif pattern == "zero":
        zs, ys = np.zeros(N), np.ones(N)
    elif pattern == "alternate":
        zs = ys = (np.arange(N) % 2).astype(np.float64)
    elif pattern == "ones":
        zs, ys = np.ones(N), np.ones(N)
    else:                                     # all four combinations
        zs, ys = (np.arange(N) % 2 == 0).astype(np.float64), (np.arange(N) // 2 % 2 == 0).astype(np.float64)
    ptr = idx = None
    if case["csr"]:
        # key 0: no target; 1: column 0; 2: column R - 1; 3: every column (the longest list there is: lists are
        # ascending and duplicate-free); 4: every column but one (the next shorter); 5: the last column tile;
        # 6 ..: a few random columns
        t = constants()["kCbTile"]
        lists = [[], [0], [R - 1], list(range(R)), [c for c in range(R) if c != R // 2],
                 list(range((R - 1) // t * t, R))]
        for _ in range(6):
            lists.append(sorted(rs.choice(R, size=min(R, 1 + rs.randint(5)), replace=False).tolist()))
        K = len(lists)
        ptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
        idx = np.array([c for l in lists for c in l], np.int64)
        key = np.arange(N, dtype=np.int64) % K
        if N > K:
            key[K:] = rs.randint(0, K, N - K)
    else:
        K = R
        key = rs.randint(0, R, N).astype(np.int64)
        key[0] = R - 1                                          # a target in the last column ...
        if N > 1:
            key[1] = 0                                          # ... and one in column 0
        if N > 2:
            key[2] = (R - 1) // constants()["kCbTile"] * constants()["kCbTile"]   # the last (partial) column tile
    if case["keys"] == "bad":
        key[0], key[-1] = -1, K
    return dict(F=F, T=T, zs=zs.astype(F32), ys=ys.astype(F32), key=key, ptr=ptr, idx=idx, K=K)


def zlib_seed(text):
    import zlib
    return zlib.crc32(text.encode()) & 0x7FFFFFFF


def certificate(g, r):
    """The quantum of the exact twin's gradient terms and whether its sums are exact: (ok_grads, ok_loss)."""
    N, R = g["F"].shape[0], g["T"].shape[0]
    inv = 1.0 / (N * R)
    assert math.log2(N * R) == round(math.log2(N * R))
    assert (r["z"] <= -129).all()
    ok_g = exact(inv, r["dF"].s) and exact(inv, r["dT"].s)
    ok_l = exact(1.0, r["row_loss"].s) and float(np.abs(r["term"]).sum()) <= 2.0 ** 24
    return ok_g, ok_l


# ---- the step in dense form ------------------------------------------------------------------------------------------

def csr_of(item2attributes, num_items):
    """(ptr [num_items + 2], idx): the categories of item id k (the reference's dict: key 0 is the pad and has none),
    ascending and duplicate-free."""
    lists = [[]] + [sorted(set(int(a) for a in item2attributes[k]["categories"])) for k in range(1, num_items + 1)]
    ptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    return ptr, np.array([a for l in lists for a in l], np.int64)


def _bce(logits, targets, rows_on=None):
    terms = torch.nn.functional.binary_cross_entropy_with_logits(logits, targets, reduction="none")
    if rows_on is not None:                                           # the variant: a mean over the set rows only
        on = rows_on.to(terms.dtype)
        return (terms * on[..., None]).sum() / (on.sum().clamp(min=1) * terms.shape[-1])
    return terms.mean()


def step(t, X, masks, pos_seg, neg_seg, ptr, idx, heads, blocks, variant=None):
    """One pre-training step on the leaves ``t`` in dense form: dict(aap, mip, map, sp_pos, sp_neg: the model's four
    outputs; aap_loss, mip_loss, map_loss, sp_loss, loss).  ``masks`` bool [B, L]; the segment-masked sequence is
    not an input: the reference encodes it and never uses the result."""
    X = torch.as_tensor(np.asarray(X), dtype=torch.int64)
    m = torch.as_tensor(np.asarray(masks), dtype=torch.bool)
    dt = t["item_embedding.weight"].dtype
    B, L = X.shape
    A, R = t["attribute_embedding.weight"].shape[0], t["item_embedding.weight"].shape[0]
    h = gr.encode(t, (m * X).numpy(), heads, blocks)
    h_pos = gr.encode(t, np.asarray(pos_seg), heads, blocks)
    h_neg = gr.encode(t, np.asarray(neg_seg), heads, blocks)
    mf, nf = m.to(dt)[..., None], (~m).to(dt)[..., None]
    aap_actual = torch.as_tensor(dense_targets(X.reshape(-1).numpy(), ptr, idx, len(ptr) - 1, A)).to(dt).view(B, L, A)
    mip_actual = torch.nn.functional.one_hot(X, R).to(dt)
    if variant == "mip_without_column_0":
        mip_actual = mip_actual.clone()
        mip_actual[..., 0] = 0
    FW = h @ t["aap_weight.weight"].T
    aap = FW @ t["attribute_embedding.weight"].T
    mip = (h @ t["mip_weight.weight"].T) @ t["item_embedding.weight"].T
    mapo = (h @ t["map_weight.weight"].T) @ t["attribute_embedding.weight"].T if variant == "map_through_map_weight" \
        else FW @ t["attribute_embedding.weight"].T
    pos_at = L - 2 if variant == "sp_at_L_minus_2" else L - 1
    SW = h[:, pos_at] @ t["sp_weight.weight"].T
    sp_pos, sp_neg = (SW * h_pos[:, pos_at]).sum(-1), (SW * h_neg[:, pos_at]).sum(-1)
    rows = variant == "mean_over_unmasked_rows"
    aap_in = aap * mf if variant == "aap_logits_masked" else aap
    aap_loss = _bce(aap_in, aap_actual * mf, m if rows else None)
    mipf = mf if variant == "mip_mask_not_inverted" else nf
    mip_loss = _bce(mip * mipf, mip_actual * mipf, (mipf[..., 0] > 0) if rows else None)
    map_loss = _bce(mapo * nf, aap_actual * nf, ~m if rows else None)
    sp_out = torch.cat([sp_neg, sp_pos])
    first, second = (torch.ones(B, dtype=dt), torch.zeros(B, dtype=dt)) if variant == "sp_targets_swapped" \
        else (torch.zeros(B, dtype=dt), torch.ones(B, dtype=dt))
    sp_loss = _bce(sp_out, torch.cat([first, second]))
    return dict(aap=aap, mip=mip, map=mapo, sp_pos=sp_pos, sp_neg=sp_neg, aap_loss=aap_loss, mip_loss=mip_loss,
                map_loss=map_loss, sp_loss=sp_loss, loss=aap_loss + mip_loss + map_loss + sp_loss,
                F_aap=FW.reshape(B * L, -1), F_mip=(h @ t["mip_weight.weight"].T).reshape(B * L, -1))


OUTPUTS = ("aap", "mip", "map", "sp_pos", "sp_neg")
LOSSES = ("aap_loss", "mip_loss", "map_loss", "sp_loss", "loss")


def step_and_grads(state, batch, ptr, idx, heads, blocks, dtype=torch.float64, variant=None):
    """dict(the outputs and losses as arrays / floats, grads {name: array or None}) of one step + backward."""
    t = gr.tensors(state, dtype)
    out = step(t, batch["X"], batch["masks"], batch["pos"], batch["neg"], ptr, idx, heads, blocks, variant)
    out["loss"].backward()
    res = {k: out[k].detach().numpy().copy() for k in OUTPUTS + ("F_aap", "F_mip")}
    res.update({k: float(out[k].detach()) for k in LOSSES})
    res["grads"] = {k: (None if v.grad is None else v.grad.numpy().copy()) for k, v in t.items()}
    return res


def train(state, batches, ptr, idx, heads, blocks, epochs, lr, dtype):
    """trainers/s3rec_trainer.py:118-167 at dropout 0 with torch.optim.Adam over every parameter (a parameter
    without a gradient is skipped): ([[batch losses] per epoch], final state as arrays)."""
    t = gr.tensors(state, dtype)
    opt = torch.optim.Adam(list(t.values()), lr=lr)
    losses = []
    for _ in range(epochs):
        per_batch = []
        for b in batches:
            out = step(t, b["X"], b["masks"], b["pos"], b["neg"], ptr, idx, heads, blocks)
            opt.zero_grad()
            out["loss"].backward()
            opt.step()
            per_batch.append(float(out["loss"].detach()))
        losses.append(per_batch)
    return losses, {k: v.detach().numpy().copy() for k, v in t.items()}


def loss_bars(state, batches, ptr, idx, heads, blocks):
    """{loss name: bar} for a scalar loss of ANY of ``batches``.  A maximum needs samples — a single |f32 - f64| can be
    anything down to zero — so the samples are the same loss on every recorded batch (the rule of
    tests/test_gpu_s3rec_train.py for its batch losses): BAR_FACTOR * max_b |f32_b - f64_b|."""
    runs = [(step_and_grads(state, b, ptr, idx, heads, blocks, dtype=torch.float64),
             step_and_grads(state, b, ptr, idx, heads, blocks, dtype=torch.float32)) for b in batches]
    return {k: BAR_FACTOR * max(abs(r32[k] - r64[k]) for r64, r32 in runs) for k in LOSSES}


def fused_loss_bars(state, batch, ptr, idx, heads, blocks, r64=None):
    """{aap_loss, mip_loss, map_loss: closed-form bar of yr_s3rec_catalogue_bce's loss} on the float64 restatement's own
    F and T of ``batch``: what the fused path may add to ``loss_bars`` (its inputs carry the encoder's error, the
    kernel adds its own)."""
    r64 = r64 or step_and_grads(state, batch, ptr, idx, heads, blocks, dtype=torch.float64)
    X, m = np.asarray(batch["X"]).reshape(-1), np.asarray(batch["masks"]).reshape(-1)
    on, off, ones = m.astype(np.float64), (~m).astype(np.float64), np.ones(m.shape[0])
    A, I = np.asarray(state["attribute_embedding.weight"]), np.asarray(state["item_embedding.weight"])
    K = len(ptr) - 1
    return {"aap_loss": float(catalogue_bce(r64["F_aap"], A, ones, on, X, ptr, idx, K)["e_loss"]),
            "mip_loss": float(catalogue_bce(r64["F_mip"], I, off, off, X)["e_loss"]),
            "map_loss": float(catalogue_bce(r64["F_aap"], A, off, off, X, ptr, idx, K)["e_loss"]), "sp_loss": 0.0}


def bar_of(a32, a64):
    """BAR_FACTOR * max |f32 - f64| of one tensor or scalar of the restatement."""
    return BAR_FACTOR * float(np.max(np.abs(np.asarray(a32, np.float64) - np.asarray(a64, np.float64))))


# ---- the masking law, device-free ---------------------------------------------------------------------------------

def check_segments(X, seg_masked, pos, neg, L, other_row=None):
    """Assert the properties of ``segment_masking`` on host arrays; returns the segment lengths."""
    X, seg_masked, pos, neg = (np.asarray(a) for a in (X, seg_masked, pos, neg))
    B = X.shape[0]
    lens = np.empty(B, np.int64)
    for b in range(B):
        gone = np.flatnonzero(seg_masked[b] != X[b])
        # the masked stretch is contiguous (where X is 0 already, masking shows nothing: recover it from pos)
        cand = [(n, s) for n in range(2, L // 2) for s in range(0, L - n)
                if (seg_masked[b] == np.where((np.arange(L) >= s) & (np.arange(L) < s + n), 0, X[b])).all()
                and (pos[b, L - n:] == X[b, s:s + n]).all() and (pos[b, :L - n] == 0).all()]
        assert cand, ("no segment explains row", b, gone)
        lens[b] = min(n for n, _ in cand)
    return lens
