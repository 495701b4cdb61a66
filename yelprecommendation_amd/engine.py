"""Thin host wrappers: torch tensors in, C-ABI calls out (include/yelprec_engine.h).

PyTorch is plumbing here — it owns device memory and the stream; every arithmetic
op of the hot path runs in the hand-written HIP kernels of ``csrc/``.  All tensors
must live on a ROCm device (``tensor.is_cuda``); there is no CPU or eager fallback.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import DEFINES, EngineError, check, query_size

# the header's #define values under their Python names (include/yelprec_engine.h is the one place they are written)
LOSS_PARTIALS = DEFINES["YR_LOSS_PARTIALS"]
FLAG_BAD_USER, FLAG_BAD_ITEM = DEFINES["YR_FLAG_BAD_USER"], DEFINES["YR_FLAG_BAD_ITEM"]
OPT_ADAM, OPT_ADAMW = DEFINES["YR_OPT_ADAM"], DEFINES["YR_OPT_ADAMW"]
PULL_USER_PHASE, PULL_ITEM_PHASE = DEFINES["YR_PULL_USER_PHASE"], DEFINES["YR_PULL_ITEM_PHASE"]
SUPPORTED_WIDTHS = (16, 32, 64, 128)
# BPR-MF alone also takes the wide widths: push-form training (csrc/bpr_mf.hip), the slab sweep of the fused
# evaluation for k <= 16 (csrc/eval_topk.hip) and the score GEMM.  The pull form stays at SUPPORTED_WIDTHS.
WIDE_WIDTHS = (256, 512, 1024)
MF_WIDTHS = SUPPORTED_WIDTHS + WIDE_WIDTHS


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """hipStream_t of torch's current stream on the current device (follows torch.cuda.stream()).
    The raw accessor costs 0.3 us per call against 2.7 us for current_stream().cuda_stream — it is on
    every launch."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, dtype, name: str) -> int:
    if not isinstance(t, torch.Tensor):
        raise EngineError(f"{name}: expected a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise EngineError(f"{name}: tensor is on {t.device}; the engine runs on MI355X only (no CPU fallback)")
    if t.dtype != dtype:
        raise EngineError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise EngineError(f"{name}: tensor must be contiguous")
    return t.data_ptr()


def _rows(t: torch.Tensor, dtype, name: str) -> int:
    """A 2-D row-major operand whose rows may be views into a wider buffer (stride(1) == 1)."""
    if isinstance(t, torch.Tensor) and t.dim() == 2 and t.is_cuda and t.dtype == dtype and t.stride(1) == 1 \
            and t.stride(0) >= t.shape[1]:
        return t.data_ptr()
    return _dev(t, dtype, name)


def _opt(t, dtype, name):
    return None if t is None else _dev(t, dtype, name)


def _table_dims(U: torch.Tensor, I: torch.Tensor):
    if U.dim() != 2 or I.dim() != 2 or U.shape[1] != I.shape[1]:
        raise EngineError(f"tables must be [rows, D] with equal D, got {tuple(U.shape)} / {tuple(I.shape)}")
    return U.shape[0], I.shape[0], U.shape[1]


def new_error_flag(device) -> torch.Tensor:
    return torch.zeros(1, dtype=torch.int32, device=device)


def raise_on_flag(flag: torch.Tensor, what: str = "index"):
    """Host-side check of an err_flag word (one device sync)."""
    v = int(flag.item())
    if v:
        kinds = [k for b, k in ((FLAG_BAD_USER, "user"), (FLAG_BAD_ITEM, "item")) if v & b]
        flag.zero_()
        raise IndexError(f"{what}: out-of-range {' and '.join(kinds)} id(s) in a batch")


def mf_score(U, I, user, item, out=None, err_flag=None):
    """out[b] = U[user[b]] . I[item[b]]    (reference models/mf.py:20-23)."""
    lib = _lib.load()
    nu, ni, d = _table_dims(U, I)
    B = user.numel()
    if item.numel() != B:
        raise EngineError("user and item index tensors differ in length")
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=U.device)
    check(lib.yr_mf_score(_dev(U, torch.float32, "U"), _dev(I, torch.float32, "I"),
                          _dev(user, torch.int64, "user"), _dev(item, torch.int64, "item"),
                          B, d, nu, ni, _dev(out, torch.float32, "out"),
                          _opt(err_flag, torch.int32, "err_flag"), _stream()), "yr_mf_score")
    return out


def mf_score_backward(U, I, user, item, gout, gradU, gradI, err_flag=None):
    """gradU[user[b]] += gout[b] I[item[b]]; gradI[item[b]] += gout[b] U[user[b]]."""
    lib = _lib.load()
    nu, ni, d = _table_dims(U, I)
    B = user.numel()
    check(lib.yr_mf_score_backward(_dev(U, torch.float32, "U"), _dev(I, torch.float32, "I"),
                                   _dev(user, torch.int64, "user"), _dev(item, torch.int64, "item"),
                                   _dev(gout, torch.float32, "gout"), B, d, nu, ni,
                                   _dev(gradU, torch.float32, "gradU"), _dev(gradI, torch.float32, "gradI"),
                                   _opt(err_flag, torch.int32, "err_flag"), _stream()), "yr_mf_score_backward")


def bpr_mf_fwd_bwd(U, I, user, pos, neg, gradU, gradI, loss_partials, inv_batch=None, err_flag=None):
    """Fused BPR forward + loss (+ backward into dense gradU/gradI unless both None).

    reference trainers/mf_trainer.py:106-111.  ``loss_partials`` (float32[LOSS_PARTIALS])
    receives unscaled partial sums of softplus(-(s+ - s-)); see :func:`loss_finalize`.
    """
    lib = _lib.load()
    nu, ni, d = _table_dims(U, I)
    B = user.numel()
    if pos.numel() != B or neg.numel() != B:
        raise EngineError("user/pos/neg index tensors differ in length")
    if loss_partials.numel() != LOSS_PARTIALS:
        raise EngineError(f"loss_partials must hold {LOSS_PARTIALS} floats")
    if inv_batch is None:
        inv_batch = 1.0 / B if B else 0.0
    if gradU is not None and (gradU.shape != U.shape or gradI.shape != I.shape):
        raise EngineError("gradient buffers must match the table shapes")
    check(lib.yr_bpr_mf_fwd_bwd(_dev(U, torch.float32, "U"), _dev(I, torch.float32, "I"),
                                _dev(user, torch.int64, "user"), _dev(pos, torch.int64, "pos"),
                                _dev(neg, torch.int64, "neg"), B, d, nu, ni, float(inv_batch),
                                _opt(gradU, torch.float32, "gradU"), _opt(gradI, torch.float32, "gradI"),
                                _dev(loss_partials, torch.float32, "loss_partials"),
                                _opt(err_flag, torch.int32, "err_flag"), _stream()), "yr_bpr_mf_fwd_bwd")


PULL_MAX_BUCKETS = 16383      # csrc/bpr_pull.hip kMaxBuckets
PULL_MAX_USERS = (1 << 26) - 1


def pull_bucket_rows(d):
    """Rows per owner bucket of the pull step (1024 / D): the granularity of item-row chunks."""
    return 1024 // int(d)


def pull_supported(num_users, num_items, d):
    """Table shapes the pull step covers (include/yelprec_engine.h, limits of yr_bpr_mf_pull_step)."""
    if d not in SUPPORTED_WIDTHS:
        return False
    r = pull_bucket_rows(d)
    ru = 4 if (-(-num_users // r) < 768 and r > 4) else r       # few user rows: buckets of 4 rows (csrc/bpr_pull.hip)
    return (-(-num_users // ru) <= PULL_MAX_BUCKETS and -(-num_items // r) <= PULL_MAX_BUCKETS
            and num_users <= PULL_MAX_USERS)


def bpr_mf_pull_workspace(max_batch, num_users, num_items, d, device):
    """Scratch buffer for :func:`bpr_mf_pull_step` (uint8 tensor, 256-byte aligned by torch)."""
    n = query_size("yr_bpr_mf_pull_workspace_bytes", max_batch, num_users, num_items, d)
    return torch.empty(n, dtype=torch.uint8, device=device)


PULL_RULE_FIELDS = ("split_min", "split_target", "row_min", "row_target", "row_quad", "row_max_parts",
                    "row_task_pool", "row_split_compiled")


def bpr_mf_pull_split_summary(batch, num_users, num_items, d, workspace=None):
    """Which item buckets the pull step shares between workgroups (yr_bpr_mf_pull_split_summary), for tests and
    measurement scripts.  Returns a dict: the thresholds in force for (batch, num_items, d) under the names of
    ``PULL_RULE_FIELDS`` and, with the ``workspace`` of a partition whose user phase has run (one device sync),
    ``tasks`` / ``slots`` / ``row_tasks`` (what the batch wants) and ``parts`` (int32 array per item bucket:
    1 whole, P > 1 parts by tile range, -S rows shared by S parts)."""
    import ctypes
    import numpy as np
    lib = _lib.load()
    rule = (ctypes.c_int32 * 8)()
    counters = (ctypes.c_int32 * 4)()
    nb = query_size("yr_bpr_mf_pull_item_buckets", num_items, d)
    parts = np.zeros(nb, np.int32)
    if workspace is None:
        rc = lib.yr_bpr_mf_pull_split_summary(None, 0, int(batch), int(d), int(num_users), int(num_items), None, None,
                                              rule, None)
    else:
        rc = lib.yr_bpr_mf_pull_split_summary(workspace.data_ptr(), workspace.numel(), int(batch), int(d),
                                              int(num_users), int(num_items), counters, parts.ctypes.data, rule,
                                              _stream())
    check(rc, "yr_bpr_mf_pull_split_summary")
    out = dict(zip(PULL_RULE_FIELDS, (int(v) for v in rule)))
    if workspace is not None:
        out.update(tasks=int(counters[0]), slots=int(counters[1]), row_tasks=int(counters[2]), parts=parts)
    return out


def bpr_mf_pull_step(U_old, U_new, I, mU, vU, mI, vI, user, pos, neg, step, lr, loss_partials, workspace,
                     beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False, inv_batch=None,
                     gradI_out=None, err_flag=None, loss_out=None, loss_accum=None, deterministic=False):
    """One whole BPR-MF step (forward, loss, both gradients, dense Adam) without float atomics.

    reference trainers/mf_trainer.py:106-112.  Reads ``U_old``, writes ``U_new`` (distinct
    buffers, ping-ponged by the caller), updates ``I`` and the Adam state in place; with
    ``gradI_out`` the item pass emits the dense item gradient instead of applying Adam.
    """
    lib = _lib.load()
    nu, ni, d = _table_dims(U_old, I)
    B = user.numel()
    if pos.numel() != B or neg.numel() != B:
        raise EngineError("user/pos/neg index tensors differ in length")
    if U_new.shape != U_old.shape or U_new.data_ptr() == U_old.data_ptr():
        raise EngineError("U_new must be a distinct buffer of U_old's shape")
    if loss_partials.numel() != LOSS_PARTIALS:
        raise EngineError(f"loss_partials must hold {LOSS_PARTIALS} floats")
    if inv_batch is None:
        inv_batch = 1.0 / B if B else 0.0
    step_size, bc2_sqrt = adam_scalars(step, lr, beta1, beta2)
    f32 = torch.float32
    check(lib.yr_bpr_mf_pull_step(
        _dev(U_old, f32, "U_old"), _dev(U_new, f32, "U_new"), _dev(I, f32, "I"),
        _dev(mU, f32, "mU"), _dev(vU, f32, "vU"), _opt(mI, f32, "mI"), _opt(vI, f32, "vI"),
        _opt(gradI_out, f32, "gradI_out"),
        _dev(user, torch.int64, "user"), _dev(pos, torch.int64, "pos"), _dev(neg, torch.int64, "neg"),
        B, d, nu, ni, float(inv_batch), float(lr), float(step_size), float(bc2_sqrt), float(beta1), float(beta2),
        float(eps), float(weight_decay), OPT_ADAMW if decoupled else OPT_ADAM, 1 if deterministic else 0,
        _dev(workspace, torch.uint8, "workspace"), workspace.numel(),
        _dev(loss_partials, f32, "loss_partials"), _opt(loss_out, f32, "loss_out"),
        _opt(loss_accum, torch.float64, "loss_accum"), _opt(err_flag, torch.int32, "err_flag"), _stream()),
        "yr_bpr_mf_pull_step")


def triplet_sample(row_user, row_item, avoid_ptr, avoid_idx, num_users, num_items, seed, epoch, shuffle=True,
                   first=0, count=None, err_flag=None):
    """(user, pos, neg) for stream positions [first, first + count) of one epoch (csrc/triplets.hip;
    reference train.py:76-77 + data/datasets/mf_dataset.py:18-32)."""
    lib = _lib.load()
    n_rows = row_user.numel()
    count = n_rows - first if count is None else int(count)
    i64 = torch.int64
    out = [torch.empty(count, dtype=i64, device=row_user.device) for _ in range(3)]
    if avoid_ptr.numel() != num_users + 1:
        raise EngineError("avoid_ptr must hold num_users + 1 offsets")
    check(lib.yr_triplet_sample(_dev(row_user, i64, "row_user"), _dev(row_item, i64, "row_item"), n_rows,
                                _dev(avoid_ptr, i64, "avoid_ptr"),
                                _dev(avoid_idx, i64, "avoid_idx") if avoid_idx.numel() else _dev(avoid_ptr, i64, "avoid_ptr"),
                                int(num_users), int(num_items), int(seed) & (2**64 - 1), int(epoch) & (2**64 - 1),
                                1 if shuffle else 0, int(first), count,
                                *(_dev(t, i64, "out") if count else None for t in out),
                                _opt(err_flag, torch.int32, "err_flag"), _stream()), "yr_triplet_sample")
    return tuple(out)


# "rows": one wave per output row (default: the faster form on MI355X at Yelp2018 size, 76 us per launch);
# "sliced": feature slices pinned per XCD — half the fabric traffic (425 -> 217 MB, L2 hits 52 -> 76 %) but
# 80-89 us: the product is bound by the three dependent loads per short row, not by bytes
SPMM_FORM = "rows"


def spmm_csr(graph, X, out=None, accumulate=False, form=None):
    """Y = L X (or Y += L X) with L a :class:`yelprecommendation_amd.graph.LaplacianCSR`
    (reference models/ngcf.py:64,67: torch.sparse.mm(L, E))."""
    lib = _lib.load()
    n, d = X.shape
    if n != graph.n:
        raise EngineError(f"X has {n} rows, the graph {graph.n}")
    if out is None:
        if accumulate:
            raise EngineError("accumulate needs an output buffer")
        out = torch.empty_like(X)
    form = form or SPMM_FORM
    if form not in ("rows", "sliced"):
        raise EngineError("form must be 'rows' or 'sliced'")
    if form == "sliced":
        check(lib.yr_spmm_csr_sliced(_dev(graph.rowptr, torch.int32, "rowptr"), _dev(graph.col, torch.int32, "col"),
                                     _dev(graph.val, torch.float32, "val"), _dev(X, torch.float32, "X"),
                                     _dev(out, torch.float32, "Y"), n, d, 1 if accumulate else 0,
                                     _opt(graph.row_order, torch.int32, "row_order"), _stream()), "yr_spmm_csr_sliced")
        return out
    check(lib.yr_spmm_csr(_dev(graph.rowptr, torch.int32, "rowptr"), _dev(graph.col, torch.int32, "col"),
                          _dev(graph.val, torch.float32, "val"), _dev(X, torch.float32, "X"),
                          _dev(out, torch.float32, "Y"), n, d, 1 if accumulate else 0,
                          _opt(graph.heavy_rows, torch.int32, "heavy_rows"), graph.n_heavy, graph.heavy_threshold,
                          _stream()), "yr_spmm_csr")
    return out


NGCF_MAX_LAYERS = DEFINES["YR_NGCF_MAX_LAYERS"]


def _ptr_array(tensors, what):
    import ctypes
    if not 0 < len(tensors) <= NGCF_MAX_LAYERS:
        raise EngineError(f"{what}: between 1 and {NGCF_MAX_LAYERS} layer buffers")
    return (ctypes.c_void_p * len(tensors))(*[_dev(t, torch.float32, what) for t in tensors])


class NGCFRowSet:
    """A set of graph nodes for the batch-aware propagation: ``flags`` int32[N] (1 = member), ``rows`` int32[N]
    of which the first ``count[0]`` entries list the members in no particular order — ascending when the set was built
    with ``ordered=True`` (the count stays on the device),
    ``max_rows`` the host's upper bound of the count (sizes grids only); ``push``: few rows — the backward product
    scatters from them (spmm_csr_push_rows)."""
    __slots__ = ("flags", "rows", "count", "max_rows", "push")

    def __init__(self, n, device, max_rows, push=False):
        self.flags = torch.empty(n, dtype=torch.int32, device=device)
        self.rows = torch.empty(n, dtype=torch.int32, device=device)
        self.count = torch.empty(1, dtype=torch.int32, device=device)
        self.max_rows, self.push = int(min(max_rows, n)), bool(push)


def _frontier_order(lib, out):
    """The set's list rebuilt ascending from its flags (yr_ngcf_frontier_order): the same list in every run."""
    check(lib.yr_ngcf_frontier_order(out.flags.data_ptr(), out.flags.numel(), out.rows.data_ptr(), out.count.data_ptr(),
                                     _stream()), "yr_ngcf_frontier_order")
    return out


def ngcf_frontier_mark(num_users, num_items, user_id, pos_ids, neg_ids=None, max_rows=None, push=False, ordered=False):
    """The rows a batch's scores read — user_id, num_users + pos_ids, num_users + neg_ids (reference
    models/ngcf.py:31-32,37-39) — as an NGCFRowSet.  ``ordered``: the list ascending instead of in arrival order."""
    lib = _lib.load()
    i64 = torch.int64
    B = user_id.numel()
    out = NGCFRowSet(num_users + num_items, user_id.device, (2 if neg_ids is None else 3) * B if max_rows is None else max_rows, push)
    check(lib.yr_ngcf_frontier_mark(_dev(user_id, i64, "user_id") if B else None, _dev(pos_ids, i64, "pos_ids") if B else None,
                                    _dev(neg_ids, i64, "neg_ids") if (neg_ids is not None and B) else None, B,
                                    num_users, num_items, out.flags.data_ptr(), out.rows.data_ptr(), out.count.data_ptr(),
                                    1, _stream()), "yr_ngcf_frontier_mark")
    return _frontier_order(lib, out) if ordered else out


def ngcf_frontier_expand(graph, rows, max_rows=None, push=False, ordered=False):
    """The given NGCFRowSet plus all neighbours of its rows in the graph, as a new NGCFRowSet (``ordered``: its list
    ascending; the input's order never matters, only its members)."""
    lib = _lib.load()
    out = NGCFRowSet(graph.n, rows.flags.device, graph.n if max_rows is None else max_rows, push)
    check(lib.yr_ngcf_frontier_expand(_dev(graph.rowptr, torch.int32, "rowptr"), _dev(graph.col, torch.int32, "col"),
                                      graph.n, rows.rows.data_ptr(), rows.count.data_ptr(), rows.max_rows,
                                      out.flags.data_ptr(), out.rows.data_ptr(), out.count.data_ptr(), 1, _stream()),
          "yr_ngcf_frontier_expand")
    return _frontier_order(lib, out) if ordered else out


def spmm_csr_subset(graph, X, out, row_active=None, accumulate=False, rows=None):
    """:func:`spmm_csr` on the rows flagged in ``row_active`` (int32 flags; None: all); other rows of ``out`` are left
    as they are.  ``rows`` (NGCFRowSet, instead of ``row_active``): the same with the set's list driving the launch
    (cheap for small sets)."""
    if rows is not None:
        row_active = rows.flags
    lib = _lib.load()
    n, d = X.shape
    if n != graph.n or out.shape != X.shape:
        raise EngineError(f"X / out must be [{graph.n}, D]")
    check(lib.yr_spmm_csr_subset(_dev(graph.rowptr, torch.int32, "rowptr"), _dev(graph.col, torch.int32, "col"),
                                 _dev(graph.val, torch.float32, "val"), _dev(X, torch.float32, "X"),
                                 _dev(out, torch.float32, "Y"), n, d, 1 if accumulate else 0,
                                 _opt(graph.heavy_rows, torch.int32, "heavy_rows"), graph.n_heavy, graph.heavy_threshold,
                                 _opt(row_active, torch.int32, "row_active"),
                                 None if rows is None else rows.rows.data_ptr(),
                                 None if rows is None else rows.count.data_ptr(), 0 if rows is None else rows.max_rows,
                                 _stream()),
          "yr_spmm_csr_subset")
    return out


def spmm_csr_push_rows(graph, X, out, rows):
    """out[j] += sum over the rows r of ``rows`` (NGCFRowSet) of L[r, j] * X[r]: for the symmetric L the product
    out += L X restricted to those columns, as a scatter from the listed rows (yr_spmm_csr_push_rows)."""
    lib = _lib.load()
    n, d = X.shape
    if n != graph.n or out.shape != X.shape:
        raise EngineError(f"X / out must be [{graph.n}, D]")
    check(lib.yr_spmm_csr_push_rows(_dev(graph.rowptr, torch.int32, "rowptr"), _dev(graph.col, torch.int32, "col"),
                                    _dev(graph.val, torch.float32, "val"), _dev(X, torch.float32, "X"),
                                    _dev(out, torch.float32, "Y"), n, d, rows.rows.data_ptr(), rows.count.data_ptr(),
                                    rows.max_rows, _stream()), "yr_spmm_csr_push_rows")
    return out


def ngcf_score(layers, num_users, user_id, pos_ids, neg_ids=None, err_flag=None):
    """Scores of the concatenated layer embeddings (reference models/ngcf.py:44-58): returns
    ``pos`` or ``(pos, neg)``, each the sum over layers of per-layer dot products."""
    lib = _lib.load()
    n, d = layers[0].shape
    B = user_id.numel()
    i64 = torch.int64
    pos = torch.empty(B, dtype=torch.float32, device=layers[0].device)
    neg = torch.empty_like(pos) if neg_ids is not None else None
    check(lib.yr_ngcf_score_fwd(_ptr_array(layers, "layers"), len(layers), _dev(user_id, i64, "user_id"),
                                _dev(pos_ids, i64, "pos_ids"), _dev(neg_ids, i64, "neg_ids") if neg_ids is not None else None,
                                B, d, num_users, n - num_users, pos.data_ptr(),
                                neg.data_ptr() if neg is not None else None,
                                err_flag.data_ptr() if err_flag is not None else None, _stream()), "yr_ngcf_score_fwd")
    return pos if neg is None else (pos, neg)


def ngcf_owned_score_workspace_bytes(n, B):
    """Bytes of scratch :func:`ngcf_score_backward` needs with ``deterministic=True`` (EngineError for refused sizes)."""
    return query_size("yr_ngcf_owned_score_workspace_bytes", n, B)


def ngcf_owned_dw_workspace_bytes(rows, d):
    """Bytes of scratch :func:`ngcf_dense_bwd` needs with ``deterministic=True`` over at most ``rows`` rows."""
    return query_size("yr_ngcf_owned_dw_workspace_bytes", rows, d)


def _ngcf_scratch(workspace, nbytes, device, what):
    if workspace is None:
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < nbytes:
        raise EngineError(f"{what}: workspace must be a contiguous uint8 tensor of at least {nbytes} bytes")
    return workspace


def ngcf_score_backward(layers, dlayers, num_users, user_id, pos_ids, neg_ids, gpos, gneg, err_flag=None,
                        deterministic=False, workspace=None):
    """dlayers[k] += gradient of :func:`ngcf_score` w.r.t. layers[k] (float atomics).  ``deterministic``: no float
    atomics — every touched row of dlayers[k] is its content on entry plus the row's per-triplet contributions in
    ascending triplet index (yr_ngcf_owned_score_bwd; ``workspace``: uint8 scratch of
    :func:`ngcf_owned_score_workspace_bytes`, allocated when None)."""
    lib = _lib.load()
    n, d = layers[0].shape
    i64, f32 = torch.int64, torch.float32
    if len(layers) != len(dlayers):
        raise EngineError("layers / dlayers length mismatch")
    if deterministic:
        B = user_id.numel()
        ws = _ngcf_scratch(workspace, ngcf_owned_score_workspace_bytes(n, B), layers[0].device, "ngcf_score_backward")
        check(lib.yr_ngcf_owned_score_bwd(_ptr_array(layers, "layers"), _ptr_array(dlayers, "dlayers"), len(layers),
                                          _dev(user_id, i64, "user_id") if B else None,
                                          _dev(pos_ids, i64, "pos_ids") if B else None,
                                          _dev(neg_ids, i64, "neg_ids") if (neg_ids is not None and B) else None,
                                          _dev(gpos, f32, "gpos") if B else None,
                                          _dev(gneg, f32, "gneg") if (neg_ids is not None and B) else None,
                                          B, d, num_users, n - num_users, ws.data_ptr(), ws.numel(),
                                          err_flag.data_ptr() if err_flag is not None else None, _stream()),
              "yr_ngcf_owned_score_bwd")
        return
    check(lib.yr_ngcf_score_bwd(_ptr_array(layers, "layers"), _ptr_array(dlayers, "dlayers"), len(layers),
                                _dev(user_id, i64, "user_id"), _dev(pos_ids, i64, "pos_ids"),
                                _dev(neg_ids, i64, "neg_ids") if neg_ids is not None else None,
                                _dev(gpos, f32, "gpos"), _dev(gneg, f32, "gneg") if neg_ids is not None else None,
                                user_id.numel(), d, num_users, n - num_users,
                                err_flag.data_ptr() if err_flag is not None else None, _stream()), "yr_ngcf_score_bwd")


def ngcf_dense_fwd(E, Z, W1, W2, out=None, rows=None):
    """leaky_relu((Z + E) W1^T + (E * Z) W2^T)   (reference models/ngcf.py:64-72).  ``rows`` (NGCFRowSet): only
    those rows are computed (and written)."""
    lib = _lib.load()
    n, d = E.shape
    if out is None:
        out = torch.empty_like(E)
    f32 = torch.float32
    if rows is not None:
        check(lib.yr_ngcf_dense_fwd_rows(_dev(E, f32, "E"), _dev(Z, f32, "Z"), _dev(W1, f32, "W1"), _dev(W2, f32, "W2"),
                                         n, d, _dev(out, f32, "Eout"), rows.rows.data_ptr(), rows.count.data_ptr(),
                                         rows.max_rows, None, _stream()), "yr_ngcf_dense_fwd_rows")
        return out
    check(lib.yr_ngcf_dense_fwd(_dev(E, f32, "E"), _dev(Z, f32, "Z"), _dev(W1, f32, "W1"), _dev(W2, f32, "W2"),
                                n, d, _dev(out, f32, "Eout"), _stream()), "yr_ngcf_dense_fwd")
    return out


def ngcf_dense_bwd(dEout, Eout, E, Z, W1, W2, dE, dW1, dW2, dZ=None, W1T=None, W2T=None, rows=None,
                   deterministic=False, workspace=None):
    """Backward of :func:`ngcf_dense_fwd`: dE += ..., dW1 += ..., dW2 += ..., returns dZ.
    ``W1T / W2T``: the transposed weights if the caller already has them (one batched transpose
    for all layers instead of two small launches per layer).  ``rows`` (NGCFRowSet): the rows outside it have
    dEout = 0 and are skipped (their dZ is not written).  ``deterministic``: dW1 / dW2 without float atomics — the
    workgroups' partial sums go to slots of ``workspace`` (uint8 scratch of :func:`ngcf_owned_dw_workspace_bytes`,
    allocated when None) and are added to dW in workgroup order (yr_ngcf_owned_dense_bwd_weight); the data part has one
    owner per output in both modes."""
    lib = _lib.load()
    n, d = E.shape
    f32 = torch.float32
    if dZ is None:
        dZ = torch.empty_like(E)
    if W1T is None:
        W1T, W2T = W1.t().contiguous(), W2.t().contiguous()  # [in, out] layout for the data-gradient GEMM
    if deterministic:
        bound = n if rows is None else rows.max_rows
        ws = _ngcf_scratch(workspace, ngcf_owned_dw_workspace_bytes(bound, d), E.device, "ngcf_dense_bwd")
        r, c, m = (None, None, 0) if rows is None else (rows.rows.data_ptr(), rows.count.data_ptr(), rows.max_rows)
        check(lib.yr_ngcf_owned_dense_bwd_weight(_dev(dEout, f32, "dEout"), _dev(Eout, f32, "Eout"), _dev(E, f32, "E"),
                                                 _dev(Z, f32, "Z"), n, d, _dev(dW1, f32, "dW1"), _dev(dW2, f32, "dW2"),
                                                 r, c, m, ws.data_ptr(), ws.numel(), _stream()),
              "yr_ngcf_owned_dense_bwd_weight")
        if rows is not None:
            check(lib.yr_ngcf_dense_bwd_data_rows(_dev(dEout, f32, "dEout"), _dev(Eout, f32, "Eout"), _dev(E, f32, "E"),
                                                  _dev(Z, f32, "Z"), _dev(W1T, f32, "W1T"), _dev(W2T, f32, "W2T"), n, d,
                                                  _dev(dZ, f32, "dZ"), _dev(dE, f32, "dE"), r, c, m, _stream()),
                  "yr_ngcf_dense_bwd_data_rows")
        else:
            check(lib.yr_ngcf_dense_bwd_data(_dev(dEout, f32, "dEout"), _dev(Eout, f32, "Eout"), _dev(E, f32, "E"),
                                             _dev(Z, f32, "Z"), _dev(W1T, f32, "W1T"), _dev(W2T, f32, "W2T"), n, d,
                                             _dev(dZ, f32, "dZ"), _dev(dE, f32, "dE"), _stream()),
                  "yr_ngcf_dense_bwd_data")
        return dZ
    if rows is not None:
        r, c, m = rows.rows.data_ptr(), rows.count.data_ptr(), rows.max_rows
        check(lib.yr_ngcf_dense_bwd_weight_rows(_dev(dEout, f32, "dEout"), _dev(Eout, f32, "Eout"), _dev(E, f32, "E"),
                                                _dev(Z, f32, "Z"), n, d, _dev(dW1, f32, "dW1"), _dev(dW2, f32, "dW2"),
                                                r, c, m, _stream()), "yr_ngcf_dense_bwd_weight_rows")
        check(lib.yr_ngcf_dense_bwd_data_rows(_dev(dEout, f32, "dEout"), _dev(Eout, f32, "Eout"), _dev(E, f32, "E"),
                                              _dev(Z, f32, "Z"), _dev(W1T, f32, "W1T"), _dev(W2T, f32, "W2T"), n, d,
                                              _dev(dZ, f32, "dZ"), _dev(dE, f32, "dE"), r, c, m, _stream()),
              "yr_ngcf_dense_bwd_data_rows")
        return dZ
    check(lib.yr_ngcf_dense_bwd_weight(_dev(dEout, f32, "dEout"), _dev(Eout, f32, "Eout"), _dev(E, f32, "E"),
                                       _dev(Z, f32, "Z"), n, d, _dev(dW1, f32, "dW1"), _dev(dW2, f32, "dW2"),
                                       _stream()), "yr_ngcf_dense_bwd_weight")
    check(lib.yr_ngcf_dense_bwd_data(_dev(dEout, f32, "dEout"), _dev(Eout, f32, "Eout"), _dev(E, f32, "E"),
                                     _dev(Z, f32, "Z"), _dev(W1T, f32, "W1T"), _dev(W2T, f32, "W2T"), n, d,
                                     _dev(dZ, f32, "dZ"), _dev(dE, f32, "dE"), _stream()), "yr_ngcf_dense_bwd_data")
    return dZ


ACT_IDENTITY, ACT_SIGMOID, ACT_RELU = 0, 1, 2
COUNT_WORDS, COUNT_SLOTS = DEFINES["YR_COUNT_WORDS"], DEFINES["YR_COUNT_SLOTS"]


def gemm_f32(A, B, transA=False, transB=False, out=None, bias=None, act=ACT_IDENTITY, accumulate=False,
             split_k=1, alpha_count=None, rowsum=None):
    """out (+)= op(A) @ op(B) on the f32 matrix cores.  A, B 2-D row-major f32 GPU tensors;
    ``transA``: use A^T, ``transB``: use B^T (nn.Linear's ``x @ W^T`` is ``transB=True``).
    ``alpha_count`` (spread int32 count, COUNT_WORDS words): the product is scaled by 1 / count; ``rowsum`` ([M] f32): receives
    alpha * the row sums of op(A) (yr_gemm_f32_ex)."""
    lib = _lib.load()
    f32 = torch.float32
    M, K = (A.shape[1], A.shape[0]) if transA else (A.shape[0], A.shape[1])
    K2, N = (B.shape[1], B.shape[0]) if transB else (B.shape[0], B.shape[1])
    if K != K2:
        raise EngineError(f"inner dimensions differ: {K} vs {K2}")
    if out is None:
        if accumulate:
            raise EngineError("accumulate needs an output buffer")
        out = (torch.zeros if split_k > 1 else torch.empty)((M, N), dtype=f32, device=A.device)
    if out.shape != (M, N) or out.stride(1) != 1:
        raise EngineError("bad output buffer")
    if alpha_count is not None and alpha_count.numel() != COUNT_WORDS:
        raise EngineError(f"alpha_count: a spread count of {COUNT_WORDS} int32 words")
    if alpha_count is not None or rowsum is not None:
        if rowsum is not None and rowsum.numel() != M:
            raise EngineError("rowsum needs one element per row of op(A)")
        check(lib.yr_gemm_f32_ex(1 if transA else 0, 1 if transB else 0, M, N, K, _rows(A, f32, "A"), A.stride(0),
                                 _rows(B, f32, "B"), B.stride(0), out.data_ptr(), out.stride(0),
                                 _opt(bias, f32, "bias"), int(act), 1 if accumulate else 0, int(split_k),
                                 _opt(alpha_count, torch.int32, "alpha_count"), _opt(rowsum, f32, "rowsum"),
                                 _stream()), "yr_gemm_f32_ex")
        return out
    check(lib.yr_gemm_f32(1 if transA else 0, 1 if transB else 0, M, N, K, _rows(A, f32, "A"), A.stride(0),
                          _rows(B, f32, "B"), B.stride(0), out.data_ptr(), out.stride(0),
                          _opt(bias, f32, "bias"), int(act), 1 if accumulate else 0, int(split_k), _stream()),
          "yr_gemm_f32")
    return out


def spread_count(value, device):
    """A spread count holding ``value`` (tests; the kernels fill it with atomics)."""
    c = torch.zeros(COUNT_WORDS, dtype=torch.int32, device=device)
    c[0] = int(value)
    return c


def cdae_decode_loss_partials(B, I):
    return int(_lib.load().yr_cdae_decode_loss_partials(int(B), int(I)))


def cdae_decode_loss(z, Wo, bo, target, negative_mask, act, G, partial_loss, count, pred=None):
    """Decoder of the CDAE training step with the NS-BCE / BCE loss in its epilogue (yr_cdae_decode_loss):
    G = d loss / d pre-activation without the 1 / count factor, per-workgroup loss partials, count of the
    selected positions (``count`` must be zero on entry)."""
    lib = _lib.load()
    f32 = torch.float32
    B, H = z.shape
    I = Wo.shape[0]
    if partial_loss.numel() < cdae_decode_loss_partials(B, I) or G.shape != (B, I) or target.shape != (B, I):
        raise EngineError("bad buffers for cdae_decode_loss")
    if count.numel() != COUNT_WORDS:
        raise EngineError(f"count: a spread count of {COUNT_WORDS} int32 words")
    if pred is not None and (pred.shape != G.shape or pred.stride() != G.stride()):
        raise EngineError("pred must have the layout of G")
    check(lib.yr_cdae_decode_loss(_dev(z, f32, "z"), _dev(Wo, f32, "Wo"), _opt(bo, f32, "bo"),
                                  _dev(target, f32, "target"), _opt(negative_mask, f32, "negative_mask"), B, I, H,
                                  int(act), _rows(G, f32, "G"), G.stride(0),
                                  None if pred is None else _rows(pred, f32, "pred"),
                                  _dev(partial_loss, f32, "partial_loss"), _dev(count, torch.int32, "count"),
                                  _stream()), "yr_cdae_decode_loss")
    return G


class TrainLists:
    """A CDAE training batch as lists (yr_cdae_train_lists): ``rows`` — the encoder's input, a SparseRows of
    dropout_p(train items) — and ``loss`` — (columns, targets, counts) of the NS-BCE positions (positives +
    sampled negatives).  The buffers are sized for the worst case once per (device, B, I) and reused by the
    next batch made from the same ``pool`` — ONE batch of a pool is alive at a time: the next one overwrites the
    storage, and a consumer handed a batch that is no longer the pool's latest gets an EngineError from
    :meth:`alive` (CDAEStep.step_lists, CDAETrainer._scored_by_lists and loss_dense call it) instead of silently
    reading another batch's lists.  Every CDAEBatchLoader owns its pool, so the train / valid / test loaders do
    not alias each other; without ``pool`` a class-level one is used."""
    _pool = {}

    def __init__(self, ptr, idx, users, num_users, num_items, neg_times, neg_seed, drop_seed, p, err_flag=None,
                 extra=None, pool=None, batch_rows=None, targets=None):
        """``extra``: (ptr, idx) of a second per-user CSR whose items are positives of the loss list too (the
        held-out items in validation) without entering the encoder list.
        ``batch_rows``: ``users`` holds SEVERAL batches of that many rows (the last may be short) and ``neg_seed`` /
        ``drop_seed`` are int64 device tensors with one seed per batch — one launch makes exactly the lists one
        TrainLists per batch would (yr_cdae_train_lists_batched).
        ``targets``: (ptr, idx) of the per-user CSR the plain-BCE loss of these rows reads (cdae_catalogue_bce: every
        catalogue position, no loss list); kept as ``self.targets`` beside the lists, not read here."""
        lib = _lib.load()
        B, I = users.numel(), int(num_items)
        dev = users.device
        key = (dev, B, I)
        pool = TrainLists._pool if pool is None else pool
        slot = pool.get(key)
        if slot is None:
            n, parts = B * SPARSE_PARTS * sparse_part_columns(I), B * SPARSE_PARTS
            mk = lambda m, dt: torch.empty(m, dtype=dt, device=dev)
            slot = [(mk(n, torch.int32), mk(n, torch.float32), mk(parts, torch.int32),
                     mk(n, torch.int32), mk(n, torch.float32), mk(parts, torch.int32)), 0]
            pool.clear()                                # a batch of the old shape keeps its own references
            pool[key] = slot
        slot[1] += 1
        self._slot, self._generation = slot, slot[1]
        buf = slot[0]
        i64 = torch.int64
        some = lambda t: t if t.numel() else torch.zeros(1, dtype=i64, device=dev)   # an empty index: never read, needs an address
        if batch_rows is not None:
            nb = -(-B // int(batch_rows)) if B else 0
            if not (torch.is_tensor(neg_seed) and torch.is_tensor(drop_seed) and neg_seed.numel() >= nb
                    and drop_seed.numel() >= nb):
                raise EngineError("batched TrainLists: one neg / drop seed per batch (int64 device tensors)")
            check(lib.yr_cdae_train_lists_batched(
                _dev(ptr, i64, "ptr"), _dev(some(idx), i64, "idx"), None if extra is None else _dev(extra[0], i64, "ptr2"),
                None if extra is None else _dev(some(extra[1]), i64, "idx2"), _dev(users, i64, "users"), B, int(num_users),
                I, int(neg_times), _dev(neg_seed, i64, "neg_seeds"), _dev(drop_seed, i64, "drop_seeds"), int(batch_rows),
                float(p), *(t.data_ptr() for t in buf), _opt(err_flag, torch.int32, "err_flag"), _stream()),
                "yr_cdae_train_lists_batched")
        else:
            check(lib.yr_cdae_train_lists(_dev(ptr, i64, "ptr"), _dev(some(idx), i64, "idx"),
                                          None if extra is None else _dev(extra[0], i64, "ptr2"),
                                          None if extra is None else _dev(some(extra[1]), i64, "idx2"), _dev(users, i64, "users"), B,
                                          int(num_users), I, int(neg_times), int(neg_seed) & (2**64 - 1),
                                          int(drop_seed) & (2**64 - 1), float(p), *(t.data_ptr() for t in buf),
                                          _opt(err_flag, torch.int32, "err_flag"), _stream()), "yr_cdae_train_lists")
        self.rows = SparseRows.from_buffers(buf[0], buf[1], buf[2], B, I)
        self.loss = (buf[3], buf[4], buf[5])
        self.targets = targets
        self.B, self.I = B, I

    def alive(self):
        """Raise when a later batch of the same pool has overwritten this batch's storage."""
        if self._slot[1] != self._generation:
            raise EngineError("TrainLists: this batch's buffers were reused by a later batch of the same loader "
                              "(one batch of a loader is alive at a time; consume it before fetching the next)")
        return self

    def loss_dense(self):
        """(target, negative_mask) [B, I] the loss lists stand for (tests)."""
        self.alive()
        t = SparseRows.from_buffers(self.loss[0], self.loss[1] + 1.0, self.loss[2], self.B, self.I).to_dense()
        return (t == 2.0).float(), (t == 1.0).float()


def cdae_sampled_decode_splits(B):
    return int(_lib.load().yr_cdae_sampled_decode_splits(int(B)))


def cdae_sampled_decode(loss_lists, z, Wo, bo, act, dz, dWo, dbo, partial_loss, count):
    """Decoder forward + loss + all three decoder gradients on the loss positions only (yr_cdae_sampled_decode);
    everything it adds to comes out WITHOUT the 1 / count of the mean loss.  ``dz = dWo = dbo = None``: the loss
    partials and the count only (validation)."""
    lib = _lib.load()
    f32 = torch.float32
    lc, lv, ln = loss_lists
    B, H = z.shape
    I = Wo.shape[0]
    if partial_loss.numel() < B * cdae_sampled_decode_splits(B) or count.numel() != COUNT_WORDS:
        raise EngineError("bad buffers for cdae_sampled_decode")
    check(lib.yr_cdae_sampled_decode(_dev(lc, torch.int32, "loss_cols"), _dev(lv, f32, "loss_targets"),
                                     _dev(ln, torch.int32, "loss_count"), _dev(z, f32, "z"), _dev(Wo, f32, "Wo"),
                                     _opt(bo, f32, "bo"), B, I, H, int(act), _opt(dz, f32, "dz"), _opt(dWo, f32, "dWo"),
                                     _opt(dbo, f32, "dbo"), _dev(partial_loss, f32, "partial_loss"), _dev(count, torch.int32, "count"),
                                     _stream()), "yr_cdae_sampled_decode")


# ---- CDAE without negative sampling (csrc/cdae_catalogue.hip: the catalogue BCE) ----
CDAE_CATALOGUE_HIDDEN = (16, 32, 64, 128)      # the widths yr_cdae_catalogue_bce is built for


def cdae_catalogue_bce_workspace_floats(B, I, H):
    """Floats of the catalogue-BCE workspace (yr_cdae_catalogue_bce_workspace_floats)."""
    return query_size("yr_cdae_catalogue_bce_workspace_floats", B, I, H)


def cdae_catalogue_bce(z, Wo, bo, users, tgt_ptr, tgt_idx, act, grads=True, workspace=None, err_flag=None, out=None):
    """(row_loss [B], dz [B, H] or None, dWo [I, H] or None, dbo [I] or None) of yr_cdae_catalogue_bce: torch's BCELoss
    between act(z Wo^T + bo) and the 0/1 rows the per-user CSR (``tgt_ptr`` [K + 1], ``tgt_idx``, int64, item ids
    ascending) gives the rows' ``users``, over ALL B I positions.  ``row_loss`` holds the rows' sums of terms (not
    divided); the gradients carry the mean's 1 / (B I).  ``grads`` False is the loss-only call.  ``out``: the
    (row_loss, dz, dWo, dbo) to write into instead of new tensors (a training step's own buffers)."""
    lib = _lib.load()
    f32, i64 = torch.float32, torch.int64
    if z.dim() != 2 or Wo.dim() != 2 or z.shape[1] != Wo.shape[1]:
        raise EngineError(f"cdae_catalogue_bce: z [B, H] and Wo [I, H] expected, got {tuple(z.shape)} / {tuple(Wo.shape)}")
    (B, H), I = z.shape, Wo.shape[0]
    if bo is None or bo.numel() != I:
        raise EngineError("cdae_catalogue_bce: bo holds one entry per row of Wo")
    if users.numel() != B:
        raise EngineError("cdae_catalogue_bce: users holds one entry per row of z")
    if tgt_ptr is None or tgt_idx is None or tgt_ptr.numel() < 1:
        raise EngineError("cdae_catalogue_bce: the targets are a CSR (tgt_ptr [K + 1], tgt_idx)")
    if int(act) not in (ACT_IDENTITY, ACT_SIGMOID):
        raise EngineError("cdae_catalogue_bce: the output activation is the identity or the sigmoid")
    K = tgt_ptr.numel() - 1
    dev = z.device
    if workspace is None:
        n = cdae_catalogue_bce_workspace_floats(B, I, H)
        workspace = torch.empty(n if grads else n // (1 + H), dtype=f32, device=dev)
    if out is not None:
        row_loss, dz, dWo, dbo = out
        if row_loss.numel() != B or (grads and (dz.shape != (B, H) or dWo.shape != (I, H) or dbo.numel() != I)):
            raise EngineError("cdae_catalogue_bce: out = (row_loss [B], dz [B, H], dWo [I, H], dbo [I])")
        if not grads:
            dz = dWo = dbo = None
    else:
        row_loss = torch.zeros(B, dtype=f32, device=dev)
        dz = torch.empty((B, H), dtype=f32, device=dev) if grads else None
        dWo = torch.empty((I, H), dtype=f32, device=dev) if grads else None
        dbo = torch.empty(I, dtype=f32, device=dev) if grads else None
    # an empty CSR has no storage to point at: its offsets array stands in (never dereferenced: every list is empty)
    idx = _dev(tgt_idx, i64, "tgt_idx") if tgt_idx.numel() else _dev(tgt_ptr, i64, "tgt_ptr")
    check(lib.yr_cdae_catalogue_bce(_dev(z, f32, "z"), _dev(Wo, f32, "Wo"), _dev(bo, f32, "bo"),
                                    _dev(users, i64, "users"), _dev(tgt_ptr, i64, "tgt_ptr"), idx, B, I, K, H, int(act),
                                    _dev(row_loss, f32, "row_loss") if B else None, _opt(dz, f32, "dz") if B else None,
                                    _opt(dWo, f32, "dWo") if I else None, _opt(dbo, f32, "dbo") if I else None,
                                    _dev(workspace, f32, "workspace") if workspace.numel() else None,
                                    workspace.numel(), _opt(err_flag, torch.int32, "flag"), _stream()),
          "yr_cdae_catalogue_bce")
    return row_loss, dz, dWo, dbo


def cdae_loss_finalize_batched(partial_loss, splits, loss_count, rows, batch_rows, means, arrive, loss_accum):
    """loss_accum += sum over the batches of ``batch_rows`` rows of (the batch's loss partials / its positions):
    the validation loss of several batches scored by one cdae_sampled_decode launch (yr_cdae_loss_finalize_batched)."""
    lib = _lib.load()
    check(lib.yr_cdae_loss_finalize_batched(_dev(partial_loss, torch.float32, "partial_loss"), int(splits),
                                            _dev(loss_count, torch.int32, "loss_count"), int(rows), int(batch_rows),
                                            _dev(means, torch.float32, "means"), _dev(arrive, torch.int32, "arrive"),
                                            _opt(loss_accum, torch.float64, "loss_accum"), _stream()),
          "yr_cdae_loss_finalize_batched")


def cdae_loss_finalize(partial_loss, n_partials, count, stats, loss_accum=None):
    """stats[0] = sum(partials) / count, stats[1] = count; ``loss_accum`` (float64 device scalar) += stats[0]."""
    lib = _lib.load()
    check(lib.yr_cdae_loss_finalize(_dev(partial_loss, torch.float32, "partial_loss"), int(n_partials),
                                    _dev(count, torch.int32, "count"), _dev(stats, torch.float32, "stats"),
                                    _opt(loss_accum, torch.float64, "loss_accum"), _stream()), "yr_cdae_loss_finalize")


def cdae_hidden_bwd(dz, z, act, user, dV, touched_users, dbh, partial_loss=None, n_partials=0, count=None,
                    stats=None, loss_accum=None, scale_dz=False):
    """dz <- dz * act'(z) (``scale_dz``: dz / count first); dbh = column sums; dV[user] += dz (rows marked in
    ``touched_users``); with ``n_partials`` > 0 also the loss of the step into ``stats`` / ``loss_accum``."""
    lib = _lib.load()
    f32 = torch.float32
    B, H = dz.shape
    check(lib.yr_cdae_hidden_bwd(_dev(dz, f32, "dz"), _dev(z, f32, "z"), int(act), _dev(user, torch.int64, "user"),
                                 B, H, dV.shape[0], _dev(dV, f32, "dV"), _opt(touched_users, torch.uint8, "touched"),
                                 _dev(dbh, f32, "dbh"), _opt(partial_loss, f32, "partial_loss"), int(n_partials),
                                 _opt(count, torch.int32, "count"), _opt(stats, f32, "stats"),
                                 _opt(loss_accum, torch.float64, "loss_accum"), 1 if scale_dz else 0, _stream()),
          "yr_cdae_hidden_bwd")


def cdae_hidden_init(bias, V, user, err_flag=None):
    """zpre[b] = bias + V[user[b]]   (reference models/cdae.py:49)."""
    lib = _lib.load()
    B, H = user.numel(), V.shape[1]
    out = torch.empty((B, H), dtype=torch.float32, device=V.device)
    check(lib.yr_cdae_hidden_init(out.data_ptr(), _dev(bias, torch.float32, "bias"), _dev(V, torch.float32, "V"),
                                  _dev(user, torch.int64, "user"), B, H, V.shape[0],
                                  _opt(err_flag, torch.int32, "err_flag"), _stream()), "yr_cdae_hidden_init")
    return out


def dropout(x, rnd, p):
    lib = _lib.load()
    out = torch.empty_like(x)
    check(lib.yr_dropout(_dev(x, torch.float32, "x"), _dev(rnd, torch.float32, "rnd"), float(p), x.numel(),
                         out.data_ptr(), _stream()), "yr_dropout")
    return out


SPARSE_PARTS = 32       # csrc/cdae_sparse.hip kParts


def sparse_part_columns(I):
    """Columns per sub-list of a SparseRows row (list buffers hold B * SPARSE_PARTS * this many entries)."""
    return int(_lib.load().yr_cdae_sparse_part_columns(int(I)))


class SparseRows:
    """(column, value) lists of the non-zeros of dropout_p(x), 32 sub-lists per row (csrc/cdae_sparse.hip);
    the list buffers are sized for the worst case once per batch shape and reused by the next call."""
    _pool = {}

    def __init__(self, x, seed=0, p=0.0, count=None, negative_mask=None, loss_lists=None):
        """``negative_mask`` + ``loss_lists`` (cols int32, targets f32, count int32 buffers like this object's):
        the same pass also writes the loss positions of every row — target + negative_mask != 0 — as
        (column, target) lists (yr_cdae_compact_pair)."""
        lib = _lib.load()
        B, I = x.shape
        self.cpp = int(lib.yr_cdae_sparse_part_columns(I))
        key = (x.device, B, I)
        buf = SparseRows._pool.get(key)
        if buf is None:
            n = B * SPARSE_PARTS * self.cpp
            buf = (torch.empty(n, dtype=torch.int32, device=x.device), torch.empty(n, dtype=torch.float32, device=x.device))
            SparseRows._pool = {key: buf}                  # one batch shape at a time
        self.cols, self.vals = buf
        self.count = torch.empty(B * SPARSE_PARTS, dtype=torch.int32, device=x.device) if count is None else count
        self.B, self.I = B, I
        if negative_mask is not None:
            lc, lv, ln = loss_lists
            if lc.numel() < self.cols.numel() or lv.numel() < self.cols.numel() or ln.numel() < self.count.numel():
                raise EngineError("loss list buffers too small")
            check(lib.yr_cdae_compact_pair(_dev(x, torch.float32, "x"), _dev(negative_mask, torch.float32, "negative_mask"),
                                           B, I, int(seed) & (2**64 - 1), float(p), self.cols.data_ptr(),
                                           self.vals.data_ptr(), self.count.data_ptr(), _dev(lc, torch.int32, "loss_cols"),
                                           _dev(lv, torch.float32, "loss_targets"), _dev(ln, torch.int32, "loss_count"),
                                           _stream()), "yr_cdae_compact_pair")
            return
        check(lib.yr_cdae_compact_rows(_dev(x, torch.float32, "x"), B, I, int(seed) & (2**64 - 1), float(p),
                                       self.cols.data_ptr(), self.vals.data_ptr(), self.count.data_ptr(), _stream()),
              "yr_cdae_compact_rows")

    @classmethod
    def from_buffers(cls, cols, vals, count, B, I):
        """Lists that something else filled (yr_cdae_train_lists)."""
        self = cls.__new__(cls)
        self.cols, self.vals, self.count, self.B, self.I = cols, vals, count, int(B), int(I)
        self.cpp = sparse_part_columns(I)
        return self

    def to_dense(self):
        """The dense matrix the lists stand for (tests)."""
        B, P, cpp = self.B, SPARSE_PARTS, self.cpp
        out = torch.zeros(B, self.I, dtype=torch.float32, device=self.cols.device)
        m = torch.arange(cpp, device=out.device)[None, :] < self.count[:, None]          # [B*P, cpp]
        rows = torch.arange(B, device=out.device).repeat_interleave(P)[:, None].expand(-1, cpp)[m]
        out[rows, self.cols.view(B * P, cpp)[m].long()] = self.vals.view(B * P, cpp)[m]
        return out

    def row_columns(self, r):
        """Columns of row r in list order (tests)."""
        c = self.cols.view(self.B, SPARSE_PARTS, self.cpp)[r]
        n = self.count.view(self.B, SPARSE_PARTS)[r]
        return torch.cat([c[q, :int(n[q])] for q in range(SPARSE_PARTS)])


def cdae_sparse_encode(rows: "SparseRows", Wh, bh, V, user, act, err_flag=None, out=None, transposed=False):
    """z = act(Wh . rows + bh + V[user])   (reference models/cdae.py:49, sparse input).  ``transposed``: ``Wh`` is the
    [I, H] working copy (yr_cdae_sparse_encode_t)."""
    lib = _lib.load()
    H = Wh.shape[1] if transposed else Wh.shape[0]
    z = torch.empty(rows.B, H, dtype=torch.float32, device=Wh.device) if out is None else out
    fn = lib.yr_cdae_sparse_encode_t if transposed else lib.yr_cdae_sparse_encode
    check(fn(rows.cols.data_ptr(), rows.vals.data_ptr(), rows.count.data_ptr(),
                                    _dev(Wh, torch.float32, "Wh"), _dev(bh, torch.float32, "bh"),
                                    _dev(V, torch.float32, "V"), _dev(user, torch.int64, "user"), rows.B, rows.I, H,
                                    V.shape[0], int(act), z.data_ptr(), _opt(err_flag, torch.int32, "err_flag"),
                                    _stream()), "yr_cdae_sparse_encode")
    return z


def cdae_sparse_dwh_t(rows: "SparseRows", dz, dWhT, touched_items):
    """dWhT [I, H] (zero where unmarked) += rows^T . dz, rows marked in ``touched_items`` (yr_cdae_sparse_dwh_t)."""
    lib = _lib.load()
    check(lib.yr_cdae_sparse_dwh_t(rows.cols.data_ptr(), rows.vals.data_ptr(), rows.count.data_ptr(),
                                   _dev(dz, torch.float32, "dz"), rows.B, rows.I, dz.shape[1],
                                   _dev(dWhT, torch.float32, "dWhT"), _dev(touched_items, torch.uint8, "touched_items"),
                                   _stream()), "yr_cdae_sparse_dwh_t")


def cdae_hidden_bwd_dwh_t(rows: "SparseRows", dz, z, act, user, count, dV, touched_users, dbh, dWhT, touched_items,
                          partial_loss, n_partials, stats, loss_accum=None, scale_dz=False):
    """cdae_hidden_bwd + cdae_sparse_dwh_t in one launch (yr_cdae_hidden_bwd_dwh_t); ``dbh`` must be zero on entry."""
    lib = _lib.load()
    f32 = torch.float32
    check(lib.yr_cdae_hidden_bwd_dwh_t(rows.cols.data_ptr(), rows.vals.data_ptr(), rows.count.data_ptr(),
                                       _dev(dz, f32, "dz"), _dev(z, f32, "z"), int(act), 1 if scale_dz else 0,
                                       _dev(count, torch.int32, "count"), _dev(user, torch.int64, "user"), rows.B,
                                       rows.I, dz.shape[1], dV.shape[0], _dev(dV, f32, "dV"),
                                       _opt(touched_users, torch.uint8, "touched_users"), _dev(dbh, f32, "dbh"),
                                       _dev(dWhT, f32, "dWhT"), _dev(touched_items, torch.uint8, "touched_items"),
                                       _opt(partial_loss, f32, "partial_loss"), int(n_partials),
                                       _opt(stats, f32, "stats"), _opt(loss_accum, torch.float64, "loss_accum"),
                                       _stream()), "yr_cdae_hidden_bwd_dwh_t")


# ---- the reproducible form of the list-batch step (csrc/cdae_owned.hip: owner-pass gradients, no float atomics) ----
CDAE_OWNED_HIDDEN = (16, 32, 64, 128, 256, 512, 1024)


def cdae_owned_workspace_bytes(B, I, H):
    """Bytes of the workspace yr_cdae_owned_decode and yr_cdae_owned_hidden_bwd share (yr_cdae_owned_workspace_bytes)."""
    return query_size("yr_cdae_owned_workspace_bytes", B, I, H)


def _owned_workspace(workspace, B, I, H, what):
    if workspace is None or not workspace.is_cuda or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise EngineError(f"{what}: workspace must be a contiguous uint8 device tensor")
    if workspace.numel() < cdae_owned_workspace_bytes(B, I, H):
        raise EngineError(f"{what}: workspace smaller than cdae_owned_workspace_bytes({B}, {I}, {H})")
    return workspace.data_ptr(), workspace.numel()


def cdae_owned_decode(loss_lists, z, Wo, bo, act, dz, dWo, dbo, partial_loss, count, workspace):
    """cdae_sampled_decode with all three gradients, every sum by the owner of its destination in ascending row order
    (yr_cdae_owned_decode): dz written whole, dWo / dbo rows of the batch's loss columns stored, nothing else touched;
    ``count`` zero on entry.  Two calls on the same operands give the same bits."""
    lib = _lib.load()
    f32 = torch.float32
    lc, lv, ln = loss_lists
    if z.dim() != 2 or Wo.dim() != 2 or z.shape[1] != Wo.shape[1]:
        raise EngineError(f"cdae_owned_decode: z [B, H] and Wo [I, H] expected, got {tuple(z.shape)} / {tuple(Wo.shape)}")
    (B, H), I = z.shape, Wo.shape[0]
    if dz is None or dWo is None or dbo is None or dz.shape != (B, H) or dWo.shape != (I, H) or dbo.numel() != I:
        raise EngineError("cdae_owned_decode: dz [B, H], dWo [I, H] and dbo [I] are all required")
    if bo is not None and bo.numel() != I:
        raise EngineError("cdae_owned_decode: bo holds one entry per row of Wo")
    if partial_loss.numel() < B * cdae_sampled_decode_splits(B) or count.numel() != COUNT_WORDS:
        raise EngineError("bad buffers for cdae_owned_decode")
    n = B * SPARSE_PARTS * sparse_part_columns(I) if I else 0
    if lc.numel() < n or lv.numel() < n or ln.numel() < B * SPARSE_PARTS:
        raise EngineError("cdae_owned_decode: loss list buffers too small")
    ws, ws_bytes = _owned_workspace(workspace, B, I, H, "cdae_owned_decode")
    check(lib.yr_cdae_owned_decode(_dev(lc, torch.int32, "loss_cols"), _dev(lv, f32, "loss_targets"),
                                   _dev(ln, torch.int32, "loss_count"), _dev(z, f32, "z"), _dev(Wo, f32, "Wo"),
                                   _opt(bo, f32, "bo"), B, I, H, int(act), _dev(dz, f32, "dz"), _dev(dWo, f32, "dWo"),
                                   _dev(dbo, f32, "dbo"), _dev(partial_loss, f32, "partial_loss"),
                                   _dev(count, torch.int32, "count"), ws, ws_bytes, _stream()), "yr_cdae_owned_decode")


def cdae_owned_hidden_bwd(rows: "SparseRows", dz, z, act, user, count, dV, touched_users, dbh, dWhT, touched_items,
                          partial_loss, n_partials, stats, loss_accum, workspace, scale_dz=False):
    """cdae_hidden_bwd_dwh_t with every sum by the owner of its destination in ascending row order
    (yr_cdae_owned_hidden_bwd): ``dbh``, the ``dV`` rows of the batch's users and the ``dWhT`` rows of its input items
    are stored, not added to."""
    lib = _lib.load()
    f32 = torch.float32
    if dz.dim() != 2 or z.shape != dz.shape or dV.dim() != 2 or dV.shape[1] != dz.shape[1]:
        raise EngineError("cdae_owned_hidden_bwd: dz and z [B, H], dV [users, H] expected")
    B, H = dz.shape
    if rows.B != B or user.numel() != B or dbh.numel() != H or dWhT.shape != (rows.I, H) or touched_items.numel() != rows.I:
        raise EngineError("cdae_owned_hidden_bwd: rows, user [B], dbh [H], dWhT [I, H] and touched_items [I] must agree")
    if count.numel() != COUNT_WORDS:
        raise EngineError(f"count: a spread count of {COUNT_WORDS} int32 words")
    ws, ws_bytes = _owned_workspace(workspace, B, rows.I, H, "cdae_owned_hidden_bwd")
    check(lib.yr_cdae_owned_hidden_bwd(_dev(rows.cols, torch.int32, "cols"), _dev(rows.vals, f32, "vals"),
                                       _dev(rows.count, torch.int32, "count"),
                                       _dev(dz, f32, "dz"), _dev(z, f32, "z"), int(act), 1 if scale_dz else 0,
                                       _dev(count, torch.int32, "count"), _dev(user, torch.int64, "user"), B,
                                       rows.I, H, dV.shape[0], _dev(dV, f32, "dV"),
                                       _opt(touched_users, torch.uint8, "touched_users"), _dev(dbh, f32, "dbh"),
                                       _dev(dWhT, f32, "dWhT"), _dev(touched_items, torch.uint8, "touched_items"),
                                       _opt(partial_loss, f32, "partial_loss"), int(n_partials),
                                       _opt(stats, f32, "stats"), _opt(loss_accum, torch.float64, "loss_accum"),
                                       ws, ws_bytes, _stream()), "yr_cdae_owned_hidden_bwd")


_dwh_scratch = {}


def cdae_sparse_dwh(rows: "SparseRows", dz, dWh):
    """dWh (zero on entry) = dz^T . rows (dWh [H, I]); the transposed scratch and the column-claim words live per (device, I, H)."""
    lib = _lib.load()
    H = dz.shape[1]
    key = (dz.device, rows.I, H)
    sc = _dwh_scratch.get(key)
    if sc is None:
        dev = dz.device
        sc = _dwh_scratch[key] = [torch.zeros(rows.I, H, dtype=torch.float32, device=dev),
                                  torch.zeros(rows.I, dtype=torch.int32, device=dev),
                                  torch.empty(rows.I, dtype=torch.int32, device=dev),
                                  torch.zeros(1, dtype=torch.int32, device=dev), 0]
    sc[4] = sc[4] % 0x7ffffff0 + 1                       # a fresh non-zero epoch per call
    check(lib.yr_cdae_sparse_dwh(rows.cols.data_ptr(), rows.vals.data_ptr(), rows.count.data_ptr(),
                                 _dev(dz, torch.float32, "dz"), rows.B, rows.I, H, _dev(dWh, torch.float32, "dWh"),
                                 sc[0].data_ptr(), sc[1].data_ptr(), sc[4], sc[2].data_ptr(), sc[3].data_ptr(),
                                 _stream()), "yr_cdae_sparse_dwh")
    return dWh


def sigmoid_(x):
    lib = _lib.load()
    check(lib.yr_sigmoid(_dev(x, torch.float32, "x"), x.numel(), _stream()), "yr_sigmoid")
    return x


def sigmoid_bwd(dy, y, out=None):
    """dy * y * (1 - y); ``out`` may be ``dy`` itself (in place) or omitted (new tensor)."""
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(dy)
    check(lib.yr_sigmoid_bwd(_dev(dy, torch.float32, "dy"), _dev(y, torch.float32, "y"), _dev(out, torch.float32, "g"),
                             dy.numel(), _stream()), "yr_sigmoid_bwd")
    return out


def sigmoid_bwd_(g, y):
    return sigmoid_bwd(g, y, out=g)


def dropout_seeded(x, seed, p):
    """nn.Dropout(p) in training mode with the mask drawn inside the kernel from (seed, position)."""
    lib = _lib.load()
    out = torch.empty_like(x)
    check(lib.yr_dropout_seeded(_dev(x, torch.float32, "x"), int(seed) & 0xFFFFFFFFFFFFFFFF, float(p), x.numel(),
                                out.data_ptr(), _stream()), "yr_dropout_seeded")
    return out


def colsum(X, out=None, accumulate=False):
    lib = _lib.load()
    rows, cols = X.shape
    if out is None:
        out = torch.empty(cols, dtype=torch.float32, device=X.device)
    check(lib.yr_colsum(_dev(X, torch.float32, "X"), rows, cols, _dev(out, torch.float32, "out"),
                        1 if accumulate else 0, _stream()), "yr_colsum")
    return out


def row_scatter_add(G, user, dV):
    lib = _lib.load()
    check(lib.yr_row_scatter_add(_dev(G, torch.float32, "G"), _dev(user, torch.int64, "user"), G.shape[0],
                                 G.shape[1], dV.shape[0], _dev(dV, torch.float32, "dV"), _stream()),
          "yr_row_scatter_add")


def nsbce_fwd(pred, target, negative_mask):
    """(stats, workspace): stats[0] = mean BCE over nonzero(target + negative_mask), stats[1] = count."""
    lib = _lib.load()
    f32 = torch.float32
    ws = torch.empty(2 * LOSS_PARTIALS, dtype=f32, device=pred.device)
    stats = torch.empty(2, dtype=f32, device=pred.device)
    check(lib.yr_nsbce_fwd(_dev(pred, f32, "pred"), _dev(target, f32, "target"), _opt(negative_mask, f32, "neg"),
                           pred.numel(), ws.data_ptr(), stats.data_ptr(), _stream()), "yr_nsbce_fwd")
    return stats


def nsbce_bwd(pred, target, negative_mask, stats, gout):
    lib = _lib.load()
    f32 = torch.float32
    dpred = torch.empty_like(pred)
    check(lib.yr_nsbce_bwd(_dev(pred, f32, "pred"), _dev(target, f32, "target"), _opt(negative_mask, f32, "neg"),
                           _dev(stats, f32, "stats"), _dev(gout, f32, "gout"), pred.numel(), dpred.data_ptr(),
                           _stream()), "yr_nsbce_bwd")
    return dpred


def loss_finalize(loss_partials, scale, loss_out=None, loss_accum=None):
    """loss_out[0] = scale * sum(partials); loss_accum[0] (float64) += the same."""
    lib = _lib.load()
    if loss_out is None:
        loss_out = torch.empty(1, dtype=torch.float32, device=loss_partials.device)
    check(lib.yr_loss_finalize(_dev(loss_partials, torch.float32, "loss_partials"), float(scale),
                               _dev(loss_out, torch.float32, "loss_out"),
                               _opt(loss_accum, torch.float64, "loss_accum"), _stream()), "yr_loss_finalize")
    return loss_out


MASK_VALUE = -3.40282e+38     # reference trainers/mf_trainer.py:167


def topk_masked(scores, mask_ptr, mask_idx, k, mask_value=MASK_VALUE, out=None, mask_rows=None):
    """Row-wise top-k of ``scores[R, N]`` with per-row masked columns (CSR) forced to
    ``mask_value`` first (reference trainers/mf_trainer.py:163-178).  -> int64 [R, k].
    ``mask_rows`` [R]: row r's mask list is CSR row ``mask_rows[r]`` (a batch of users pointing into one
    per-user CSR) instead of row r."""
    lib = _lib.load()
    if scores.dim() != 2 or scores.stride(1) != 1:
        raise EngineError("scores must be [rows, cols] with unit column stride")
    if not scores.is_cuda or scores.dtype != torch.float32:
        raise EngineError("scores must be a float32 GPU tensor (no CPU fallback)")
    R, N = scores.shape
    if out is None:
        out = torch.empty((R, k), dtype=torch.int64, device=scores.device)
    if mask_ptr is not None and mask_rows is None and mask_ptr.numel() != R + 1:
        raise EngineError("mask_ptr must have rows + 1 entries")
    if mask_idx is not None and mask_idx.numel() == 0:
        mask_ptr = mask_idx = mask_rows = None             # every list empty: an empty tensor has no address to pass
    if mask_rows is not None and mask_rows.numel() != R:
        raise EngineError("mask_rows must have one entry per row")
    check(lib.yr_topk_masked(scores.data_ptr(), R, N, scores.stride(0) if R > 1 else N,
                             _opt(mask_ptr, torch.int64, "mask_ptr"), _opt(mask_idx, torch.int64, "mask_idx"),
                             _opt(mask_rows, torch.int64, "mask_rows"),
                             float(mask_value), int(k), _dev(out, torch.int64, "out"), _stream()),
          "yr_topk_masked")
    return out


def mf_scores_gemm(U, I, users, out=None, err_flag=None):
    """scores[r, j] = U[users[r]] . I[j] for every item j — the reference's per-user
    ``model([u]*I, arange(I))`` (trainers/mf_trainer.py:138-140) as one f32 MFMA GEMM."""
    lib = _lib.load()
    nu, ni, d = _table_dims(U, I)
    n = users.numel()
    if out is None:
        out = torch.empty((n, ni), dtype=torch.float32, device=U.device)
    if out.dim() != 2 or out.shape[0] < n or out.shape[1] < ni or out.stride(1) != 1:
        raise EngineError("scores buffer must be [>= rows, >= num_items] with unit column stride")
    check(lib.yr_mf_scores_gemm(_dev(U, torch.float32, "U"), _dev(I, torch.float32, "I"),
                                _dev(users, torch.int64, "users"), n, d, nu, ni, out.data_ptr(), out.stride(0),
                                _opt(err_flag, torch.int32, "err_flag"), _stream()), "yr_mf_scores_gemm")
    return out[:n]


def sort_mask_rows(mask_ptr, mask_idx):
    """Mask lists with the item ids ascending inside each row (index bookkeeping, done once per
    eval set): what :func:`mf_eval_topk` requires."""
    n = mask_ptr.numel() - 1
    if mask_idx.numel() == 0:
        return mask_idx
    rows = torch.repeat_interleave(torch.arange(n, device=mask_idx.device), mask_ptr[1:] - mask_ptr[:-1])
    span = int(mask_idx.max().item()) + 1
    order = torch.argsort(rows * span + mask_idx)
    return mask_idx[order].contiguous()


def fused_eval_supports(k, d):
    """The fused evaluation kernel keeps top-k lists of 4 / 10 / 16 / 32 entries in registers (32: up to D = 64;
    the wide widths 256 / 512 / 1024 like D = 128: k <= 16)."""
    return k <= 16 or (k <= 32 and d <= 64)


EVAL_MODES = {"f32": DEFINES["YR_EVAL_F32"], "bf16x3": DEFINES["YR_EVAL_BF16X3"]}
EVAL_FORMS = {None: 0, "two_roles": DEFINES["YR_EVAL_TWO_ROLES"], "four_waves": DEFINES["YR_EVAL_FOUR_WAVES"]}


def mf_eval_topk(U, I, users, mask_ptr, mask_idx_sorted, k, mask_value=MASK_VALUE, out=None, sliced=True,
                 item_bias=None, precision="bf16x3", prescan=None, hint=None, form=None):
    """Fused full-catalogue scoring + mask + top-k (no score matrix).  ``mask_idx_sorted``: CSR mask
    lists with ascending ids inside each row (see :func:`sort_mask_rows`).  ``sliced=False`` withholds
    the room for the partial lists, i.e. forces the one-slice form of the kernel (tests).  ``item_bias``: scores
    U[u] . I[j] + item_bias[j] (the CDAE decoder before its sigmoid).  ``precision``: "bf16x3" — f32 scores from
    three-term bfloat16 splits of both operands on the bf16 matrix instructions (six partial products, error below
    the f32 rounding of a product) — or "f32", the f32 matrix instruction itself.  ``prescan``: None = the
    library's rule (catalogues of 16,384 items and more), False / True = never / always run the sampling launch that
    gives the lists their starting thresholds (same result either way; ``sliced=False`` implies False).
    ``hint``: int64 [n, k] item ids, e.g. the result of the previous evaluation of the same rows (may be ``out``
    itself): the lists start from the smallest score among a row's k hint items, which the row's k-th best score
    cannot be below — the result does not depend on it, a good hint saves most candidate insertions and the
    prescan launch.  ``form``: None = the library's rule (from 2,048 rows the two-role sweep at D = 128, and at D = 64
    for k > 10 when a hint gives the thresholds; the four-wave sweep otherwise), "two_roles" / "four_waves" = that form where both exist (YR_EVAL_TWO_ROLES / YR_EVAL_FOUR_WAVES:
    same lists; tests and comparisons)."""
    lib = _lib.load()
    nu, ni, d = _table_dims(U, I)
    n = users.numel()
    if mask_idx_sorted is not None and mask_idx_sorted.numel() == 0:
        mask_ptr = mask_idx_sorted = None              # every list empty: an empty tensor has no address to pass
    mode = EVAL_MODES[precision]
    planes_only = query_size("yr_mf_eval_topk_planes_bytes", ni, d) if mode else 0
    if prescan is False or not sliced:
        mode |= DEFINES["YR_EVAL_NO_PRESCAN"]
    elif prescan:
        mode |= DEFINES["YR_EVAL_FORCE_PRESCAN"]
    mode |= EVAL_FORMS[form]
    if out is None:
        out = torch.empty((n, k), dtype=torch.int64, device=U.device)
    if hint is not None and tuple(hint.shape) != (n, k):
        raise EngineError(f"hint must be [{n}, {k}] item ids, got {tuple(hint.shape)}")
    flag = new_error_flag(U.device)
    if sliced:
        ws_bytes = query_size("yr_mf_eval_topk_workspace_bytes", n, ni, d, k, mode)
    else:
        ws_bytes = planes_only + (-(-n * 4 // 256) * 256 if hint is not None else 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=U.device) if ws_bytes else None
    check(lib.yr_mf_eval_topk_bias(_dev(U, torch.float32, "U"), _dev(I, torch.float32, "I"),
                              _opt(item_bias, torch.float32, "item_bias"),
                              _dev(users, torch.int64, "users"), n, d, nu, ni,
                              _opt(mask_ptr, torch.int64, "mask_ptr"), _opt(mask_idx_sorted, torch.int64, "mask_idx"),
                              float(mask_value), int(k), _dev(out, torch.int64, "out"),
                              ws.data_ptr() if ws is not None else None, ws_bytes, mode,
                              _opt(hint, torch.int64, "hint"), flag.data_ptr(), _stream()),
          "yr_mf_eval_topk")
    raise_on_flag(flag, "mf_eval_topk")
    return out


def ngcf_eval_supports(k):
    """The layered sweep (:func:`ngcf_eval_topk`) keeps lists of 4 / 10 / 16 entries in registers."""
    return k <= 16


def ngcf_eval_topk(layers, num_users, users, mask_ptr, mask_idx_sorted, k, mask_value=MASK_VALUE, out=None,
                   sliced=True, hint=None):
    """:func:`mf_eval_topk` for NGCF's score, the sum over the layer buffers of per-layer dot products (reference
    models/ngcf.py:44-58 against the whole catalogue): ``layers`` = the K + 1 outputs of ``NGCF.propagate``, each
    [num_users + num_items, D] with the users first.  One f32 accumulator per score over all (K + 1) D products on
    the f32 matrix instruction; the layers are not concatenated and no score matrix is written.  ``mask_idx_sorted``,
    ``sliced`` and ``hint`` as in :func:`mf_eval_topk`; k <= 16 (:func:`ngcf_eval_supports`)."""
    lib = _lib.load()
    ptrs = _ptr_array(layers, "layers")
    n_all, d = layers[0].shape
    if any(tuple(E.shape) != (n_all, d) for E in layers):
        raise EngineError("layers must all be [num_users + num_items, D]")
    ni = n_all - num_users
    n = users.numel()
    if mask_idx_sorted is not None and mask_idx_sorted.numel() == 0:
        mask_ptr = mask_idx_sorted = None              # every list empty: an empty tensor has no address to pass
    dev = layers[0].device
    if out is None:
        out = torch.empty((n, k), dtype=torch.int64, device=dev)
    if hint is not None and tuple(hint.shape) != (n, k):
        raise EngineError(f"hint must be [{n}, {k}] item ids, got {tuple(hint.shape)}")
    flag = new_error_flag(dev)
    if sliced:
        ws_bytes = query_size("yr_ngcf_eval_topk_workspace_bytes", n, ni, len(layers), d, k)
    else:
        ws_bytes = -(-n * 4 // 256) * 256 if hint is not None else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    check(lib.yr_ngcf_eval_topk(ptrs, len(layers), d, _dev(users, torch.int64, "users"), n,
                                int(num_users), ni, _opt(mask_ptr, torch.int64, "mask_ptr"),
                                _opt(mask_idx_sorted, torch.int64, "mask_idx"), float(mask_value), int(k),
                                _dev(out, torch.int64, "out"), ws.data_ptr() if ws is not None else None, ws_bytes,
                                _opt(hint, torch.int64, "hint"), flag.data_ptr(), _stream()),
          "yr_ngcf_eval_topk")
    raise_on_flag(flag, "ngcf_eval_topk")
    return out


def mf_recommend(U, I, users, mask_ptr, mask_idx, k, chunk_users=4096, fused=None):
    """Top-k unmasked items for each user id in ``users`` (reference
    trainers/mf_trainer.py:134-144 + :163-178, batched), all on the device.
    ``fused`` (default when k <= 16, or k <= 32 with D <= 64): one kernel, scores on the matrix cores with mask + top-k in the
    epilogue.  Otherwise: score GEMM into a chunked buffer + the row-wise masked top-k kernel."""
    nu_tab, ni, d = _table_dims(U, I)
    n = users.numel()
    if fused is None:
        fused = fused_eval_supports(k, d)
    if fused:
        return mf_eval_topk(U, I, users.contiguous(), mask_ptr, sort_mask_rows(mask_ptr, mask_idx), k)
    out = torch.empty((n, k), dtype=torch.int64, device=U.device)
    flag = new_error_flag(U.device)
    chunk_users = max(1, min(chunk_users, n))
    scores = torch.empty((chunk_users, ni), dtype=torch.float32, device=U.device)
    ptr_host = mask_ptr.cpu()
    for lo in range(0, n, chunk_users):
        hi = min(lo + chunk_users, n)
        mf_scores_gemm(U, I, users[lo:hi].contiguous(), out=scores, err_flag=flag)
        ptr = (mask_ptr[lo:hi + 1] - mask_ptr[lo]).contiguous()
        topk_masked(scores[:hi - lo], ptr, mask_idx[int(ptr_host[lo]):], k, out=out[lo:hi])
    raise_on_flag(flag, "mf_recommend")
    return out


def csr_rows_to_dense(ptr, idx, users, num_items, out=None, accumulate=False, err_flag=None):
    """[len(users), num_items] float32 0/1 rows from a per-user item CSR (device-side counterpart of
    the dense masks of reference cdae_data_pipeline.py:33-37)."""
    lib = _lib.load()
    B = users.numel()
    if out is None:
        if accumulate:
            raise EngineError("accumulate needs an output buffer")
        out = torch.empty((B, num_items), dtype=torch.float32, device=users.device)
    i64 = torch.int64
    ii = idx if idx.numel() else torch.zeros(1, dtype=i64, device=users.device)
    check(lib.yr_csr_rows_to_dense(_dev(ptr, i64, "ptr"), _dev(ii, i64, "idx"), _dev(users, i64, "users"), B,
                                   ptr.numel() - 1, int(num_items), 1 if accumulate else 0,
                                   _dev(out, torch.float32, "out"),
                                   err_flag.data_ptr() if err_flag is not None else None, _stream()),
          "yr_csr_rows_to_dense")
    return out


def negative_mask(positives, neg_times, seed, err_flag=None):
    """Exactly ``neg_times * positives`` distinct non-positive items per row, uniformly at random
    (reference cdae_dataset.py:20-34); ``err_flag`` gets FLAG_BAD_ITEM if a row has too few
    non-positives (where np.random.choice raises)."""
    lib = _lib.load()
    B, I = positives.shape
    out = torch.empty_like(positives)
    check(lib.yr_negative_mask(_dev(positives, torch.float32, "positives"), B, I, int(neg_times),
                               int(seed) & 0xFFFFFFFFFFFFFFFF, out.data_ptr(),
                               err_flag.data_ptr() if err_flag is not None else None, _stream()), "yr_negative_mask")
    return out


def rank_metrics(topk, pos_ptr, pos_idx, pos_rows=None):
    """(precision, recall, map, ndcg)@k of reference metric.py computed on the device from the top-k
    lists ``topk [n, k]`` and the held-out items (CSR, original order).  Returns a float64[10] device
    tensor: the four metrics, the number of users with a non-empty list, then the four un-normalised
    sums and n (for a cross-rank reduction); one host sync to read it."""
    lib = _lib.load()
    n, k = topk.shape
    if pos_rows is None and pos_ptr.numel() != n + 1:
        raise EngineError("pos_ptr must have rows + 1 entries")
    if pos_rows is not None and pos_rows.numel() != n:
        raise EngineError("pos_rows must have one entry per row")
    ws = torch.empty(query_size("yr_rank_metrics_workspace_bytes", n) // 8, dtype=torch.float64, device=topk.device)
    out = torch.empty(10, dtype=torch.float64, device=topk.device)
    idx = pos_idx if pos_idx.numel() else torch.zeros(1, dtype=torch.int64, device=topk.device)
    check(lib.yr_rank_metrics(_dev(topk, torch.int64, "topk"), n, k, _dev(pos_ptr, torch.int64, "pos_ptr"),
                              _dev(idx, torch.int64, "pos_idx"), _opt(pos_rows, torch.int64, "pos_rows"),
                              ws.data_ptr(), out.data_ptr(), _stream()),
          "yr_rank_metrics")
    return out


# ---- ranks of every held-out item against the catalogue (csrc/catalogue_rank.hip) and the metrics at any cutoff ----
CATALOGUE_RANK_CAP = DEFINES["YR_CATALOGUE_RANK_CAP"]     # targets per slot of the rank sweep
SWEEP_TILE = 32              # csrc/s3rec_cb.h kSweepTile: rows (slots) per row tile, items per swept tile
SWEEP_COL_CHUNK = 2048       # csrc/s3rec_cb.h kSweepColChunk: items per workgroup of the catalogue sweeps
SWEEP_GRID_MAX = 2048        # csrc/s3rec_cb.h kSweepGridMax: workgroups per launch, the kernels loop from there
METRICS_PER_K = DEFINES["YR_METRICS_PER_K"]
METRICS_MAX_KS = DEFINES["YR_METRICS_MAX_KS"]


def catalogue_rank_slots(pos_lengths):
    """Slots the rank sweep cuts rows with these target counts into (ceil(len / CATALOGUE_RANK_CAP) each)."""
    return sum(-(-int(n) // CATALOGUE_RANK_CAP) for n in pos_lengths)


def catalogue_ranks(layers_user, layers_item, users, pos_ptr, pos_idx, mask_ptr, mask_idx_sorted, want_score=False,
                    err_flag=None, out=None, score_out=None):
    """rank [nnz] int64 of yr_catalogue_ranks, aligned with ``pos_idx``: the 0-based place of every held-out item
    of row n (``pos_ptr`` / ``pos_idx``, original order) in the row's full prediction — the unmasked items by score
    descending then id ascending, then the masked ones (``mask_ptr`` / ``mask_idx_sorted``, ids ascending inside a
    row; both None: no mask) by id — what the reference's evaluation (trainers/mf_trainer.py:134-178, metric.py)
    compares with ``actual``, for every cutoff at once.  Scores: the sum over the pairs
    ``(layers_user[l] [num_users, D], layers_item[l] [num_items, D])`` of the dot products, one f32 accumulator, layers
    ascending.  MF passes ``[U], [I]``; NGCF ``[E_l[:num_users]], [E_l[num_users:]]``.  -1 for a refused id
    (``err_flag`` given: the bits are left there; else an IndexError).  ``want_score``: (rank, score [nnz] f32).
    ``out`` / ``score_out``: the [nnz] buffers to write (exactly nnz entries are written)."""
    lib = _lib.load()
    f32, i64 = torch.float32, torch.int64
    if len(layers_user) != len(layers_item):
        raise EngineError("catalogue_ranks: one item-side table per user-side table")
    pu, pi = _ptr_array(layers_user, "layers_user"), _ptr_array(layers_item, "layers_item")
    nu, d = layers_user[0].shape
    ni = layers_item[0].shape[0]
    if any(tuple(t.shape) != (nu, d) for t in layers_user) or any(tuple(t.shape) != (ni, d) for t in layers_item):
        raise EngineError("catalogue_ranks: tables must be [num_users, D] / [num_items, D] in every layer")
    n, nnz = users.numel(), pos_idx.numel()
    if pos_ptr.numel() != n + 1 or (mask_ptr is not None and mask_ptr.numel() != n + 1):
        raise EngineError("catalogue_ranks: pos_ptr and mask_ptr hold rows + 1 entries")
    if (mask_ptr is None) != (mask_idx_sorted is None):
        raise EngineError("catalogue_ranks: mask_ptr and mask_idx come together")
    if mask_idx_sorted is not None and mask_idx_sorted.numel() == 0:
        mask_ptr = mask_idx_sorted = None              # every list empty: an empty tensor has no address to pass
    dev = layers_user[0].device
    ws_bytes = query_size("yr_catalogue_ranks_workspace_bytes", n, nnz, ni, len(layers_user), d)
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    rank = out if out is not None else torch.empty(nnz, dtype=i64, device=dev)
    want_score = want_score or score_out is not None
    score = score_out if score_out is not None else (torch.empty(nnz, dtype=f32, device=dev) if want_score else None)
    if rank.numel() != nnz or (score is not None and score.numel() != nnz):
        raise EngineError("catalogue_ranks: the output buffers hold one entry per entry of pos_idx")
    flag = err_flag if err_flag is not None else new_error_flag(dev)
    check(lib.yr_catalogue_ranks(pu, pi, len(layers_user), d, _dev(users, i64, "users"), n, nu, ni,
                                 _dev(pos_ptr, i64, "pos_ptr"), _dev(pos_idx, i64, "pos_idx") if nnz else None, nnz,
                                 _opt(mask_ptr, i64, "mask_ptr"), _opt(mask_idx_sorted, i64, "mask_idx"),
                                 _dev(rank, i64, "rank") if nnz else None,
                                 _dev(score, f32, "score") if want_score and nnz else None,
                                 ws.data_ptr(), ws_bytes, _dev(flag, torch.int32, "err_flag"), _stream()),
          "yr_catalogue_ranks")
    if err_flag is None:
        raise_on_flag(flag, "catalogue_ranks")
    return (rank, score) if want_score else rank


class RankMetrics(dict):
    """``{k: (precision, recall, map, ndcg, hr)}`` with ``mrr`` and ``auc`` (also under those keys), ``raw`` the
    float64 tensor of yr_metrics_from_ranks and ``ten(k)`` the ten-vector :func:`rank_metrics` returns at k."""

    def ten(self, k):
        i = self.ks.index(int(k))
        return self.raw[i * METRICS_PER_K:i * METRICS_PER_K + 10]


def metrics_from_ranks(rank, pos_ptr, ks, num_items=None, mask_ptr=None):
    """precision / recall / MAP / NDCG / HR @k for every k of ``ks`` (each >= 1, no upper limit), MRR and AUC from the
    ranks of the held-out items (:func:`catalogue_ranks`; ``pos_ptr`` [n + 1] the rows of ``rank``), with the quirks
    of reference metric.py that :func:`rank_metrics` reproduces.  Definitions beyond the reference's four:
    HR@k = the share of users with a non-empty list that have a hit among the first k; MRR = the mean over those users
    of 1 / (their best rank + 1); AUC = the mean, over the users that have at least one (target, unmasked non-target)
    pair, of the share of such pairs with the target ahead in the list order (ties by id; a masked target is behind
    every non-target) — it needs ``num_items`` and the ``mask_ptr`` the ranks were taken under, and is NaN without.
    -> :class:`RankMetrics`; one host sync."""
    lib = _lib.load()
    i64 = torch.int64
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= METRICS_MAX_KS or any(k < 1 for k in ks):
        raise EngineError(f"metrics_from_ranks: 1 to {METRICS_MAX_KS} cutoffs, each at least 1")
    n = pos_ptr.numel() - 1
    dev = pos_ptr.device
    if mask_ptr is not None and mask_ptr.numel() != n + 1:
        raise EngineError("metrics_from_ranks: mask_ptr must have rows + 1 entries")
    ws = torch.empty(query_size("yr_metrics_from_ranks_workspace_bytes", n, len(ks)) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(len(ks) * METRICS_PER_K + 6, dtype=torch.float64, device=dev)
    kt = torch.tensor(ks, dtype=i64, device=dev)
    check(lib.yr_metrics_from_ranks(_dev(rank, i64, "rank") if rank.numel() else None, n, _dev(pos_ptr, i64, "pos_ptr"),
                                    kt.data_ptr(), len(ks), -1 if num_items is None else int(num_items),
                                    _opt(mask_ptr, i64, "mask_ptr"), ws.data_ptr(), out.data_ptr(), _stream()),
          "yr_metrics_from_ranks")
    host = out.tolist()
    res = RankMetrics()
    res.raw, res.ks = out, ks
    for i, k in enumerate(ks):
        v = host[i * METRICS_PER_K:(i + 1) * METRICS_PER_K]
        res[k] = (v[0], v[1], v[2], v[3], v[10])
    res.mrr = res["mrr"] = host[len(ks) * METRICS_PER_K]
    res.auc = res["auc"] = host[len(ks) * METRICS_PER_K + 1]
    return res


def bpr_loss_fwd(pos, neg, loss_partials):
    """Partial sums of softplus(-(pos - neg))  (reference loss.py:25-27)."""
    lib = _lib.load()
    B = pos.numel()
    if neg.numel() != B:
        raise EngineError("pos and neg differ in length")
    check(lib.yr_bpr_loss_fwd(_dev(pos, torch.float32, "pos"), _dev(neg, torch.float32, "neg"), B,
                              _dev(loss_partials, torch.float32, "loss_partials"), _stream()), "yr_bpr_loss_fwd")


def bpr_loss_bwd(pos, neg, gout, gpos, gneg):
    """d mean(-logsigmoid(pos-neg)) / d pos, d neg, scaled by the scalar gout."""
    lib = _lib.load()
    B = pos.numel()
    check(lib.yr_bpr_loss_bwd(_dev(pos, torch.float32, "pos"), _dev(neg, torch.float32, "neg"),
                              _dev(gout, torch.float32, "gout"), 1.0 / B if B else 0.0, B,
                              _dev(gpos, torch.float32, "gpos"), _dev(gneg, torch.float32, "gneg"), _stream()),
          "yr_bpr_loss_bwd")


def adam_scalars(step: int, lr: float, beta1: float, beta2: float):
    """Host doubles of torch's Adam step: (lr / (1 - b1^t), sqrt(1 - b2^t))."""
    return lr / (1.0 - beta1 ** step), (1.0 - beta2 ** step) ** 0.5


def adam_dense(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
               decoupled=False, zero_grad=False):
    """Dense Adam/AdamW step in place (reference trainers/base_trainer.py:34-38)."""
    lib = _lib.load()
    n = p.numel()
    if g.numel() != n or m.numel() != n or v.numel() != n:
        raise EngineError("p/g/m/v sizes differ")
    step_size, bc2_sqrt = adam_scalars(step, lr, beta1, beta2)
    check(lib.yr_adam_dense(_dev(p, torch.float32, "p"), _dev(g, torch.float32, "g"),
                            _dev(m, torch.float32, "m"), _dev(v, torch.float32, "v"), n,
                            float(lr), float(step_size), float(bc2_sqrt), float(beta1), float(beta2),
                            float(eps), float(weight_decay), OPT_ADAMW if decoupled else OPT_ADAM,
                            1 if zero_grad else 0, _stream()), "yr_adam_dense")


ADAM_MULTI_MAX = DEFINES["YR_ADAM_MULTI_MAX"]


def adam_dense_flat(tensors, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False,
                    grad_count=None):
    """One launch, 16 bytes per lane, for up to ADAM_MULTI_MAX tensors of any size (yr_adam_dense_flat).
    ``tensors``: (p, g, m, v, touched, clear[, scaled]) — ``touched`` a uint8 mark per row of p (or None),
    ``clear`` 1 / True: the gradient is zeroed after it is read, 2: only where it is non-zero, ``scaled`` whether it is first multiplied by
    1 / ``grad_count`` (a spread int32 count on the device)."""
    import ctypes
    lib = _lib.load()
    if len(tensors) > ADAM_MULTI_MAX:
        raise EngineError(f"at most {ADAM_MULTI_MAX} tensors per launch")
    step_size, bc2_sqrt = adam_scalars(step, lr, beta1, beta2)
    f32 = torch.float32
    n = len(tensors)
    cols = [(ctypes.c_void_p * n)(*[_dev(t[k], f32, name) for t in tensors]) for k, name in enumerate("pgmv")]
    for t in tensors:
        if not (t[0].numel() == t[1].numel() == t[2].numel() == t[3].numel()):
            raise EngineError("p/g/m/v sizes differ")
    counts = (ctypes.c_int64 * n)(*[t[0].numel() for t in tensors])
    marks = (ctypes.c_void_p * n)(*[_opt(t[4], torch.uint8, "touched") for t in tensors])
    widths = (ctypes.c_int * n)(*[int(t[0].shape[-1]) if t[4] is not None else 0 for t in tensors])
    clear = (ctypes.c_int * n)(*[int(t[5]) for t in tensors])
    scaled = (ctypes.c_int * n)(*[1 if len(t) > 6 and t[6] else 0 for t in tensors])
    if grad_count is not None and grad_count.numel() != COUNT_WORDS:
        raise EngineError(f"grad_count: a spread count of {COUNT_WORDS} int32 words")
    check(lib.yr_adam_dense_flat(cols[0], cols[1], cols[2], cols[3], counts, marks, widths, clear, scaled,
                                 _opt(grad_count, torch.int32, "grad_count"), n, float(lr),
                                 float(step_size), float(bc2_sqrt), float(beta1), float(beta2), float(eps),
                                 float(weight_decay), OPT_ADAMW if decoupled else OPT_ADAM, _stream()),
          "yr_adam_dense_flat")


def sgd_dense(p, g, lr, weight_decay=0.0, zero_grad=False):
    """Dense SGD step in place (reference trainers/base_trainer.py:39-40)."""
    lib = _lib.load()
    n = p.numel()
    check(lib.yr_sgd_dense(_dev(p, torch.float32, "p"), _dev(g, torch.float32, "g"), n,
                           float(lr), float(weight_decay), 1 if zero_grad else 0, _stream()), "yr_sgd_dense")


# ---------------------------------------------------------------------------------------------- DCN
DCN_MAX_F, DCN_MAX_H, DCN_MAX_L = 512, 1024, 8          # csrc/dcn.hip kDcnMaxF / kDcnMaxH / kDcnMaxL


def _dcn_attr_args(attrs):
    """(cat_ids, sc_ids, Lmax) arguments of yr_dcn_assemble / _bwd.  attrs: (cat_ids int32 [rows, Lmax],
    sc_ids int32 [rows], num_cats, num_sc)."""
    cat_ids, sc_ids = attrs[0], attrs[1]
    return [_dev(cat_ids, torch.int32, "cat_ids"), _dev(sc_ids, torch.int32, "sc_ids"), int(cat_ids.shape[1])]


def dcn_assemble(U, I, C, S, attrs, user, item_a, item_b=None, attr_per_row=False, out=None, err_flag=None):
    """x0 rows [U[user] | I[item] | mean C[cats] | S[sc]] (B rows; 2B with item_b: pos rows then neg rows).
    ``user=None``: the item-only rows (3 D wide); ``item_a=None``: item = row (x_item of the whole catalogue)."""
    lib = _lib.load()
    cat_ids, sc_ids, num_cats, num_sc = attrs
    D = I.shape[1]
    B = item_a.numel() if item_a is not None else (I.shape[0] if not attr_per_row else cat_ids.shape[0])
    rows = 2 * B if item_b is not None else B
    width = (4 if user is not None else 3) * D
    if out is None:
        out = torch.empty((rows, width), dtype=torch.float32, device=I.device)
    if out.shape[0] < rows or out.shape[1] != width or out.stride(1) != 1:
        raise EngineError("dcn_assemble: bad output buffer")
    nu = U.shape[0] if U is not None else 0
    check(lib.yr_dcn_assemble(_opt(U, torch.float32, "U"), _dev(I, torch.float32, "I"), _dev(C, torch.float32, "C"),
                              _dev(S, torch.float32, "S"), *_dcn_attr_args(attrs),
                              D, nu, I.shape[0], int(num_cats), int(num_sc), _opt(user, torch.int64, "user"),
                              _opt(item_a, torch.int64, "item_a"), _opt(item_b, torch.int64, "item_b"), B,
                              1 if attr_per_row else 0, out.data_ptr(), out.stride(0), _opt(err_flag, torch.int32, "flag"),
                              _stream()), "yr_dcn_assemble")
    return out


DCN_OWNED_CHUNK = DEFINES["YR_DCN_OWNED_CHUNK"]        # entries per chunk of an inverted attribute list


class DCNAttrLists:
    """The item -> attribute table inverted for the ordered scatter (yr_dcn_owned_assemble_bwd): per category its items
    in ascending order, each with the number of its slots that name the category (``cat_ptr`` [num_cats + 1],
    ``cat_item``, ``cat_mult``), the same per state-city (``sc_ptr``, ``sc_item``), and the running chunk counts
    ``cat_chunk_ptr`` / ``sc_chunk_ptr`` [rows + 1] of lists cut into chunks of DCN_OWNED_CHUNK entries.  int32 tensors;
    slots and state-cities out of range are in no list."""
    FIELDS = ("cat_ptr", "cat_item", "cat_mult", "cat_chunk_ptr", "sc_ptr", "sc_item", "sc_chunk_ptr")

    def __init__(self, cat_ids, sc_ids, num_cats, num_sc, device=None, chunk=DCN_OWNED_CHUNK):
        import numpy as np
        cat = cat_ids.detach().cpu().numpy().astype(np.int64).reshape(len(sc_ids), -1)
        sc = sc_ids.detach().cpu().numpy().astype(np.int64).reshape(-1)
        ni, lmax = cat.shape
        items = np.repeat(np.arange(ni, dtype=np.int64), lmax)
        flat = cat.reshape(-1)
        ok = (flat >= 0) & (flat < num_cats)
        # (category, item) pairs with their multiplicity, ascending by category then item
        pair, mult = np.unique(flat[ok] * ni + items[ok], return_counts=True)
        self.num_cats, self.num_sc, self.num_items, self.Lmax, self.chunk = int(num_cats), int(num_sc), ni, lmax, int(chunk)
        tables = {"cat_ptr": _list_ptr(pair // ni, num_cats), "cat_item": pair % ni, "cat_mult": mult}
        ok = (sc >= 0) & (sc < num_sc)
        it = np.flatnonzero(ok)
        order = np.argsort(sc[it], kind="stable")                        # items stay ascending inside a state-city
        tables.update(sc_ptr=_list_ptr(sc[it][order], num_sc), sc_item=it[order])
        for k in ("cat", "sc"):
            n = -(-np.diff(tables[k + "_ptr"]) // chunk)
            tables[k + "_chunk_ptr"] = np.concatenate([[0], np.cumsum(n)])
        self.cat_chunks, self.sc_chunks = int(tables["cat_chunk_ptr"][-1]), int(tables["sc_chunk_ptr"][-1])
        for k in self.FIELDS:
            t = torch.from_numpy(np.ascontiguousarray(tables[k]).astype(np.int32))
            if t.numel() == 0:
                t = torch.zeros(1, dtype=torch.int32)                    # never read: a list without entries
            setattr(self, k, t.to(device) if device is not None else t)


def _list_ptr(keys, rows):
    import numpy as np
    return np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=rows))])


def dcn_owned_head_workspace_bytes(units, F, H, L):
    """Bytes of scratch :func:`dcn_head` needs with ``deterministic=True`` and gradients (EngineError when refused)."""
    return query_size("yr_dcn_owned_head_workspace_bytes", units, F, H, L)


def dcn_owned_scatter_workspace_bytes(num_users, num_items, B, D, lists):
    """Bytes of scratch :func:`dcn_assemble_bwd` needs with ``deterministic=True`` for a batch of B triplets."""
    return query_size("yr_dcn_owned_scatter_workspace_bytes", num_users, num_items, B, D, lists.cat_chunks,
                      lists.sc_chunks)


def dcn_assemble_bwd(dx, attrs, user, item_a, item_b, gU, gI, gC, gS, num_users, attr_per_row=False, err_flag=None,
                     deterministic=False, lists=None, workspace=None):
    """Dense scatter-add of d x0 into the four table gradients (the category mean hands dx / Lmax to every slot).
    ``deterministic``: no float atomics (yr_dcn_owned_assemble_bwd, the triplet form only) — every touched row is its
    content on entry plus its contributions in the order of include/yelprec_engine.h; ``lists``: the
    :class:`DCNAttrLists` of ``attrs`` (built when None), ``workspace``: uint8 scratch of
    :func:`dcn_owned_scatter_workspace_bytes` (allocated when None)."""
    lib = _lib.load()
    cat_ids, sc_ids, num_cats, num_sc = attrs
    D = gI.shape[1]
    B = item_a.numel() if item_a is not None else dx.shape[0]
    if deterministic:
        if lists is None:
            lists = DCNAttrLists(cat_ids, sc_ids, num_cats, num_sc, device=gI.device)
        ws = _ngcf_scratch(workspace, dcn_owned_scatter_workspace_bytes(num_users, gI.shape[0], B, D, lists), gI.device,
                           "dcn_assemble_bwd")
        i32 = torch.int32
        check(lib.yr_dcn_owned_assemble_bwd(
            _rows(dx, torch.float32, "dx"), dx.stride(0), *_dcn_attr_args(attrs), D, int(num_users), gI.shape[0],
            int(num_cats), int(num_sc), _opt(user, torch.int64, "user"), _opt(item_a, torch.int64, "item_a"),
            _opt(item_b, torch.int64, "item_b"), B, 1 if attr_per_row else 0,
            _dev(lists.cat_ptr, i32, "cat_ptr"), _dev(lists.cat_item, i32, "cat_item"),
            _dev(lists.cat_mult, i32, "cat_mult"), _dev(lists.cat_chunk_ptr, i32, "cat_chunk_ptr"), lists.cat_chunks,
            _dev(lists.sc_ptr, i32, "sc_ptr"), _dev(lists.sc_item, i32, "sc_item"),
            _dev(lists.sc_chunk_ptr, i32, "sc_chunk_ptr"), lists.sc_chunks,
            _opt(gU, torch.float32, "gU"), _dev(gI, torch.float32, "gI"), _dev(gC, torch.float32, "gC"),
            _dev(gS, torch.float32, "gS"), ws.data_ptr(), ws.numel(), _opt(err_flag, torch.int32, "flag"), _stream()),
            "yr_dcn_owned_assemble_bwd")
        return
    check(lib.yr_dcn_assemble_bwd(_rows(dx, torch.float32, "dx"), dx.stride(0),
                                  *_dcn_attr_args(attrs), D, int(num_users),
                                  gI.shape[0], int(num_cats), int(num_sc), _opt(user, torch.int64, "user"),
                                  _opt(item_a, torch.int64, "item_a"), _opt(item_b, torch.int64, "item_b"), B,
                                  1 if attr_per_row else 0, _opt(gU, torch.float32, "gU"), _dev(gI, torch.float32, "gI"),
                                  _dev(gC, torch.float32, "gC"), _dev(gS, torch.float32, "gS"),
                                  _opt(err_flag, torch.int32, "flag"), _stream()), "yr_dcn_assemble_bwd")


def relu_bwd_(g, y):
    """g <- g * (y > 0) in place (y: the post-ReLU activation)."""
    lib = _lib.load()
    if g.shape != y.shape:
        raise EngineError("relu_bwd: shapes differ")
    check(lib.yr_relu_bwd(_dev(g, torch.float32, "g"), _dev(y, torch.float32, "y"), g.numel(), _stream()), "yr_relu_bwd")
    return g


def dcn_head(x0, h, cw, cb, Wo, bo, bpr, inv_batch=0.0, pred=None, gpred=None, grads=None, loss_partials=None,
             deterministic=False, workspace=None):
    """Cross network + output layer + sigmoid (+ BPR loss) over the rows of x0 / h (yr_dcn_head).
    ``bpr``: rows [0, B) and [B, 2B) are the pos / neg rows of B triplets.  ``grads``: (dh, dx0, dcw, dcb, dWo, dbo)
    — dh and dx0 are written, the weight gradients accumulated.  ``deterministic``: the weight gradients without float
    atomics, summed per wave, per workgroup and over the workgroups in a fixed order (yr_dcn_head_ordered; everything
    else comes out equal bit for bit); ``workspace``: uint8 scratch of :func:`dcn_owned_head_workspace_bytes`
    (allocated when None)."""
    lib = _lib.load()
    f32 = torch.float32
    rows, F = x0.shape
    H = h.shape[1]
    L = cw.shape[0]
    units = rows // 2 if bpr else rows
    if h.shape[0] != rows or cw.shape != (L, F) or cb.shape != (L, F) or Wo.numel() != H + F:
        raise EngineError("dcn_head: inconsistent shapes")
    dh = dx0 = dcw = dcb = dWo = dbo = None
    if grads is not None:
        dh, dx0, dcw, dcb, dWo, dbo = grads
    if deterministic:
        ws = None
        if grads is not None:
            ws = _ngcf_scratch(workspace, dcn_owned_head_workspace_bytes(units, F, H, L), x0.device, "dcn_head")
        check(lib.yr_dcn_head_ordered(
            _rows(x0, f32, "x0"), x0.stride(0), _rows(h, f32, "h"), h.stride(0), units, F, H, L,
            _dev(cw, f32, "cw"), _dev(cb, f32, "cb"), _dev(Wo, f32, "Wo"), _dev(bo, f32, "bo"),
            1 if bpr else 0, float(inv_batch), _opt(pred, f32, "pred"), _opt(gpred, f32, "gpred"),
            None if dh is None else _rows(dh, f32, "dh"), 0 if dh is None else dh.stride(0),
            None if dx0 is None else _rows(dx0, f32, "dx0"), 0 if dx0 is None else dx0.stride(0),
            _opt(dcw, f32, "dcw"), _opt(dcb, f32, "dcb"), _opt(dWo, f32, "dWo"), _opt(dbo, f32, "dbo"),
            _opt(loss_partials, f32, "loss_partials"), None if ws is None else ws.data_ptr(),
            0 if ws is None else ws.numel(), _stream()), "yr_dcn_head_ordered")
        return
    check(lib.yr_dcn_head(_rows(x0, f32, "x0"), x0.stride(0), _rows(h, f32, "h"), h.stride(0), units, F, H, L,
                          _dev(cw, f32, "cw"), _dev(cb, f32, "cb"), _dev(Wo, f32, "Wo"), _dev(bo, f32, "bo"),
                          1 if bpr else 0, float(inv_batch), _opt(pred, f32, "pred"), _opt(gpred, f32, "gpred"),
                          None if dh is None else _rows(dh, f32, "dh"), 0 if dh is None else dh.stride(0),
                          None if dx0 is None else _rows(dx0, f32, "dx0"), 0 if dx0 is None else dx0.stride(0),
                          _opt(dcw, f32, "dcw"), _opt(dcb, f32, "dcb"), _opt(dWo, f32, "dWo"), _opt(dbo, f32, "dbo"),
                          _opt(loss_partials, f32, "loss_partials"), _stream()), "yr_dcn_head")


def dcn_score(Au, Bi, Pu, Pi, users, W2, b2, Wo, bo, cw, cb, out, err_flag=None):
    """out[r, i] = the DCN sigmoid output of (users[r], item i) for the whole catalogue (yr_dcn_score); the first
    hidden layer arrives split as Au (per user) + Bi (per item, bias included), the cross / output dot products of
    x0 as Pu + Pi.  W2 None: one hidden layer."""
    lib = _lib.load()
    f32 = torch.float32
    n = users.numel()
    num_users, H1 = Au.shape
    num_items = Bi.shape[0]
    L, F = cw.shape
    H2 = W2.shape[0] if W2 is not None else 0
    if Pu.shape != (num_users, L + 1) or Pi.shape != (num_items, L + 1) or Bi.shape[1] != H1:
        raise EngineError("dcn_score: inconsistent shapes")
    if out.dim() != 2 or out.shape[0] < n or out.shape[1] < num_items or out.stride(1) != 1:
        raise EngineError("dcn_score: bad output buffer")
    check(lib.yr_dcn_score(_rows(Au, f32, "Au"), Au.stride(0), _rows(Bi, f32, "Bi"), Bi.stride(0),
                           _dev(Pu, f32, "Pu"), _dev(Pi, f32, "Pi"), _dev(users, torch.int64, "users"), n, num_users,
                           num_items, H1, H2, _opt(W2, f32, "W2"), _opt(b2, f32, "b2"), _dev(Wo, f32, "Wo"),
                           _dev(bo, f32, "bo"), _dev(cw, f32, "cw"), _dev(cb, f32, "cb"), L, F, out.data_ptr(),
                           out.stride(0) if n > 1 else num_items, _opt(err_flag, torch.int32, "flag"), _stream()),
          "yr_dcn_score")
    return out


# ---- S3Rec scoring (csrc/s3rec.hip) ----
S3REC_MAX_L, S3REC_MAX_HEADS, S3REC_MAX_BLOCKS = 64, 4, 4


def s3rec_block_floats(E, heads):
    """Floats of one block in the packed parameter buffer (layout: include/yelprec_engine.h)."""
    return (4 * heads + 2) * E * E + 7 * E


def s3rec_encode(item_emb, pos_enc, params, X, heads, blocks, last_only=False, out=None, err_flag=None):
    """h [B, L, E] of every position of the sequences X [B, L] (int64), or h[:, L - 1] as [B, E] with ``last_only``
    (yr_s3rec_encode): the embedding layer and the self-attention blocks in one launch."""
    lib = _lib.load()
    f32 = torch.float32
    if X.dim() != 2 or item_emb.dim() != 2 or pos_enc.shape != (X.shape[1], item_emb.shape[1]):
        raise EngineError(f"s3rec_encode: X [B, L], item_emb [num_items + 1, E], pos_enc [L, E] expected, got "
                          f"{tuple(X.shape)} / {tuple(item_emb.shape)} / {tuple(pos_enc.shape)}")
    (B, L), E = X.shape, item_emb.shape[1]
    if params.numel() != blocks * s3rec_block_floats(E, heads):
        raise EngineError(f"s3rec_encode: packed parameters hold {params.numel()} floats, "
                          f"{blocks * s3rec_block_floats(E, heads)} expected")
    shape = (B, E) if last_only else (B, L, E)
    if out is None:
        out = torch.empty(shape, dtype=f32, device=X.device)
    elif tuple(out.shape) != shape:
        raise EngineError(f"s3rec_encode: out {tuple(out.shape)}, expected {shape}")
    check(lib.yr_s3rec_encode(_dev(item_emb, f32, "item_emb"), _dev(pos_enc, f32, "pos_enc"),
                              _dev(params, f32, "params"), _dev(X, torch.int64, "X"), B, L, E, heads, blocks,
                              item_emb.shape[0] - 1, 1 if last_only else 0, _dev(out, f32, "out"),
                              _opt(err_flag, torch.int32, "flag"), _stream()), "yr_s3rec_encode")
    return out


def _s3rec_out(out, shapes, device, what):
    if out is None:
        return tuple(torch.empty(s, dtype=torch.float32, device=device) for s in shapes)
    if len(out) != 2 or any(tuple(t.shape) != s for t, s in zip(out, shapes)):
        raise EngineError(f"{what}: out must be two tensors of shapes {shapes}")
    return tuple(out)


def s3rec_seq_scores(item_emb, h, pos_items, neg_items, out=None, err_flag=None):
    """(pos_preds, neg_preds), each [B * L]: <item_emb[items[b, i]], h[b, i]> at every position (yr_s3rec_seq_scores)."""
    lib = _lib.load()
    f32 = torch.float32
    E = item_emb.shape[1]
    rows = h.numel() // E
    if pos_items.numel() != rows or neg_items.numel() != rows:
        raise EngineError("s3rec_seq_scores: one positive and one negative item per position expected")
    pos, neg = _s3rec_out(out, ((rows,), (rows,)), h.device, "s3rec_seq_scores")
    check(lib.yr_s3rec_seq_scores(_dev(item_emb, f32, "item_emb"), _dev(h, f32, "h"),
                                  _dev(pos_items, torch.int64, "pos_items"), _dev(neg_items, torch.int64, "neg_items"),
                                  rows, E, item_emb.shape[0] - 1, _dev(pos, f32, "pos_preds"), _dev(neg, f32, "neg_preds"),
                                  _opt(err_flag, torch.int32, "flag"), _stream()), "yr_s3rec_seq_scores")
    return pos, neg


def s3rec_candidate_scores(item_emb, h_last, pos_item, neg_items, out=None, err_flag=None):
    """(pos_pred [B, 1], neg_preds [B, C]): the last position's h against the positive and the C sampled candidates
    (yr_s3rec_candidate_scores)."""
    lib = _lib.load()
    f32 = torch.float32
    B, E = h_last.shape
    if neg_items.dim() != 2 or neg_items.shape[0] != B or neg_items.shape[1] < 1 or pos_item.numel() != B:
        raise EngineError("s3rec_candidate_scores: pos_item [B] and neg_items [B, C >= 1] expected")
    C = neg_items.shape[1]
    pos, neg = _s3rec_out(out, ((B, 1), (B, C)), h_last.device, "s3rec_candidate_scores")
    check(lib.yr_s3rec_candidate_scores(_dev(item_emb, f32, "item_emb"), _dev(h_last, f32, "h_last"),
                                        _dev(pos_item, torch.int64, "pos_item"),
                                        _dev(neg_items, torch.int64, "neg_items"), B, C, E, item_emb.shape[0] - 1,
                                        _dev(pos, f32, "pos_pred"), _dev(neg, f32, "neg_preds"),
                                        _opt(err_flag, torch.int32, "flag"), _stream()), "yr_s3rec_candidate_scores")
    return pos, neg


# ---- S3Rec training (csrc/s3rec.hip: the stash-keeping forward, the backward, the item gradient) ----
_S3REC_WS_ARRAYS = (("h_in", 1, 0), ("qkv", 0, 3), ("A", 0, 1), ("x1", 1, 0), ("xh1", 1, 0), ("relu", 1, 0),
                    ("xh2", 1, 0), ("rstd", None, None), ("g2", 1, 0), ("gx2", 1, 0), ("d2m", 1, 0), ("dz1", 1, 0),
                    ("g1", 1, 0), ("gx1", 1, 0), ("d1m", 1, 0), ("dqkv", 0, 3), ("dA", 0, 1))


def s3rec_train_workspace_floats(B, L, E, heads, blocks):
    """Floats of the training workspace (yr_s3rec_train_workspace_floats)."""
    return query_size("yr_s3rec_train_workspace_floats", B, L, E, heads, blocks)


def s3rec_workspace_views(ws, B, L, E, heads, blocks):
    """[{name: [B L, width] view}] per block of the training workspace (layout: include/yelprec_engine.h)."""
    R, at, out = B * L, 0, []
    for _ in range(blocks):
        views = {}
        for name, e, he in _S3REC_WS_ARRAYS:
            width = 4 if e is None else (e + he * heads) * E
            views[name] = ws[at:at + R * width].view(R, width)
            at += R * width
        out.append(views)
    if at != ws.numel():
        raise EngineError(f"s3rec workspace: {ws.numel()} floats, the layout takes {at}")
    return out


def _s3rec_train_dims(params, X, E, heads, blocks, ws, what):
    if X.dim() != 2:
        raise EngineError(f"{what}: X [B, L] expected, got {tuple(X.shape)}")
    if params.numel() != blocks * s3rec_block_floats(E, heads):
        raise EngineError(f"{what}: packed parameters hold {params.numel()} floats, "
                          f"{blocks * s3rec_block_floats(E, heads)} expected")
    if ws.dim() != 1:
        raise EngineError(f"{what}: the workspace is a flat f32 buffer")
    return X.shape


def s3rec_encode_train(item_emb, pos_enc, params, X, heads, blocks, seed=0, p=0.0, workspace=None, out=None,
                       err_flag=None):
    """(h [B, L, E], workspace): yr_s3rec_encode_train — the encoder in train() mode (dropout ``p`` from ``seed``)
    keeping what s3rec_backward consumes in ``workspace`` (allocated when None)."""
    lib = _lib.load()
    f32 = torch.float32
    if item_emb.dim() != 2 or X.dim() != 2 or pos_enc.shape != (X.shape[1], item_emb.shape[1]):
        raise EngineError(f"s3rec_encode_train: X [B, L], item_emb [num_items + 1, E], pos_enc [L, E] expected, got "
                          f"{tuple(X.shape)} / {tuple(item_emb.shape)} / {tuple(pos_enc.shape)}")
    E = item_emb.shape[1]
    if workspace is None:
        workspace = torch.empty(s3rec_train_workspace_floats(X.shape[0], X.shape[1], E, heads, blocks), dtype=f32,
                                device=X.device)
    B, L = _s3rec_train_dims(params, X, E, heads, blocks, workspace, "s3rec_encode_train")
    if out is None:
        out = torch.empty((B, L, E), dtype=f32, device=X.device)
    elif tuple(out.shape) != (B, L, E):
        raise EngineError(f"s3rec_encode_train: out {tuple(out.shape)}, expected {(B, L, E)}")
    check(lib.yr_s3rec_encode_train(_dev(item_emb, f32, "item_emb"), _dev(pos_enc, f32, "pos_enc"),
                                    _dev(params, f32, "params"), _dev(X, torch.int64, "X"), B, L, E, heads, blocks,
                                    item_emb.shape[0] - 1, int(seed) & 0xFFFFFFFFFFFFFFFF, float(p), _dev(out, f32, "out"),
                                    _dev(workspace, f32, "workspace"), workspace.numel(),
                                    _opt(err_flag, torch.int32, "flag"), _stream()), "yr_s3rec_encode_train")
    return out, workspace


def s3rec_backward(params, X, dh_out, workspace, heads, blocks, seed=0, p=0.0, d_emb=None):
    """d_emb [B, L, E] from dh_out [B, L, E]; the deltas of every block go to ``workspace`` (yr_s3rec_backward)."""
    lib = _lib.load()
    f32 = torch.float32
    E = dh_out.shape[-1]
    B, L = _s3rec_train_dims(params, X, E, heads, blocks, workspace, "s3rec_backward")
    if tuple(dh_out.shape) != (B, L, E):
        raise EngineError(f"s3rec_backward: dh_out {tuple(dh_out.shape)}, expected {(B, L, E)}")
    if d_emb is None:
        d_emb = torch.empty((B, L, E), dtype=f32, device=X.device)
    elif tuple(d_emb.shape) != (B, L, E):
        raise EngineError(f"s3rec_backward: d_emb {tuple(d_emb.shape)}, expected {(B, L, E)}")
    check(lib.yr_s3rec_backward(_dev(params, f32, "params"), _dev(X, torch.int64, "X"), _dev(dh_out, f32, "dh_out"),
                                B, L, E, heads, blocks, int(seed) & 0xFFFFFFFFFFFFFFFF, float(p),
                                _dev(workspace, f32, "workspace"), workspace.numel(), _dev(d_emb, f32, "d_emb"),
                                _stream()), "yr_s3rec_backward")
    return d_emb


S3REC_GRAD_CHUNK_ROWS = 2048
S3REC_GRAD_STREAM_JOBS = 16     # chunk products from which _s3rec_rows_products deals them to four streams


_s3rec_side_streams = {}


def _s3rec_rows_products(jobs):
    """out [M, N] = D^T Xm over the rows for every (D, Xm, out) of ``jobs``, summed on two levels: a product per
    S3REC_GRAD_CHUNK_ROWS rows, then a column sum over the partial products — no atomics, and the f32 rounding of a
    sum over B L rows stays that of a sum over a chunk (one accumulator chain over 12,850 rows measured 1.7 x the
    tests' bar).  A chunk's product fills a handful of workgroups (one per 64 x 64 output tile), so the
    chunk products of a large batch are dealt to four streams that rejoin before the column sums."""
    chunk = S3REC_GRAD_CHUNK_ROWS
    small, chunked = [], []
    for D, Xm, out in jobs:
        if D.shape[0] <= chunk:
            small.append((D, Xm, out))
        else:
            parts = torch.empty(((D.shape[0] + chunk - 1) // chunk, out.numel()), dtype=torch.float32, device=D.device)
            chunked.append((parts, out))
            small.extend((D[c * chunk:(c + 1) * chunk], Xm[c * chunk:(c + 1) * chunk], parts[c].view(out.shape))
                         for c in range(parts.shape[0]))
    if len(small) < S3REC_GRAD_STREAM_JOBS:
        for D, Xm, out in small:
            gemm_f32(D, Xm, transA=True, out=out)
    else:
        cur = torch.cuda.current_stream()
        side = _s3rec_side_streams.setdefault(cur.device, [torch.cuda.Stream(cur.device) for _ in range(3)])
        for st in side:
            st.wait_stream(cur)
        for k, (D, Xm, out) in enumerate(small):
            with torch.cuda.stream(cur if k % 4 == 0 else side[k % 4 - 1]):
                gemm_f32(D, Xm, transA=True, out=out)
        for st in side:
            cur.wait_stream(st)
    for parts, out in chunked:
        colsum(parts, out=out.view(-1))


def _s3rec_rows_sum(D, B, L, out):
    """out [width] = the column sums of D [B L, width], summed on two levels: over the sequences, then over the
    positions (the order d positional_encoding takes)."""
    colsum(colsum(D.view(B, L * D.shape[1])).view(L, D.shape[1]), out=out)
    return out


def s3rec_param_grads(workspace, B, L, E, heads, blocks, out=None):
    """The gradient of the packed parameter buffer from the stash and the deltas of a backward pass: per block four
    transposed products over the B L rows (yr_gemm_f32, no atomics: _s3rec_rows_products) and seven column sums
    (yr_colsum), each ending in its place of the packed layout."""
    n = s3rec_block_floats(E, heads)
    if out is None:
        out = torch.empty(blocks * n, dtype=torch.float32, device=workspace.device)
    EE, HE = E * E, heads * E
    jobs = []
    for blk, v in enumerate(s3rec_workspace_views(workspace, B, L, E, heads, blocks)):
        g = out[blk * n:(blk + 1) * n]
        at = 0

        def take(rows, cols):
            nonlocal at
            t = g[at:at + rows * cols]
            at += rows * cols
            return t.view(rows, cols) if rows > 1 else t

        jobs.append((v["dqkv"], v["h_in"], take(3 * HE, E)))
        jobs.append((v["d1m"], v["A"], take(E, HE)))
        _s3rec_rows_sum(v["d1m"], B, L, take(1, E))
        _s3rec_rows_sum(v["gx1"], B, L, take(1, E))
        _s3rec_rows_sum(v["g1"], B, L, take(1, E))
        jobs.append((v["dz1"], v["x1"], take(E, E)))
        _s3rec_rows_sum(v["dz1"], B, L, take(1, E))
        jobs.append((v["d2m"], v["relu"], take(E, E)))
        _s3rec_rows_sum(v["d2m"], B, L, take(1, E))
        _s3rec_rows_sum(v["gx2"], B, L, take(1, E))
        _s3rec_rows_sum(v["g2"], B, L, take(1, E))
        assert at == n == (4 * heads + 2) * EE + 7 * E
    _s3rec_rows_products(jobs)
    return out


def s3rec_score_grad(item_emb, pos_items, neg_items, dpos, dneg, err_flag=None):
    """dh_out [rows, E] = dpos[r] item_emb[pos_items[r]] + dneg[r] item_emb[neg_items[r]] (yr_s3rec_score_grad)."""
    lib = _lib.load()
    f32 = torch.float32
    rows, E = dpos.numel(), item_emb.shape[1]
    if pos_items.numel() != rows or neg_items.numel() != rows or dneg.numel() != rows:
        raise EngineError("s3rec_score_grad: one positive, one negative and two score gradients per position expected")
    out = torch.empty((rows, E), dtype=f32, device=item_emb.device)
    check(lib.yr_s3rec_score_grad(_dev(item_emb, f32, "item_emb"), _dev(pos_items, torch.int64, "pos_items"),
                                  _dev(neg_items, torch.int64, "neg_items"), _dev(dpos, f32, "dpos"),
                                  _dev(dneg, f32, "dneg"), rows, E, item_emb.shape[0] - 1, out.data_ptr(),
                                  _opt(err_flag, torch.int32, "flag"), _stream()), "yr_s3rec_score_grad")
    return out


def s3rec_item_grad(X, pos_items, neg_items, d_emb, h, dpos, dneg, d_item, err_flag=None):
    """d_item [num_items + 1, E] += the three item_embedding lookups' gradients (yr_s3rec_item_grad): the lookups are
    sorted by id here (a stable sort: index preparation), the sums run in the kernels in a fixed order."""
    lib = _lib.load()
    f32 = torch.float32
    rows, E = dpos.numel(), d_item.shape[1]
    if any(t.numel() != rows for t in (X, pos_items, neg_items, dneg)) or d_emb.numel() != rows * E \
            or h.numel() != rows * E:
        raise EngineError("s3rec_item_grad: X, pos_items, neg_items, dpos, dneg of B L entries and d_emb, h [B, L, E] expected")
    for t, name in ((X, "X"), (pos_items, "pos_items"), (neg_items, "neg_items")):
        _dev(t, torch.int64, name)
    sorted_ids, order = torch.sort(torch.cat([X.reshape(-1), pos_items.reshape(-1), neg_items.reshape(-1)]), stable=True)
    partial = torch.empty((3 * rows, E), dtype=f32, device=d_item.device)
    check(lib.yr_s3rec_item_grad(_dev(sorted_ids, torch.int64, "sorted_ids"), _dev(order, torch.int64, "order"),
                                 _dev(d_emb, f32, "d_emb"), _dev(h, f32, "h"), _dev(dpos, f32, "dpos"),
                                 _dev(dneg, f32, "dneg"), rows, E, d_item.shape[0] - 1, partial.data_ptr(),
                                 _dev(d_item, f32, "d_item"), _opt(err_flag, torch.int32, "flag"), _stream()),
          "yr_s3rec_item_grad")
    return d_item


# ---- S3Rec pre-training (csrc/s3rec_pretrain.hip: the catalogue BCE) ----
def s3rec_item_grad_one(X, d_emb, d_item, err_flag=None):
    """d_item [num_items + 1, E] += d_emb rows scattered by X alone: yr_s3rec_item_grad with the two score lists
    switched off (zero coefficients on lookups of X itself, which add exact zeros in the same fixed order)."""
    zero = torch.zeros(X.numel(), dtype=torch.float32, device=d_emb.device)
    return s3rec_item_grad(X, X, X, d_emb, d_emb, zero, zero, d_item, err_flag=err_flag)


def s3rec_catalogue_bce_workspace_floats(N, R, E):
    """Floats of the catalogue-BCE workspace (yr_s3rec_catalogue_bce_workspace_floats)."""
    return query_size("yr_s3rec_catalogue_bce_workspace_floats", N, R, E)


def s3rec_catalogue_bce(F, T, zscale, yscale, key, tgt_ptr=None, tgt_idx=None, grads=True, want_dF=None, want_dT=None,
                        workspace=None, err_flag=None):
    """(loss [1], row_loss [N], dF [N, E] or None, dT [R, E] or None) of yr_s3rec_catalogue_bce: the BCE-with-logits
    mean over all N R elements of z = zscale <F, T> against y = yscale [r in targets(key)], the targets a CSR over the
    keys (``tgt_ptr`` [K + 1], ``tgt_idx``, int64) or, without one, the key's own column.  ``grads`` False is the
    loss-only call; ``want_dF`` / ``want_dT`` pick one gradient."""
    lib = _lib.load()
    f32, i64 = torch.float32, torch.int64
    if F.dim() != 2 or T.dim() != 2 or F.shape[1] != T.shape[1]:
        raise EngineError(f"s3rec_catalogue_bce: F [N, E] and T [R, E] expected, got {tuple(F.shape)} / {tuple(T.shape)}")
    (N, E), R = F.shape, T.shape[0]
    if zscale.numel() != N or yscale.numel() != N or key.numel() != N:
        raise EngineError("s3rec_catalogue_bce: zscale, yscale and key hold one entry per row of F")
    if (tgt_ptr is None) != (tgt_idx is None):
        raise EngineError("s3rec_catalogue_bce: tgt_ptr and tgt_idx come together")
    K = R if tgt_ptr is None else tgt_ptr.numel() - 1
    want_dF = grads if want_dF is None else want_dF
    want_dT = grads if want_dT is None else want_dT
    dev = F.device
    if workspace is None:
        workspace = torch.empty(s3rec_catalogue_bce_workspace_floats(N, R, E), dtype=f32, device=dev)
    loss = torch.zeros(1, dtype=f32, device=dev)
    row_loss = torch.zeros(N, dtype=f32, device=dev)
    dF = torch.empty((N, E), dtype=f32, device=dev) if want_dF else None
    dT = torch.empty((R, E), dtype=f32, device=dev) if want_dT else None
    # an empty CSR has no storage to point at: its offsets array stands in (never dereferenced: every list is empty)
    idx = None if tgt_idx is None else (_dev(tgt_idx, i64, "tgt_idx") if tgt_idx.numel() else _dev(tgt_ptr, i64, "tgt_ptr"))
    check(lib.yr_s3rec_catalogue_bce(_dev(F, f32, "F"), _dev(T, f32, "T"), _dev(zscale, f32, "zscale"),
                                     _dev(yscale, f32, "yscale"), _dev(key, i64, "key"), _opt(tgt_ptr, i64, "tgt_ptr"),
                                     idx, N, R, K, E, loss.data_ptr(), row_loss.data_ptr() if N else None,
                                     _opt(dF, f32, "dF") if N else None, _opt(dT, f32, "dT") if R else None,
                                     _dev(workspace, f32, "workspace") if workspace.numel() else None,
                                     workspace.numel(), _opt(err_flag, torch.int32, "flag"), _stream()),
          "yr_s3rec_catalogue_bce")
    return loss, row_loss, dF, dT


# ---- S3Rec full-catalogue evaluation (csrc/s3rec_rank.hip: the catalogue rank) ----
def s3rec_catalogue_rank_workspace_bytes(N, R, E):
    """Bytes of the catalogue-rank workspace (yr_s3rec_catalogue_rank_workspace_bytes)."""
    return query_size("yr_s3rec_catalogue_rank_workspace_bytes", N, R, E)


def s3rec_catalogue_rank(H, T, target, excl_ptr=None, excl_idx=None, excl_rows=None, first_col=1, want_score=False,
                         err_flag=None):
    """rank [N] int64 of yr_s3rec_catalogue_rank: the 0-based place of column ``target[n]`` among the columns
    [first_col, R) of <H[n], T[r]> in the list order (score descending, id ascending among equal scores), the columns
    of CSR row ``excl_rows[n]`` (default n) of ``excl_ptr`` / ``excl_idx`` (ascending inside a row) left out; -1 for a
    row without a target.  ``want_score`` True: (rank, target_score [N] float32)."""
    lib = _lib.load()
    f32, i64 = torch.float32, torch.int64
    if H.dim() != 2 or T.dim() != 2 or H.shape[1] != T.shape[1]:
        raise EngineError(f"s3rec_catalogue_rank: H [N, E] and T [R, E] expected, got {tuple(H.shape)} / {tuple(T.shape)}")
    (N, E), R = H.shape, T.shape[0]
    if target.numel() != N or (excl_rows is not None and excl_rows.numel() != N):
        raise EngineError("s3rec_catalogue_rank: target (and excl_rows) hold one entry per row of H")
    if (excl_ptr is None) != (excl_idx is None):
        raise EngineError("s3rec_catalogue_rank: excl_ptr and excl_idx come together")
    K = 0 if excl_ptr is None else excl_ptr.numel() - 1
    dev = H.device
    ws_bytes = s3rec_catalogue_rank_workspace_bytes(N, R, E)
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    rank = torch.empty(N, dtype=i64, device=dev)
    score = torch.empty(N, dtype=f32, device=dev) if want_score else None
    # an empty CSR has no storage to point at: its offsets array stands in (never dereferenced: every list is empty)
    idx = None if excl_idx is None else (_dev(excl_idx, i64, "excl_idx") if excl_idx.numel() else _dev(excl_ptr, i64, "excl_ptr"))
    check(lib.yr_s3rec_catalogue_rank(_dev(H, f32, "H"), _dev(T, f32, "T"), _dev(target, i64, "target"),
                                      _opt(excl_ptr, i64, "excl_ptr"), idx, _opt(excl_rows, i64, "excl_rows"), N, R, K,
                                      E, int(first_col), rank.data_ptr() if N else None,
                                      score.data_ptr() if want_score and N else None,
                                      ws.data_ptr() if ws.numel() else None, ws_bytes,
                                      _opt(err_flag, torch.int32, "flag"), _stream()), "yr_s3rec_catalogue_rank")
    return (rank, score) if want_score else rank


S3REC_MODES = {"train": DEFINES["YR_S3REC_TRAIN"], "valid": DEFINES["YR_S3REC_VALID"], "test": DEFINES["YR_S3REC_TEST"]}
S3REC_MAX_NEG = 128


def s3rec_batches(beh_ptr, beh_idx, avoid_ptr, avoid_idx, num_items, users, L, mode, seed, epoch, n_neg=None,
                  err_flag=None):
    """The S3Rec batch rows of ``users`` (csrc/s3rec_batches.hip; reference s3rec_data_pipeline.py:13-50 +
    s3rec_dataset.py:21-57), int64 on the device: ``mode`` 'train' / 'valid' gives (X [B, L], pos_items [B, L],
    neg_items [B, L]), 'test' gives (X [B, L], pos_item [B], neg_items [B, n_neg]) with ``n_neg`` <= 128 mutually
    distinct negatives.  A user's rows are a pure function of (seed, epoch, mode, user)."""
    lib = _lib.load()
    if mode not in S3REC_MODES:
        raise EngineError(f"s3rec_batches: unknown mode {mode!r}")
    i64 = torch.int64
    num_users, B, L = beh_ptr.numel() - 1, users.numel(), int(L)
    if avoid_ptr.numel() != num_users + 1:
        raise EngineError("s3rec_batches: beh_ptr and avoid_ptr must both hold num_users + 1 offsets")
    test = mode == "test"
    n_neg = (99 if test else L) if n_neg is None else int(n_neg)
    dev = beh_ptr.device
    X = torch.empty((B, L), dtype=i64, device=dev)
    pos = torch.empty((B,) if test else (B, L), dtype=i64, device=dev)
    neg = torch.empty((B, max(n_neg, 0)), dtype=i64, device=dev)
    # an empty CSR has no storage to point at: its offsets array stands in (never dereferenced: every row is empty)
    idx_or = lambda idx, ptr, name: _dev(idx, i64, name) if idx.numel() else _dev(ptr, i64, name)
    check(lib.yr_s3rec_batches(_dev(beh_ptr, i64, "beh_ptr"), idx_or(beh_idx, beh_ptr, "beh_idx"),
                               _dev(avoid_ptr, i64, "avoid_ptr"), idx_or(avoid_idx, avoid_ptr, "avoid_idx"),
                               num_users, int(num_items), _dev(users, i64, "users"), B, L, S3REC_MODES[mode], n_neg,
                               int(seed) & (2**64 - 1), int(epoch) & (2**64 - 1),
                               X.data_ptr() if B else None, pos.data_ptr() if B else None,
                               neg.data_ptr() if neg.numel() else None, _opt(err_flag, torch.int32, "err_flag"),
                               _stream()), "yr_s3rec_batches")
    return X, pos, neg
