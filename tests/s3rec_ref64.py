"""NumPy restatement of the S3Rec scoring kernels (csrc/s3rec.hip) for the tests: the eval()-mode encoder of
reference models/s3rec.py:53-71,184-214 and its two score forms (:73-115), with a ``dtype`` argument (float64: the
judge; float32: the measure of what f32 arithmetic costs on a case).  Importable helper, no fixtures (like
ngcf_ref64.py); runs without a GPU.  Parameters travel as a dict under the model's ``state_dict`` names.

The bar.  Softmax and two LayerNorms per block sit between the sums, so no closed-form bound exists.  Per case and
per compared tensor

    bar = BAR_FACTOR * max |restatement_f32 - restatement_f64|

measured on the restatement alone, never on the kernel.  The compared tensors are h (every position) and the scores
in the groups the reference consumes them in: ``seq`` = [pos_preds, neg_preds] (one BPR mean) and ``cand`` =
[pos_pred | neg_preds] (one ranking per row) — a maximum over samples needs samples, and pos_pred alone has one per
sequence.  The factor 8 covers what the kernel does differently from
NumPy's float32: the matrix instruction's summation order and the device exp / sqrt / divide.  tests/
test_s3rec_ref64.py checks that every wrong reading of the semantics in VARIANTS moves a case's output by more than
its bar; the generators therefore keep the weights at the reference's initialisation scale (larger attention / FFN
weights raise the f32 error faster than they raise the effect of the weakest variant, LayerNorm eps dropped).
"""
import math

import numpy as np

BAR_FACTOR = 8.0
LN_EPS = 1e-5
SENTINEL = 7.25                              # pre-fill around the kernels' outputs
NUM_ITEMS = 50                               # catalogue of the generated cases: ids 0 .. 50, row 50 the last
WIDTHS = (16, 32, 64, 128)
LENGTHS = (1, 2, 31, 32, 33, 50, 63, 64)     # both tile counts, their ends, the reference's 50
CANDIDATES = (1, 2, 99, 100)

# wrong readings of the semantics; each maps to (what it changes, where it can show at all)
VARIANTS = {
    "key_mask_dropped": "K is not multiplied by pad[j]",
    "key_mask_inverted": "the rows of the PADDED keys are zeroed instead",
    "head_divisor": "S / sqrt(E / heads)",
    "key0_hidden_from_last": "the last query does not see key 0",
    "ln_eps_dropped": "LayerNorm without eps",
    "pos_not_at_padding": "no positional row at padded positions",
    "out_bias_dropped": "attention output without b_o",
    "evaluate_at_L_minus_2": "candidate scores from position L - 2",
}


def applies(variant, case):
    """Where a variant cannot change any output, by the definition itself: with one key the softmax is 1 whatever
    the score, so nothing that only changes scores shows at L = 1; the per-head divisor equals sqrt(E) at one head;
    positions 0 and L - 2 need L > 1."""
    if variant in ("key_mask_dropped", "key_mask_inverted"):
        return case["L"] > 1
    if variant == "head_divisor":
        return case["L"] > 1 and case["heads"] > 1
    if variant in ("key0_hidden_from_last", "evaluate_at_L_minus_2"):
        return case["L"] > 1
    return True


# ------------------------------------------------------------------------------------------------ the restatement
def _ln(x, g, b, eps, dt):
    mean = x.mean(-1, keepdims=True, dtype=dt)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True, dtype=dt)
    return d / np.sqrt(var + dt(eps)) * g + b


def encode(p, X, heads, blocks, dtype=np.float64, variant=None):
    """h [B, L, E] of every position (section "Each of num_blocks blocks" of the kernel's contract)."""
    dt = np.dtype(dtype).type
    c = lambda name: np.asarray(p[name], dtype=dt)      # noqa: E731
    X = np.asarray(X)
    B, L = X.shape
    table = c("item_embedding.weight")
    E = table.shape[1]
    pad = X <= 0
    pos = np.broadcast_to(c("positional_encoding"), (B, L, E))
    if variant == "pos_not_at_padding":
        pos = pos * (~pad)[..., None].astype(dt)
    h = table[np.clip(X, 0, None)] + pos
    keep = np.tril(np.ones((L, L), dtype=bool))           # keys j <= i; the others are excluded, not penalised
    if variant == "key0_hidden_from_last" and L > 1:
        keep[L - 1, 0] = False
    kmask = pad
    if variant == "key_mask_inverted":
        kmask = ~pad
    div = dt(math.sqrt(E / heads if variant == "head_divisor" else E))
    eps = 0.0 if variant == "ln_eps_dropped" else LN_EPS
    for b in range(blocks):
        att = []
        for hd in range(heads):
            pre = f"multihead_attns.{b}."
            Q = h @ c(f"{pre}q_weights.{hd}.weight").T
            K = h @ c(f"{pre}k_weights.{hd}.weight").T
            if variant != "key_mask_dropped":
                K = K * kmask[..., None].astype(dt)
            V = h @ c(f"{pre}v_weights.{hd}.weight").T
            S = Q @ K.transpose(0, 2, 1) / div
            S = np.where(keep, S, dt(-np.inf))
            S = S - S.max(-1, keepdims=True)
            P = np.exp(S)
            P = P / P.sum(-1, keepdims=True, dtype=dt)
            att.append(P @ V)
        attn = np.concatenate(att, -1) @ c(f"multihead_attns.{b}.output.weight").T
        if variant != "out_bias_dropped":
            attn = attn + c(f"multihead_attns.{b}.output.bias")
        x1 = _ln(h + attn, c(f"layernorm1s.{b}.weight"), c(f"layernorm1s.{b}.bias"), eps, dt)
        f1 = np.maximum(x1 @ c(f"ffn1s.{b}.weight").T + c(f"ffn1s.{b}.bias"), dt(0))
        f2 = f1 @ c(f"ffn2s.{b}.weight").T + c(f"ffn2s.{b}.bias")
        # reference models/s3rec.py:70: the second residual adds the block's INPUT, not x1
        h = _ln(h + f2, c(f"layernorm2s.{b}.weight"), c(f"layernorm2s.{b}.bias"), eps, dt)
        assert h.dtype == np.dtype(dtype)
    return h


def finetune(p, X, pos_items, neg_items, heads, blocks, dtype=np.float64, variant=None, h=None):
    """(pos_preds, neg_preds), each [B * L] (``h``: the encoder's output where the caller already has it)."""
    h = encode(p, X, heads, blocks, dtype, variant) if h is None else h
    table = np.asarray(p["item_embedding.weight"], dtype=dtype)
    E = table.shape[1]
    hr = h.reshape(-1, E)
    return ((table[np.asarray(pos_items).reshape(-1)] * hr).sum(-1, dtype=dtype),
            (table[np.asarray(neg_items).reshape(-1)] * hr).sum(-1, dtype=dtype))


def evaluate(p, X, pos_item, neg_items, heads, blocks, dtype=np.float64, variant=None, h=None):
    """(pos_pred [B, 1], neg_preds [B, C]) from the last position."""
    h = encode(p, X, heads, blocks, dtype, variant) if h is None else h
    L = h.shape[1]
    at = L - 2 if variant == "evaluate_at_L_minus_2" and L > 1 else L - 1
    table = np.asarray(p["item_embedding.weight"], dtype=dtype)
    hl = h[:, at]
    pos = (table[np.asarray(pos_item).reshape(-1)] * hl).sum(-1, dtype=dtype)[:, None]
    neg = (table[np.asarray(neg_items)] * hl[:, None, :]).sum(-1, dtype=dtype)
    return pos, neg


def bar(f32_value, f64_value):
    return BAR_FACTOR * float(np.max(np.abs(np.asarray(f32_value, dtype=np.float64) - f64_value)))


# ------------------------------------------------------------------------------------------------ generators
def make_params(E, L, heads, blocks, num_items=NUM_ITEMS, attributes_count=5, seed=0):
    """Parameters at the reference's initialisation scale (Xavier embeddings and FFN weights, PyTorch's default
    U(+-1/sqrt(fan_in)) for the attention Linears and the biases, positional rows U[0, 1)), with the LayerNorm
    weights and every bias moved by 0.1 N(0, 1): a fresh LayerNorm is the identity and would hide its affine part."""
    rs = np.random.RandomState(seed)
    u = lambda bound, *shape: rs.uniform(-bound, bound, shape).astype(np.float32)      # noqa: E731
    n = lambda *shape: (0.1 * rs.standard_normal(shape)).astype(np.float32)            # noqa: E731
    p = {"positional_encoding": rs.uniform(0, 1, (L, E)).astype(np.float32),
         "item_embedding.weight": u(math.sqrt(6.0 / (num_items + 1 + E)), num_items + 1, E),
         "attribute_embedding.weight": u(math.sqrt(6.0 / (attributes_count + E)), attributes_count, E)}
    for b in range(blocks):
        for kind in "qkv":
            for hd in range(heads):
                p[f"multihead_attns.{b}.{kind}_weights.{hd}.weight"] = u(1 / math.sqrt(E), E, E)
        p[f"multihead_attns.{b}.output.weight"] = u(1 / math.sqrt(heads * E), E, heads * E)
        p[f"multihead_attns.{b}.output.bias"] = u(1 / math.sqrt(heads * E), E) + n(E)
        for name in ("layernorm1s", "layernorm2s"):
            p[f"{name}.{b}.weight"] = (1 + n(E)).astype(np.float32)
            p[f"{name}.{b}.bias"] = n(E)
        for name in ("ffn1s", "ffn2s"):
            p[f"{name}.{b}.weight"] = u(math.sqrt(6.0 / (2 * E)), E, E)
            p[f"{name}.{b}.bias"] = u(1 / math.sqrt(E), E) + n(E)
    for name in ("aap_weight", "mip_weight", "map_weight", "sp_weight"):
        p[f"{name}.weight"] = u(math.sqrt(6.0 / (2 * E)), E, E)
    return p


KINDS = ("alternating", "all_padding", "one_last", "one_first", "full", "last_row")


def make_sequence(kind, L, rs, num_items=NUM_ITEMS):
    ids = rs.randint(1, num_items + 1, L).astype(np.int64)
    if kind == "alternating":                     # real, pad, real, ... ending on a real item: interior padding
        ids[(L - 1 - np.arange(L)) % 2 == 1] = 0
    elif kind == "all_padding":
        ids[:] = 0
    elif kind == "one_last":
        ids[:-1] = 0
    elif kind == "one_first":
        ids[1:] = 0
    elif kind == "last_row":                      # id = num_items: the last row of the table
        ids[:] = num_items
    return ids


def make_batch(case, seed=1):
    """X [B, L], per-position items, candidates.  Sequence 0 alternates real items and padding, sequence 1 is all
    padding, the rest walk through the other kinds (which one first depends on the case, so that the grid covers
    them all at B = 3)."""
    rs = np.random.RandomState(seed + 7919 * case["index"])
    B, L, C = case["B"], case["L"], case["C"]
    kinds = [KINDS[0], KINDS[1]] + [KINDS[2 + (b + case["index"]) % 4] for b in range(max(B - 2, 0))]
    X = np.stack([make_sequence(kinds[b], L, rs) for b in range(B)])
    items = lambda *shape: rs.randint(0, NUM_ITEMS + 1, shape).astype(np.int64)        # noqa: E731
    return dict(X=X, pos_items=items(B, L), neg_items=items(B, L), pos_item=items(B), cand=items(B, C))


def _cases():
    out = []

    def add(E, L, heads, blocks, B):
        i = len(out)
        out.append(dict(index=i, E=E, L=L, heads=heads, blocks=blocks, B=B, C=CANDIDATES[i % 4],
                        id=f"E{E}-L{L}-h{heads}-b{blocks}-B{B}"))
    for E in WIDTHS:
        for L in LENGTHS:
            add(E, L, 2, 2, 3)
    for heads in (1, 2, 4):
        for blocks in (1, 3):
            add(32, 33, heads, blocks, 3)
    add(64, 50, 2, 2, 1)
    add(64, 50, 2, 2, 257)
    add(16, 7, 1, 1, 3)
    add(128, 64, 4, 4, 3)
    return out


CASES = _cases()


def case_outputs(case, dtype=np.float64, variant=None, params=None, batch=None):
    """{h [B, L, E], seq [2, B L] = (pos_preds, neg_preds), cand [B, 1 + C] = [pos_pred | neg_preds]} of a case."""
    p = params if params is not None else make_params(case["E"], case["L"], case["heads"], case["blocks"],
                                                      seed=case["index"])
    b = batch if batch is not None else make_batch(case)
    hb = (case["heads"], case["blocks"])
    enc_variant = None if variant == "evaluate_at_L_minus_2" else variant
    h = encode(p, b["X"], *hb, dtype=dtype, variant=enc_variant)
    sp, sn = finetune(p, b["X"], b["pos_items"], b["neg_items"], *hb, dtype=dtype, h=h)
    cp, cn = evaluate(p, b["X"], b["pos_item"], b["cand"], *hb, dtype=dtype, variant=variant, h=h)
    return dict(h=h, seq=np.stack([sp, sn]), cand=np.concatenate([cp, cn], axis=1))
