"""Torch restatement of S3Rec fine-tuning for the gradient tests: ``s3rec_ref64.encode`` / ``finetune`` again, in
torch on the CPU with a ``dtype`` argument and the per-site dropout masks of the training kernels (csrc/s3rec.hip), so
that autograd gives the gradients (float64: the judge; float32: the measure of what f32 arithmetic costs on a case).
Importable helper, no tests and no fixtures in it; runs without a GPU.

The bar follows s3rec_ref64: per case and per gradient tensor

    bar = BAR_FACTOR * max |grad_f32 - grad_f64|        of this restatement alone, never of a kernel,

with the forward's factor 8 (the matrix instruction's and the split GEMM's summation order, the device exp / sqrt /
divide).  Where both gradients are exactly zero the bar is zero: the kernel's value must be exactly zero too (dW_k of
a batch with no padded key).  ``None`` marks the tensors that take no part (attribute_embedding, the four *_weight).

Dropout: ``dropout_masks`` restates the kernels' law in NumPy on the Philox of gemm_ref64 (imported, not copied):
site = 2 block + {0: attention output, 1: FFN output}, float4 group q of the flat [B, L, E] index draws
Philox4x32-10 at the counter (q lo, q hi, site, 0) under the key (seed lo, seed hi), word t belongs to element
4 q + t, kept where u01 >= (float) p; kept values are scaled by 1 / (1 - p).

VARIANTS are wrong readings of the backward pass; tests/test_s3rec_grad_ref64.py checks that each moves at least one
gradient tensor of every case it applies to past its bar.
"""
import math

import numpy as np
import torch

import s3rec_ref64 as ref
from gemm_ref64 import philox4x32, u01

BAR_FACTOR = 8.0
DROPOUT_CASES = ("E64-L50-h2-b2-B257", "E16-L7-h1-b1-B3", "E128-L64-h4-b4-B3", "E32-L33-h4-b3-B3")
DROPOUT_PS = (0.1, 0.5)
DROPOUT_SEED = 0x9E3779B97F4A7C15

VARIANTS = {
    "residual_to_x1": "the second residual adds x1 (the textbook form), not the block's input",
    "key_mask_not_in_dK": "dK is not multiplied by pad[j]",
    "scale_not_in_dS": "dS without its 1 / sqrt(E)",
    "padding_out_of_mean": "the loss is a mean over the real positions only",
    "dropout_unscaled": "dropout without its 1 / (1 - p)",
}


def applies(variant, case, p_drop=0.0):
    """Where a variant cannot change any gradient, by the definition itself: with one key the softmax is 1 whatever
    the score, so dS is zero and neither its scale nor dK exists at L = 1; the dropout scale needs p > 0."""
    if variant in ("key_mask_not_in_dK", "scale_not_in_dS"):
        return case["L"] > 1
    if variant == "dropout_unscaled":
        return p_drop > 0
    return True


def configs():
    """[(case, p)]: every case of s3rec_ref64 at p = 0, the four DROPOUT_CASES at p = 0.1 and 0.5."""
    out = [(c, 0.0) for c in ref.CASES]
    by_id = {c["id"]: c for c in ref.CASES}
    out += [(by_id[i], p) for i in DROPOUT_CASES for p in DROPOUT_PS]
    return out


def config_id(case, p):
    return case["id"] if p == 0 else f"{case['id']}-p{p}"


def dropout_masks(seed, p, B, L, E, blocks):
    """bool [2 blocks, B, L, E]: True where the element is kept at site 2 block + {0, 1}."""
    n = B * L * E
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    out = np.empty((2 * blocks, n), dtype=bool)
    for site in range(2 * blocks):
        w = philox4x32(q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), np.full_like(q, site), np.zeros_like(q),
                       seed & 0xFFFFFFFF, seed >> 32, 10)
        out[site] = u01(np.stack(w, 1).reshape(-1)[:n]) >= np.float32(p)
    return out.reshape(2 * blocks, B, L, E)


def _detached_value(value, grad_path):
    """``value`` in the forward pass, the gradient of ``grad_path`` in the backward pass."""
    return grad_path + (value - grad_path).detach()


def tensors(p, dtype, requires_grad=True):
    """The parameter dict as torch leaves of ``dtype``."""
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad) for k, v in p.items()}


def encode(t, X, heads, blocks, p_drop=0.0, masks=None, variant=None):
    """h [B, L, E] from the leaves ``t``; ``masks``: dropout_masks(...) or None."""
    X = torch.as_tensor(np.asarray(X))
    B, L = X.shape
    table = t["item_embedding.weight"]
    dt, E = table.dtype, table.shape[1]
    pad = (X <= 0)
    h = table[X.clamp(min=0)] + t["positional_encoding"]
    keep = torch.tril(torch.ones((L, L), dtype=torch.bool))
    padf = pad[..., None].to(dt)
    div = math.sqrt(E)
    scale = 1.0 if variant == "dropout_unscaled" else 1.0 / (1.0 - p_drop)

    def drop(x, site):
        if masks is None or p_drop == 0:
            return x
        return x * torch.as_tensor(masks[site]).to(dt) * scale

    for b in range(blocks):
        att = []
        for hd in range(heads):
            pre = f"multihead_attns.{b}."
            Q = h @ t[f"{pre}q_weights.{hd}.weight"].T
            Kraw = h @ t[f"{pre}k_weights.{hd}.weight"].T
            K = Kraw * padf
            if variant == "key_mask_not_in_dK":
                K = _detached_value(K, Kraw)
            V = h @ t[f"{pre}v_weights.{hd}.weight"].T
            Sraw = Q @ K.transpose(1, 2)
            S = Sraw / div
            if variant == "scale_not_in_dS":
                S = _detached_value(S, Sraw)
            S = torch.where(keep, S, torch.tensor(-math.inf, dtype=dt))
            P = torch.softmax(S, dim=-1)
            att.append(P @ V)
        attn = torch.cat(att, -1) @ t[f"multihead_attns.{b}.output.weight"].T + t[f"multihead_attns.{b}.output.bias"]
        x1 = torch.nn.functional.layer_norm(h + drop(attn, 2 * b), (E,), t[f"layernorm1s.{b}.weight"],
                                            t[f"layernorm1s.{b}.bias"], ref.LN_EPS)
        f1 = torch.relu(x1 @ t[f"ffn1s.{b}.weight"].T + t[f"ffn1s.{b}.bias"])
        f2 = f1 @ t[f"ffn2s.{b}.weight"].T + t[f"ffn2s.{b}.bias"]
        res = x1 if variant == "residual_to_x1" else h          # reference models/s3rec.py:70 adds the block's INPUT
        h = torch.nn.functional.layer_norm(res + drop(f2, 2 * b + 1), (E,), t[f"layernorm2s.{b}.weight"],
                                           t[f"layernorm2s.{b}.bias"], ref.LN_EPS)
    return h


def finetune(t, X, pos_items, neg_items, heads, blocks, p_drop=0.0, masks=None, variant=None):
    """(pos_preds, neg_preds, h)."""
    h = encode(t, X, heads, blocks, p_drop, masks, variant)
    table = t["item_embedding.weight"]
    hr = h.reshape(-1, table.shape[1])
    pos = (table[torch.as_tensor(np.asarray(pos_items)).reshape(-1)] * hr).sum(-1)
    neg = (table[torch.as_tensor(np.asarray(neg_items)).reshape(-1)] * hr).sum(-1)
    return pos, neg, h


def bpr_loss(pos, neg, X=None, variant=None):
    """mean(-logsigmoid(pos - neg)) over all B L positions (reference loss.py:19-27), padding included."""
    terms = -torch.nn.functional.logsigmoid(pos - neg)
    if variant == "padding_out_of_mean":
        real = (torch.as_tensor(np.asarray(X)).reshape(-1) > 0).to(terms.dtype)
        return (terms * real).sum() / real.sum().clamp(min=1)
    return terms.mean()


def loss_and_grads(p, batch, heads, blocks, dtype=torch.float64, p_drop=0.0, seed=DROPOUT_SEED, variant=None):
    """dict(h, pos, neg, loss, grads {state_dict name: array, or None where the tensor takes no part}) of one
    finetune + BPRLoss + backward."""
    t = tensors(p, dtype)
    X = np.asarray(batch["X"])
    E = np.asarray(p["item_embedding.weight"]).shape[1]
    masks = dropout_masks(seed, p_drop, X.shape[0], X.shape[1], E, blocks) if p_drop > 0 else None
    pos, neg, h = finetune(t, X, batch["pos_items"], batch["neg_items"], heads, blocks, p_drop, masks, variant)
    loss = bpr_loss(pos, neg, X, variant)
    loss.backward()
    grads = {k: (None if v.grad is None else v.grad.numpy().copy()) for k, v in t.items()}
    return dict(h=h.detach().numpy(), pos=pos.detach().numpy(), neg=neg.detach().numpy(), loss=float(loss.detach()),
                grads=grads)


def bars(g32, g64):
    """{name: BAR_FACTOR * max |g32 - g64|} over the tensors that take part."""
    return {k: BAR_FACTOR * float(np.max(np.abs(g32[k].astype(np.float64) - g64[k]))) for k, v in g64.items()
            if v is not None}


def group(name):
    """The tensor group a gradient is reported under (DESIGN 4.10 lists max err / bar per group)."""
    for key, g in (("item_embedding", "item"), ("positional", "pos"), ("q_weights", "Wq"), ("k_weights", "Wk"),
                   ("v_weights", "Wv"), ("output.weight", "Wo"), ("output.bias", "bo"), ("layernorm1s", "ln1"),
                   ("ffn1s", "ffn1"), ("ffn2s", "ffn2"), ("layernorm2s", "ln2")):
        if key in name:
            return g
    return name


def case_setup(case):
    """(params, batch) of a case of s3rec_ref64."""
    return (ref.make_params(case["E"], case["L"], case["heads"], case["blocks"], seed=case["index"]),
            ref.make_batch(case))


def train(state, batches, heads, blocks, epochs, lr, dtype):
    """trainers/s3rec_trainer.py:233-247 at dropout 0 with torch.optim.Adam over every parameter: ([[batch losses]
    per epoch], final state as arrays); an epoch's return value is the sum of its batch losses."""
    t = tensors(state, dtype)
    opt = torch.optim.Adam(list(t.values()), lr=lr)
    losses = []
    for _ in range(epochs):
        per_batch = []
        for b in batches:
            pos, neg, _ = finetune(t, b["X"], b["pos_items"], b["neg_items"], heads, blocks)
            opt.zero_grad()
            loss = bpr_loss(pos, neg)
            loss.backward()
            opt.step()
            per_batch.append(float(loss.detach()))
        losses.append(per_batch)
    return losses, {k: v.detach().numpy().copy() for k, v in t.items()}
