"""Float64 restatement of the reference's DCN (models/dcn.py:42-62) for the tests: the einsum cross network, the
deep tower, the sigmoid output and BPRLoss, with torch autograd for the gradients, and torch.optim.Adam's update.
Parameters are a dict keyed like the reference's state_dict."""
import numpy as np
import torch


def params64(state):
    return {k: torch.as_tensor(np.asarray(v), dtype=torch.float64).clone().requires_grad_(True) for k, v in state.items()}


def n_layers(P, prefix="cross_weights."):
    return sum(1 for k in P if k.startswith(prefix))


def x0_rows(P, user, item, cat_ids, sc_ids):
    """[U[user] | I[item] | mean C[cat_ids[item]] | S[sc_ids[item]]] (padded mean, padding rows included)."""
    cats = torch.as_tensor(np.asarray(cat_ids)[np.asarray(item)], dtype=torch.int64)
    sc = torch.as_tensor(np.asarray(sc_ids)[np.asarray(item)], dtype=torch.int64)
    u = torch.as_tensor(np.asarray(user), dtype=torch.int64)
    i = torch.as_tensor(np.asarray(item), dtype=torch.int64)
    return torch.cat([P["user_embedding.weight"][u], P["item_embedding.weight"][i],
                      P["attributes_embeddings.0.weight"][cats].mean(dim=1), P["attributes_embeddings.1.weight"][sc]], 1)


def cross_einsum(x, ws, bs):
    prev = x
    for w, b in zip(ws, bs):
        prev = torch.matmul(torch.einsum('bi,bj->bij', (x, prev)), w) + b + prev
    return prev


def cross_closed(x, ws, bs):
    alpha = torch.ones(x.shape[0], 1, dtype=x.dtype)
    beta = torch.zeros(x.shape[1], dtype=x.dtype)
    for w, b in zip(ws, bs):
        s = alpha * (x @ w).unsqueeze(1) + (beta @ w)
        alpha = alpha + s
        beta = beta + b
    return alpha * x + beta


def deep(P, x):
    k = 0
    while f"deep.{k}.weight" in P:
        x = torch.relu(x @ P[f"deep.{k}.weight"].T + P[f"deep.{k}.bias"])
        k += 2
    return x


def head(P, x, h):
    L = n_layers(P)
    xl = cross_einsum(x, [P[f"cross_weights.{l}"] for l in range(L)], [P[f"cross_bias.{l}"] for l in range(L)])
    z = torch.cat([h, xl], 1) @ P["output_layer.weight"].T + P["output_layer.bias"]
    return torch.sigmoid(z).reshape(-1)


def predict(P, user, item, cat_ids, sc_ids):
    x = x0_rows(P, user, item, cat_ids, sc_ids)
    return head(P, x, deep(P, x))


def bpr_loss(P, user, pos, neg, cat_ids, sc_ids):
    pp = predict(P, user, pos, cat_ids, sc_ids)
    pn = predict(P, user, neg, cat_ids, sc_ids)
    return torch.mean(-torch.nn.functional.logsigmoid(pp - pn)), pp, pn


def grads(P, user, pos, neg, cat_ids, sc_ids):
    for p in P.values():
        p.grad = None
    loss, pp, pn = bpr_loss(P, user, pos, neg, cat_ids, sc_ids)
    loss.backward()
    return loss, pp, pn, {k: p.grad.detach().clone() for k, p in P.items()}


def adam_step(P, G, lr, t=1, b1=0.9, b2=0.999, eps=1e-8):
    """First Adam step from zero moments (torch.optim.Adam, weight_decay 0)."""
    out = {}
    for k, p in P.items():
        g = G[k]
        m = (1 - b1) * g
        v = (1 - b2) * g * g
        out[k] = p.detach() - lr / (1 - b1 ** t) * m / ((v / (1 - b2 ** t)).sqrt() + eps)
    return out


def score_rows(P, users, cat_ids, sc_ids, num_items):
    """float64 sigmoid outputs [len(users), num_items]."""
    with torch.no_grad():
        items = np.arange(num_items)
        return torch.stack([predict(P, np.full(num_items, u), items, cat_ids, sc_ids) for u in users]).numpy()
