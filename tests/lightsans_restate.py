"""Float64 torch restatement of LightSANs (reference code/REC/model/IDNet/lightsans.py with model/layers.py:620-673 FeedForward and
:762-932 ItemToInterestAggregation / LightMultiHeadAttention / LightTransformerEncoder).  Gradients come from autograd.  Dropout
is injected as keep-masks (oracle/dropout_rng.keep_mask, the library's counter hash) in the layout of the model's sites:
"input" [B, L, D] (stream 0), (i, "attn") [B, H, L, K] (1 + 3i), (i, "attn_out") [B, L, D] (2 + 3i), (i, "ffn_out") (3 + 3i).
Parameters are a dict of reference state_dict names -> tensors."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle.dropout_rng import keep_mask


def _act(name):
    return {"gelu": lambda x: x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))), "relu": torch.relu,
            "swish": lambda x: x * torch.sigmoid(x), "tanh": torch.tanh, "sigmoid": torch.sigmoid}[name]


def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _drop(x, keep, p):
    return x if keep is None or p == 0 else x * keep.to(x.dtype) / (1.0 - p)


def _heads(x, H):                  # [..., L, D] -> [..., H, L, dh]
    *lead, L, D = x.shape
    return x.reshape(*lead, L, H, D // H).transpose(-3, -2)


def pos_probs(pqk, H):
    """pqk [L, 2D] = pq | pk -> A [H, L, L]: softmax over the queries (dim -2) of (pq * (2 dh)^-1/2) pk^T / sqrt(dh)."""
    L, D2 = pqk.shape
    D = D2 // 2
    dh = D // H
    pq = _heads(pqk[:, :D], H) * float(dh * 2) ** -0.5
    pk = _heads(pqk[:, D:], H)
    return torch.softmax(pq @ pk.transpose(-1, -2) / math.sqrt(dh), dim=-2)


def core(qkv, theta, A, H, K, keep=None, p=0.0):
    """The low-rank attention: qkv [B, L, 3D], theta [2, D, K], A [H, L, L] -> ctx [B, L, D] (head-merged)."""
    B, L, D3 = qkv.shape
    D = D3 // 3
    dh = D // H
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]

    def pool(x, th):
        pi = torch.softmax(x @ th, dim=-2)                   # [B, L, K], over l
        return torch.einsum("nij,nik->nkj", x, pi)          # [B, K, D]

    Kp, Vp = pool(k, theta[0]), pool(v, theta[1])
    S = _heads(q, H) @ _heads(Kp, H).transpose(-1, -2) / math.sqrt(dh)     # [B, H, L, K]
    P = _drop(torch.softmax(S, dim=-2), keep, p)
    ctx = P @ _heads(Vp, H) + A.unsqueeze(0) @ _heads(v, H)
    return ctx.transpose(1, 2).reshape(B, L, D)


def masks(seed, B, L, D, H, K, n_layers, p_hidden, p_attn):
    """The keep-masks of one training step (seed = the model's base seed + its completed-step counter)."""
    t = lambda a: torch.from_numpy(a)
    m = {"input": t(keep_mask(seed, 0, (B, L, D), p_hidden))}
    for i in range(n_layers):
        m[(i, "attn")] = t(keep_mask(seed, 1 + 3 * i, (B, H, L, K), p_attn))
        m[(i, "attn_out")] = t(keep_mask(seed, 2 + 3 * i, (B, L, D), p_hidden))
        m[(i, "ffn_out")] = t(keep_mask(seed, 3 + 3 * i, (B, L, D), p_hidden))
    return m


def encode(P, seq, n_layers, H, K, eps=1e-12, act="gelu", drop=None, p_hidden=0.0, p_attn=0.0):
    """seq [B, L] ids -> last-layer states [B, L, D]."""
    drop = drop or {}
    L = seq.shape[1]
    e = P["item_embedding.weight"][seq]
    x = _drop(_ln(e, P["LayerNorm.weight"], P["LayerNorm.bias"], eps), drop.get("input"), p_hidden)
    pos = P["position_embedding.weight"][:L]
    for i in range(n_layers):
        m = f"trm_encoder.layer.{i}.multi_head_attention."
        f = f"trm_encoder.layer.{i}.feed_forward."
        lin = lambda z, name: z @ P[name + ".weight"].t() + P[name + ".bias"]
        qkv = torch.cat([lin(x, m + "query"), lin(x, m + "key"), lin(x, m + "value")], dim=-1)
        pe = _ln(pos, P[m + "pos_ln.weight"], P[m + "pos_ln.bias"], eps)
        A = pos_probs(torch.cat([lin(pe, m + "pos_q_linear"), lin(pe, m + "pos_k_linear")], dim=-1), H)
        theta = torch.stack([P[m + "attpooling_key.theta"], P[m + "attpooling_value.theta"]])
        ctx = core(qkv, theta, A, H, K, drop.get((i, "attn")), p_attn)
        a = _ln(_drop(lin(ctx, m + "dense"), drop.get((i, "attn_out")), p_hidden) + x, P[m + "LayerNorm.weight"],
                P[m + "LayerNorm.bias"], eps)
        y = lin(_act(act)(lin(a, f + "dense_1")), f + "dense_2")
        x = _ln(_drop(y, drop.get((i, "ffn_out")), p_hidden) + a, P[f + "LayerNorm.weight"], P[f + "LayerNorm.bias"], eps)
    return x


def loss_fn(P, items, n_layers, H, K, **kw):
    """items [B, L+2] = history | positive | negative -> mean_b -log(sigmoid(pos - neg) + 1e-8) (1e-8 inside the log)."""
    out = encode(P, items[:, :-2], n_layers, H, K, **kw)[:, -1]
    e = P["item_embedding.weight"]
    x = (out * e[items[:, -2]]).sum(-1) - (out * e[items[:, -1]]).sum(-1)
    return (-torch.log(torch.sigmoid(x) + 1e-8)).mean()


def forward_backward(sd, items, n_layers, H, K, **kw):
    """-> (loss float, {name: gradient ndarray}).  The table's padding row gets no gradient (padding_idx = 0)."""
    P = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
    loss = loss_fn(P, torch.as_tensor(np.asarray(items)), n_layers, H, K, **kw)
    loss.backward()
    g = {k: v.grad.numpy().copy() for k, v in P.items()}
    g["item_embedding.weight"][0] = 0.0
    return float(loss.detach()), g


def predict(sd, item_seq, n_layers, H, K, **kw):
    P = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in sd.items()}
    out = encode(P, torch.as_tensor(np.asarray(item_seq)), n_layers, H, K, **kw)[:, -1]
    return (out @ P["item_embedding.weight"].t()).numpy()


def adamw_trajectory(sd, batches, n_layers, H, K, lr, wd, **kw):
    """torch.optim.AdamW over every parameter (the table's padding row has a zero gradient) -> (losses, final params)."""
    P = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
    opt = torch.optim.AdamW(list(P.values()), lr=lr, weight_decay=wd)
    losses = []
    for items in batches:
        opt.zero_grad()
        loss = loss_fn(P, torch.as_tensor(np.asarray(items)), n_layers, H, K, **kw)
        loss.backward()
        P["item_embedding.weight"].grad[0] = 0.0
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: v.detach().numpy().copy() for k, v in P.items()}


def unpack(g, name, n_layers=2):
    """A flat group of tests/golden/lightsans_tiny.npz -> {state_dict name: array} for the model with n_layers layers.  The
    groups of the two-layer model (sd, n2.*) hold every key; n1.grad holds the keys without layer 1 (the fixture's one-layer
    model is its two-layer parameters without layer 1)."""
    keys = [str(k) for k in g["keys"]]
    shapes = [tuple(int(x) for x in s[1:1 + int(s[0])]) for s in g["shapes"]]
    flat = g[name]
    full = sum(int(np.prod(s)) for s in shapes)
    layout = [(k, s) for k, s in zip(keys, shapes) if flat.size == full or ".layer.1." not in k]
    out, off = {}, 0
    for k, s in layout:
        n = int(np.prod(s))
        out[k] = flat[off:off + n].reshape(s)
        off += n
    assert off == flat.size, f"{name}: {flat.size} values for {off} parameters"
    return {k: v for k, v in out.items() if n_layers == 2 or ".layer.1." not in k}
