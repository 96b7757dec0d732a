"""MF restated in float64 from the formulas (mf.py forward / predict / compute_item_all, MLPLayers with BatchNorm1d + tanh):

    tower(x) = per layer  tanh(gamma (z - mu) / sqrt(var + eps) + beta),  z = x W^T + b
               training: mu / var = the batch mean / biased variance; running stats <- 0.9 running + 0.1 (mu, unbiased var)
               eval: mu / var = the running statistics
    x_b = <u_b, i+_b> - <u_b, i-_b>,   loss = -mean(1e-8 + log sigmoid(x_b))

State is a dict of float64 tensors under the reference's state_dict names.  Gradients come from torch's float64 autograd over
these formulas; AdamW is torch.optim.AdamW's update, written out."""
import numpy as np
import torch

EPS = 1e-5
MOMENTUM = 0.1


def state_from(g, prefix):
    """{name: float64 tensor} of the golden's initial state_dict under `prefix` (e.g. 'c1.sd.')."""
    return {k[len(prefix):]: torch.from_numpy(np.asarray(g[k])).to(torch.float64 if g[k].dtype != np.int64 else torch.int64).clone()
            for k in g.files if k.startswith(prefix)}


def _tower(P, tower, n_layers, x, train):
    for k in range(n_layers):
        lin, bn = f"{tower}_mlp_layers.mlp_layers.{4 * k + 1}.", f"{tower}_mlp_layers.mlp_layers.{4 * k + 2}."
        z = x @ P[lin + "weight"].T + P[lin + "bias"]
        if train:
            R = z.shape[0]
            mu = z.mean(0)
            var = ((z - mu) ** 2).mean(0)
            with torch.no_grad():
                P[bn + "running_mean"] = (1 - MOMENTUM) * P[bn + "running_mean"] + MOMENTUM * mu
                P[bn + "running_var"] = (1 - MOMENTUM) * P[bn + "running_var"] + MOMENTUM * var * R / (R - 1)
                P[bn + "num_batches_tracked"] = P[bn + "num_batches_tracked"] + 1
        else:
            mu, var = P[bn + "running_mean"], P[bn + "running_var"]
        x = torch.tanh(P[bn + "weight"] * (z - mu) / torch.sqrt(var + EPS) + P[bn + "bias"])
    return x


def loss(P, n_layers, user, item, train=True):
    """0-dim float64 loss of one training step; updates P's BatchNorm buffers when train."""
    user, item = torch.as_tensor(user), torch.as_tensor(item)
    u = _tower(P, "user", n_layers, P["user_embedding.weight"][user], train)
    it = _tower(P, "item", n_layers, P["item_embedding.weight"][item.reshape(-1)], train)
    it = it.view(user.shape[0], 2, -1)
    x = (u * it[:, 0]).sum(-1) - (u * it[:, 1]).sum(-1)
    return -torch.mean(1e-8 + torch.nn.functional.logsigmoid(x))


def noise_driven(name):
    """The Linear bias in front of a BatchNorm has a zero gradient in exact arithmetic (the batch mean removes it), so AdamW turns
    its rounding noise into steps of about +-lr, and the running mean inherits them: along a trajectory these are only bounded
    (|drift| <= 4 lr per step), never compared to a tolerance of rounding size."""
    return (name.endswith("running_mean") or (name.endswith(".bias") and "_mlp_layers." in name
                                              and (int(name.split(".")[2]) % 4) == 1))


def trainable(P):
    return [k for k in P if not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"))]


def loss_and_grads(P, n_layers, user, item):
    names = trainable(P)
    for k in names:
        P[k] = P[k].detach().requires_grad_(True)
    L = loss(P, n_layers, user, item, train=True)
    gs = torch.autograd.grad(L, [P[k] for k in names])
    for k in names:
        P[k] = P[k].detach()
    return float(L.detach()), dict(zip(names, gs))


def predict(P, n_layers, users):
    with torch.no_grad():
        feat = _tower(P, "item", n_layers, P["item_embedding.weight"], False)
        u = _tower(P, "user", n_layers, P["user_embedding.weight"][torch.as_tensor(users)], False)
        return u @ feat.T


def adamw(P, n_layers, batches, lr, wd, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.AdamW over the trainable parameters, one step per (user, item) batch -> losses."""
    b1, b2 = betas
    names = trainable(P)
    m = {k: torch.zeros_like(P[k]) for k in names}
    v = {k: torch.zeros_like(P[k]) for k in names}
    losses = []
    for t, (u, it) in enumerate(batches, start=1):
        L, g = loss_and_grads(P, n_layers, u, it)
        losses.append(L)
        for k in names:
            P[k] = P[k] * (1 - lr * wd)
            m[k] = b1 * m[k] + (1 - b1) * g[k]
            v[k] = b2 * v[k] + (1 - b2) * g[k] ** 2
            denom = (v[k] / (1 - b2 ** t)).sqrt() + eps
            P[k] = P[k] - lr / (1 - b1 ** t) * m[k] / denom
    return losses, m, v

