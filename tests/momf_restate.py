"""Restatement of the reference's MOMF head (REC/model/PixelNet/momf.py:50-71, MLPLayers of REC/model/layers.py:239-294 with
BatchNorm1d + tanh) over rows of an encoder output E, in plain torch, in whatever dtype and on whatever device the parameters are
handed over: float64 is the yardstick of the tests, float32 shows how far the reference's own arithmetic is from it.  Test
infrastructure only; nothing under pixelrec_amd imports this.

    u_b = tower_u(user_embedding[user_b])      i_{b,t} = tower_i(E[index_{b,t}])      index [B, 2] positions (positive, negative)
    x_b = <u_b, i_{b,0}> - <u_b, i_{b,1}>      loss = -mean_b log sigmoid(x_b)        NO 1e-8 (momf.py:59)
    tower(x) = per layer  tanh(gamma (z - mu) / sqrt(var + eps) + beta),  z = x W^T + b
               training: mu / var = the batch mean / biased variance over the rows the tower is given (B user rows; the 2B item rows
               of index.view(-1), a repeated position counted once per occurrence); running stats <- 0.9 running + 0.1 (mu,
               unbiased var); eval: mu / var = the running statistics

log sigmoid is written as logsigmoid (finite for every x); the reference's log(sigmoid(x)) is the same number wherever sigmoid(x) has
not underflowed.  P holds the reference's state_dict entries outside the encoder under their names.
"""
import torch

EPS = 1e-5
MOMENTUM = 0.1
E_KEY = "E"
TABLE = "user_embedding.weight"
_STATS = ("running_mean", "running_var", "num_batches_tracked")


def tower_names(n_layers):
    """The towers' state_dict names in the reference's order (Linear w, b, BatchNorm w, b, running_mean, running_var, count)."""
    out = []
    for tower in ("user", "item"):
        for k in range(n_layers):
            lin, bn = f"{tower}_mlp_layers.mlp_layers.{4 * k + 1}.", f"{tower}_mlp_layers.mlp_layers.{4 * k + 2}."
            out += [lin + "weight", lin + "bias", bn + "weight", bn + "bias"] + [bn + s for s in _STATS]
    return out


def state_names(n_layers):
    """The reference's state_dict keys in front of visual_encoder.*."""
    return tower_names(n_layers) + [TABLE]


def trainable(names):
    return [k for k in names if not k.endswith(_STATS)]


def tower(P, which, n_layers, x, train, stats=None):
    """MLPLayers([D] + hidden, 0, 'tanh', bn=True) on x [R, D]; `stats`: a dict that receives the running statistics after a
    training pass (P is left alone)."""
    for k in range(n_layers):
        lin, bn = f"{which}_mlp_layers.mlp_layers.{4 * k + 1}.", f"{which}_mlp_layers.mlp_layers.{4 * k + 2}."
        z = x @ P[lin + "weight"].T + P[lin + "bias"]
        if train:
            R = z.shape[0]
            mu = z.mean(0)
            var = ((z - mu) ** 2).mean(0)
            if stats is not None:
                with torch.no_grad():
                    stats[bn + "running_mean"] = (1 - MOMENTUM) * P[bn + "running_mean"] + MOMENTUM * mu
                    stats[bn + "running_var"] = (1 - MOMENTUM) * P[bn + "running_var"] + MOMENTUM * var * R / (R - 1)
                    stats[bn + "num_batches_tracked"] = P[bn + "num_batches_tracked"] + 1
        else:
            mu, var = P[bn + "running_mean"], P[bn + "running_var"]
        x = torch.tanh(P[bn + "weight"] * (z - mu) / torch.sqrt(var + EPS) + P[bn + "bias"])
    return x


def loss_of(P, n_layers, E, user, index, stats=None):
    """0-dim training loss (momf.py:50-60) on the encoder rows E [M, D]; user int [B], index int [B, 2]."""
    user, index = torch.as_tensor(user, device=E.device), torch.as_tensor(index, device=E.device)
    u = tower(P, "user", n_layers, P[TABLE][user], True, stats)
    it = tower(P, "item", n_layers, E[index.reshape(-1)], True, stats).view(user.shape[0], 2, -1)
    x = (u * it[:, 0]).sum(-1) - (u * it[:, 1]).sum(-1)
    return -torch.nn.functional.logsigmoid(x).mean()


def loss_and_grads(P, n_layers, E, user, index):
    """-> (loss as a float, {name: gradient}, running statistics after the pass): the gradient of E under E_KEY (rows nobody reads
    come out as exact zeros), of the user table dense under TABLE."""
    names = trainable(list(P))
    Q = {k: (v.detach().clone().requires_grad_(True) if k in names else v) for k, v in P.items()}
    Ex = E.detach().clone().requires_grad_(True)
    stats = {}
    loss = loss_of(Q, n_layers, Ex, user, index, stats)
    loss.backward()
    grads = {k: Q[k].grad.detach() for k in names}
    grads[E_KEY] = Ex.grad.detach()
    return float(loss.detach()), grads, stats


def item_features(P, n_layers, enc_rows):
    """compute_item (momf.py:69-71) on encoder rows: the eval-mode item tower."""
    with torch.no_grad():
        return tower(P, "item", n_layers, enc_rows, False)


def predict(P, n_layers, users, item_feature):
    """scores [B, N] (momf.py:62-67): the eval-mode user tower times item_feature^T."""
    with torch.no_grad():
        u = tower(P, "user", n_layers, P[TABLE][torch.as_tensor(users, device=item_feature.device)], False)
        return u @ item_feature.T
