"""VBPR restated in float64 from the formulas (vbpr.py forward / predict / compute_item_all).  With Dh = embedding_size // 2,
frozen v_feat [I, F], W = feature_projection.weight [Dh, F], w_b = bias_projection.weight [1, F]:

    e_{b,t} = W v_feat[item_{b,t}]            beta_{b,t} = w_b . v_feat[item_{b,t}]            (t = positive, negative)
    s_{b,t} = <uid_b, iid_{b,t}> + <um_b, e_{b,t}> + beta_{b,t}
    loss    = -mean_b log(1e-8 + sigmoid(s_{b,0} - s_{b,1}))
    predict = uid iid^T + um (W v_feat)^T + w_b . v_feat

State is a dict of float64 tensors under the reference's state_dict names.  Gradients come from torch's float64 autograd over
these formulas; AdamW is torch.optim.AdamW's update, written out, with the reference's two parameter groups (names that contain
the fragment: modal_lr / modal_decay; the rest: rec_lr / rec_decay)."""
import numpy as np
import torch

NAMES = ("feature_projection.weight", "bias_projection.weight", "user_id_embedding.weight", "item_id_embedding.weight",
         "user_modal_embedding.weight")


def state_from(g, prefix):
    """{name: float64 tensor} of the golden's initial state_dict under `prefix` (e.g. 'sd.')."""
    return {k[len(prefix):]: torch.from_numpy(np.asarray(g[k])).to(torch.float64).clone() for k in g.files if k.startswith(prefix)}


def scores(P, v_feat, user, item):
    """s [B, 2] of the pairs (user [B], item [B, 2])."""
    user, item = torch.as_tensor(user), torch.as_tensor(item)
    v = torch.as_tensor(v_feat, dtype=torch.float64)[item]                       # [B, 2, F]
    e = v @ P["feature_projection.weight"].T                                     # [B, 2, Dh]
    beta = (v * P["bias_projection.weight"][0]).sum(-1)
    uid, um = P["user_id_embedding.weight"][user][:, None], P["user_modal_embedding.weight"][user][:, None]
    return (uid * P["item_id_embedding.weight"][item]).sum(-1) + (um * e).sum(-1) + beta


def loss(P, v_feat, user, item):
    s = scores(P, v_feat, user, item)
    return -torch.mean(torch.log(1e-8 + torch.sigmoid(s[:, 0] - s[:, 1])))


def loss_and_grads(P, v_feat, user, item):
    for k in NAMES:
        P[k] = P[k].detach().requires_grad_(True)
    L = loss(P, v_feat, user, item)
    gs = torch.autograd.grad(L, [P[k] for k in NAMES])
    for k in NAMES:
        P[k] = P[k].detach()
    return float(L.detach()), dict(zip(NAMES, gs))


def predict(P, v_feat, users):
    with torch.no_grad():
        v = torch.as_tensor(v_feat, dtype=torch.float64)
        feat = v @ P["feature_projection.weight"].T
        bias = v @ P["bias_projection.weight"][0]
        u = torch.as_tensor(users)
        return (P["user_id_embedding.weight"][u] @ P["item_id_embedding.weight"].T + P["user_modal_embedding.weight"][u] @ feat.T
                + bias)


def adamw(P, v_feat, batches, modal, rec, fragment="projection", betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.AdamW with two groups, one step per (user, item) batch -> (losses, m, v).  modal / rec = (lr, weight_decay) of
    the names that contain `fragment` / of the rest."""
    b1, b2 = betas
    m = {k: torch.zeros_like(P[k]) for k in NAMES}
    v = {k: torch.zeros_like(P[k]) for k in NAMES}
    losses = []
    for t, (u, it) in enumerate(batches, start=1):
        L, g = loss_and_grads(P, v_feat, u, it)
        losses.append(L)
        for k in NAMES:
            lr, wd = modal if fragment in k else rec
            P[k] = P[k] * (1 - lr * wd)
            m[k] = b1 * m[k] + (1 - b1) * g[k]
            v[k] = b2 * v[k] + (1 - b2) * g[k] ** 2
            denom = (v[k] / (1 - b2 ** t)).sqrt() + eps
            P[k] = P[k] - lr / (1 - b1 ** t) * m[k] / denom
    return losses, m, v
