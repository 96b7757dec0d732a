"""ACF restated from the formulas (acf.py forward / predict / compute_item_all), in the dtype of the state it is handed (float64,
or float32 for the reference's own arithmetic).  With the frozen v_feat [I, h, w, F] (H = h w regions), E = embedding_size, a batch
row [profile (L, left-padded with 0) | positive | negative | user id], r = (b, p), mask_r = [profile_r != 0]:

    x_{r,h} = relu(dim_reductor(v_feat[profile_r, h]))      x~ = feats.w_x(x)      u~_b = feats.w_u(user_embedding[uid_b])
    beta_r  = softmax_H(feats.w(relu(x~_{r,h} + u~_b)))      pooled_r = mask_r sum_h beta_{r,h} x_{r,h}
    alpha_b = softmax_P(w(relu(w_u(user_b) + w_p(item_model[profile_r]) + w_x(pooled_r)))), masked p at -inf, empty profile -> 0
    user_b  = w_u(user_embedding[uid_b]) + sum_p alpha_{b,p} item_model[profile_r]
    loss    = -mean_b log(1e-8 + sigmoid(<user_b, item_model[pos_b]> - <user_b, item_model[neg_b]>))
    predict = user item_model^T

State is a dict of tensors under the reference's 18 parameter names.  Gradients come from torch's autograd over these formulas;
item row 0 is nn.Embedding's padding row (its gradient is zero); AdamW is torch.optim.AdamW's update, written out."""
import numpy as np
import torch

U = "user_model."
LINEARS = (U + "feats.dim_reductor", U + "feats.w_x", U + "feats.w_u", U + "feats.w", U + "w_u", U + "w_p", U + "w_x", U + "w")
NAMES = (("item_model.weight",) + tuple(f"{l}.{k}" for l in LINEARS[:4] for k in ("weight", "bias"))
         + (U + "user_embedding.weight",) + tuple(f"{l}.{k}" for l in LINEARS[4:] for k in ("weight", "bias")))
ALIAS = U + "profile_embedding.weight"
STATE_KEYS = NAMES[:10] + (ALIAS,) + NAMES[10:]           # the reference's state_dict: 19 keys, the alias after user_embedding
BOUNDED = (U + "feats.w.bias", U + "w.bias")             # constant along their softmax axis: they influence no output


def state_from(g, prefix, dtype=torch.float64):
    """{name: tensor} of the 18 parameters stored in the golden under `prefix` (e.g. 'sd.')."""
    return {k: torch.from_numpy(np.asarray(g[prefix + k])).to(dtype).clone() for k in NAMES}


def _lin(P, name, x):
    return x @ P[name + ".weight"].T + P[name + ".bias"]


def user_vectors(P, v_feat, profile, uid, want=False):
    """user [B, E] of (profile [B, L], uid [B]); want=True also returns (beta [B, L, H], alpha [B, L])."""
    dt = P["item_model.weight"].dtype
    profile, uid = torch.as_tensor(profile), torch.as_tensor(uid)
    v = torch.as_tensor(v_feat, dtype=dt)
    f = v[profile].flatten(2, 3)                                                   # [B, L, H, F]
    mask = profile != 0
    user = P[U + "user_embedding.weight"][uid]
    x = torch.relu(_lin(P, U + "feats.dim_reductor", f))
    xt = _lin(P, U + "feats.w_x", x)
    ut = _lin(P, U + "feats.w_u", user)
    beta = torch.softmax(_lin(P, U + "feats.w", torch.relu(xt + ut[:, None, None, :])), dim=2)        # [B, L, H, 1]
    pooled = mask[..., None].to(dt) * (beta * x).sum(2)
    prof = P["item_model.weight"][profile]
    uw = _lin(P, U + "w_u", user)
    a = torch.relu(uw[:, None, :] + _lin(P, U + "w_p", prof) + _lin(P, U + "w_x", pooled))
    t = _lin(P, U + "w", a)[..., 0].masked_fill(~mask, float("-inf"))
    alpha = torch.softmax(t, dim=1)
    alpha = alpha.masked_fill(torch.isnan(alpha), 0.0)
    out = uw + (alpha[..., None] * prof).sum(1)
    return (out, beta[..., 0], alpha) if want else out


def loss(P, v_feat, rows):
    rows = torch.as_tensor(rows)
    user = user_vectors(P, v_feat, rows[:, :-3], rows[:, -1])
    it = P["item_model.weight"][rows[:, -3:-1]]                                    # [B, 2, E]
    s = (user[:, None, :] * it).sum(-1)
    return -torch.mean(torch.log(1e-8 + torch.sigmoid(s[:, 0] - s[:, 1])))


def loss_and_grads(P, v_feat, rows):
    """-> (loss, {name: gradient}) for the 18 parameters; the padding row of item_model gets no gradient (padding_idx = 0)."""
    for k in NAMES:
        P[k] = P[k].detach().requires_grad_(True)
    L = loss(P, v_feat, rows)
    gs = torch.autograd.grad(L, [P[k] for k in NAMES], allow_unused=True)
    for k in NAMES:
        P[k] = P[k].detach()
    g = {k: (torch.zeros_like(P[k]) if x is None else x) for k, x in zip(NAMES, gs)}
    g["item_model.weight"] = g["item_model.weight"].clone()
    g["item_model.weight"][0] = 0
    return float(L.detach()), g


def predict(P, v_feat, windows):
    """scores [B, I] of evaluation rows [profile (L) | user id]."""
    with torch.no_grad():
        windows = torch.as_tensor(windows)
        return user_vectors(P, v_feat, windows[:, :-1], windows[:, -1]) @ P["item_model.weight"].T


def adamw(P, v_feat, batches, lr, wd, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.AdamW, one group, one step per batch -> (losses, m, v)."""
    b1, b2 = betas
    m = {k: torch.zeros_like(P[k]) for k in NAMES}
    v = {k: torch.zeros_like(P[k]) for k in NAMES}
    losses = []
    for t, rows in enumerate(batches, start=1):
        L, g = loss_and_grads(P, v_feat, rows)
        losses.append(L)
        for k in NAMES:
            P[k] = P[k] * (1 - lr * wd)
            m[k] = b1 * m[k] + (1 - b1) * g[k]
            v[k] = b2 * v[k] + (1 - b2) * g[k] ** 2
            denom = (v[k] / (1 - b2 ** t)).sqrt() + eps
            P[k] = P[k] - lr / (1 - b1 ** t) * m[k] / denom
    return losses, m, v
