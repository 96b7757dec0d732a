"""CuratorNet restated in float64 from its equations (no reference code): the common tower, the max / mean pooling over all L
positions (padding included, the mean divides by L, the max keeps the first of equal positions), the profile tower, the pair
loss, and AdamW as torch.optim.AdamW defines it.  The CPU test pins it to the reference's golden fixture; the GPU tests compare
the kernels with it."""
import torch

SCALE = 1.0507009873554804934193349852946
ALPHA = 1.6732632423543772848170429916717
LINEARS = ("selu_common1", "selu_common2", "selu_pu1", "selu_pu2", "selu_pu3")
NAMES = tuple(f"{lin}.{kind}" for lin in LINEARS for kind in ("weight", "bias"))      # the ten trainable tensors, reference order
KEYS = ("embedding.weight",) + NAMES                                                   # the state_dict's eleven keys


class _Selu(torch.autograd.Function):
    """selu(x) = s x for x > 0, else s a (exp(x) - 1); derivative s for x > 0, else s a exp(x) -- s a at exactly 0."""

    @staticmethod
    def forward(ctx, x):
        neg = torch.clamp(x, max=0.0)
        ctx.save_for_backward(x, torch.exp(neg))
        return torch.where(x > 0, SCALE * x, SCALE * ALPHA * torch.expm1(neg))

    @staticmethod
    def backward(ctx, g):
        x, ex = ctx.saved_tensors
        return g * torch.where(x > 0, torch.full_like(x, SCALE), SCALE * ALPHA * ex)


selu = _Selu.apply


def selu_grad(x):
    x = x.detach().clone().requires_grad_(True)
    selu(x).sum().backward()
    return x.grad


def pool(h):
    """h [B, L, E] -> ([B, 2E] = [max over L | mean over L], argmax [B, E]); torch.argmax returns the first maximal position."""
    idx = torch.argmax(h, dim=1)                                   # [B, E]
    mx = torch.gather(h, 1, idx.unsqueeze(1)).squeeze(1)
    return torch.cat((mx, h.sum(1) / h.shape[1]), dim=-1), idx


def state_from(npz, prefix):
    return {k: torch.tensor(npz[prefix + k], dtype=torch.float64) for k in KEYS}


def common(P, x):
    h = selu(x @ P["selu_common1.weight"].T + P["selu_common1.bias"])
    return selu(h @ P["selu_common2.weight"].T + P["selu_common2.bias"])


def profile_tower(P, cat):
    for lin in ("selu_pu1", "selu_pu2", "selu_pu3"):
        cat = selu(cat @ P[lin + ".weight"].T + P[lin + ".bias"])
    return cat


def loss_fn(P, profile, target):
    """profile int64 [B, L], target int64 [B, 2] = (positive, negative) -> the training loss."""
    feat = P["embedding.weight"]
    profile, target = torch.as_tensor(profile), torch.as_tensor(target)
    u = profile_tower(P, pool(common(P, feat[profile]))[0])
    it = common(P, feat[target])                                   # [B, 2, E]
    x = (u.unsqueeze(1) * it).sum(-1)
    return -torch.log(1e-8 + torch.sigmoid(x[:, 0] - x[:, 1])).mean()


def loss_and_grads(P, profile, target):
    Q = {k: v.detach().clone().requires_grad_(k != "embedding.weight") for k, v in P.items()}
    L = loss_fn(Q, profile, target)
    L.backward()
    return float(L.detach()), {k: Q[k].grad for k in NAMES}


def compute_item_all(P):
    with torch.no_grad():
        return common(P, P["embedding.weight"])


def user_vectors(P, item_seq, item_feature):
    with torch.no_grad():
        return profile_tower(P, pool(item_feature[torch.as_tensor(item_seq)])[0])


def predict(P, item_seq, item_feature=None):
    feat = compute_item_all(P) if item_feature is None else item_feature
    return user_vectors(P, item_seq, feat) @ feat.T


def adamw(P, batches, lr, wd, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.AdamW over the ten trainable tensors, in place on P -> the losses before each step."""
    m = {k: torch.zeros_like(P[k]) for k in NAMES}
    v = {k: torch.zeros_like(P[k]) for k in NAMES}
    losses = []
    for t, (profile, target) in enumerate(batches, start=1):
        L, g = loss_and_grads(P, profile, target)
        losses.append(L)
        for k in NAMES:
            P[k] = P[k] * (1.0 - lr * wd)
            m[k] = betas[0] * m[k] + (1 - betas[0]) * g[k]
            v[k] = betas[1] * v[k] + (1 - betas[1]) * g[k] * g[k]
            denom = v[k].sqrt() / (1 - betas[1] ** t) ** 0.5 + eps
            P[k] = P[k] - (lr / (1 - betas[0] ** t)) * m[k] / denom
    return losses
