"""Restatement of the reference's WideDeep (REC/model/IDNet/widedeep.py with MLPLayers, REC/model/layers.py:239-281) in plain torch,
in whatever dtype and on whatever device the parameters are handed over: float64 is the yardstick of the tests, float32 shows how
far the reference's own arithmetic is from it.  Test infrastructure only; nothing under pixelrec_amd imports this.

Two forms of the same function:

  literal   y(row) = sum_w wide[row_w] + wide_bias + predict(mlp(concat_w deep[row_w]));  x_b = y(+) - y(-)      (widedeep.py:49-63)
  native    the first Linear split into its history block (once per sample) and its target block (per plane), and the head in the
            cancelled form x_b = <a_last(+) - a_last(-), w_p> + wide[p_b] - wide[n_b]; scoring through T = deep W1t^T + b1 (per
            item) and h_b = W1h xh_b (per user)

    loss = -mean_b log(1e-8 + sigmoid(x_b))
"""
import torch
import torch.nn.functional as F

from tests.din_restate import WALK_K, walk_histories, walk_users  # noqa: F401  (the walk cases share DIN's users and histories)

WBIAS, WIDE, DEEP = "wide_bias", "wide_item_embedding.weight", "deep_item_embedding.weight"
PRED_W, PRED_B = "deep_predict_layer.weight", "deep_predict_layer.bias"


def lin(i):
    return f"mlp_layers.mlp_layers.{3 * i + 1}"


def names(n_layers):
    """The reference's parameter (= state_dict) names in its order: a module's own parameter (wide_bias) comes before its
    submodules'; the MLP's Linears sit at mlp_layers.{1, 4, ...}."""
    out = [WBIAS, WIDE, DEEP]
    for i in range(n_layers):
        out += [lin(i) + ".weight", lin(i) + ".bias"]
    return out + [PRED_W, PRED_B]


def n_layers_of(P):
    return sum(1 for k in P if k.startswith("mlp_layers.") and k.endswith(".weight"))


def state_from(npz, prefix, dtype, device="cpu"):
    keys = [str(k) for k in npz[prefix + "keys"]]
    return {k: torch.as_tensor(npz[prefix + k]).to(device=device, dtype=dtype) for k in keys}


def planes(rows):
    """[B, L + 2] rows (profile | positive | negative) -> the reference's [B, 2, L + 1] input (OneTowerTrainDataset's two planes)."""
    rows = torch.as_tensor(rows)
    prof = rows[:, :-2]
    return torch.stack((torch.cat((prof, rows[:, -2:-1]), 1), torch.cat((prof, rows[:, -1:]), 1)), 1)


def mlp(P, x, first=0):
    for i in range(first, n_layers_of(P)):
        x = torch.relu(x @ P[lin(i) + ".weight"].T + P[lin(i) + ".bias"])
    return x


# ---- literal --------------------------------------------------------------------------------------------------------------------
def y_literal(P, ids):
    """ids [M, L + 1] -> y [M]: widedeep.py:53-60 (and :71-77), literally."""
    wide = F.embedding(ids, P[WIDE], padding_idx=0).sum(-2) + P[WBIAS]                       # [M, 1]
    x = F.embedding(ids, P[DEEP], padding_idx=0).reshape(ids.shape[0], -1)
    deep = mlp(P, x) @ P[PRED_W].T + P[PRED_B]
    return (wide + deep).squeeze(-1)


def loss_literal(P, rows):
    inp = planes(rows).to(P[DEEP].device)
    B = inp.shape[0]
    out = y_literal(P, inp.reshape(2 * B, -1)).view(B, 2)
    weight = torch.tensor([[1.0], [-1.0]], dtype=out.dtype, device=out.device)
    return -torch.mean(torch.log(1e-8 + torch.sigmoid(out @ weight)))


# ---- native ---------------------------------------------------------------------------------------------------------------------
def loss_native(P, rows):
    rows = torch.as_tensor(rows, device=P[DEEP].device)
    prof, tgt = rows[:, :-2], rows[:, -2:]
    B, L = prof.shape
    D = P[DEEP].shape[1]
    W1, b1 = P[lin(0) + ".weight"], P[lin(0) + ".bias"]
    xh = F.embedding(prof, P[DEEP], padding_idx=0).reshape(B, L * D)
    xt = F.embedding(tgt, P[DEEP], padding_idx=0).reshape(2 * B, D)
    zh, zt = xh @ W1[:, :L * D].T, xt @ W1[:, L * D:].T
    a = mlp(P, torch.relu(zh.repeat_interleave(2, 0) + zt + b1), first=1).view(B, 2, -1)
    wide = F.embedding(tgt, P[WIDE], padding_idx=0).squeeze(-1)                              # [B, 2]
    x = (a[:, 0] - a[:, 1]) @ P[PRED_W].view(-1) + wide[:, 0] - wide[:, 1]
    return -torch.mean(torch.log(1e-8 + torch.sigmoid(x)))


def loss_and_grads(P, rows, form="literal"):
    """-> (loss as a float, {name: gradient}); row 0 of both tables gets no gradient (padding_idx=0).  In the native form the two
    cancelled biases take no part in the loss: their gradient is an exact zero."""
    Q = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    loss = (loss_literal if form == "literal" else loss_native)(Q, rows)
    loss.backward()
    return float(loss.detach()), {k: (v.grad.detach() if v.grad is not None else torch.zeros_like(v)) for k, v in Q.items()}


def predict_literal(P, windows, chunk=4):
    """windows [B, L] -> scores [B, N]: widedeep.py:66-79 on CandiEvalDataset's [item_num, L + 1] matrix per user, `chunk` users at a
    time."""
    N = P[DEEP].shape[0]
    windows = torch.as_tensor(windows, device=P[DEEP].device)
    out = []
    for lo in range(0, windows.shape[0], chunk):
        w = windows[lo:lo + chunk]
        b, L = w.shape
        ids = torch.cat((w[:, None, :].expand(b, N, L), torch.arange(N, device=w.device)[None, :, None].expand(b, N, 1)), -1)
        out.append(y_literal(P, ids.reshape(b * N, L + 1)).view(b, N))
    return torch.cat(out)


def predict_factorised(P, windows):
    """The same scores through the factorised first Linear: T = deep W1t^T + b1 once per item, h_b = W1h xh_b once per user."""
    deep = P[DEEP]
    windows = torch.as_tensor(windows, device=deep.device)
    N, D = deep.shape
    B, L = windows.shape
    W1, b1 = P[lin(0) + ".weight"], P[lin(0) + ".bias"]
    T = deep @ W1[:, L * D:].T + b1                                                           # [N, h1]
    hb = deep[windows].reshape(B, L * D) @ W1[:, :L * D].T                                    # [B, h1]
    sb = P[WIDE].view(-1)[windows].sum(1) + P[WBIAS] + P[PRED_B]                              # [B]
    a = mlp(P, torch.relu(T[None] + hb[:, None]), first=1)                                    # [B, N, h_last]
    return sb[:, None] + P[WIDE].view(-1)[None] + a @ P[PRED_W].view(-1)


def masked_topk(scores, windows_hist, K):
    """scores [B, N] with column 0 and every (user, history item) pair set to -inf -> torch.topk(K).  windows_hist: list of id
    lists, one per user."""
    s = scores.clone()
    s[:, 0] = float("-inf")
    for b, h in enumerate(windows_hist):
        if len(h):
            s[b, torch.as_tensor(list(h), device=s.device)] = float("-inf")
    return torch.topk(s, min(K, s.shape[1]), dim=-1), s


def adamw(P, batches, lr, wd, form="literal"):
    """torch.optim.AdamW over the reference's parameters, one step per batch; P is updated in place.  -> list of losses."""
    params = {k: torch.nn.Parameter(v.detach().clone()) for k, v in P.items()}
    opt = torch.optim.AdamW(list(params.values()), lr=lr, weight_decay=wd)
    fn = loss_literal if form == "literal" else loss_native
    losses = []
    for rows in batches:
        opt.zero_grad()
        loss = fn(params, rows)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    for k in P:
        P[k] = params[k].detach().clone()
    return losses


# ---- the inputs of the fused top-k tests (tests/test_gpu_widedeep.py; tools/make_golden_widedeep.py --measure uses the same) ----
TOPK_ITEM_NUMS, TOPK_BS, TOPK_K = (127, 131, 257, 1000), (1, 5), 10
TOPK_HIDDEN = ((4,), (12,), (12, 4), (80, 40), (128, 128))
TOPK_DL = ((8, 4), (64, 10))
TOPK_SEED = 4            # the first seed at which float64 alone excuses no (user, rank) cell under the final bound (seeds 0-3: two each)


def topk_case(item_num, B, D, L, hidden, seed=None):
    """-> (P float32 xavier-normal state with small random biases (wide_bias and the predict bias non-zero), window int64 [B, L],
    histories: one id list per user).  User 0 has a full window; in a B = 5 batch user 1's window is all padding, user 2 keeps fewer
    than K items unmasked, users 3 and 4 have one and two padded positions.  Every history holds the window's items plus items
    outside it (the FULL history is longer than the window).  topk_histories() adds the float64 top-3 of user 0 to its history."""
    seed = TOPK_SEED if seed is None else seed
    g = torch.Generator().manual_seed(100003 * seed + 7 * item_num + 31 * B + 1009 * D + L + 13 * sum(hidden) + len(hidden))
    P = {}
    keys = names(len(hidden))
    P[WBIAS] = torch.randn(1, generator=g) * 0.1
    P[WIDE] = torch.randn(item_num, 1, generator=g) * (2.0 / (item_num + 1)) ** 0.5
    P[DEEP] = torch.randn(item_num, D, generator=g) * (2.0 / (item_num + D)) ** 0.5
    sizes = [(L + 1) * D] + list(hidden) + [1]
    for i, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        P[keys[3 + 2 * i]] = torch.randn(b, a, generator=g) * (2.0 / (a + b)) ** 0.5
        P[keys[4 + 2 * i]] = torch.randn(b, generator=g) * 0.1
    window = torch.randint(1, item_num, (B, L), generator=g)
    if B > 1:
        window[1, :] = 0
    for b in range(3, B):
        window[b, :min(L - 1, b - 2)] = 0
    hist = []
    for b in range(B):
        extra = torch.randint(1, item_num, (L + 3,), generator=g).tolist()
        h = set(window[b][window[b] != 0].tolist()) | set(extra)
        if b == 2:
            keep = set(torch.randperm(item_num - 1, generator=g)[:TOPK_K - 3].add(1).tolist())
            h = set(range(1, item_num)) - (keep - h)
        hist.append(sorted(h))
    return P, window, hist


def topk_histories(s64, hist):
    """The histories with user 0's float64 top-3 (among its unmasked items) added: a history that masks the best items."""
    top, _ = masked_topk(s64[:1], hist[:1], 3)
    out = [sorted(set(hist[0]) | set(int(i) for i, v in zip(top.indices[0].tolist(), top.values[0].tolist()) if v > float("-inf")))]
    return out + [list(h) for h in hist[1:]]


def topk_grid():
    for item_num in TOPK_ITEM_NUMS:
        for hidden in TOPK_HIDDEN:
            for D, L in TOPK_DL:
                for B in TOPK_BS:
                    yield item_num, hidden, D, L, B


# ---- the inputs of the multi-tile walk tests (tests/test_gpu_topk_walk.py; tests/test_topk_walk_cases.py checks them on the CPU) ----
# name -> (item_num, B, L, hidden, D, seed); see tests/din_restate.py WALK_CASES for the regimes
WALK_CASES = {
    "one split, small": (300, 512, 10, (12, 4), 16, 0),
    "one split, shipped": (300, 512, 10, (80, 40), 64, 0),
    "one split, one layer": (300, 512, 10, (12,), 16, 0),
    "short splits": (600, 128, 10, (12, 4), 16, 0),
    "limits": (257, 3, 64, (128, 128), 8, 0),
    "hidden 4": (257, 3, 64, (4,), 8, 0),
}


def walk_case(item_num, B, L, hidden, D, seed):
    """-> (P as topk_case builds it, window, histories) with walk_users' users: random pad lengths, an all-padding window (user 4: it
    reads row 0 of both tables and is ranked like any other), a history longer than 256 items, a user who keeps fewer than K items."""
    g = torch.Generator().manual_seed(1000003 * seed + 7 * item_num + 31 * B + 1009 * D + 101 * L + 13 * sum(hidden) + len(hidden))
    P = {}
    keys = names(len(hidden))
    P[WBIAS] = torch.randn(1, generator=g) * 0.1
    P[WIDE] = torch.randn(item_num, 1, generator=g) * (2.0 / (item_num + 1)) ** 0.5
    P[DEEP] = torch.randn(item_num, D, generator=g) * (2.0 / (item_num + D)) ** 0.5
    sizes = [(L + 1) * D] + list(hidden) + [1]
    for i, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        P[keys[3 + 2 * i]] = torch.randn(b, a, generator=g) * (2.0 / (a + b)) ** 0.5
        P[keys[4 + 2 * i]] = torch.randn(b, generator=g) * 0.1
    window, hist = walk_users(item_num, B, L, g)
    return P, window, hist


def scores64(P, window, device="cpu"):
    """predict_factorised on .double() parameters, on `device`."""
    return predict_factorised({k: v.to(device=device, dtype=torch.float64) for k, v in P.items()}, window.to(device)).cpu()
