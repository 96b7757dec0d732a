"""Restatement of the reference's DIN (REC/model/IDNet/din.py with SequenceAttLayer, REC/model/layers.py:460-514) in plain torch,
in whatever dtype and on whatever device the parameters are handed over: float64 is the yardstick of the tests, float32 shows how
far the reference's own arithmetic is from it.  Test infrastructure only; nothing under pixelrec_amd imports this.

    x      = cat[q, k, q - k, q * k]                                       per (candidate q, history item k_l)
    s_l    = dense(sigmoid(... sigmoid(W1 x + b1) ...)),  0 at padding,  / sqrt(D)
    score  = sum_l s_l <k_l, q>
    loss   = -mean(log(sigmoid(pos - neg) + 1e-8)) + 0.01 ||item_emb||_2 / B         (item_emb = all B (L + 2) gathered rows)
"""
import torch
import torch.nn.functional as F

TABLE = "item_embedding.weight"


def names(n_layers):
    """The reference's parameter (= state_dict) names in its order: the MLP's Linears sit at mlp_layers.{1, 4, ...}."""
    out = []
    for i in range(n_layers):
        out += [f"attention.att_mlp_layers.mlp_layers.{3 * i + 1}.weight", f"attention.att_mlp_layers.mlp_layers.{3 * i + 1}.bias"]
    return out + ["attention.dense.weight", "attention.dense.bias", TABLE]


def n_layers_of(P):
    return sum(1 for k in P if k.startswith("attention.att_mlp_layers") and k.endswith(".weight"))


def state_from(npz, prefix, dtype, device="cpu"):
    keys = [str(k) for k in npz[prefix + "keys"]]
    return {k: torch.as_tensor(npz[prefix + k]).to(device=device, dtype=dtype) for k in keys}


def attention_scores(P, q, keys, mask):
    """q [M, D], keys [M, L, D], mask bool [M, L] (True = padding) -> score [M]: layers.py:483-514 and din.py:53, literally."""
    D = q.shape[-1]
    L = keys.shape[1]
    qq = q.repeat(1, L).view(-1, L, D)
    x = torch.cat([qq, keys, qq - keys, qq * keys], dim=-1)
    for i in range(n_layers_of(P)):
        x = torch.sigmoid(x @ P[f"attention.att_mlp_layers.mlp_layers.{3 * i + 1}.weight"].T
                          + P[f"attention.att_mlp_layers.mlp_layers.{3 * i + 1}.bias"])
    out = (x @ P["attention.dense.weight"].T + P["attention.dense.bias"]).transpose(-1, -2).squeeze(1)
    out = out.masked_fill(mask, 0.0).unsqueeze(1) / (D ** 0.5)
    user = torch.matmul(out, keys).squeeze(1)
    return (user * q).sum(-1)


def loss_of(P, rows):
    rows = torch.as_tensor(rows, device=P[TABLE].device)
    emb = F.embedding(rows, P[TABLE], padding_idx=0)
    seq, pos, neg = emb[:, :-2], emb[:, -2], emb[:, -1]
    mask = rows[:, :-2] == 0
    ps, ns = attention_scores(P, pos, seq, mask), attention_scores(P, neg, seq, mask)
    mba = 0.01 * torch.norm(emb, 2) / emb.shape[0]
    return -(torch.log((ps - ns).sigmoid() + 1e-8)).mean(-1) + mba


def loss_and_grads(P, rows):
    """-> (loss as a float, {name: gradient}); the table's row 0 gets no gradient (padding_idx=0)."""
    Q = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    loss = loss_of(Q, rows)
    loss.backward()
    return float(loss.detach()), {k: v.grad.detach() for k, v in Q.items()}


def predict_literal(P, windows, chunk=4):
    """windows [B, L] -> scores [B, N]: din.py:87-103 on CandiEvalDataset's [item_num, L + 1] matrix per user, `chunk` users at a
    time."""
    table = P[TABLE]
    windows = torch.as_tensor(windows, device=table.device)
    N, D = table.shape
    out = []
    for lo in range(0, windows.shape[0], chunk):
        w = windows[lo:lo + chunk]
        b, L = w.shape
        seq = w[:, None, :].expand(b, N, L).reshape(b * N, L)
        keys = table[seq]
        cand = table[None].expand(b, N, D).reshape(b * N, D)
        out.append(attention_scores(P, cand, keys, seq == 0).view(b, N))
    return torch.cat(out)


def predict_factorised(P, windows):
    """The same scores through the factorised first Linear: A q + b1 once per item, Bm k once per window row, C (q * k) as a product
    of the item table with C scaled by the window row."""
    table = P[TABLE]
    windows = torch.as_tensor(windows, device=table.device)
    N, D = table.shape
    nl = n_layers_of(P)
    W1, b1 = P["attention.att_mlp_layers.mlp_layers.1.weight"], P["attention.att_mlp_layers.mlp_layers.1.bias"]
    A = W1[:, :D] + W1[:, 2 * D:3 * D]
    Bm = W1[:, D:2 * D] - W1[:, 2 * D:3 * D]
    C = W1[:, 3 * D:]
    aq = table @ A.T + b1                                             # [N, h1]
    k = table[windows]                                                # [B, L, D]
    bk = k @ Bm.T                                                     # [B, L, h1]
    cq = torch.einsum("nd,bld,hd->blnh", table, k, C)                 # [B, L, N, h1]
    x = torch.sigmoid(aq[None, None] + bk[:, :, None] + cq)
    for i in range(1, nl):
        x = torch.sigmoid(x @ P[f"attention.att_mlp_layers.mlp_layers.{3 * i + 1}.weight"].T
                          + P[f"attention.att_mlp_layers.mlp_layers.{3 * i + 1}.bias"])
    s = (x @ P["attention.dense.weight"].T + P["attention.dense.bias"]).squeeze(-1)          # [B, L, N]
    s = s.masked_fill((windows == 0)[:, :, None], 0.0) / (D ** 0.5)
    return (s * torch.einsum("bld,nd->bln", k, table)).sum(1)


def masked_topk(scores, windows_hist, K):
    """scores [B, N] with column 0 and every (user, history item) pair set to -inf -> torch.topk(K).  windows_hist: list of id
    lists, one per user."""
    s = scores.clone()
    s[:, 0] = float("-inf")
    for b, h in enumerate(windows_hist):
        if len(h):
            s[b, torch.as_tensor(list(h), device=s.device)] = float("-inf")
    return torch.topk(s, K, dim=-1), s


def adamw(P, batches, lr, wd):
    """torch.optim.AdamW over the reference's parameters, one step per batch; P is updated in place.  -> list of losses."""
    params = {k: torch.nn.Parameter(v.detach().clone()) for k, v in P.items()}
    opt = torch.optim.AdamW(list(params.values()), lr=lr, weight_decay=wd)
    losses = []
    for rows in batches:
        opt.zero_grad()
        loss = loss_of(params, rows)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    for k in P:
        P[k] = params[k].detach().clone()
    return losses


# ---- the inputs of the fused top-k tests (tests/test_gpu_din.py test 5; the tolerance measurement of DESIGN.md uses the same) ----
TOPK_ITEM_NUMS, TOPK_BS, TOPK_LS, TOPK_K = (13, 131, 257), (1, 3), (1, 4, 10), 10
TOPK_HIDDEN = {(16,): 8, (12, 4): 16, (80, 40): 64}          # hidden widths -> embedding_size of the case


def topk_case(item_num, B, L, hidden, seed=0):
    """-> (P float32 xavier-normal state with small random biases, window int64 [B, L], histories: one id list per user).
    User 0 has a full window; later users have padded windows (the last position always real).  Every history holds the window's
    items plus items outside it (longer than the window, masked, no part in the attention); the last user of a B = 3 batch keeps
    fewer than K items unmasked.  topk_histories() adds the float64 top-3 of user 0 to its history."""
    D = TOPK_HIDDEN[tuple(hidden)]
    g = torch.Generator().manual_seed(1000 * seed + 7 * item_num + 31 * B + L + sum(hidden))
    P = {}
    sizes = [4 * D] + list(hidden) + [1]
    keys = names(len(hidden))
    for i, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        std = (2.0 / (a + b)) ** 0.5
        P[keys[2 * i]] = torch.randn(b, a, generator=g) * std
        P[keys[2 * i + 1]] = torch.randn(b, generator=g) * 0.1
    P[TABLE] = torch.randn(item_num, D, generator=g) * (2.0 / (item_num + D)) ** 0.5
    window = torch.randint(1, item_num, (B, L), generator=g)
    for b in range(1, B):
        window[b, :min(L - 1, b)] = 0
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


# ---- the inputs of the multi-tile walk tests (tests/test_gpu_topk_walk.py; tests/test_topk_walk_cases.py checks them on the CPU) ----
WALK_K = 10
WALK_BORDERS = (127, 128, 129, 255, 256)                     # the last / first items of the 128-item tiles
WALK_KEEP = (100, 120, 127, 128, 130, 200)                   # what the "fewer than K" user keeps: two tiles, both sides of a border
WALK_STALE_USERS = range(5, 69)                              # the users walk_histories() may give a stale-bitmap item
# name -> (item_num, B, L, hidden, D, seed): the smallest shapes that reach each regime of the split rule
# n_split = min(ceil(512 / B), tiles).  Seeds: the first for which float64 alone excuses well under 2 % of the cells.
WALK_CASES = {
    "one split, small": (300, 512, 10, (12, 4), 16, 0),      # 3 tiles (the last holds 44 items), n_split 1, per 3
    "one split, shipped": (300, 512, 10, (80, 40), 64, 0),
    "short splits": (600, 128, 10, (12, 4), 16, 0),          # 5 tiles, n_split 4, per 2: the splits own 2, 2, 1, 0 tiles
    "short splits, one layer": (600, 128, 4, (16,), 8, 0),
    "limits": (257, 3, 64, (128, 128), 128, 0),              # one tile per workgroup from here on
    "hidden 5": (257, 3, 4, (5,), 16, 0),
    "hidden 127 33": (257, 3, 4, (127, 33), 16, 0),
    "hidden 1": (257, 3, 4, (1,), 16, 0),
    "chunks": (300, 5, 4, (12, 4), 16, 0),
}


def walk_users(item_num, B, L, g):
    """-> (window int64 [B, L] left-padded with 0, histories: one sorted id list per user), shared by the DIN and WideDeep cases.
    Pad lengths are random (1..L real positions) except: user 0 has a full window, user 4 an all-padding one.  Every history holds
    the window's items plus L + 3 random ones; user 1's is longer than 256 items where the catalogue allows (the stride of the
    kernels' history loop), user 2 keeps only WALK_KEEP (fewer than K items, in two tiles), user 3's holds WALK_BORDERS."""
    window = torch.randint(1, item_num, (B, L), generator=g)
    n_real = torch.randint(1, L + 1, (B,), generator=g)
    n_real[0] = L
    if B > 4:
        n_real[4] = 0
    window[torch.arange(L)[None, :] < (L - n_real)[:, None]] = 0
    hist = []
    for b in range(B):
        h = set(window[b][window[b] != 0].tolist()) | set(torch.randint(1, item_num, (L + 3,), generator=g).tolist())
        if b == 1:
            h |= set(torch.randperm(item_num - 1, generator=g)[:min(260, item_num - 30)].add(1).tolist())
        if b == 2:
            h = set(range(1, item_num)) - (set(WALK_KEEP) - h)
        if b == 3:
            h |= set(i for i in WALK_BORDERS if i < item_num)
        hist.append(sorted(h))
    return window, hist


def walk_histories(s64, hist, tol_abs, users=WALK_STALE_USERS):
    """-> (histories, stale): user 0's float64 top-3 masked (topk_histories), and for every user u of `users` whose float64 best
    unmasked item y is >= 129, the item y - 128 -- the same bit of the history bitmap one tile earlier -- added to its history,
    provided the float64 gaps at ranks 1 and 2 then exceed 2 tol_abs.  stale = [(u, y)]: y must come back at rank 1."""
    out = topk_histories(s64, hist)
    stale = []
    for u in users:
        if u >= len(out):
            break
        top, _ = masked_topk(s64[u:u + 1], out[u:u + 1], 1)
        y = int(top.indices[0, 0])
        if y < 129 or top.values[0, 0] == float("-inf") or (y - 128) in out[u]:
            continue
        h = sorted(set(out[u]) | {y - 128})
        v = masked_topk(s64[u:u + 1], [h], 3)[0].values[0]
        if float(v[0] - v[1]) > 2 * tol_abs and float(v[1] - v[2]) > 2 * tol_abs:
            out[u] = h
            stale.append((u, y))
    return out, stale


def walk_case(item_num, B, L, hidden, D, seed):
    """-> (P float32 xavier-normal state with small random biases, window, histories) -- topk_case's weights, walk_users' users."""
    g = torch.Generator().manual_seed(1000003 * seed + 7 * item_num + 31 * B + 101 * L + 13 * D + sum(hidden) + len(hidden))
    P = {}
    sizes = [4 * D] + list(hidden) + [1]
    keys = names(len(hidden))
    for i, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        P[keys[2 * i]] = torch.randn(b, a, generator=g) * (2.0 / (a + b)) ** 0.5
        P[keys[2 * i + 1]] = torch.randn(b, generator=g) * 0.1
    P[TABLE] = torch.randn(item_num, D, generator=g) * (2.0 / (item_num + D)) ** 0.5
    window, hist = walk_users(item_num, B, L, g)
    return P, window, hist


def scores64(P, window, device="cpu", chunk=32):
    """predict_factorised on .double() parameters, `chunk` users at a time ([B, L, N, h1] in float64 is large), on `device`."""
    P64 = {k: v.to(device=device, dtype=torch.float64) for k, v in P.items()}
    return torch.cat([predict_factorised(P64, window[lo:lo + chunk].to(device)) for lo in range(0, window.shape[0], chunk)]).cpu()
