"""VISRANK restated in float64 from the formulas (visrank.py predict, trainer.py:333-336 masks, collector's torch.topk).  Per user
with the full history `hist`:

    w = hist[-window:]                                  h = len(w)
    S[r, j] = <v[w[r]], v[j]> / (max(|v[w[r]]|, eps) max(|v[j]|, eps))          eps = 1e-8, row 0 of v as loaded
    k = min(top_num, h) (average_top_k) | 1 (maximum) | h (anything else)
    score[j] = mean of the k largest of S[:, j];   score[0] = -inf
    masked[j] = -inf for j = 0 and every j in hist (the FULL history);   top-K of masked, descending
"""
import numpy as np

EPS = 1e-8


def tol(F: int) -> float:
    """2 (F + 8) 2^-24: the worst-case bound gamma_F on an fp32 dot product of two unit vectors plus a few ulps per operand for
    the normalisation, doubled.  Derived, not measured."""
    return 2.0 * (F + 8) * 2.0 ** -24


def choose_k(method, top_num, h: int) -> int:
    if method == "average_top_k":
        return min(int(top_num), h)
    if method == "maximum":
        return 1
    return h


def unit_rows(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.maximum(np.sqrt((v * v).sum(1, keepdims=True)), EPS)


def scores(v, hist, method, top_num=None, window=50, unit=None):
    """float64 [item_num]: steps 1-5 (score[0] = -inf, history not masked yet)."""
    u = unit_rows(v) if unit is None else unit
    w = np.asarray(hist, dtype=np.int64)[-window:]
    h = len(w)
    if h == 0:
        raise ValueError("the mean of nothing")
    S = u[w] @ u.T                                             # [h, N]
    k = choose_k(method, top_num, h)
    top = -np.sort(-S, axis=0)[:k]
    s = top.mean(0)
    s[0] = -np.inf
    return s


def masked_scores(v, hist, method, top_num=None, window=50, unit=None):
    """Step 6: column 0 and every item of the FULL history at -inf."""
    s = scores(v, hist, method, top_num, window, unit)
    s[np.asarray(hist, dtype=np.int64)] = -np.inf
    return s


def topk(v, hist, K, method, top_num=None, window=50, unit=None):
    """-> (ids [K], values [K], the masked float64 scores), descending; ties by ascending id."""
    s = masked_scores(v, hist, method, top_num, window, unit)
    order = np.lexsort((np.arange(len(s)), -s))[:K]
    return order, s[order], s


def metrics(ids, targets, ks=(5, 10)):
    """Recall@k / NDCG@k of the id lists [U, K] against one target per user (evaluator/metrics.py with one positive)."""
    ids, targets = np.asarray(ids), np.asarray(targets)
    hit = ids == targets[:, None]
    out = {}
    for k in ks:
        hk = hit[:, :k]
        out[f"recall@{k}"] = float(hk.any(1).mean())
        rank = np.where(hk.any(1), hk.argmax(1), 0)
        out[f"ndcg@{k}"] = float(np.where(hk.any(1), 1.0 / np.log2(rank + 2.0), 0.0).mean())
    return out


# ---- the inputs of the multi-tile walk tests (tests/test_gpu_topk_walk.py; tests/test_topk_walk_cases.py checks them on the CPU) ----
WALK_H, WALK_K = 50, 10
WALK_BORDERS = (127, 128, 129, 255, 256)                     # the last / first items of the 128-item tiles
WALK_KEEP = (100, 120, 127, 128, 130, 200)                   # what the "fewer than K" user keeps: two tiles, both sides of a border
WALK_STALE_USERS = range(5, 69)                              # the users walk_histories() may give a stale-bitmap item
# name -> (B, N, F, seed): the smallest shapes that reach each regime of n_split = min(ceil(512 / ceil(B / 2)), tiles)
WALK_CASES = {
    "one split": (1024, 300, 12, 0),                         # 3 tiles, n_split 1, per 3
    "short splits": (256, 600, 12, 0),                       # 5 tiles, n_split 4, per 2: the splits own 2, 2, 1, 0 tiles
    "short splits, odd batch": (255, 600, 12, 0),            # the last 2-user row block holds one user
}


def method_of(top_k):
    return ("mean", None) if top_k == 0 else (("maximum", None) if top_k == 1 else ("average_top_k", top_k))


def walk_case(B, N, F, seed, H=WALK_H):
    """-> (features float32 [N, F], histories: one id array per user, 1..89 items).  User 0 and WALK_STALE_USERS have at least H
    items (an item put in front of such a history stays outside the window), user 1's history is longer than 256 items (the
    stride of the kernel's history loop), user 2 keeps only WALK_KEEP (fewer than K items, in two tiles), user 3's starts with
    WALK_BORDERS."""
    rng = np.random.default_rng(1000 * seed + 7 * B + N + F)
    v = rng.standard_normal((N, F)).astype(np.float32)
    lens = rng.integers(1, 90, size=B)
    lens[0] = 60
    for u in WALK_STALE_USERS:
        lens[u] = rng.integers(H, 90)
    hists = [rng.integers(1, N, size=int(n)) for n in lens]
    hists[1] = rng.permutation(np.arange(1, N))[:min(260, N - 30)]
    hists[2] = rng.permutation(np.array([i for i in range(1, N) if i not in WALK_KEEP]))
    hists[3] = np.concatenate((np.array(WALK_BORDERS), hists[3]))
    return v, hists


def walk_histories(v, hists, top_k, unit, H=WALK_H, users=WALK_STALE_USERS):
    """-> (histories, stale) for one reduction: user 0's float64 top-3 put in front of its history (masked, outside the window),
    and for every user u of `users` whose float64 best unmasked item y is >= 129 the item y - 128 -- the same bit of the history
    bitmap one tile earlier -- put in front of its history, provided the float64 gaps at ranks 1 and 2 then exceed 2 tol(F).
    stale = [(u, y)]: y must come back at rank 1."""
    method, top_num = method_of(top_k)
    F = v.shape[1]
    out = [np.asarray(h) for h in hists]
    assert len(out[0]) >= H
    out[0] = np.concatenate((topk(v, out[0], 3, method, top_num, H, unit)[0], out[0]))
    stale = []
    for u in users:
        h = out[u]
        assert len(h) >= H
        y = int(topk(v, h, 1, method, top_num, H, unit)[0][0])
        if y < 129 or (y - 128) in h:
            continue
        h2 = np.concatenate((np.array([y - 128]), h))
        vals = topk(v, h2, 3, method, top_num, H, unit)[1]
        if vals[0] - vals[1] > 2 * tol(F) and vals[1] - vals[2] > 2 * tol(F):
            out[u] = h2
            stale.append((u, y))
    return out, stale
