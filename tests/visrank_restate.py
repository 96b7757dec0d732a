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
