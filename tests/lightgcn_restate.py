"""A float64 NumPy restatement of the reference's LightGCN (REC/model/IDNet/lightgcn.py, layers.py:13-22) for the tests -- written
from its arithmetic: E_final = mean(E_0 .. E_K) with E_{k+1} = A E_k over the CSR of data.dataload.norm_adj_csr, the pair loss
-mean(1e-8 + log sigmoid(<u, i+> - <u, i->)) and its gradient (A is symmetric: d E_0 = (1/(K+1)) sum_k A^k G_final), and
torch.optim.AdamW's update."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp


def csr_matrix(row_ptr, col, w, n=None):
    n = len(row_ptr) - 1 if n is None else n
    return sp.csr_matrix((np.asarray(w, np.float64), np.asarray(col, np.int64), np.asarray(row_ptr, np.int64)), shape=(n, n))


def propagate(A, e0, K):
    e, acc = e0, e0.copy()
    for _ in range(K):
        e = A @ e
        acc = acc + e
    return acc / (K + 1)


def log_sigmoid(x):
    return np.minimum(x, 0.0) - np.log1p(np.exp(-np.abs(x)))


def sigmoid_neg(x):
    """1 - sigmoid(x), without cancellation."""
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, e / (1.0 + e), 1.0 / (1.0 + e))


def pair_head(ef, U, user, item):
    """-> (loss, x [B], coef [B] = d loss / d x, G_final)."""
    u, p, n = ef[user], ef[U + item[:, 0]], ef[U + item[:, 1]]
    x = (u * p).sum(-1) - (u * n).sum(-1)
    B = len(user)
    loss = float(np.mean(-(1e-8 + log_sigmoid(x))))
    coef = -sigmoid_neg(x) / B
    g = np.zeros_like(ef)
    np.add.at(g, user, coef[:, None] * (p - n))
    np.add.at(g, U + item[:, 0], coef[:, None] * u)
    np.add.at(g, U + item[:, 1], -coef[:, None] * u)
    return loss, x, coef, g


def loss_and_grad(A, e0, K, U, user, item):
    """-> (loss, d loss / d E_0)."""
    ef = propagate(A, e0, K)
    loss, _, _, g = pair_head(ef, U, user, item)
    return loss, propagate(A, g, K)


class AdamW:
    """torch.optim.AdamW (decoupled weight decay, bias-corrected moments) on one float64 array."""

    def __init__(self, lr, wd, betas=(0.9, 0.999), eps=1e-8):
        self.lr, self.wd, self.b1, self.b2, self.eps = lr, wd, betas[0], betas[1], eps
        self.t, self.m, self.v = 0, None, None

    def step(self, p, g):
        if self.m is None:
            self.m, self.v = np.zeros_like(p), np.zeros_like(p)
        self.t += 1
        p = p * (1.0 - self.lr * self.wd)
        self.m = self.b1 * self.m + (1 - self.b1) * g
        self.v = self.b2 * self.v + (1 - self.b2) * g * g
        mh = self.m / (1 - self.b1 ** self.t)
        vh = self.v / (1 - self.b2 ** self.t)
        return p - self.lr * mh / (np.sqrt(vh) + self.eps)
