"""Float64 NumPy restatement of SRGNN (reference code/REC/model/IDNet/srgnn.py with collate_fn.graph_train_collate's session
graph): the graph at a chosen node count, the gated GNN cell, the attention readout, the pair loss and every gradient by hand.
Parameters are a dict of reference state_dict names -> arrays; gnn.linear_edge_f is read by nothing and gets no gradient."""
from __future__ import annotations

import numpy as np


def session_graph(seq, n_nodes=None):
    """seq [B, L] int (right-padded with 0) -> (nodes [B, n], alias [B, L], A [B, n, 2n] float64), padded to n_nodes (default L)
    nodes: the collate's rule (distinct ids ascending, then 0), with the padding to n instead of the batch's largest count."""
    seq = np.asarray(seq, dtype=np.int64)
    B, L = seq.shape
    n = L if n_nodes is None else int(n_nodes)
    nodes = np.zeros((B, n), dtype=np.int64)
    alias = np.zeros((B, L), dtype=np.int64)
    A = np.zeros((B, n, 2 * n))
    for b in range(B):
        u = np.unique(seq[b])
        assert len(u) <= n, "n_nodes below the session's distinct ids"
        nodes[b, :len(u)] = u
        alias[b] = np.searchsorted(u, seq[b])
        adj = np.zeros((n, n))
        for i in range(L - 1):
            if seq[b, i + 1] == 0:
                break
            adj[alias[b, i], alias[b, i + 1]] = 1.0
        indeg = adj.sum(0)
        outdeg = adj.sum(1)
        indeg[indeg == 0] = 1.0
        outdeg[outdeg == 0] = 1.0
        A[b, :, :n] = (adj / indeg[None, :]).T          # A_in[v][u] = adj[u][v] / indeg(v)
        A[b, :, n:] = adj / outdeg[:, None]             # A_out[u][v] = adj[u][v] / outdeg(u)
    return nodes, alias, A


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def last_index(mask):
    """sum(mask) - 1 with torch's wrap of -1 to the last slot (an empty history)."""
    L = mask.shape[1]
    last = mask.sum(1).astype(np.int64) - 1
    return np.where(last < 0, last + L, last)


def forward_backward(P, item_seq, mask, target, step, n_nodes=None, want_grad=True):
    """-> (loss, grads {name: array}, extras).  P: reference state_dict (float64 arrays)."""
    P = {k: np.asarray(v, dtype=np.float64) for k, v in P.items()}
    item_seq = np.asarray(item_seq, dtype=np.int64)
    mask = np.asarray(mask, dtype=np.int64)
    target = np.asarray(target, dtype=np.int64)
    B, L = item_seq.shape
    emb = P["embedding.weight"]
    D = emb.shape[1]
    nodes, alias, A = session_graph(item_seq, n_nodes)
    n = nodes.shape[1]
    Ain, Aout = A[:, :, :n], A[:, :, n:]
    Wei, bei = P["gnn.linear_edge_in.weight"], P["gnn.linear_edge_in.bias"]
    Weo, beo = P["gnn.linear_edge_out.weight"], P["gnn.linear_edge_out.bias"]
    Wih, Whh, bih, bhh = P["gnn.w_ih"], P["gnn.w_hh"], P["gnn.b_ih"], P["gnn.b_hh"]
    biah, boah = P["gnn.b_iah"], P["gnn.b_oah"]
    H = emb[nodes]
    cache = []
    for _ in range(step):
        Ein = H @ Wei.T + bei
        Eout = H @ Weo.T + beo
        X = np.concatenate([Ain @ Ein + biah, Aout @ Eout + boah], axis=2)
        gi = X @ Wih.T + bih
        gh = H @ Whh.T + bhh
        r = _sig(gi[..., :D] + gh[..., :D])
        z = _sig(gi[..., D:2 * D] + gh[..., D:2 * D])
        nn_ = np.tanh(gi[..., 2 * D:] + r * gh[..., 2 * D:])
        Hy = nn_ + z * (H - nn_)
        cache.append((H, X, gh, r, z, nn_))
        H = Hy
    Hn = H
    bidx = np.arange(B)
    sh = Hn[bidx[:, None], alias]                                   # [B, L, D]
    last = last_index(mask)
    ht = sh[bidx, last]
    W1, b1, W2, b2 = P["linear_one.weight"], P["linear_one.bias"], P["linear_two.weight"], P["linear_two.bias"]
    w3 = P["linear_three.weight"]
    Wt, bt = P["linear_transform.weight"], P["linear_transform.bias"]
    q1 = ht @ W1.T + b1
    q2 = sh @ W2.T + b2
    s = _sig(q1[:, None, :] + q2)
    alpha = (s @ w3.T)[..., 0]                                      # [B, L]
    mf = mask.astype(np.float64)
    a = (alpha[..., None] * sh * mf[..., None]).sum(1)
    cat = np.concatenate([a, ht], axis=1)
    o = cat @ Wt.T + bt
    ep, en = emb[target[:, 0]], emb[target[:, 1]]
    x = (o * ep).sum(1) - (o * en).sum(1)
    loss = -np.mean(1e-8 + np.log(_sig(x)))
    extras = dict(nodes=nodes, alias=alias, A=A, out=o, cat=cat, alpha=alpha, Hn=Hn)
    if not want_grad:
        return loss, None, extras
    G = {k: np.zeros_like(v) for k, v in P.items() if not k.startswith("gnn.linear_edge_f")}
    dx = -(1.0 - _sig(x)) / B
    do = dx[:, None] * (ep - en)
    np.add.at(G["embedding.weight"], target[:, 0], dx[:, None] * o)
    np.add.at(G["embedding.weight"], target[:, 1], -dx[:, None] * o)
    G["linear_transform.weight"] = do.T @ cat
    G["linear_transform.bias"] = do.sum(0)
    dcat = do @ Wt
    da, dht = dcat[:, :D], dcat[:, D:].copy()
    dalpha = mf * (da[:, None, :] * sh).sum(-1)
    dsh = (alpha * mf)[..., None] * da[:, None, :]
    G["linear_three.weight"] = (dalpha[..., None] * s).sum((0, 1))[None, :]
    dpre = dalpha[..., None] * w3[0] * s * (1.0 - s)
    G["linear_two.weight"] = np.einsum("bti,btj->ij", dpre, sh)
    G["linear_two.bias"] = dpre.sum((0, 1))
    dsh += dpre @ W2
    dq1 = dpre.sum(1)
    G["linear_one.weight"] = dq1.T @ ht
    G["linear_one.bias"] = dq1.sum(0)
    dht += dq1 @ W1
    dsh[bidx, last] += dht
    dH = np.zeros_like(Hn)
    for b in range(B):
        np.add.at(dH[b], alias[b], dsh[b])
    for Hp, X, gh, r, z, nn_ in reversed(cache):
        dnn = dH * (1.0 - z)
        dz = dH * (Hp - nn_)
        dh = dH * z
        dpn = dnn * (1.0 - nn_ ** 2)
        dr = dpn * gh[..., 2 * D:]
        dpz = dz * z * (1.0 - z)
        dpr = dr * r * (1.0 - r)
        dgi = np.concatenate([dpr, dpz, dpn], axis=2)
        dgh = np.concatenate([dpr, dpz, dpn * r], axis=2)
        G["gnn.w_ih"] += np.einsum("bni,bnj->ij", dgi, X)
        G["gnn.b_ih"] += dgi.sum((0, 1))
        G["gnn.w_hh"] += np.einsum("bni,bnj->ij", dgh, Hp)
        G["gnn.b_hh"] += dgh.sum((0, 1))
        dh += dgh @ Whh
        dX = dgi @ Wih
        din, dout = dX[..., :D], dX[..., D:]
        G["gnn.b_iah"] += din.sum((0, 1))
        G["gnn.b_oah"] += dout.sum((0, 1))
        dEin = np.transpose(Ain, (0, 2, 1)) @ din
        dEout = np.transpose(Aout, (0, 2, 1)) @ dout
        G["gnn.linear_edge_in.weight"] += np.einsum("bni,bnj->ij", dEin, Hp)
        G["gnn.linear_edge_in.bias"] += dEin.sum((0, 1))
        G["gnn.linear_edge_out.weight"] += np.einsum("bni,bnj->ij", dEout, Hp)
        G["gnn.linear_edge_out.bias"] += dEout.sum((0, 1))
        dh += dEin @ Wei + dEout @ Weo
        dH = dh
    for b in range(B):
        np.add.at(G["embedding.weight"], nodes[b], dH[b])
    return loss, G, extras


def predict(P, item_seq, step, n_nodes=None):
    """scores [B, N] of srgnn.py predict (mask = item_seq != 0 for right-padded histories)."""
    item_seq = np.asarray(item_seq, dtype=np.int64)
    B = item_seq.shape[0]
    mask = (item_seq != 0).astype(np.int64)
    _, _, ex = forward_backward(P, item_seq, mask, np.ones((B, 2), dtype=np.int64), step, n_nodes, want_grad=False)
    return ex["out"] @ np.asarray(P["embedding.weight"], dtype=np.float64).T
