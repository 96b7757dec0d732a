"""Torch restatement of MOSRGNN's head (reference code/REC/model/PixelNet/mosrgnn.py) in any dtype, under autograd: the session
graph from srgnn_restate.session_graph (the collate's rule at L nodes), H_0 = E[nodes], the gated cells, the attention readout
and the pair loss, with E [M, D] -- the encoder's rows, each image encoded once -- in the item table's place.  P maps the
reference's parameter names (NAMES: gnn.* without linear_edge_f, then the four Linears) to tensors of E's dtype."""
from __future__ import annotations

import numpy as np
import torch

from tests import srgnn_restate as SR

E_KEY = "E"
NAMES = ["gnn.w_ih", "gnn.w_hh", "gnn.b_ih", "gnn.b_hh", "gnn.b_iah", "gnn.b_oah", "gnn.linear_edge_in.weight",
         "gnn.linear_edge_in.bias", "gnn.linear_edge_out.weight", "gnn.linear_edge_out.bias", "linear_one.weight", "linear_one.bias",
         "linear_two.weight", "linear_two.bias", "linear_three.weight", "linear_transform.weight", "linear_transform.bias"]
EDGE_F = ["gnn.linear_edge_f.weight", "gnn.linear_edge_f.bias"]


def shapes(D):
    """{name: shape} of NAMES at embedding_size D."""
    return {"gnn.w_ih": (3 * D, 2 * D), "gnn.w_hh": (3 * D, D), "gnn.b_ih": (3 * D,), "gnn.b_hh": (3 * D,), "gnn.b_iah": (D,),
            "gnn.b_oah": (D,), "gnn.linear_edge_in.weight": (D, D), "gnn.linear_edge_in.bias": (D,),
            "gnn.linear_edge_out.weight": (D, D), "gnn.linear_edge_out.bias": (D,), "linear_one.weight": (D, D),
            "linear_one.bias": (D,), "linear_two.weight": (D, D), "linear_two.bias": (D,), "linear_three.weight": (1, D),
            "linear_transform.weight": (D, 2 * D), "linear_transform.bias": (D,)}


def encode(P, E, item_seq, step):
    """item_seq [B, L] int positions into E (right-padded with 0) -> out [B, D] = linear_transform([a | ht])."""
    seq = np.asarray(item_seq, dtype=np.int64)
    B, L = seq.shape
    D = E.shape[1]
    nodes, alias, A = SR.session_graph(seq)
    mask = seq != 0
    dev = E.device
    last = torch.from_numpy(SR.last_index(mask.astype(np.int64))).to(dev)
    A = torch.from_numpy(A).to(device=dev, dtype=E.dtype)
    Ain, Aout = A[:, :, :L], A[:, :, L:]
    H = E[torch.from_numpy(nodes).to(dev)]                                             # [B, L, D]
    for _ in range(step):
        Ein = H @ P["gnn.linear_edge_in.weight"].T + P["gnn.linear_edge_in.bias"]
        Eout = H @ P["gnn.linear_edge_out.weight"].T + P["gnn.linear_edge_out.bias"]
        X = torch.cat((Ain @ Ein + P["gnn.b_iah"], Aout @ Eout + P["gnn.b_oah"]), dim=2)
        gi = X @ P["gnn.w_ih"].T + P["gnn.b_ih"]
        gh = H @ P["gnn.w_hh"].T + P["gnn.b_hh"]
        r = torch.sigmoid(gi[..., :D] + gh[..., :D])
        z = torch.sigmoid(gi[..., D:2 * D] + gh[..., D:2 * D])
        n = torch.tanh(gi[..., 2 * D:] + r * gh[..., 2 * D:])
        H = n + z * (H - n)
    bidx = torch.arange(B, device=dev)
    sh = H[bidx[:, None], torch.from_numpy(alias).to(dev)]                             # [B, L, D]
    ht = sh[bidx, last]
    q1 = ht @ P["linear_one.weight"].T + P["linear_one.bias"]
    q2 = sh @ P["linear_two.weight"].T + P["linear_two.bias"]
    alpha = torch.sigmoid(q1[:, None, :] + q2) @ P["linear_three.weight"].T            # [B, L, 1]
    a = (alpha * sh * torch.from_numpy(mask).to(device=dev, dtype=E.dtype)[..., None]).sum(1)
    return torch.cat((a, ht), dim=1) @ P["linear_transform.weight"].T + P["linear_transform.bias"]


def loss_of(P, E, item_seq, target, step):
    """-> 0-dim loss = -mean(1e-8 + log sigmoid(<out, E[p]> - <out, E[n]>)) (mosrgnn.py:71-73)."""
    out = encode(P, E, item_seq, step)
    t = torch.from_numpy(np.asarray(target, dtype=np.int64)).to(E.device)
    x = (out * E[t[:, 0]]).sum(-1) - (out * E[t[:, 1]]).sum(-1)
    return -torch.mean(1e-8 + torch.log(torch.sigmoid(x)))


def loss_and_grads(P, E, item_seq, target, step):
    """-> (loss as a 0-dim tensor, {name: gradient} for NAMES and E_KEY), all in E's dtype."""
    Q = {k: v.detach().clone().requires_grad_(True) for k, v in P.items() if k in NAMES}
    Eg = E.detach().clone().requires_grad_(True)
    loss = loss_of(Q, Eg, item_seq, target, step)
    loss.backward()
    grads = {k: v.grad for k, v in Q.items()}
    grads[E_KEY] = Eg.grad
    return loss.detach(), grads


def predict(P, feat, item_seq, step):
    """scores [B, N] = encode(...) feat^T (mosrgnn.py:77-83)."""
    return encode(P, feat, item_seq, step) @ feat.T
