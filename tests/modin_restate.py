"""Restatement of the reference's MODIN head (REC/model/PixelNet/modin.py:49-61 and :66-82 with SequenceAttLayer,
REC/model/layers.py:460-514) over rows of an encoder output E, in plain torch, in whatever dtype and on whatever device the
parameters are handed over: float64 is the yardstick of the tests, float32 shows how far the reference's own arithmetic is from it.
The attention is tests/din_restate.py's, by import.  Test infrastructure only; nothing under pixelrec_amd imports this.

    emb    = E[index]                                  index [S, L + 2] = [profile | positive | negative] positions, 0 = "no item"
    score  = sum_l s_l <k_l, q>                        s_l = 0 where the profile position is 0 (it still READS E[0])
    loss   = -mean(log(sigmoid(pos - neg) + 1e-8))     NO regulariser (modin.py:61)
"""
import torch

from tests.din_restate import attention_scores, n_layers_of  # noqa: F401

E_KEY = "E"


def names(n_layers):
    """The reference's attention parameter names in its order: the MLP's Linears sit at mlp_layers.{1, 4, ...}."""
    out = []
    for i in range(n_layers):
        out += [f"attention.att_mlp_layers.mlp_layers.{3 * i + 1}.weight", f"attention.att_mlp_layers.mlp_layers.{3 * i + 1}.bias"]
    return out + ["attention.dense.weight", "attention.dense.bias"]


def loss_of(P, E, index):
    """P: the attention tensors by the reference's names; E [M, D]; index int [S, L + 2] -> 0-dim loss (modin.py:49-61)."""
    index = torch.as_tensor(index, device=E.device)
    emb = E[index]
    seq, pos, neg = emb[:, :-2], emb[:, -2], emb[:, -1]
    mask = index[:, :-2] == 0
    ps, ns = attention_scores(P, pos, seq, mask), attention_scores(P, neg, seq, mask)
    return -(torch.log((ps - ns).sigmoid() + 1e-8)).mean(-1)


def loss_and_grads(P, E, index):
    """-> (loss as a float, {name: gradient}) with the gradient of E under E_KEY (rows nobody reads, and row 0 where it is only
    read under the mask, come out as exact zeros)."""
    Q = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    Ex = E.detach().clone().requires_grad_(True)
    loss = loss_of(Q, Ex, index)
    loss.backward()
    grads = {k: v.grad.detach() for k, v in Q.items()}
    grads[E_KEY] = Ex.grad.detach()
    return float(loss.detach()), grads


def reference_form(windows, item_num):
    """CandiEvalDataset's id tensor [B, item_num, L + 1]: the window repeated per candidate, the candidate id last."""
    windows = torch.as_tensor(windows)
    B, L = windows.shape
    cand = torch.arange(item_num, dtype=windows.dtype)[None, :, None].expand(B, item_num, 1)
    return torch.cat((windows[:, None, :].expand(B, item_num, L), cand), dim=-1)


def predict(P, feat, item_seq, chunk=4):
    """scores [B, N] over the item matrix feat [N, D] (modin.py:66-82).  item_seq: the reference's [B, N, L + 1] id tensor, or
    [B, L] windows (expanded to that form); `chunk` users at a time."""
    item_seq = torch.as_tensor(item_seq, device=feat.device)
    N, D = feat.shape
    if item_seq.dim() == 2:
        item_seq = reference_form(item_seq.cpu(), N).to(feat.device)
    out = []
    for lo in range(0, item_seq.shape[0], chunk):
        blk = item_seq[lo:lo + chunk]
        b = blk.shape[0]
        flat = blk.flatten(0, 1)
        emb = feat[flat]
        user_seq, cand = emb[:, :-1], emb[:, -1]
        out.append(attention_scores(P, cand, user_seq, flat[:, :-1] == 0).view(b, -1))
    return torch.cat(out)
