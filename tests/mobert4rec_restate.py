"""Restatement of the reference's MOBERT4Rec head (REC/model/PixelNet/mobert4rec.py:87-111 and :113-132) over rows of an encoder
output E, in plain torch, in whatever dtype and on whatever device the parameters are handed over: float64 is the yardstick of the
tests, float32 shows how far the reference's own arithmetic is from it.  A thin wrapper: the head IS tests/bert4rec_restate.py's
forward_loss with item_embedding.weight := E.  Test infrastructure only; nothing under pixelrec_amd imports this.

    x_t  = LayerNorm(E[index[b,0,t]] + position_embedding[t]) -> TransformerEncoder (a key is real where index[b,0,t] != 0)
    loss = sum over masked_index != 0 of -log(1e-8 + sigmoid(<out_t, E[index[b,1,t]]> - <out_t, E[index[b,2,t]]>)) / B
"""
import numpy as np
import torch

from tests import bert4rec_restate as B4

E_KEY = "E"
TABLE = "item_embedding.weight"


def names(n_layers):
    """The reference's block parameter names in its registration order (mobert4rec.py:35-47)."""
    out = ["position_embedding.weight"]
    for i in range(n_layers):
        a, f = f"trm_encoder.layer.{i}.multi_head_attention.", f"trm_encoder.layer.{i}.feed_forward."
        for mod in ("query", "key", "value", "dense", "LayerNorm"):
            out += [a + mod + ".weight", a + mod + ".bias"]
        for mod in ("dense_1", "dense_2", "LayerNorm"):
            out += [f + mod + ".weight", f + mod + ".bias"]
    return out + ["LayerNorm.weight", "LayerNorm.bias"]


def loss_of(P, E, index, masked_index, cfg):
    """P: the block tensors by the reference's names; E [M, D]; index int [B, 3, P] positions into E; masked_index [B, P]
    -> 0-dim loss."""
    index = torch.as_tensor(index, device=E.device)
    masked_index = torch.as_tensor(masked_index, device=E.device)
    return B4.forward_loss({**P, TABLE: E}, index, masked_index, cfg)


def loss_and_grads(P, E, index, masked_index, cfg):
    """-> (loss as a float, {name: gradient}) with the gradient of E under E_KEY (rows nobody reads come out as exact zeros; row 0
    keeps what autograd gives it -- the reference has no padding_idx here)."""
    Q = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    Ex = E.detach().clone().requires_grad_(True)
    loss = loss_of(Q, Ex, index, masked_index, cfg)
    loss.backward()
    grads = {k: (v.grad.detach() if v.grad is not None else torch.zeros_like(v)) for k, v in Q.items()}
    grads[E_KEY] = Ex.grad.detach() if Ex.grad is not None else torch.zeros_like(Ex)
    return float(loss.detach()), grads


def reference_positions(input_ids, masked_index):
    """The reference's one image per (position, input | positive | negative) behind a zero image, as positions [B, 3, P]: input
    (b, t) at 1 + 3 (b P + t) where input_ids != 0, its positive / negative at + 1 / + 2 where masked_index != 0, 0 elsewhere."""
    input_ids, masked_index = torch.as_tensor(input_ids), torch.as_tensor(masked_index)
    B, P = input_ids.shape
    out = torch.zeros(B, 3, P, dtype=torch.int64)
    for b in range(B):
        for t in range(P):
            base = 1 + 3 * (b * P + t)
            if int(input_ids[b, t]) != 0:
                out[b, 0, t] = base
            if int(masked_index[b, t]) != 0:
                out[b, 1, t], out[b, 2, t] = base + 1, base + 2
    return out


@torch.no_grad()
def predict(P, item_feature, item_seq, cfg, item_num):
    """scores [B, item_num]: the mask row item_feature[item_num] appended to the window, P positions encoded, the last one scored
    against item_feature[:item_num] (mobert4rec.py:113-132)."""
    item_seq = torch.as_tensor(item_seq, device=item_feature.device)
    seq = torch.cat((item_seq, torch.full((item_seq.shape[0], 1), item_num, dtype=item_seq.dtype, device=item_seq.device)), dim=-1)
    return B4.encode({**P, TABLE: item_feature}, seq, cfg)[:, -1] @ item_feature[:item_num].t()


def golden_state(g):
    """The state_dict stored in tests/golden/mobert4rec_tiny.npz, in the reference's key order: the floating tensors are held as
    int16 = 1024 x weight (every weight is a multiple of 2^-10), which this undoes exactly."""
    out = {}
    for k in g["sd.keys"]:
        a = np.asarray(g["sd." + str(k)])
        out[str(k)] = torch.from_numpy(a.astype(np.float32) / 1024) if a.dtype == np.int16 else torch.from_numpy(a.copy())
    return out


def golden_store(g):
    """The store's normalised images fp32 [item_num, 3, H, W] (held as int8 = 16 x pixel; row 0 the zero image)."""
    return torch.from_numpy(np.asarray(g["store"]).astype(np.float32) / 16)
