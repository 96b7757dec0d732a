"""A plain-PyTorch fp32 restatement of the reference's BERT4Rec (REC/model/IDNet/bert4rec.py) for the tests -- written from its
arithmetic, on the shared encoder layer of oracle.sasrec_oracle.  Parameters are a dict keyed like the reference's state_dict
(item_embedding.weight has item_num + 1 rows: row item_num is the mask token; position_embedding.weight has L + 1 rows)."""
from __future__ import annotations

import numpy as np
import torch

from oracle import sasrec_oracle as O


def padding_mask(seq):
    """get_attention_mask (bert4rec.py:150-155): 0 on real keys, -1e9 on keys that are 0; no causal term.  [B,1,1,L] fp32."""
    return torch.where((seq != 0)[:, None, None, :], 0.0, -1e9)


def encode(p, seq, cfg):
    """ids [B, P] -> last-layer states [B, P, D] (bert4rec.py:76-90 / :118-131), dropout off."""
    P = seq.shape[1]
    x = p["item_embedding.weight"][seq] + p["position_embedding.weight"][:P][None]
    h = O.layer_norm(x, p["LayerNorm.weight"], p["LayerNorm.bias"], cfg["layer_norm_eps"])
    mask = padding_mask(seq)
    for i in range(cfg["n_layers"]):
        h = O.encoder_layer(p, i, h, mask, cfg["n_heads"], cfg["layer_norm_eps"], act=cfg.get("hidden_act", "gelu"))
    return h


def forward_loss(p, items, masked_index, cfg):
    """items [B, 3, P] (masked | original | negatives), masked_index [B, P] -> sum_masked -log(1e-8 + sigmoid(pos - neg)) / B."""
    out = encode(p, items[:, 0], cfg)
    E = p["item_embedding.weight"]
    sel = masked_index != 0
    pos = (out * E[items[:, 1]]).sum(-1)[sel]
    neg = (out * E[items[:, 2]]).sum(-1)[sel]
    return -(torch.log(1e-8 + torch.sigmoid(pos - neg))).sum(-1) / masked_index.shape[0]


def loss_and_grads(p, items, masked_index, cfg):
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    loss = forward_loss(leaf, items, masked_index, cfg)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}
    grads["item_embedding.weight"][0].zero_()          # padding_idx=0
    return loss.detach(), grads


@torch.no_grad()
def predict(p, item_seq, item_feature, cfg, mask_token):
    """Append the mask token, encode L+1 positions, score the last one (bert4rec.py:115-135)."""
    seq = torch.cat((item_seq, torch.full((item_seq.shape[0], 1), mask_token, dtype=item_seq.dtype)), dim=-1)
    return encode(p, seq, cfg)[:, -1] @ item_feature.t()


def adamw_trajectory(p, batches, cfg, lr=1e-4, weight_decay=0.1):
    """torch.optim.AdamW over the restatement, one step per (items, masked_index): -> (losses, parameters after the last)."""
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    opt = torch.optim.AdamW(list(leaf.values()), lr=lr, weight_decay=weight_decay)
    losses = []
    for items, mask in batches:
        opt.zero_grad()
        loss = forward_loss(leaf, items, mask, cfg)
        loss.backward()
        leaf["item_embedding.weight"].grad[0].zero_()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: v.detach() for k, v in leaf.items()}


def golden_params(g):
    """The state_dict stored in tests/golden/bert4rec_tiny.npz."""
    return {k[3:]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith("sd.")}
