"""VISRANK (ViNet) -- drop-in for `REC.model.ViNet.visrank.VISRANK` (code/REC/model/ViNet/visrank.py): training-free visual
ranking on the frozen features v_feat [I, F].  Per user with the full history `hist` (valid: user_seq[:-2], test: [:-1]):

    w = hist[-history_window:]   (the reference hard-codes 50)        h = len(w)
    S[r, j] = cosine_similarity(v_feat[w[r]], v_feat[j])             float32, eps 1e-8; row 0 of v_feat is used as loaded
    score[j] = mean of the k largest of S[:, j]                       k = min(top_num, h) | 1 | h   (method average_top_k | maximum | other)
    score[0] = -inf

There is nothing to train: `forward` returns None, the only parameter is the reference's zero-size `placeholder`, and
`compute_item_all` returns None.

Two evaluation paths:
  * `fused_topk_batch(window, hist_ptr, hist_items, K)`: csrc/visrank.hip -- the rows of v_feat are normalised once
    (`ops.visrank_unit_rows`), then one fused launch per batch scores every item against every window row on the fp32-operand
    MFMA, reduces over the window, applies the masks and keeps the top K; the [B h, I] similarities never reach memory.
    Taken when the reduction keeps at most 16 values (top_num <= 16, maximum) or all of them (top_num >= history_window, mean).
  * `predict(user, item_feature)`: the literal path (`eval_fused_topk: False`, or top_num in 17..window-1) through the
    library GEMM and torch ops.  `user` is the reference's 1-D unpadded history -> [I], or a [B, H] window batch left-padded with
    0 -> [B, I].

Contract kept: `input_type = PAIR`; `__init__(config, dataload)` with `method`, `top_num`, `v_feat_path` (plus the optional
`history_window`, 1..64, default 50); `state_dict` = {placeholder}, so reference checkpoints load with strict=True; `v_feat` is
neither a parameter nor a buffer.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..utils.enum_type import InputType
from .basemodel import BaseModel

FUSED_TOP_MAX = 16          # longest k-largest list the fused kernel keeps in registers (pxr_visrank_topk_f32)
WINDOW_MAX = 64


class VISRANK(BaseModel):
    input_type = InputType.PAIR

    def __init__(self, config, dataload):
        super().__init__()
        self.method = config["method"]
        if self.method == "average_top_k":
            self.k = int(config["top_num"])
            if self.k < 1:
                raise ValueError(f"top_num must be at least 1, got {self.k}")
        elif self.method == "maximum":
            self.k = 1
        else:
            self.k = None                                    # the mean over the window (visrank.py:19-20)
        w = config["history_window"] if "history_window" in config else None
        self.history_window = 50 if w is None else int(w)    # visrank.py:39 user[-50:]
        if not 1 <= self.history_window <= WINDOW_MAX:
            raise ValueError(f"history_window must be in 1..{WINDOW_MAX}, got {self.history_window}")
        self.item_num = dataload.item_num
        self.v_feat_path = config["v_feat_path"]
        v = np.load(self.v_feat_path, allow_pickle=True)
        v = torch.tensor(np.asarray(v), dtype=torch.float)
        if v.dim() != 2 or v.shape[0] != self.item_num:
            raise ValueError(f"v_feat_path {self.v_feat_path}: the feature matrix must be [item_num, F] with item_num = "
                             f"{self.item_num} rows, got shape {tuple(v.shape)}")
        if v.shape[1] % 4:
            raise ValueError(f"v_feat_path {self.v_feat_path}: the feature width F must be a multiple of 4 (16-byte vector "
                             f"accesses), got F = {v.shape[1]}")
        self.v_feat = v.contiguous()                         # frozen: a plain attribute, not in the state_dict (visrank.py:25)
        self.feature_dim = v.shape[1]
        self.module = None
        self.placeholder = nn.Parameter(torch.zeros(0))
        self._unit = None

    # ------------------------------------------------------------------------------------------ the reduction
    def reduction(self):
        """-> (top_k of pxr_visrank_topk_f32 | None when the fused kernel does not take it): 0 = the mean over the window."""
        if self.k is None or self.k >= self.history_window:
            return 0
        return self.k if self.k <= FUSED_TOP_MAX else None

    @property
    def fused_topk_supported(self) -> bool:
        return self.reduction() is not None

    def unit_rows(self):
        """v_feat with unit rows on the placeholder's device, made once."""
        dev = self.placeholder.device
        if self._unit is None or self._unit.device != dev:
            self._unit = ops.visrank_unit_rows(self.v_feat.to(dev), 1e-8)
        return self._unit

    def forward(self, inputs=None):
        return None

    @torch.no_grad()
    def compute_item_all(self):
        return None

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def fused_topk_batch(self, window, hist_ptr, hist_items, K: int):
        """window int64 [B, history_window] left-padded with 0 + the CSR of the full histories -> top-K ids int64 [B, K]."""
        top_k = self.reduction()
        if top_k is None:
            raise ops._l.PxrError(f"VISRANK: top_num = {self.k} is not fused (1..{FUSED_TOP_MAX}, or >= history_window)")
        idx, _ = ops.visrank_topk(self.unit_rows(), window.contiguous(), top_k, K, hist_ptr, hist_items)
        return idx

    @torch.no_grad()
    def predict(self, user, item_feature=None):
        unit = self.unit_rows()
        N, F = unit.shape
        user = user.to(unit.device)
        single = user.dim() == 1
        win = user[-self.history_window:].view(1, -1) if single else user[:, -self.history_window:]
        B, H = win.shape
        valid = win != 0
        h = valid.sum(1)
        if single:
            h = torch.full_like(h, H)                        # the reference form has no padding: every row counts
            valid = torch.ones_like(valid)
        if H == 0 or bool((h == 0).any()):
            raise ValueError("VISRANK.predict: a user without history (the mean of nothing)")
        rows = unit[win.reshape(-1)].contiguous()            # [B H, F]
        S = torch.empty(B * H, N, dtype=torch.float32, device=unit.device)
        ops.gemm(True, True, B * H, N, F, rows, F, unit, F, S, N)
        S = S.view(B, H, N)
        if self.k is None:
            k = h
            top = S.masked_fill(~valid[:, :, None], 0.0)
        else:
            k = torch.clamp(h, max=self.k)
            kmax = min(self.k, H)
            top = torch.topk(S.masked_fill(~valid[:, :, None], -np.inf), kmax, dim=1).values
            keep = torch.arange(kmax, device=unit.device)[None, :] < k[:, None]
            top = top.masked_fill(~keep[:, :, None], 0.0)
        scores = top.sum(1) / k[:, None].to(torch.float32)
        scores[:, 0] = -np.inf
        return scores[0] if single else scores
