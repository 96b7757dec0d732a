"""VBPR (ViNet) -- drop-in for `REC.model.ViNet.vbpr.VBPR` (code/REC/model/ViNet/vbpr.py) on the hand-written gfx950 kernels of
csrc/vbpr.hip and the library's fp32-operand GEMMs.  With Dh = embedding_size // 2 and the frozen features v_feat [I, F]:

    e_{b,t} = W v_feat[item_{b,t}]            beta_{b,t} = w_b . v_feat[item_{b,t}]            (t = positive, negative)
    s_{b,t} = <uid_b, iid_{b,t}> + <um_b, e_{b,t}> + beta_{b,t}
    loss    = -mean_b log(1e-8 + sigmoid(s_{b,0} - s_{b,1}))

W = feature_projection.weight [Dh, F] and w_b = bias_projection.weight [1, F] (both without bias); uid / iid / um are rows of
user_id_embedding [U, Dh], item_id_embedding [I, Dh], user_modal_embedding [U, Dh].  `mlp_hidden_size` and `dropout_prob` are read
and unused, as in the reference.

The tables: all three are views of ONE [1 + U + I + U, Dh] buffer in the reference's parameter order -- user id row u at 1 + u,
item id row i at 1 + U + i, user modal row u at 1 + U + I + u, row 0 a spare nothing reads (VBPR has no padding id, and the
sparse-row kernels treat id 0 as padding / an empty slot).  PxrAdamW updates that buffer lazily (optim.table_spans): the step's 4B
rows are caught up before the forward reads them, the backward leaves the table gradient as sparse rows (`sparse_table_grad`, one
slot per occurrence, deterministic) and only those rows are updated -- O(B Dh) per step instead of the reference's dense AdamW
over every row of three tables.  The two projections live in the flat buffer of PxrAdamW's one launch.  With the shipped
`decay_check_name: 'projection'` the reference's two parameter groups are exactly flat buffer and table buffer
(`split_flat_table_groups`, optim.flat_table_adamw).

A step: rows -> catch-up -> feature gather with the visual bias fused -> projection GEMM -> pair head; backward: pair head
backward (de, the sparse rows) -> bias-projection column sum -> weight-gradient GEMM.

Evaluation: the score uid iid^T + um e^T + bias is one inner product of [uid | um | 1 | 0...] with [iid | e | bias | 0...]
(width 2 Dh + 1 padded to a multiple of 32): `scoring_item_matrix()` packs the item side once per evaluation, `encode_last` the
query side per batch, and the fused top-k scores them.  `predict` is the reference's literal formula.

Contract kept: `input_type = PAIR`; `__init__(config, dataload)` with `embedding_size`, `mlp_hidden_size`, `dropout_prob`,
`v_feat_path`; forward((user [B], item [B, 2])) -> loss; `compute_item_all` (W v_feat, and `total_visual_bias`) and `predict(user,
item_feature)`; `state_dict` keys and order of the reference (the two projections, then the three tables; xavier-normal init), so
reference checkpoints load with strict=True; `v_feat` is neither a parameter nor a buffer.  One process: the data-parallel
exchange is not built for this model.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..lib import PxrError
from ..utils.enum_type import InputType
from .packed import LazyTableModel, TrainStep, _Rows, dense_gemm, one_process


class VBPR(LazyTableModel):
    input_type = InputType.PAIR
    # the optimizer may run the flat buffer (the projections) and the table buffer under separate scalars: optim.flat_table_adamw
    split_flat_table_groups = True

    def __init__(self, config, dataload):
        super().__init__()
        one_process(self)
        self.mlp_hidden_size = config["mlp_hidden_size"] if "mlp_hidden_size" in config else None      # read and unused (vbpr.py:12-13)
        self.dropout_prob = config["dropout_prob"] if "dropout_prob" in config else None
        self.embedding_size = int(config["embedding_size"]) // 2
        Dh = self.embedding_size
        if Dh <= 0 or Dh % 4 or Dh > 4096:
            raise ValueError(f"embedding_size // 2 must be a positive multiple of 4, at most 4096 (16-byte vector accesses); "
                             f"got embedding_size // 2 = {Dh}")
        self.user_num = dataload.user_num
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
        self.v_feat = v.contiguous()                       # frozen: a plain attribute, not in the state_dict (vbpr.py:24)
        self.feature_dim = F = v.shape[1]
        # the reference's module order (vbpr.py:30-36); nn.Linear(bias=False) and nn.Embedding both hold one `weight`
        self.feature_projection = _Rows(Dh, F)
        self.bias_projection = _Rows(1, F)
        self.user_id_embedding = _Rows(self.user_num, Dh)
        self.item_id_embedding = _Rows(self.item_num, Dh)
        self.user_modal_embedding = _Rows(self.user_num, Dh)
        for mod in (self.feature_projection, self.bias_projection, self.user_id_embedding, self.item_id_embedding,
                    self.user_modal_embedding):            # vbpr.py _init_weights through self.apply, in module order
            nn.init.xavier_normal_(mod.weight.data)
        self.store_ifeatures = None
        self.total_visual_bias = None

    # ------------------------------------------------------------------------------------------ packing
    def _flat_specs(self):
        """Flat layout: the two projections in the reference's parameter order."""
        return [("W", self.feature_projection.weight), ("wb", self.bias_projection.weight)]

    def rec_parameter_names(self):
        """{reference parameter name: flat-buffer key} in the reference's registration order (optim.native_to_torch_state); the
        tables map to None -- their state is the table's (optim.table_spans)."""
        return {"feature_projection.weight": "W", "bias_projection.weight": "wb", "user_id_embedding.weight": None,
                "item_id_embedding.weight": None, "user_modal_embedding.weight": None}

    def table_parameter_spans(self):
        """Rows of the table buffer each table parameter occupies (optim.table_spans), in the reference's order."""
        U, I = self.user_num, self.item_num
        return {"user_id_embedding.weight": (1, 1 + U), "item_id_embedding.weight": (1 + U, 1 + U + I),
                "user_modal_embedding.weight": (1 + U + I, 1 + U + I + U)}

    def _after_pack(self, dev):
        self.v_feat = self.v_feat.to(dev)

    # ------------------------------------------------------------------------------------------ training
    def forward(self, input):
        user, item = input
        if not self.training:
            raise PxrError("VBPR.forward is the training loss (vbpr.py forward); use compute_item_all / predict to score")
        self._ensure_packed()
        user, item = user.reshape(-1).contiguous(), item.contiguous()
        return TrainStep.apply(self._anchor, self, user, item)

    def _forward_train(self, user, item):
        B, Dh, F = user.numel(), self.embedding_size, self.feature_dim
        rows = ops.vbpr_rows(user, item, self.user_num, self.item_num, out=self._buf("rows", (4 * B,), torch.int64))
        if self._table_hooks is not None:
            self._table_hooks.catch_up_ids(rows)          # the step's rows, current through the last step before anything reads them
        x, beta = ops.vbpr_gather(self.v_feat, item.view(-1), self._p("wb").view(-1), out=self._buf("x", (2 * B, F)),
                                  beta=self._buf("beta", (2 * B,)))
        e = ops.linear_fwd(x, self._p("W"), None)                                  # [2B, Dh]
        loss, coef = ops.vbpr_pair_fwd(self._table, rows, e, beta, B, out=self._buf("head", (2 * B + 1,)))
        self._saved = dict(B=B, rows=rows, coef=coef, x=x, e=e)
        return loss

    def _backward_train(self, gsd):
        s = self._take_saved()
        B, Dh = s["B"], self.embedding_size
        sp = self._sparse_rows(4 * B)
        de, csign = self._buf("de", (2 * B, Dh)), self._buf("csign", (2 * B,))
        ops.vbpr_pair_bwd(self._table, s["rows"], s["e"], s["coef"], B, de, csign, sp, self.grad_scale, gsd)
        ops.vbpr_bias_grad(s["x"], csign, self._p("wb", grad=True).view(-1))
        ops.grouped_linear_bwd_weight([(de, s["x"], self._p("W", grad=True), None)])
        self.sparse_table_grad = sp
        self._step_done()

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def compute_item_all(self):
        """W v_feat [I, Dh] over the whole catalogue; keeps total_visual_bias [I] = w_b . v_feat (vbpr.py compute_item_all)."""
        self._ensure_packed()
        self.sync_table()
        _, self.total_visual_bias = ops.vbpr_gather(self.v_feat, None, self._p("wb").view(-1), copy=False)
        self.store_ifeatures = ops.linear_fwd(self.v_feat, self._p("W"), None)
        return self.store_ifeatures

    @torch.no_grad()
    def scoring_item_matrix(self):
        """[I, P] = [item id row | W v_feat | total_visual_bias | 0...] from the last compute_item_all(): the item side of the score
        as one inner product (the Trainer's fused top-k reads it in place of the item feature)."""
        if self.store_ifeatures is None:
            raise PxrError("VBPR: call compute_item_all() before scoring")
        lo, hi = self.table_parameter_spans()["item_id_embedding.weight"]
        return ops.vbpr_pack(self._table[lo:hi], self.store_ifeatures, self.total_visual_bias)

    @torch.no_grad()
    def encode_last(self, user, item_feature=None):
        """user int64 [B] -> (q [B, 1, P], q [B, P]): [user id row | user modal row | 1 | 0...], the query side of the fused scoring
        against scoring_item_matrix()."""
        self._ensure_packed()
        self.sync_table()
        user = user.reshape(-1).contiguous()
        B = user.numel()
        rows = ops.vbpr_rows(user, None, self.user_num, self.item_num)
        q = ops.vbpr_pack(self._table, self._table, None, rows[:B], rows[B:])
        return q.view(B, 1, -1), q

    @torch.no_grad()
    def predict(self, user, item_feature):
        """scores [B, I] = uid iid^T + um item_feature^T + total_visual_bias (vbpr.py predict)."""
        feat = item_feature if item_feature is not None else self.store_ifeatures
        if feat is None or self.total_visual_bias is None:
            raise PxrError("VBPR: call compute_item_all() before scoring")
        self._ensure_packed()
        self.sync_table()
        feat = feat if feat.is_contiguous() else feat.contiguous()
        user = user.reshape(-1).contiguous()
        B = user.numel()
        rows = ops.vbpr_rows(user, None, self.user_num, self.item_num)
        u = ops.embed_gather(self._table, rows)                                    # [2B, Dh]: id rows | modal rows
        lo, hi = self.table_parameter_spans()["item_id_embedding.weight"]
        s_id, s_mo = dense_gemm(u[:B], self._table[lo:hi]), dense_gemm(u[B:], feat)
        ops.raise_on_bad_indices(u.device)     # a user id outside the table raises, like the reference's indexing
        return s_id.add_(s_mo).add_(self.total_visual_bias)
