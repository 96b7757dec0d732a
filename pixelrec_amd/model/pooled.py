"""DSSM and FM (IDNet) -- drop-ins for `REC.model.IDNet.dssm.DSSM` and `REC.model.IDNet.fm.FM` (code/REC/model/IDNet/dssm.py,
fm.py; MLPLayers and BaseFactorizationMachine of code/REC/model/layers.py) on the hand-written gfx950 kernels of csrc/pool.hip and
the MODE_POOL segment sum of csrc/embed_grad.hip.  With the item table e [I, D], a sample b with the profile items i_{b,1..L}
(left-padded with 0), the positive p_b and the negative n_b, m_l = [i_l != 0] and cnt = sum_l m_l:

    DSSM:  U_b = (sum_l m_l e[i_l]) / (cnt + 1e-8)   (an fp32 division; cnt = 0 gives exactly 0)      u_b = mlp(U_b)
    FM:    u_b = H_b = sum_l m_l e[i_l]
    x_b = <u_b, e[p_b]> - <u_b, e[n_b]>              loss = -mean_b log(1e-8 + sigmoid(x_b))

DSSM's mlp is MLPLayers(mlp_hidden_size, dropout_prob): the size list is `mlp_hidden_size` ITSELF, per layer Dropout -> Linear ->
ReLU, no BatchNorm; `[]` (the shipped config) or a one-entry list is the identity.

FM's reference runs BaseFactorizationMachine over [profile | p] and over [profile | n] and subtracts: score = 1/2 (|sum_f v_f|^2 -
sum_f |v_f|^2).  The history-history terms are the same in both scores and cancel exactly, which leaves x = <H, e[p]> - <H, e[n]>
with the gradients p - n on every real history row, H on p and -H on n: FM is DSSM without the MLP and with sum pooling.  The
kernels compute that form.  The reference computes the literal form in fp32 and loses digits to the cancellation; that difference
is bounded in the tests (tests/pool_restate.py holds both forms), not imitated.

One decision about the reference: both of its `forward`s begin with `inputs = inputs[0].unsqueeze(0)`, so it trains on the FIRST
sample of every batch and discards the rest -- a leftover.  These models train on every row of the batch; on a one-row batch they
compute exactly what the reference computes, which is what the fixtures compare.

The table is ONE [1 + I, D] buffer, item i at row 1 + i, row 0 a spare nothing reads: `item_embedding.weight` is the view of rows
1 .. I, so the padding item is an ordinary row of the lazy AdamW (PxrAdamW): caught up with the step's rows before the forward
reads, decayed on the reference's trajectory, never given a gradient.  A step: row list + catch-up -> pooling fused with the pair
head (no MLP: one launch) or pooling -> MLP -> head -> the compact gradient block G [3B, D] (one row per sample for its whole
history, one per target) -> stable sort + MODE_POOL segment sum into `sparse_table_grad`.  No [B (L + 2), D] buffer is written.

Contract kept: `input_type = SEQ`; `__init__(config, dataload)` with `embedding_size`, `mlp_hidden_size`, `dropout_prob`;
forward -> loss; `compute_item_all()` -> the table; `encode_last(window)` -> the queries of the fused top-k; `predict(item_seq,
item_feature)` = q item_feature^T (an all-padding window pools to exactly 0); `state_dict` keys and order of the reference, so
reference checkpoints load with strict=True.  One process: the data-parallel exchange is not built for these models.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..lib import PxrError
from ..utils.enum_type import InputType
from .packed import (LazyTableModel, TrainStep, _ActMLP, _Rows, check_width16, dense_scores, hidden_sizes, linear_names, linear_specs,
                     one_process, split_planes, split_tail)


def pool_queries(name, feat, item_seq, mean):
    """item_seq int64 [B, L] left-padded with 0 -> the pooled rows of feat [N, D] (masked sum, or masked mean), [B, D]: the
    evaluation form of the training kernel, shared by the ID models here and the pixel models of mopooled.py."""
    item_seq = item_seq.to(feat.device).contiguous()
    if item_seq.dim() != 2 or item_seq.shape[1] < 1:
        raise ValueError(f"{name}: item_seq must be [B, L] with L >= 1, got {tuple(item_seq.shape)}")
    B, L = item_seq.shape
    q, _ = ops.pool_rows(feat, item_seq, B, L, mean, pad_row=0)
    return q


_PAIR_TEXT = "{name}: expected a profile [B, L] (L >= 1) and targets [B, 2] (positive, negative), got {{profile}} and {{tail}}"


class _PooledPair(LazyTableModel):
    """What DSSM and FM share: the table, the row list, the pooled pair step and the evaluation."""

    input_type = InputType.SEQ
    pool_mean = False                  # DSSM: masked mean; FM: masked sum
    flat_align = 4

    def _init_common(self, config, dataload):
        one_process(self)
        self.embedding_size = D = int(config["embedding_size"])
        check_width16(D)
        self.mlp_hidden_size = hidden_sizes(config["mlp_hidden_size"] if "mlp_hidden_size" in config else None)
        p = config["dropout_prob"] if "dropout_prob" in config else 0.0
        self.dropout_prob = float(p or 0.0)
        self.item_num = dataload.item_num
        L = config["MAX_ITEM_LIST_LENGTH"] if "MAX_ITEM_LIST_LENGTH" in config else None
        self.max_seq_length = int(L) if L else None
        s = config["seed"] if "seed" in config else None
        self._drop_seed = int(s) if s is not None else 2020

    def _init_weights(self):
        for mod in self.modules():                          # the reference's _init_weights, in module order
            if isinstance(mod, (nn.Linear, _Rows)):
                nn.init.xavier_normal_(mod.weight.data)     # nn.Embedding(padding_idx=0): the init overwrites row 0
                if getattr(mod, "bias", None) is not None:
                    nn.init.constant_(mod.bias.data, 0)

    # ------------------------------------------------------------------------------------------ packing
    n_layers = 0

    def _flat_specs(self):
        return []

    def table_parameter_spans(self):
        """Rows of the table buffer the table parameter occupies (optim.table_spans)."""
        return {"item_embedding.weight": (1, 1 + self.item_num)}

    # ------------------------------------------------------------------------------------------ training
    def forward(self, input):
        if not self.training:
            raise PxrError(f"{type(self).__name__}.forward is the training loss; use encode_last / predict to score")
        self._ensure_packed()
        profile, target = self._split_input(input)
        return TrainStep.apply(self._anchor, self, profile, target)

    def _mlp_fwd(self, x, train):
        """x [B, D] -> (u, saved per layer (input, relu')): Dropout -> Linear -> ReLU per layer."""
        saved = []
        p = self.dropout_prob
        for k in range(self.n_layers):
            xin = ops.dropout(x, p, self._drop_seed, k, step_dev=self._drop_dev) if (train and p > 0) else x
            x, d = ops.linear_fwd(xin, self._p(f"l{k}.w"), self._p(f"l{k}.b"), act="relu")
            saved.append((xin, d))
        return x, saved

    def _forward_train(self, profile, target):
        B, L = profile.shape
        D = self.embedding_size
        n = B * (L + 2)
        rows, gidx = ops.din_rows(profile, target, self.item_num, out=self._buf("rows", (2, n), torch.int64))
        if self._table_hooks is not None:
            self._table_hooks.catch_up_ids(rows)          # the step's rows (the padding item's too), current before anything reads them
        U, w, head = self._buf("U", (B, D)), self._buf("w", (B,)), self._buf("head", (2 * B + 1,))
        if not self.n_layers:
            loss, coef, _, _, _ = ops.pool_pair_fwd(self._table, rows, B, L, self.pool_mean, U=U, w=w, out=head)
            self._saved = dict(B=B, L=L, rows=rows, gidx=gidx, U=U, w=w, coef=coef)
            return loss
        ops.pool_rows(self._table, rows, B, L, self.pool_mean, U=U, w=w)
        u, saved = self._mlp_fwd(U, True)
        it = ops.embed_gather(self._table, rows[B * L:], out=self._buf("it", (2 * B, D)))
        loss, coef = ops.curator_pair_fwd(u, it, B, out=head)
        self._saved = dict(B=B, L=L, rows=rows, gidx=gidx, U=U, w=w, coef=coef, u=u, it=it, mlp=saved)
        return loss

    def _table_grad(self, gidx, B, L, G, w):
        """The compact block -> sparse rows: history occurrence (b, l) reads w[b] G[b], target j reads G[B + j]; no gradient row per
        occurrence is written (tools/pool_bench.py overrides this with the materialised form to price the difference)."""
        return ops.pool_table_grad(gidx, B, L, G, w, self._table.shape[0], out=self._sparse_rows(B * (L + 2)))

    def _backward_train(self, gsd):
        s = self._take_saved()
        B, L, D = s["B"], s["L"], self.embedding_size
        G = self._buf("G", (3 * B, D))
        if not self.n_layers:
            ops.pool_pair_bwd(self._table, s["rows"], B, L, s["U"], s["coef"], self.grad_scale, gsd, G=G)
        else:
            p = self.dropout_prob
            gp = lambda k: self._p(k, grad=True)
            du = self._buf("du", (B, D))
            ops.mf_pair_bwd(s["u"], s["it"], s["coef"], du, G[B:], self.grad_scale, gsd)       # d u, and d e[p], d e[n] in place
            saved = s["mlp"]
            dz = ops.mul(du, saved[-1][1], out=du)                                            # through the last ReLU
            problems = []
            for k in reversed(range(self.n_layers)):
                xin, _ = saved[k]
                problems.append((dz, xin, gp(f"l{k}.w"), gp(f"l{k}.b")))
                W = self._p(f"l{k}.w")
                if p == 0:
                    dz = ops.linear_bwd_input(dz, W, out=G[:B]) if k == 0 else ops.linear_bwd_input(dz, W, mul=saved[k - 1][1])
                    continue
                dx = ops.linear_bwd_input(dz, W)
                dx = ops.dropout(dx, p, self._drop_seed, k, step_dev=self._drop_dev)           # the mask's backward is itself
                if k == 0:
                    G[:B].copy_(dx)
                else:
                    dz = ops.mul(dx, saved[k - 1][1], out=dx)
            ops.grouped_linear_bwd_weight(problems)
        self.sparse_table_grad = self._table_grad(s["gidx"], B, L, G, s["w"])
        self._step_done()

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def compute_item_all(self):
        """The (flushed) item table [I, D] (compute_item_all of dssm.py / fm.py)."""
        self._ensure_packed()
        self.sync_table()
        return self.item_embedding.weight

    @torch.no_grad()
    def encode_last(self, item_seq, item_feature=None):
        """item_seq int64 [B, L] left-padded with 0 -> (q [B, 1, D], q [B, D]): the pooled window (through the MLP, DSSM), the
        queries of the fused scoring against item_feature (default: compute_item_all()).  The pooling is the training kernel's:
        the pooled vector of a window is bit-identical in both."""
        self._ensure_packed()
        feat = item_feature if item_feature is not None else self.compute_item_all()
        feat = (feat if feat.is_contiguous() else feat.contiguous()).data
        q = pool_queries(type(self).__name__, feat, item_seq, self.pool_mean)
        if self.n_layers:
            q, _ = self._mlp_fwd(q, False)
        return q.view(q.shape[0], 1, -1), q

    @torch.no_grad()
    def predict(self, item_seq, item_feature=None):
        """scores [B, I] = q item_feature^T (predict of dssm.py / fm.py)."""
        feat = item_feature if item_feature is not None else self.compute_item_all()
        feat = (feat if feat.is_contiguous() else feat.contiguous()).data
        _, q = self.encode_last(item_seq, feat)
        return dense_scores(q, feat)


class DSSM(_PooledPair):
    """dssm.py: masked-mean pooling -> MLPLayers(mlp_hidden_size, dropout_prob) -> pair head.  forward([profile (L) | positive |
    negative] int64 [B, L + 2], or the same as (profile [B, L], target [B, 2])) -> loss over EVERY row (the reference's forward
    keeps row 0 of the batch only).  `user_embedding` is the reference's second name for the item table: both keys are in the
    state_dict, one parameter."""

    pool_mean = True

    def __init__(self, config, dataload):
        super().__init__()
        self._init_common(config, dataload)
        D, hidden = self.embedding_size, self.mlp_hidden_size
        if hidden and (hidden[0] != D or hidden[-1] != D or any(h <= 0 or h % 4 or h > 4096 for h in hidden)):
            raise ValueError(f"mlp_hidden_size is the MLP's whole size list: it must be [] or start and end with embedding_size "
                             f"({D}), every entry a positive multiple of 4, at most 4096; got {hidden}")
        self.n_layers = max(0, len(hidden) - 1)
        self.out_size = D
        self.item_embedding = _Rows(self.item_num, D)
        self.user_embedding = self.item_embedding           # dssm.py:25: one table under two names
        self.mlp_layers = _ActMLP(hidden, nn.ReLU, self.dropout_prob)    # MLPLayers(mlp_hidden_size, dropout_prob)
        self._init_weights()

    def _linears(self):
        return [(f"l{k}", f"mlp_layers.mlp_layers.{3 * k + 1}", self.mlp_layers.mlp_layers[3 * k + 1]) for k in range(self.n_layers)]

    def _flat_specs(self):
        return linear_specs(self._linears())

    def rec_parameter_names(self):
        """{reference parameter name: flat-buffer key} in the reference's registration order (optim.native_to_torch_state): the
        table first (its state is the table buffer's: None), then the MLP.  `user_embedding.weight` is `item_embedding.weight`
        and is not a parameter of its own."""
        return {"item_embedding.weight": None, **linear_names(self._linears())}

    def _split_input(self, input):
        if torch.is_tensor(input) and (input.dim() != 2 or input.shape[1] < 3):
            raise ValueError(f"DSSM: expected [B, L + 2] ids (profile, positive, negative), got {tuple(input.shape)}")
        return split_tail(input, 2, _PAIR_TEXT.format(name="DSSM"))


class FM(_PooledPair):
    """fm.py: x = FM([profile | p]) - FM([profile | n]) = <H, e[p]> - <H, e[n]> with H the masked sum.  forward(the reference's
    [B, 2, L + 1] int64 tensor -- plane 0 = [profile | positive], plane 1 = [profile | negative] -- or (profile [B, L], target
    [B, 2])) -> loss over EVERY row (the reference's forward keeps row 0 of the batch only).  No parameter besides the table;
    `mlp_hidden_size` and `dropout_prob` are read and ignored, as in the reference."""

    pool_mean = False

    def __init__(self, config, dataload):
        super().__init__()
        self._init_common(config, dataload)
        self.out_size = self.mlp_hidden_size[-1] if self.mlp_hidden_size else self.embedding_size     # fm.py:19: never used
        self.item_embedding = _Rows(self.item_num, self.embedding_size)
        self._init_weights()

    def rec_parameter_names(self):
        return {"item_embedding.weight": None}

    def _split_input(self, input):
        return split_planes(input, "FM", _PAIR_TEXT.format(name="FM"))
