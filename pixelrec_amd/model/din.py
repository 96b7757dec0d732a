"""DIN (IDNet) -- drop-in for `REC.model.IDNet.din.DIN` (code/REC/model/IDNet/din.py, with SequenceAttLayer of
code/REC/model/layers.py:460-514) on the hand-written gfx950 kernels of csrc/din.hip and the library's fp32-operand GEMMs with the
sigmoid epilogue.  With the item table e [I, D], a sample b with the profile items i_{b,1..L} (left-padded with 0), the positive
p_b and the negative n_b, k_l = e[i_{b,l}] and a candidate q:

    s_l(q)   = dense(sigmoid(... sigmoid(W1 [q | k_l | q - k_l | q * k_l] + b1) ...))     0 where i_{b,l} == 0, then / sqrt(D)
    score(q) = sum_l s_l(q) <k_l, q>                                       (softmax_stag=False: the weights are NOT normalised)
    loss     = -mean_b log(sigmoid(score(e[p_b]) - score(e[n_b])) + 1e-8) + 0.01 ||e[rows]||_2 / B

The regulariser's norm runs over all B (L + 2) gathered rows, padding positions included: they read row 0, which the reference's
xavier_normal_ leaves non-zero.  Row 0 never receives a gradient (padding_idx=0) and is still decayed by AdamW every step.

The table is ONE [1 + I, D] buffer, item i at row 1 + i, row 0 a spare nothing reads (the sparse-row machinery treats id 0 as an
empty slot): `item_embedding.weight` is the view of rows 1 .. I, so the padding item is an ordinary row of the lazy AdamW -- caught
up before the forward reads it, decayed on the reference's trajectory, never given a gradient.  The attention tensors live in the
flat buffer of PxrAdamW's one launch.

A step: row list + catch-up -> attention-input kernel ([2 B L, 4 D] operand, pair rows (candidate, sample, position)) -> the MLP
Linears with the sigmoid epilogue (activation and derivative in one pass) -> head forward (dense, mask, 1 / sqrt(D), scores, loss,
regulariser; one fixed reduction order) -> head backward -> the MLP's input-gradient GEMMs -> fold kernel (one gradient row per
occurrence) -> stable sort + segmented sum into `sparse_table_grad`; the weight gradients in one grouped launch.

Evaluation: the first Linear factorises (W1 x = A q + Bm k + C (q * k): DESIGN.md), so `fused_topk_batch` scores and ranks a whole
batch of users in one launch of pxr_din_topk_f32 without any [B, L, N, *] tensor; A q + b1 is made once per evaluation and cached
until train().  `predict` takes the reference's [B, item_num, L + 1] id tensor, or a plain [B, L] window batch scored in candidate
chunks through the library GEMMs (what `eval_fused_topk: False` uses).

Contract kept: `input_type = SEQ`; `__init__(config, dataload)` with `embedding_size`, `mlp_hidden_size`, `dropout_prob` (read and
ignored, as in the reference: its only consumer is commented out); forward([profile (L) | positive | negative] int64 [B, L + 2],
or the same as (profile [B, L], target [B, 2])) -> loss; `compute_item_all()` -> the table; `state_dict` keys and order of the
reference (xavier-normal weights and table, zero biases), so reference checkpoints load with strict=True.  One process: the
data-parallel exchange is not built for this model.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..lib import PxrError
from ..utils.enum_type import InputType
from .packed import (LazyTableModel, TrainStep, _ActMLP, _Rows, check_width16, hidden_sizes, linear_names, linear_specs, one_process,
                     split_tail)


class _Attention(nn.Module):
    """SequenceAttLayer's parameter layout; never called."""

    def __init__(self, sizes):
        super().__init__()
        self.att_mlp_layers = _ActMLP(sizes, nn.Sigmoid)       # MLPLayers(sizes, activation='Sigmoid', bn=False)
        self.dense = nn.Linear(sizes[-1], 1)


class DinEval:
    """The evaluation DIN and MODIN share, parametrised by where the item rows come from (`_item_rows()`: DIN's flushed table,
    MODIN's encoded catalogue).  Mixed into a PackedModel with DIN's attention layout (`l0`, [`l1`], `dense` in the flat buffer),
    `embedding_size`, `mlp_hidden_size`, `max_seq_length`, `_eval_cache` and `_mlp`."""

    PREDICT_CHUNK_ROWS = 1 << 16       # (candidate, window row) pairs per chunk of the GEMM-path predict

    def _item_rows(self):
        """The contiguous float32 [N, D] matrix the fused scoring reads (and `predict` without an `item_feature`)."""
        raise NotImplementedError

    def _drop_eval_cache(self):
        self._eval_cache = None                # the A q + b1 matrix goes when training resumes

    @property
    def fused_topk_supported(self) -> bool:
        return ops.din_topk_supported(self.embedding_size, self.mlp_hidden_size, self.max_seq_length or 1)

    def _eval_tensors(self):
        """(A q + b1 [N, h1], Bm, C, the item rows [N, D]) of the factorised first Linear: once per evaluation, cached until
        `_drop_eval_cache()` (train(), load_state_dict, a repack)."""
        if self._eval_cache is None:
            self._ensure_packed()
            feat = self._item_rows()
            A, Bm, C = ops.din_fold_w1(self._p("l0.w"), self.embedding_size)
            aq = ops.linear_fwd(feat, A, self._p("l0.b"))
            self._eval_cache = (aq, Bm, C, feat)
        return self._eval_cache

    @torch.no_grad()
    def fused_topk_batch(self, window, hist_ptr, hist_items, K: int):
        """window int64 [B, L] left-padded with 0 + the CSR of the full histories -> top-K ids int64 [B, K] (pxr_din_topk_f32)."""
        return self.fused_topk(window, hist_ptr, hist_items, K)[0]

    @torch.no_grad()
    def fused_topk(self, window, hist_ptr, hist_items, K: int):
        """-> (ids int64 [B, K], values fp32 [B, K])."""
        window = window.contiguous()
        if not ops.din_topk_supported(self.embedding_size, self.mlp_hidden_size, window.shape[1], K):
            raise PxrError(f"{type(self).__name__}: the fused top-k takes embedding_size <= {ops.DIN_MAX_D}, one or two hidden layers of at most "
                           f"{ops.DIN_MAX_HIDDEN} units, windows of at most {ops.DIN_MAX_L} items and K <= 32; evaluate through "
                           "predict() (eval_fused_topk: False)")
        aq, Bm, C, feat = self._eval_tensors()
        two = len(self.mlp_hidden_size) == 2
        return ops.din_topk(feat, window, aq, Bm, C, self._p("l1.w") if two else None,
                            self._p("l1.b") if two else None, self._p("dense.w").view(-1), self._p("dense.b"), K, hist_ptr, hist_items)

    def _pair_scores(self, q, k, mask):
        """q, k [M, L, D] (candidate rows repeated over L, history rows), mask bool [M, L] -> score [M]: the attention MLP through
        the library GEMMs, the rest in torch ops."""
        M, L, D = k.shape
        x = torch.cat([q, k, q - k, q * k], dim=-1).view(M * L, 4 * D)
        x = self._mlp(x)[0][-1]
        s = (x @ self._p("dense.w").view(-1) + self._p("dense.b")).view(M, L)
        s = s.masked_fill(mask, 0.0) / (D ** 0.5)
        return (s * (k * q).sum(-1)).sum(-1)

    @torch.no_grad()
    def predict(self, item_seq, item_feature=None):
        """scores [B, item_num].  item_seq: the reference's [B, item_num, L + 1] id tensor (din.py:87-103: the window repeated per
        candidate, the candidate id last), or a [B, L] window batch; both in chunks of PREDICT_CHUNK_ROWS (candidate, window row)
        pairs, so [B item_num L, 4 D] never exists."""
        self._ensure_packed()
        feat = item_feature if item_feature is not None else self._item_rows()
        feat = (feat if feat.is_contiguous() else feat.contiguous()).data
        N, D = feat.shape
        item_seq = item_seq.to(feat.device)
        if item_seq.dim() == 3:
            B = item_seq.shape[0]
            flat = item_seq.reshape(-1, item_seq.shape[-1])
            win, cand = flat[:, :-1], flat[:, -1]
        elif item_seq.dim() == 2:
            B, L = item_seq.shape
            win = item_seq[:, None, :].expand(B, N, L).reshape(B * N, L)
            cand = torch.arange(N, device=feat.device).repeat(B)
        else:
            raise ValueError(f"{type(self).__name__}.predict: item_seq must be [B, item_num, L + 1] or [B, L], got {tuple(item_seq.shape)}")
        L = win.shape[1]
        step = max(1, self.PREDICT_CHUNK_ROWS // L)
        out = torch.empty(win.shape[0], dtype=torch.float32, device=feat.device)
        for lo in range(0, win.shape[0], step):
            w = win[lo:lo + step].contiguous()
            k = ops.embed_gather(feat, w)                                           # [m, L, D]
            q = ops.embed_gather(feat, cand[lo:lo + step].contiguous())[:, None, :].expand_as(k)
            out[lo:lo + step] = self._pair_scores(q, k, w == 0)
        ops.raise_on_bad_indices(feat.device)     # an id outside the catalogue raises, like the reference's indexing
        return out.view(B, -1)


class DinStep:
    """The attention step DIN and MODIN share, parametrised by where the rows live: the constructor's reading of the config, the
    attention Linears' place in the flat buffer, and the forward / backward chain between the row list and the one gradient row
    per occurrence.  Mixed into a PackedModel in front of it."""

    flat_align = 4                     # the one-element bias of `dense` would shift what follows off 16 bytes

    def _build_attention(self, config, dataload):
        """embedding_size, mlp_hidden_size, dropout_prob (read, never used: din.py:19, modin.py:20), the attention module."""
        one_process(self)
        self.embedding_size = D = int(config["embedding_size"])
        check_width16(D)
        self.mlp_hidden_size = hidden = hidden_sizes(config["mlp_hidden_size"])
        if not hidden or any(h <= 0 or h % 4 or h > 4096 for h in hidden):
            raise ValueError(f"mlp_hidden_size must hold one or more positive multiples of 4, at most 4096 each (the weight-gradient "
                             f"GEMMs' vector accesses); got {hidden}")
        self.dropout_prob = config["dropout_prob"] if "dropout_prob" in config else 0.0
        self.item_num = dataload.item_num
        L = config["MAX_ITEM_LIST_LENGTH"] if "MAX_ITEM_LIST_LENGTH" in config else None
        self.max_seq_length = int(L) if L else None
        self.att_list = [4 * D] + hidden
        self.attention = _Attention(self.att_list)
        self._eval_cache = None
        self._mlp_keys = [f"l{i}" for i in range(len(hidden))]     # the flat-buffer keys of the attention MLP's Linears

    def _linears(self):
        """(flat-buffer key, reference path, module) of the attention Linears in the reference's parameter order."""
        out = []
        for i in range(len(self.mlp_hidden_size)):
            path = f"attention.att_mlp_layers.mlp_layers.{3 * i + 1}"
            out.append((f"l{i}", path, self.attention.att_mlp_layers.mlp_layers[3 * i + 1]))
        out.append(("dense", "attention.dense", self.attention.dense))
        return out

    def _flat_specs(self):
        return linear_specs(self._linears())

    def _mlp(self, x):
        """x [M, 4 D] -> lists of the hidden layers' activations and derivatives (library GEMMs, sigmoid epilogue)."""
        return self._act_chain(x, self._mlp_keys, "sigmoid")

    def _attention_fwd(self, table, rows, gidx, profile, reg):
        """table [T, D], rows / gidx int64 [B (L + 2)] (what an occurrence reads / where its gradient goes), profile int64 [B, L]
        (0 = padding), reg the weight of ||emb||_2 / B in the loss -> loss [1]; leaves `_saved`."""
        B, L = profile.shape
        D = self.embedding_size
        n = B * (L + 2)
        emb, x = ops.din_att_input(table, rows, B, L, emb=self._buf("emb", (n, D)), x=self._buf("x", (2 * B * L, 4 * D)))
        acts, ders = self._mlp(x)
        loss, s, kq, head = ops.din_head_fwd(acts[-1], self._p("dense.w").view(-1), self._p("dense.b"), emb, profile,
                                             s=self._buf("s", (2 * B * L,)), kq=self._buf("kq", (2 * B * L,)),
                                             head=self._buf("head", (2 + 3 * B,)), reg=reg)
        self._saved = dict(B=B, L=L, profile=profile, gidx=gidx, emb=emb, x=x, acts=acts, ders=ders, s=s, kq=kq, head=head)
        return loss

    def _attention_bwd(self, gsd):
        """-> (gidx, occ [B (L + 2), D]): one gradient row per occurrence; the attention gradients are in the flat buffer."""
        s = self._take_saved()
        B, L, D = s["B"], s["L"], self.embedding_size
        n = B * (L + 2)
        nl = len(self.mlp_hidden_size)
        G = lambda k: self._p(k, grad=True)
        acts, ders = s["acts"], s["ders"]
        dz, _ = ops.din_head_bwd(acts[-1], ders[-1], self._p("dense.w").view(-1), s["profile"], s["kq"], s["head"], D,
                                 G("dense.w").view(-1), G("dense.b"), self.grad_scale, gsd,
                                 dsraw=self._buf("dsraw", (2 * B * L,)))
        dzs = self._act_chain_bwd(dz, self._mlp_keys, ders)
        dx = ops.linear_bwd_input(dzs[0], self._p("l0.w"))
        occ = ops.din_fold_bwd(dx, s["emb"], s["profile"], s["s"], s["head"], self.grad_scale, gsd, occ=self._buf("occ", (n, D)))
        # the first layer's reduction runs over 2 B L rows of 4 D inputs: a launch of its own (its token range may be split)
        ops.grouped_linear_bwd_weight([(dzs[0], s["x"], G("l0.w"), G("l0.b"))])
        if nl > 1:
            ops.grouped_linear_bwd_weight([(dzs[i], acts[i - 1], G(f"l{i}.w"), G(f"l{i}.b")) for i in range(1, nl)])
        return s["gidx"], occ


class DIN(DinStep, DinEval, LazyTableModel):
    input_type = InputType.SEQ

    def __init__(self, config, dataload):
        super().__init__()
        self._build_attention(config, dataload)
        self.item_embedding = _Rows(self.item_num, self.embedding_size)       # nn.Embedding(padding_idx=0): the init overwrites row 0 (din.py:38-40)
        for mod in self.modules():
            if isinstance(mod, (nn.Linear, _Rows)):
                nn.init.xavier_normal_(mod.weight.data)
                if getattr(mod, "bias", None) is not None:
                    nn.init.zeros_(mod.bias.data)

    # ------------------------------------------------------------------------------------------ packing
    def rec_parameter_names(self):
        """{reference parameter name: flat-buffer key} in the reference's registration order (optim.native_to_torch_state); the
        table maps to None -- its state is the table buffer's (optim.table_spans)."""
        return {**linear_names(self._linears()), "item_embedding.weight": None}

    def table_parameter_spans(self):
        """Rows of the table buffer the table parameter occupies (optim.table_spans)."""
        return {"item_embedding.weight": (1, 1 + self.item_num)}

    # ------------------------------------------------------------------------------------------ training
    def _split_input(self, input):
        """The reference's single [B, L + 2] tensor, or (profile [B, L], target [B, 2]) -> contiguous (profile, target)."""
        return split_tail(input, 2, "DIN: expected [B, L + 2] ids (profile, positive, negative), got profile {profile} and target {tail}")

    def forward(self, input):
        if not self.training:
            raise PxrError("DIN.forward is the training loss (din.py forward); use fused_topk_batch / predict to score")
        self._ensure_packed()
        profile, target = self._split_input(input)
        return TrainStep.apply(self._anchor, self, profile, target)

    def _forward_train(self, profile, target):
        rows, gidx = ops.din_rows(profile, target, self.item_num, out=self._buf("rows", (2, profile.numel() + target.numel()), torch.int64))
        if self._table_hooks is not None:
            self._table_hooks.catch_up_ids(rows)          # the step's rows (the padding item's too), current before anything reads them
        return self._attention_fwd(self._table, rows, gidx, profile, 0.01)       # din.py:79's regulariser

    def _backward_train(self, gsd):
        gidx, occ = self._attention_bwd(gsd)
        # the table gradient: stable sort of the occurrence rows + segmented sum (O(n log n); id 0 = the padding item: dropped)
        self.sparse_table_grad = ops.embed_grad_rows(gidx, occ, self._table.shape[0], out=self._sparse_rows(occ.shape[0]))
        self._step_done()

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def compute_item_all(self):
        """The (flushed) item table [I, D] (din.py compute_item_all)."""
        self._ensure_packed()
        self.sync_table()
        return self.item_embedding.weight

    def _item_rows(self):
        return self.compute_item_all().data
