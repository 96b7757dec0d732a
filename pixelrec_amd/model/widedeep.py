"""WideDeep (IDNet) -- drop-in for `REC.model.IDNet.widedeep.WideDeep` (code/REC/model/IDNet/widedeep.py, with MLPLayers of
code/REC/model/layers.py:239-281) on the hand-written gfx950 kernels of csrc/widedeep.hip and the library's fp32-operand GEMMs.
With the tables wide [I, 1] and deep [I, D], a row of W = L + 1 ids (the profile's L positions, left-padded with 0, then the target):

    y(row)  = sum_w wide[row_w] + wide_bias + predict(mlp(concat_w deep[row_w]))           mlp: (Dropout -> Linear -> ReLU) per layer
    x_b     = y([profile_b | p_b]) - y([profile_b | n_b])
    loss    = -mean_b log(1e-8 + sigmoid(x_b))

There is no padding mask anywhere: a padded position reads row 0 of both tables, which the reference's xavier_normal_ leaves
non-zero.  Row 0 never receives a gradient (padding_idx=0) and is still decayed by AdamW every step.

Three facts about the reference that this model writes down instead of imitating:

1. Width.  The reference sizes the first Linear by embedding_size * MAX_ITEM_LIST_LENGTH (widedeep.py:31), but the datasets that
   feed it (OneTowerTrainDataset, trainset.py:337; CandiEvalDataset) deliver MAX_ITEM_LIST_LENGTH + 1 ids per row.  Here
   MAX_ITEM_LIST_LENGTH stays the history length L, so ID.yaml and the batchers are unchanged, and the first Linear is
   [(L + 1) D -> h_1].  A reference model built with MAX_ITEM_LIST_LENGTH = L + 1 has exactly these shapes; its checkpoints load with
   strict=True.
2. Cancellation.  In x_b the history's wide terms, wide_bias and deep_predict_layer.bias cancel exactly:
   x_b = <a_last(+) - a_last(-), w_p> + wide[p_b] - wide[n_b].  The gradients of wide_bias, of the predict bias and of every history
   wide entry are exactly 0.  The native step computes this cancelled form; the reference computes the literal form in float32 (its
   two bias gradients are rounding residue of a sum that is zero).  The three parameters still enter predict()'s values, where a
   loaded checkpoint may hold non-zero ones.
3. Data.  The reference ships no yaml and no dataset entry for this model.  Training uses OneTowerTrainDataset's sampling -- one
   sample per training chunk: the chunk without its last item is the profile, the last item the positive, one negative drawn from
   outside the chunk -- which CuratorTrainBatcher already yields; evaluation is SeqEvalBatcher's windows with the model-side
   `fused_topk_batch`, as for DIN.

`dropout_prob > 0` raises NotImplementedError: dropout on the input layer draws different masks for the two planes of a sample, so
the shared-history form below no longer applies, and the literal path is not built.

The deep table is ONE [1 + I, D] buffer, item i at row 1 + i, row 0 a spare nothing reads (the sparse-row machinery treats id 0 as
an empty slot): `deep_item_embedding.weight` is the view of rows 1 .. I under the lazy row AdamW, caught up before the forward
reads it.  The wide table is a dense [I] vector in PxrAdamW's flat buffer beside wide_bias, the Linears and the predict layer: the
dense sweep decays every entry, which is the reference's AdamW on an [I, 1] parameter.

A step: row list + catch-up -> one gather of the B (L + 2) occurrence rows -> the first Linear SPLIT over the concatenation (the two
planes of a sample share the L history positions: Zh = Xh W1[:, :L D]^T for B rows, Zt = Xt W1[:, L D:]^T for 2 B rows, both library
GEMMs on column blocks of the one W1) -> join kernel (add, bias, ReLU, derivative) -> the deeper Linears with the ReLU epilogue ->
head forward (cancelled x_b, loss, coef) -> head backward (last-layer gradient, d w_p, exact zeros for the two cancelled biases,
the dense wide gradient) -> the input-gradient GEMMs -> join backward (the two planes' gradients of Zh added) -> dXh and dXt written
straight into one [B (L + 2), D] gradient-row buffer in occurrence order -> stable sort + segmented sum into `sparse_table_grad`.
The grouped weight-gradient launch takes no leading dimension, so the two column blocks of d W1 are plain GEMMs into the
gradient's column blocks; the deeper layers' gradients are one grouped launch.

Evaluation: T = deep W1[:, L D:]^T + b1 is made once per evaluation and cached until train(); per batch h_b = W1[:, :L D] xh_b is
one gather and one GEMM, and pxr_wd_topk_f32 scores, masks and ranks the batch in one launch without any [B, N, *] tensor.
`predict` takes a [B, L] window batch (candidate chunks through T and h_b) or the reference's [B, item_num, L + 1] id tensor (row
chunks through the split first Linear); the literal [B N, (L + 1) D] input is never built.

Contract kept: `input_type = SEQ`; `__init__(config, dataload)`; forward([B, 2, L + 1] int64, or (profile [B, L], target [B, 2]))
-> loss; `compute_item_all()` -> the deep table (the reference returns None); `state_dict` keys and order of the reference.  One
process: the data-parallel exchange is not built for this model.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..lib import PxrError
from ..utils.enum_type import InputType
from .packed import (LazyTableModel, TrainStep, _ActMLP, _Rows, check_width16, hidden_sizes, linear_names, linear_specs, one_process,
                     split_planes)


class WideDeep(LazyTableModel):
    flat_align = 4                     # the one-element biases would shift what follows off 16 bytes
    input_type = InputType.SEQ
    PREDICT_CHUNK_ROWS = 1 << 16       # (user, candidate) rows per chunk of the GEMM-path predict

    def __init__(self, config, dataload):
        super().__init__()
        one_process(self)
        self.embedding_size = D = int(config["embedding_size"])
        check_width16(D)
        self.mlp_hidden_size = hidden = hidden_sizes(config["mlp_hidden_size"] if "mlp_hidden_size" in config else None)
        if not hidden or any(h <= 0 or h % 4 or h > 4096 for h in hidden):
            raise ValueError(f"mlp_hidden_size must hold one or more positive multiples of 4, at most 4096 each (widedeep.py:33 reads "
                             f"its last entry; the weight-gradient GEMMs' vector accesses); got {hidden}")
        self.dropout_prob = float((config["dropout_prob"] if "dropout_prob" in config else 0.0) or 0.0)
        if self.dropout_prob > 0:
            raise NotImplementedError("WideDeep: dropout_prob > 0 is not built (dropout on the input layer draws different masks for "
                                      "the two planes of a sample, so the history's part of the first Linear is no longer shared)")
        L = config["MAX_ITEM_LIST_LENGTH"] if "MAX_ITEM_LIST_LENGTH" in config else None
        if not L or int(L) < 1:
            raise ValueError("WideDeep: MAX_ITEM_LIST_LENGTH (the history length L; the first Linear is [(L + 1) D -> h_1]) is required")
        self.max_seq_length = L = int(L)
        self.item_num = I = dataload.item_num
        # the reference's registration order (widedeep.py:25-33)
        self.wide_item_embedding = _Rows(I, 1)      # nn.Embedding(padding_idx=0): the init overwrites row 0 (widedeep.py:41-43)
        self.wide_bias = nn.Parameter(torch.zeros(1))
        self.deep_item_embedding = _Rows(I, D)
        self.mlp_layers = _ActMLP([(L + 1) * D] + hidden, nn.ReLU)       # MLPLayers(sizes, dropout, activation='relu', bn=False)
        self.deep_predict_layer = nn.Linear(hidden[-1], 1)
        for mod in self.modules():
            if isinstance(mod, (nn.Linear, _Rows)):
                nn.init.xavier_normal_(mod.weight.data)
                if getattr(mod, "bias", None) is not None:
                    nn.init.zeros_(mod.bias.data)
        self._eval_cache = None
        self._mlp_keys = [f"l{i}" for i in range(len(hidden))]     # the flat-buffer keys of the MLP's Linears

    # ------------------------------------------------------------------------------------------ packing
    def _linears(self):
        """(flat-buffer key, reference path, module) of the Linears in the reference's parameter order."""
        out = []
        for i in range(len(self.mlp_hidden_size)):
            out.append((f"l{i}", f"mlp_layers.mlp_layers.{3 * i + 1}", self.mlp_layers.mlp_layers[3 * i + 1]))
        out.append(("pred", "deep_predict_layer", self.deep_predict_layer))
        return out

    def _flat_specs(self):
        return [("wide.w", self.wide_item_embedding.weight), ("wide.b", self.wide_bias)] + linear_specs(self._linears())

    def rec_parameter_names(self):
        """{reference parameter name: flat-buffer key} in the order the reference's .parameters() yields them (a module's own
        parameter, wide_bias, comes before its submodules'; optim.native_to_torch_state); the deep table maps to None -- its state is
        the table buffer's (optim.table_spans)."""
        return {"wide_bias": "wide.b", "wide_item_embedding.weight": "wide.w", "deep_item_embedding.weight": None,
                **linear_names(self._linears())}

    def table_parameter_spans(self):
        """Rows of the table buffer the deep table occupies (optim.table_spans)."""
        return {"deep_item_embedding.weight": (1, 1 + self.item_num)}

    def _drop_eval_cache(self):
        self._eval_cache = None                # the per-item term T goes when training resumes

    # ------------------------------------------------------------------------------------------ training
    def _split_input(self, input):
        """The reference's [B, 2, L + 1] tensor, or (profile [B, L], target [B, 2]) -> contiguous (profile, target)."""
        profile, target = split_planes(input, "WideDeep", "WideDeep: expected a profile [B, L] and targets [B, 2] (positive, negative), got "
                                                          "{profile} and {tail}", min_len=0)
        if profile.shape[1] != self.max_seq_length:
            raise ValueError(f"WideDeep: the profile must have MAX_ITEM_LIST_LENGTH = {self.max_seq_length} positions (the first "
                             f"Linear is [(L + 1) D -> h_1]), got {profile.shape[1]}")
        return profile, target

    def forward(self, input):
        if not self.training:
            raise PxrError("WideDeep.forward is the training loss (widedeep.py forward); use fused_topk_batch / predict to score")
        self._ensure_packed()
        profile, target = self._split_input(input)
        return TrainStep.apply(self._anchor, self, profile, target)

    def _w1_blocks(self):
        """(W1h = W1[:, :L D], W1t = W1[:, L D:], leading dimension): column blocks of the one first Linear, never copied."""
        W1 = self._p("l0.w")
        LD = self.max_seq_length * self.embedding_size
        return W1, W1[:, LD:], W1.shape[1]

    def _first_layer(self, xh, xt, a1=None, der=None, zh=None, zt=None):
        """xh [B, L D], xt [2 B, D] -> (a1 [2 B, h1], der): two library GEMMs on W1's column blocks, then the join."""
        W1h, W1t, ld = self._w1_blocks()
        B, LD = xh.shape
        D, h1 = xt.shape[1], W1h.shape[0]
        zh = zh if zh is not None else torch.empty(B, h1, dtype=torch.float32, device=xh.device)
        zt = zt if zt is not None else torch.empty(2 * B, h1, dtype=torch.float32, device=xh.device)
        ops.gemm(True, True, B, h1, LD, xh, LD, W1h, ld, zh, h1)
        ops.gemm(True, True, 2 * B, h1, D, xt, D, W1t, ld, zt, h1)
        return ops.wd_join(zh, zt, self._p("l0.b"), a1=a1, der=der)

    def _deeper(self, a1, der1=None):
        """The first layer's activation (and derivative) -> (activations, derivatives) of every layer: the Linears after the first
        are library GEMMs with the ReLU epilogue."""
        acts, ders = self._act_chain(a1, self._mlp_keys[1:], "relu")
        return [a1] + acts, [der1] + ders

    def _forward_train(self, profile, target):
        B, L = profile.shape
        D, h1 = self.embedding_size, self.mlp_hidden_size[0]
        n = B * (L + 2)
        rows, gidx = ops.din_rows(profile, target, self.item_num, out=self._buf("rows", (2, n), torch.int64))
        if self._table_hooks is not None:
            self._table_hooks.catch_up_ids(rows)          # the step's rows (the padding item's too), current before anything reads them
        emb = ops.embed_gather(self._table, rows, out=self._buf("emb", (n, D)))
        xh, xt = emb[:B * L].view(B, L * D), emb[B * L:]
        a1, der = self._first_layer(xh, xt, a1=self._buf("a1", (2 * B, h1)), der=self._buf("der1", (2 * B, h1)),
                                    zh=self._buf("zh", (B, h1)), zt=self._buf("zt", (2 * B, h1)))
        acts, ders = self._deeper(a1, der)
        loss, head = ops.wd_head_fwd(acts[-1], self._p("pred.w").view(-1), self._p("wide.w").view(-1), target,
                                     head=self._buf("head", (1 + 2 * B,)))
        self._saved = dict(B=B, L=L, target=target, gidx=gidx, xh=xh, xt=xt, acts=acts, ders=ders, head=head)
        return loss

    def _backward_train(self, gsd):
        s = self._take_saved()
        B, L, D = s["B"], s["L"], self.embedding_size
        n, LD = B * (L + 2), L * D
        nl, h1 = len(self.mlp_hidden_size), self.mlp_hidden_size[0]
        G = lambda k: self._p(k, grad=True)
        acts, ders = s["acts"], s["ders"]
        dzl = ops.wd_head_bwd(acts[-1], ders[-1], self._p("pred.w").view(-1), s["target"], s["head"], G("pred.w").view(-1),
                              G("pred.b"), G("wide.w").view(-1), G("wide.b"), self.grad_scale, gsd,
                              dz=self._buf("dzl", (2 * B, self.mlp_hidden_size[-1])))
        dzs = self._act_chain_bwd(dzl, self._mlp_keys, ders)
        dz1 = dzs[0]
        dzh = ops.wd_join_bwd(dz1, dzh=self._buf("dzh", (B, h1)))
        # dXh [B, L D] and dXt [2 B, D] straight into the gradient rows, in occurrence order (history (b, l), then target 2 b + c)
        W1h, W1t, ld = self._w1_blocks()
        occ = self._buf("occ", (n, D))
        ops.gemm(True, False, B, LD, h1, dzh, h1, W1h, ld, occ[:B * L], LD)
        ops.gemm(True, False, 2 * B, D, h1, dz1, h1, W1t, ld, occ[B * L:], D)
        # d W1's two column blocks: the grouped launch takes no leading dimension, so two plain GEMMs write them in place (no
        # split-K: its partials need a dense output); d b1 is the column sum of dZ1
        gW1 = G("l0.w")
        ops.gemm(False, False, h1, LD, B, dzh, h1, s["xh"], LD, gW1, ld, use_ws=False)
        ops.gemm(False, False, h1, D, 2 * B, dz1, h1, s["xt"], D, gW1[:, LD:], ld, use_ws=False)
        ops.colsum(dz1, out=G("l0.b"))
        if nl > 1:
            ops.grouped_linear_bwd_weight([(dzs[i], acts[i - 1], G(f"l{i}.w"), G(f"l{i}.b")) for i in range(1, nl)])
        # the table gradient: stable sort of the occurrence rows + segmented sum (id 0 = the padding item: dropped)
        self.sparse_table_grad = ops.embed_grad_rows(s["gidx"], occ, self._table.shape[0], out=self._sparse_rows(n))
        self._step_done()

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def compute_item_all(self):
        """The (flushed) deep table [I, D] (the reference's compute_item_all returns None; the Trainer wants a table)."""
        self._ensure_packed()
        self.sync_table()
        return self.deep_item_embedding.weight

    @property
    def fused_topk_supported(self) -> bool:
        return ops.wd_topk_supported(self.mlp_hidden_size, self.max_seq_length)

    def _eval_T(self):
        """T [I, h1] = deep W1[:, L D:]^T + b1: once per evaluation, cached until train()."""
        if self._eval_cache is None:
            self._ensure_packed()
            self.sync_table()
            deep = self.deep_item_embedding.weight.data
            _, W1t, ld = self._w1_blocks()
            I, D = deep.shape
            h1 = W1t.shape[0]
            T = torch.empty(I, h1, dtype=torch.float32, device=deep.device)
            ops.gemm(True, True, I, h1, D, deep, D, W1t, ld, T, h1, epilogue=ops.EPI_BIAS, bias=self._p("l0.b"), use_ws=False)
            self._eval_cache = (T,)
        return self._eval_cache[0]

    def _check_window(self, window):
        if window.dim() != 2 or window.shape[1] != self.max_seq_length:
            raise ValueError(f"WideDeep: windows must be [B, MAX_ITEM_LIST_LENGTH = {self.max_seq_length}], got {tuple(window.shape)}")

    def _window_term(self, window):
        """h_b [B, h1] = W1[:, :L D] xh_b: one gather (padding reads row 0, like the reference) and one GEMM."""
        deep = self.deep_item_embedding.weight.data
        W1h, _, ld = self._w1_blocks()
        B, L = window.shape
        LD, h1 = L * deep.shape[1], W1h.shape[0]
        xw = ops.embed_gather(deep, window)
        hb = torch.empty(B, h1, dtype=torch.float32, device=deep.device)
        ops.gemm(True, True, B, h1, LD, xw, LD, W1h, ld, hb, h1)
        return hb

    @torch.no_grad()
    def fused_topk_batch(self, window, hist_ptr, hist_items, K: int):
        """window int64 [B, L] left-padded with 0 + the CSR of the full histories -> top-K ids int64 [B, K] (pxr_wd_topk_f32)."""
        return self.fused_topk(window, hist_ptr, hist_items, K)[0]

    @torch.no_grad()
    def fused_topk(self, window, hist_ptr, hist_items, K: int):
        """-> (ids int64 [B, K], values fp32 [B, K])."""
        window = window.contiguous()
        self._check_window(window)
        if not ops.wd_topk_supported(self.mlp_hidden_size, window.shape[1], K):
            raise PxrError(f"WideDeep: the fused top-k takes one or two hidden layers of at most {ops.WD_MAX_HIDDEN} units, windows of "
                           f"at most {ops.WD_MAX_L} items and K <= 32; evaluate through predict() (eval_fused_topk: False)")
        T = self._eval_T()
        two = len(self.mlp_hidden_size) == 2
        return ops.wd_topk(T, self._window_term(window), window, self._p("wide.w").view(-1), self._p("wide.b"),
                           self._p("l1.w") if two else None, self._p("l1.b") if two else None, self._p("pred.w").view(-1),
                           self._p("pred.b"), K, hist_ptr, hist_items)

    def _tail(self, a1):
        """a1 [M, h1] the first layer's activations -> the deep output [M] (deeper Linears: library GEMMs; the predict layer)."""
        acts, _ = self._deeper(a1)
        return acts[-1] @ self._p("pred.w").view(-1) + self._p("pred.b")

    @torch.no_grad()
    def predict(self, item_seq, item_feature=None):
        """scores [B, item_num].  item_seq: a [B, L] window batch -- candidates in chunks through T and h_b -- or the reference's
        [B, item_num, L + 1] id tensor (widedeep.py:66-79: the window repeated per candidate, the candidate id last) -- rows in
        chunks through the split first Linear; [B item_num, (L + 1) D] never exists.  item_feature is accepted for the Trainer's call
        and must be the deep table.  A bad id raises IndexError."""
        self._ensure_packed()
        self.sync_table()
        deep = self.deep_item_embedding.weight.data
        wide, wb = self._p("wide.w").view(-1), self._p("wide.b")
        N, D = deep.shape
        item_seq = item_seq.to(deep.device)
        if item_seq.dim() == 2:
            window = item_seq.contiguous()
            self._check_window(window)
            B = window.shape[0]
            T, hb = self._eval_T(), self._window_term(window)
            ops.raise_on_bad_indices(deep.device)          # before the wide vector is indexed by the same ids
            sb = wide[window].sum(1) + wb                  # [B]
            out = torch.empty(B, N, dtype=torch.float32, device=deep.device)
            step = max(1, self.PREDICT_CHUNK_ROWS // B)
            for lo in range(0, N, step):
                a1 = torch.relu(T[lo:lo + step][None, :, :] + hb[:, None, :])
                out[:, lo:lo + step] = self._tail(a1.view(-1, a1.shape[-1])).view(B, -1) + wide[None, lo:lo + step] + sb[:, None]
            return out
        if item_seq.dim() != 3 or item_seq.shape[2] != self.max_seq_length + 1:
            raise ValueError(f"WideDeep.predict: item_seq must be [B, item_num, L + 1] or [B, L] with L = {self.max_seq_length}, got "
                             f"{tuple(item_seq.shape)}")
        B, L = item_seq.shape[0], self.max_seq_length
        flat = item_seq.reshape(-1, L + 1)
        out = torch.empty(flat.shape[0], dtype=torch.float32, device=deep.device)
        step = max(1, self.PREDICT_CHUNK_ROWS // (L + 1))
        W1h, W1t, ld = self._w1_blocks()
        h1 = W1h.shape[0]
        for lo in range(0, flat.shape[0], step):
            ids = flat[lo:lo + step].contiguous()
            m = ids.shape[0]
            x = ops.embed_gather(deep, ids)                # [m, L + 1, D]: the chunk's rows of the literal input, no more
            ops.raise_on_bad_indices(deep.device)
            z = torch.empty(m, h1, dtype=torch.float32, device=deep.device)
            ops.gemm(True, True, m, h1, (L + 1) * D, x, (L + 1) * D, W1h, ld, z, h1, epilogue=ops.EPI_BIAS_RELU, bias=self._p("l0.b"),
                     use_ws=False)
            out[lo:lo + step] = self._tail(z) + wide[ids].sum(1) + wb
        return out.view(B, -1)
