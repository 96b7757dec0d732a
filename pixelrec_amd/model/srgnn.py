"""SRGNN (IDNet) -- drop-in for `REC.model.IDNet.srgnn.SRGNN` (code/REC/model/IDNet/srgnn.py) on the hand-written gfx950 kernels
of csrc/srgnn.hip and the library's fp32-operand GEMMs.

    session graph (nodes, alias, A = [A_in | A_out])  of item_seq [B, L], right-padded, built on the device at L nodes
    H_0 = embedding[nodes];  step times:  E = H [W_ei; W_eo]^T + [b_ei; b_eo]            (one GEMM)
                                          X = [A_in E_in + b_iah | A_out E_out + b_oah]   (pxr_srgnn_prop_f32)
                                          H = GRU gates(X W_ih^T + b_ih, H W_hh^T + b_hh, H)   (gru.hip)
    P = H [W1; W2]^T + [b1; b2] (one GEMM);  readout: s_t = sigmoid(P1[ht] + P2[alias t]), alpha_t = <w3, s_t>,
    a = sum_t alpha_t sh_t mask_t;  out = W_t [a | ht] + b_t;  loss = -mean(1e-8 + log sigmoid(<out, e+> - <out, e->))

The graph is padded to L nodes, not to the batch's largest node count as the reference's collate does: a padding node has id 0
and no edges, so every output stays the same and the step has one shape -- it is captured once and replayed (graph.py).

The item table is SASRec's: the batch's node and target ids go through the occurrence sort (id rows [B, 3L] = nodes |
target | negative, written by the graph build) before anything reads the table, a lazy PxrAdamW brings exactly those rows up
to date, and the backward leaves the table gradient as sparse rows (`sparse_table_grad`, the segment sums of embed_grad.hip).
The order inside a step is graph build -> occurrence sort -> catch-up -> gather.  Every other parameter lives in one flat
buffer (PxrAdamW's one launch); the step's weight gradients are one grouped launch -- the `step` iterations stack their rows,
so dW_ih, dW_hh and the edge weights are one product each.

Contract kept: `input_type = AUGSEQ`; `__init__(config, dataload)` with `embedding_size`, `step`; forward((item_seq [B, L],
mask [B, L], target [B, 2])) -> loss (or (item_seq, mask | target [B, L + 2]), the form the training loop stages);
`predict(item_seq, item_feature) -> [B, N]`; `compute_item_all` = embedding.weight; `state_dict` names and order of the
reference (`embedding.weight` without padding_idx, `gnn.*`, `linear_{one,two,three,transform}`), every parameter initialised
uniform(-1/sqrt(D), 1/sqrt(D)).  `gnn.linear_edge_f` is read by nothing: it gets no gradient, stays out of the flat buffer and
is never updated (torch.optim.AdamW skips a parameter without a gradient, weight decay included).
An empty history (sum(mask) = 0) reads its `ht` from the last slot, as torch's index -1 does in the reference.
One process: the data-parallel exchange is not built for this model.

Everything between the graph dict and the node gradients lives in the mixin `SrgnnStep`, which MOSRGNN (mosrgnn.py) shares: it
feeds the same step the visual encoder's rows and sums the node gradients into a dense block instead of sparse table rows.
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn as nn

from .. import ops
from ..utils.enum_type import InputType
from .packed import PackedModel, TableHooks, TrainStep, dense_scores, one_process


class _GNN(nn.Module):
    """Parameter container with the reference GNN's names (srgnn.py GNN); its forward is never called."""

    def __init__(self, hidden_size, step):
        super().__init__()
        self.step = step
        self.hidden_size = hidden_size
        self.w_ih = nn.Parameter(torch.empty(3 * hidden_size, 2 * hidden_size))
        self.w_hh = nn.Parameter(torch.empty(3 * hidden_size, hidden_size))
        self.b_ih = nn.Parameter(torch.empty(3 * hidden_size))
        self.b_hh = nn.Parameter(torch.empty(3 * hidden_size))
        self.b_iah = nn.Parameter(torch.empty(hidden_size))
        self.b_oah = nn.Parameter(torch.empty(hidden_size))
        self.linear_edge_in = nn.Linear(hidden_size, hidden_size, bias=True)
        self.linear_edge_out = nn.Linear(hidden_size, hidden_size, bias=True)
        self.linear_edge_f = nn.Linear(hidden_size, hidden_size, bias=True)


class SrgnnStep:
    """Mixin over PackedModel: SRGNN's step between "a graph dict `g` (ops.srgnn_graph's nodes / alias / A) and a row matrix" and
    "the node gradients dH [B, L, D], out_pad and coef_pad" -- the parameters behind the row matrix, their flat packing, the gated
    cells, the readout, the padded linear_transform GEMM, the pair head and their backward with the grouped weight gradients.  Where
    the rows live is the subclass's: SRGNN reads its lazily updated item table and leaves sparse rows, MOSRGNN (mosrgnn.py) reads the
    visual encoder's output and returns a dense block.  The subclass registers whatever precedes `gnn` in the reference's
    state_dict (the table, the encoder) before it calls `_build_gnn`."""

    def _build_gnn(self, config):
        """embedding_size, step and MAX_ITEM_LIST_LENGTH under the kernels' limits, then the reference's modules in its order."""
        self.hidden_size = config["embedding_size"]
        self.step = int(config["step"])
        self.max_seq_length = config["MAX_ITEM_LIST_LENGTH"]
        D = self.hidden_size
        if D % 4:
            raise ValueError("embedding_size must be a multiple of 4 (16-byte vector accesses)")
        if self.step < 1:
            raise ValueError("step must be >= 1")
        if not 1 <= self.max_seq_length <= ops.SRGNN_MAX_L:
            raise ValueError(f"MAX_ITEM_LIST_LENGTH must be in 1..{ops.SRGNN_MAX_L} for SRGNN's session graphs")
        self.gnn = _GNN(D, self.step)
        self.linear_one = nn.Linear(D, D, bias=True)
        self.linear_two = nn.Linear(D, D, bias=True)
        self.linear_three = nn.Linear(D, 1, bias=False)
        self.linear_transform = nn.Linear(2 * D, D, bias=True)
        self._gbufs = {}                                   # the session graph's buffers (ops.srgnn_graph)

    # ------------------------------------------------------------------------------------------ flat packing
    def _flat_specs(self):
        """Flat layout: the two edge Linears side by side (E is one GEMM), b_iah | b_oah (one bias of the propagation),
        linear_one | linear_two (P is one GEMM).  linear_edge_f and the rows stay outside."""
        g = self.gnn
        return [("ein.w", g.linear_edge_in.weight), ("eout.w", g.linear_edge_out.weight),
                ("ein.b", g.linear_edge_in.bias), ("eout.b", g.linear_edge_out.bias),
                ("iah", g.b_iah), ("oah", g.b_oah),
                ("w_ih", g.w_ih), ("b_ih", g.b_ih), ("w_hh", g.w_hh), ("b_hh", g.b_hh),
                ("one.w", self.linear_one.weight), ("two.w", self.linear_two.weight),
                ("one.b", self.linear_one.bias), ("two.b", self.linear_two.bias),
                ("three.w", self.linear_three.weight), ("t.w", self.linear_transform.weight), ("t.b", self.linear_transform.bias)]

    def _gnn_parameter_names(self):
        """{reference parameter name: flat-buffer key} of gnn.* and the four Linears in the reference's registration order:
        linear_edge_f (no gradient, no optimizer state) maps to None."""
        return {"gnn.w_ih": "w_ih", "gnn.w_hh": "w_hh", "gnn.b_ih": "b_ih", "gnn.b_hh": "b_hh",
                "gnn.b_iah": "iah", "gnn.b_oah": "oah", "gnn.linear_edge_in.weight": "ein.w", "gnn.linear_edge_in.bias": "ein.b",
                "gnn.linear_edge_out.weight": "eout.w", "gnn.linear_edge_out.bias": "eout.b", "gnn.linear_edge_f.weight": None,
                "gnn.linear_edge_f.bias": None, "linear_one.weight": "one.w", "linear_one.bias": "one.b",
                "linear_two.weight": "two.w", "linear_two.bias": "two.b", "linear_three.weight": "three.w",
                "linear_transform.weight": "t.w", "linear_transform.bias": "t.b"}

    def _after_pack(self, dev):
        self._gbufs = {}

    # ------------------------------------------------------------------------------------------ the network
    def _gnn_forward(self, table, nodes, A, B, train):
        """H_0 = table[nodes], then `step` gated-GNN cells.  -> (Hs [step + 1, B L, D], saved tensors | None)."""
        L, D, S = self.max_seq_length, self.hidden_size, self.step
        dev = table.device
        BL = B * L
        Hs = torch.empty(S + 1, BL, D, dtype=torch.float32, device=dev)
        ops.embed_gather(table, nodes.reshape(-1), out=Hs[0])
        Xs = torch.empty(S, BL, 2 * D, dtype=torch.float32, device=dev)
        saves = torch.empty(S, BL, 4 * D, dtype=torch.float32, device=dev) if train else None
        We, be, bah = self._p("ein.w", span=2), self._p("ein.b", span=2), self._p("iah", span=2)
        Wih, bih, Whh, bhh = self._p("w_ih"), self._p("b_ih"), self._p("w_hh"), self._p("b_hh")
        for k in range(S):
            E = ops.linear_fwd(Hs[k], We, be)                                        # [BL, 2D] = [E_in | E_out]
            ops.srgnn_prop(A, E, y=Xs[k], bias=bah)                                  # [BL, 2D] = [in | out]
            gi = ops.linear_fwd(Xs[k], Wih, bih)
            gh = ops.linear_fwd(Hs[k], Whh, bhh)
            ops.gru_gates_fwd(gi, gh, Hs[k], Hs[k + 1], saves[k] if train else None)
        return Hs, Xs, saves

    def _readout(self, Hn, alias, mask, B, train):
        """-> cat [B, 2D] = [a | ht] (+ saved sig / alpha when training)."""
        L, D = self.max_seq_length, self.hidden_size
        P = ops.linear_fwd(Hn, self._p("one.w", span=2), self._p("one.b", span=2))      # [BL, 2D] = [q1 | q2] per node
        sig = torch.empty(B, L, D, dtype=torch.float32, device=Hn.device) if train else None
        alpha = torch.empty(B, L, dtype=torch.float32, device=Hn.device) if train else None
        cat = ops.srgnn_readout_fwd(Hn, P, alias, mask, self._p("three.w").view(-1), sig=sig, alpha=alpha)
        return cat, sig, alpha

    def _step_forward(self, table, g, mask, target):
        """The graph dict `g`, mask [B, L] and target [B, 2] rows of `table` -> loss [1]; in training mode `_saved` holds what
        `_step_backward` reads."""
        B, L, D = mask.shape[0], self.max_seq_length, self.hidden_size
        Hs, Xs, saves = self._gnn_forward(table, g["nodes"], g["A"], B, self.training)
        Hn = Hs[self.step]
        cat, sig, alpha = self._readout(Hn, g["alias"], mask, B, self.training)
        # out rows L*D apart: row 0 of each session's [L, D] block, the layout the occurrence segment sums read (coef 0 elsewhere)
        out_pad = self._buf("out_pad", (B, L, D), zero=True)
        ops.gemm(True, True, B, D, 2 * D, cat, 2 * D, self._p("t.w"), 2 * D, out_pad, L * D, ops.EPI_BIAS, bias=self._p("t.b"),
                 use_ws=False)
        loss, coef = ops.srgnn_pair_fwd(out_pad, L * D, table, target, B)
        if self.training:
            self._saved = dict(B=B, g=g, Hs=Hs, Xs=Xs, saves=saves, cat=cat, sig=sig, alpha=alpha, mask=mask, target=target,
                               out_pad=out_pad, coef=coef)
        return loss

    def _step_backward(self, gsd, table, s):
        """What `_step_forward` saved -> (dH [B L, D] = d loss / d H_0 per node, coef_pad [B, L]): with s["out_pad"] the three
        terms of the rows' gradient, which the caller's segment sum joins.  The 17 weight gradients land in the flat buffer."""
        B, L, D, S = s["B"], self.max_seq_length, self.hidden_size, self.step
        BL = B * L
        dev = s["cat"].device
        g = lambda name, span=1: self._p(name, grad=True, span=span)
        dout = self._buf("dout", (B, D))
        coef_pad = self._buf("coef_pad", (B, L), zero=True)
        ops.srgnn_pair_bwd(table, s["target"], s["coef"], dout, D, self.grad_scale, gsd, coef_out=coef_pad, coef_stride=L)
        dcat = ops.linear_bwd_input(dout, self._p("t.w"))                                  # [B, 2D]
        Hs, Xs, saves = s["Hs"], s["Xs"], s["saves"]
        Hn = Hs[S]
        gr = s["g"]
        dP, dHr, dw3p = ops.srgnn_readout_bwd(dcat, Hn, gr["alias"], s["mask"], self._p("three.w").view(-1), s["sig"], s["alpha"])
        ops.colsum(dw3p, out=g("three.w").view(-1))
        dH = ops.linear_bwd_input(dP, self._p("one.w", span=2), add=dHr)                  # d loss / d H_step  [BL, D]
        dgi = torch.empty(S, BL, 3 * D, dtype=torch.float32, device=dev)
        dgh = torch.empty(S, BL, 3 * D, dtype=torch.float32, device=dev)
        dX = torch.empty(S, BL, 2 * D, dtype=torch.float32, device=dev)
        dE = torch.empty(S, BL, 2 * D, dtype=torch.float32, device=dev)
        direct = torch.empty(BL, D, dtype=torch.float32, device=dev)
        We, Wih, Whh = self._p("ein.w", span=2), self._p("w_ih"), self._p("w_hh")
        for k in reversed(range(S)):
            ops.gru_gates_bwd(dH, saves[k], Hs[k], dgi[k], dgh[k], direct)
            ops.linear_bwd_input(dgi[k], Wih, out=dX[k])
            ops.srgnn_prop(gr["A"], dX[k], y=dE[k], transpose=True)
            t1 = ops.linear_bwd_input(dgh[k], Whh, add=direct)
            dH = ops.linear_bwd_input(dE[k], We, add=t1)                                  # d loss / d H_k
        ops.colsum(dX.view(S * BL, 2 * D), out=g("iah", span=2))                          # b_iah | b_oah
        Hprev = Hs[:S].reshape(S * BL, D)
        ops.grouped_linear_bwd_weight([
            (dout, s["cat"], g("t.w"), g("t.b")),
            (dP, Hn, g("one.w", span=2), g("one.b", span=2)),
            (dgi.view(S * BL, 3 * D), Xs.view(S * BL, 2 * D), g("w_ih"), g("b_ih")),
            (dgh.view(S * BL, 3 * D), Hprev, g("w_hh"), g("b_hh")),
            (dE.view(S * BL, 2 * D), Hprev, g("ein.w", span=2), g("ein.b", span=2)),
        ])
        return dH, coef_pad

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def _encode(self, item_seq, table):
        """item_seq int64 [B, L] (right-padded; mask = item_seq != 0) with its node rows in `table` -> out [B, D]."""
        if item_seq.dim() != 2 or item_seq.shape[1] != self.max_seq_length:
            raise ValueError(f"item_seq must be [B, {self.max_seq_length}], got {tuple(item_seq.shape)}")
        item_seq = item_seq.contiguous()
        B = item_seq.shape[0]
        g = ops.srgnn_graph(item_seq, table.shape[0], want_mask=True)
        Hs, _, _ = self._gnn_forward(table, g["nodes"], g["A"], B, train=False)
        cat, _, _ = self._readout(Hs[self.step], g["alias"], g["mask"], B, train=False)
        return ops.linear_fwd(cat, self._p("t.w"), self._p("t.b"))                         # [B, D]


class SRGNN(SrgnnStep, TableHooks, PackedModel):
    input_type = InputType.AUGSEQ
    item_table_attr = "embedding"          # the reference's table name (optim.item_table_name)

    def __init__(self, config, dataload):
        super().__init__()
        one_process(self, "the graph models")
        self.item_num = dataload.item_num
        D = config["embedding_size"]
        self.embedding = nn.Embedding(self.item_num, D)
        self._build_gnn(config)
        stdv = 1.0 / math.sqrt(D)
        for w in self.parameters():                       # srgnn.py _reset_parameters, in parameter order
            w.data.uniform_(-stdv, stdv)
        self._local_sparse = None                          # the sparse table (SASRec's bookkeeping)
        self._occ_ws = self._occ_ws2 = None

    def rec_parameter_names(self):
        """{reference parameter name: flat-buffer key} in the reference's registration order (optim.native_to_torch_state):
        the table and linear_edge_f (no gradient, no optimizer state) map to None."""
        return {"embedding.weight": None, **self._gnn_parameter_names()}

    # ------------------------------------------------------------------------------------------ the table (SASRec's machinery)
    def _table_prepare(self, g, B, L, D, device):
        """Occurrence sort of the batch's node and target ids, then the lazy catch-up of exactly those rows."""
        cap = B * (L + 2)
        sp = self._local_sparse
        if sp is None or sp.cap != cap or sp.rows.shape[1] != D or sp.rows.device != device:
            sp = self._local_sparse = ops.SparseRows(cap, D, device, packed=True)
        need = ops.occ_ws_bytes(B, L)
        if self._occ_ws is None or self._occ_ws.numel() < need or self._occ_ws.device != device:
            self._occ_ws = torch.empty(need, dtype=torch.uint8, device=device)
        env = os.environ.get("PXR_SEGSUM_SPLIT", "auto")
        need2 = ops.occ_split_ws_bytes(B, L, D) if (env == "1" or (env != "0" and 3 * B * L >= 30000)) else 0
        if need2 == 0:
            self._occ_ws2 = None
        elif self._occ_ws2 is None or self._occ_ws2.numel() != need2 or self._occ_ws2.device != device:
            self._occ_ws2 = torch.zeros(need2, dtype=torch.uint8, device=device)
        ops.occ_sort(g["occ"], L, (3 * L, 0, L, 2 * L), self.item_num, sp, self._occ_ws)
        if self._table_hooks is not None:
            self._table_hooks.catch_up_rows(sp.idx, sp.n, sp.cap)
        return sp

    # ------------------------------------------------------------------------------------------ training
    def forward(self, interaction):
        """interaction = (item_seq [B, L], mask [B, L], target [B, 2]) or (item_seq, mask | target [B, L + 2]) -> 0-dim loss."""
        if len(interaction) == 3:
            item_seq, mask, target = interaction
        else:
            item_seq, tail = interaction
            L = self.max_seq_length
            mask, target = tail[:, :L], tail[:, L:L + 2]
        L = self.max_seq_length
        if item_seq.dim() != 2 or item_seq.shape[1] != L:
            raise ValueError(f"item_seq must be [B, {L}], got {tuple(item_seq.shape)}")
        self._ensure_packed()
        item_seq, mask, target = item_seq.contiguous(), mask.contiguous(), target.contiguous()
        if torch.is_grad_enabled() and self.training:
            return TrainStep.apply(self._anchor, self, item_seq, mask, target)
        was = self.training
        try:
            self.training = False
            return self._forward_train(item_seq, mask, target).view(())
        finally:
            self.training = was

    def _forward_train(self, item_seq, mask, target):
        B, L, D = item_seq.shape[0], self.max_seq_length, self.hidden_size
        table = self.embedding.weight.data
        g = ops.srgnn_graph(item_seq, self.item_num, target, want_occ=self.training, out=self._gbufs)
        if self.training:
            sp = self._table_prepare(g, B, L, D, item_seq.device)
        elif self._table_hooks is not None:
            self.sync_table()
        loss = self._step_forward(table, g, mask, target)
        if self.training:
            self._saved["sp"] = sp
        return loss

    def _backward_train(self, gsd):
        s = self._take_saved()
        B, L, D = s["B"], self.max_seq_length, self.hidden_size
        dH, coef_pad = self._step_backward(gsd, self.embedding.weight.data, s)
        sp = s["sp"]
        ops.sasrec_occ_segsum(self._occ_ws, dH.view(B, L, D), s["out_pad"], coef_pad, self.item_num, sp, 1.0, ws2=self._occ_ws2)
        self.sparse_table_grad = sp
        self._step_done()

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def encode_last(self, item_seq, item_feature=None):
        """item_seq int64 [B, L] (right-padded; mask = item_seq != 0) -> (out [B, 1, D], out [B, D]): the query vectors of the
        fused scoring (`last` with row stride D)."""
        self._ensure_packed()
        self.sync_table()
        table = self.embedding.weight.data if item_feature is None else item_feature.contiguous()
        out = self._encode(item_seq, table)
        return out.view(out.shape[0], 1, -1), out

    @torch.no_grad()
    def predict(self, item_seq, item_feature):
        """scores [B, N] = seq_output item_feature^T (srgnn.py predict: the node rows are read from item_feature)."""
        feat = item_feature if item_feature.is_contiguous() else item_feature.contiguous()
        _, out = self.encode_last(item_seq, feat)
        return dense_scores(out, feat)

    @torch.no_grad()
    def compute_item_all(self):
        self.sync_table()
        return self.embedding.weight
