"""ACF (ViNet) -- drop-in for `REC.model.ViNet.acf.ACF` (code/REC/model/ViNet/acf.py) on the hand-written gfx950 kernels of
csrc/acf.hip and the library's fp32-operand GEMMs.  With the frozen region features v_feat [I, h, w, F] (H = h w regions per item),
a user b with the profile (history) items i_{b,1..P} (left-padded with 0), r = (b, p):

    x_{r,h}  = relu(dim_reductor(v_feat[i_r, h]))          x~ = feats.w_x(x)          u~_b = feats.w_u(user_embedding[b])
    beta_r   = softmax_H(feats.w(relu(x~_{r,h} + u~_b)))    pooled_r = [i_r != 0] sum_h beta_{r,h} x_{r,h}
    alpha_b  = softmax_P over i_r != 0 of w(relu(w_u(user_b) + w_p(item_model[i_r]) + w_x(pooled_r)))      (empty profile: 0)
    user_b   = w_u(user_embedding[b]) + sum_p alpha_{b,p} item_model[i_r]                (the raw user row is NOT added: acf.py:135)
    loss     = -mean_b log sigmoid(<user_b, item_model[pos_b]> - <user_b, item_model[neg_b]>)      (MF's pair head)

The two `w` biases are constant along their softmax axis: they change no output, receive a zero gradient here (rounding noise in
the reference) and are bounded, not matched.

The tables: `item_model.weight` (= `user_model.profile_embedding.weight`, one tensor under two names) and
`user_model.user_embedding.weight` are views of ONE [1 + I + U, E] buffer -- item i at row 1 + i, user u at row 1 + I + u, row 0 a
spare nothing reads.  Item row 0 is the reference's padding row: kept, read by padded profile positions, decayed, never given a
gradient.  PxrAdamW updates the buffer lazily (optim.table_spans): the step's rows are caught up before the forward reads them, the
backward writes one gradient row per occurrence and the stable sort + segmented sum of ops.embed_grad_rows reduces them to
`sparse_table_grad`.  The 16 Linear tensors live in the flat buffer of PxrAdamW's one launch.

Evaluation: x and x~ depend on the item alone.  `compute_item_all()` computes them once for the whole catalogue (chunked over
items, straight from v_feat); `encode_last` / `predict` then gather cached rows and run the two attention kernels in forward form.
The caches (2 x I H E floats) are dropped when the model returns to train().

Contract kept: `input_type = SEQ`; `__init__(config, dataload)` with `embedding_size`, `v_feat_path`, `MAX_ITEM_LIST_LENGTH`;
forward([profile (L) | positive | negative | user id] int64 [B, L + 3], or the same as (profile [B, L], tail [B, 3])) -> loss;
`compute_item_all` (the item table), `predict([profile | user id] [B, L + 1], item_feature)`; `state_dict` keys and order of the
reference (19 keys, both aliases; kaiming-normal init, zero biases), so reference checkpoints load with strict=True; `v_feat` is
neither a parameter nor a buffer.  One process: the data-parallel exchange is not built for this model.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..lib import PxrError
from ..utils.enum_type import InputType
from .packed import LazyTableModel, TrainStep, _Rows, check_width16, dense_scores, linear_names, linear_specs, one_process, split_tail


class _FeatNet(nn.Module):
    """ACFFeatureNet's parameter layout; never called -- the kernels read its parameters."""

    def __init__(self, E, F):
        super().__init__()
        self.dim_reductor = nn.Linear(F, E)
        self.w_x = nn.Linear(E, E)
        self.w_u = nn.Linear(E, E)
        self.w = nn.Linear(E, 1)


class _UserNet(nn.Module):
    """ACFUserNet's parameter layout (profile_embedding is the item table itself); never called."""

    def __init__(self, U, E, F, item_model):
        super().__init__()
        self.feats = _FeatNet(E, F)
        self.user_embedding = _Rows(U, E)
        self.profile_embedding = item_model
        self.w_u = nn.Linear(E, E)
        self.w_p = nn.Linear(E, E)
        self.w_x = nn.Linear(E, E)
        self.w = nn.Linear(E, 1)


# flat-buffer key -> path of the Linear below the model, in the reference's parameter order
_LINEARS = (("fd", "user_model.feats.dim_reductor"), ("fx", "user_model.feats.w_x"), ("fu", "user_model.feats.w_u"),
            ("fw", "user_model.feats.w"), ("wu", "user_model.w_u"), ("wp", "user_model.w_p"), ("wx", "user_model.w_x"),
            ("w", "user_model.w"))


class ACF(LazyTableModel):
    flat_align = 4                     # the one-element biases of the two `w` Linears would shift what follows off 16 bytes
    input_type = InputType.SEQ
    EVAL_CHUNK_ROWS = 1 << 17          # rows (items x regions) per projection launch of compute_item_all

    def __init__(self, config, dataload):
        super().__init__()
        one_process(self)
        self.embedding_size = E = int(config["embedding_size"])
        check_width16(E)
        self.max_seq_length = int(config["MAX_ITEM_LIST_LENGTH"])
        self.user_num = dataload.user_num
        self.item_num = dataload.item_num
        self.v_feat_path = config["v_feat_path"]
        v = torch.tensor(np.asarray(np.load(self.v_feat_path, allow_pickle=True)), dtype=torch.float)
        if v.dim() != 4 or v.shape[0] != self.item_num:
            raise ValueError(f"v_feat_path {self.v_feat_path}: the region features must be [item_num, h, w, F] with item_num = "
                             f"{self.item_num} rows, got shape {tuple(v.shape)}")
        if v.shape[3] % 4:
            raise ValueError(f"v_feat_path {self.v_feat_path}: the feature width F must be a multiple of 4 (16-byte vector "
                             f"accesses), got F = {v.shape[3]}")
        self.regions = v.shape[1] * v.shape[2]
        if self.regions > 1024:
            raise ValueError(f"v_feat_path {self.v_feat_path}: at most 1024 regions per item, got {self.regions}")
        self.feature_dim = F = v.shape[3]
        self.v_feat = v.contiguous()                       # frozen: a plain attribute, not in the state_dict (acf.py:21)
        self.item_model = _Rows(self.item_num, E)          # nn.Embedding(padding_idx=0): the init overwrites row 0 (acf.py:34)
        self.user_model = _UserNet(self.user_num, E, F, self.item_model)
        for mod in self.modules():
            if isinstance(mod, (nn.Linear, _Rows)):
                nn.init.kaiming_normal_(mod.weight.data, nonlinearity="relu")
                if getattr(mod, "bias", None) is not None:
                    nn.init.zeros_(mod.bias.data)
        self.store_ifeatures = None
        self._x_cache = self._xt_cache = None

    # ------------------------------------------------------------------------------------------ packing
    def _linears(self):
        return [(key, path, self.get_submodule(path)) for key, path in _LINEARS]

    def _flat_specs(self):
        """Flat layout: the 16 Linear tensors in the reference's parameter order."""
        return linear_specs(self._linears())

    def rec_parameter_names(self):
        """{reference parameter name: flat-buffer key} in the reference's registration order (optim.native_to_torch_state); the
        tables map to None -- their state is the table's (optim.table_spans).  18 entries: the alias
        user_model.profile_embedding.weight is item_model.weight and is not a parameter of its own."""
        lin = self._linears()                              # the four of `feats`, then the user table, then the user net's four
        return {"item_model.weight": None, **linear_names(lin[:4]), "user_model.user_embedding.weight": None, **linear_names(lin[4:])}

    def table_parameter_spans(self):
        """Rows of the table buffer each table parameter occupies (optim.table_spans), in the reference's order."""
        I = self.item_num
        return {"item_model.weight": (1, 1 + I), "user_model.user_embedding.weight": (1 + I, 1 + I + self.user_num)}

    def _after_pack(self, dev):
        self.v_feat = self.v_feat.to(dev)

    def _drop_eval_cache(self):
        self._x_cache = self._xt_cache = None              # the per-item projections go when training resumes

    # ------------------------------------------------------------------------------------------ training
    def _split_input(self, input, n_tail):
        """The reference's single [B, L + n_tail] tensor, or (profile [B, L], tail [B, n_tail]) -> contiguous (profile, tail)."""
        return split_tail(input, n_tail, f"ACF: expected [B, L + {n_tail}] ids (profile, then {n_tail} trailing columns), got profile "
                                         "{profile} and tail {tail}")

    def forward(self, input):
        if not self.training:
            raise PxrError("ACF.forward is the training loss (acf.py forward); use compute_item_all / predict to score")
        self._ensure_packed()
        profile, tail = self._split_input(input, 3)
        return TrainStep.apply(self._anchor, self, profile, tail)

    def _features(self, profile):
        """profile [B, P] -> (g [R H, F] gathered regions, x = relu(dim_reductor(g)), x~ = feats.w_x(x))."""
        H, F = self.regions, self.feature_dim
        g = ops.embed_gather(self.v_feat.view(self.item_num, H * F), profile.view(-1)).view(-1, F)
        x = ops.linear_epi(g, self._p("fd.w"), self._p("fd.b"), ops.EPI_BIAS_RELU, tag="gemm_kernel<KC,KC,EPI_BIAS_RELU> (ACF dim_reductor)")
        xt = ops.linear_fwd(x, self._p("fx.w"), self._p("fx.b"))
        return g, x, xt

    def _user_vector(self, profile, rows, x, xt):
        """The user net after the feature Linears -> dict of everything the backward reads; 'user' is the output vector."""
        B, P = profile.shape
        R = B * P
        tr = ops.embed_gather(self._table, rows)                                   # [R + n_items + B, E]
        prof, u = tr[:R], tr[tr.shape[0] - B:]
        ut = ops.linear_fwd(u, self._p("fu.w"), self._p("fu.b"))
        uw = ops.linear_fwd(u, self._p("wu.w"), self._p("wu.b"))
        beta, pooled = ops.acf_region_fwd(x, xt, ut, self._p("fw.w").view(-1), profile, self.regions)
        pq = ops.linear_fwd(prof, self._p("wp.w"), self._p("wp.b"))
        cx = ops.linear_fwd(pooled, self._p("wx.w"), self._p("wx.b"))
        alpha, user = ops.acf_item_fwd(uw, pq, cx, prof, self._p("w.w").view(-1), profile)
        return dict(tr=tr, prof=prof, u=u, ut=ut, uw=uw, beta=beta, pooled=pooled, pq=pq, cx=cx, alpha=alpha, user=user)

    def _forward_train(self, profile, tail):
        B, P = profile.shape
        items, user = tail[:, :2].contiguous(), tail[:, 2].contiguous()
        n = B * P + 3 * B
        rows, gidx = ops.acf_rows(profile, items, user, self.item_num, self.user_num, out=self._buf("rows", (2, n), torch.int64))
        if self._table_hooks is not None:
            self._table_hooks.catch_up_ids(rows)          # the step's rows, current through the last step before anything reads them
        g, x, xt = self._features(profile)
        s = self._user_vector(profile, rows, x, xt)
        ie = s["tr"][B * P:B * P + 2 * B]
        loss, coef = ops.mf_pair_fwd(s["user"], ie, B, out=self._buf("head", (2 * B + 1,)))
        s.update(B=B, P=P, profile=profile, gidx=gidx, g=g, x=x, xt=xt, ie=ie, coef=coef)
        self._saved = s
        return loss

    def _backward_train(self, gsd):
        s = self._take_saved()
        B, P, E, H = s["B"], s["P"], self.embedding_size, self.regions
        R = B * P
        n = R + 3 * B
        G = lambda k: self._p(k, grad=True)
        occ = self._buf("occ", (n, E))                     # one gradient row per occurrence: profile | positive, negative | user
        duser = self._buf("duser", (B, E))
        ops.mf_pair_bwd(s["user"], s["ie"], s["coef"], duser, occ[R:R + 2 * B], self.grad_scale, gsd)
        da, dprof = self._buf("da", (R, E)), self._buf("dprof", (R, E))
        duw, dwp = self._buf("duw", (B, E)), self._buf("dwp", (B, E))
        ops.acf_item_bwd(duser, s["uw"], s["pq"], s["cx"], s["prof"], self._p("w.w").view(-1), s["alpha"], da, dprof, duw, dwp)
        ops.colsum(dwp, out=G("w.w").view(-1))
        ops.linear_bwd_input(da, self._p("wp.w"), add=dprof, out=occ[:R])
        dpooled = ops.linear_bwd_input(da, self._p("wx.w"))
        dxt = torch.empty_like(s["xt"])
        dut, dwr = self._buf("dut", (B, E)), self._buf("dwr", (R, E))
        ops.acf_region_bwd(dpooled, s["x"], s["xt"], s["ut"], self._p("fw.w").view(-1), s["profile"], s["beta"], dxt, dut, dwr,
                           self._buf("rws", (R, E)))
        ops.colsum(dwr, out=G("fw.w").view(-1))
        dx = ops.linear_bwd_input(dxt, self._p("fx.w"))
        ops.acf_region_dx(dx, s["x"], s["beta"], dpooled)
        du = ops.linear_bwd_input(duw, self._p("wu.w"))
        ops.linear_bwd_input(dut, self._p("fu.w"), add=du, out=occ[R + 2 * B:])
        # v_feat is frozen: dim_reductor needs no input gradient.  The two long reductions (R H rows) are launches of their own
        # (their token range is split); the four short ones share one grouped launch
        ops.grouped_linear_bwd_weight([(dx, s["g"], G("fd.w"), G("fd.b"))])
        ops.grouped_linear_bwd_weight([(dxt, s["x"], G("fx.w"), G("fx.b"))])
        ops.grouped_linear_bwd_weight([(dut, s["u"], G("fu.w"), G("fu.b")), (duw, s["u"], G("wu.w"), G("wu.b")),
                                       (da, s["prof"], G("wp.w"), G("wp.b")), (da, s["pooled"], G("wx.w"), G("wx.b"))])
        # the table gradient: stable sort of the occurrence rows + segmented sum (O(n log n), not MF's first-occurrence scan)
        self.sparse_table_grad = ops.embed_grad_rows(s["gidx"], occ, self._table.shape[0], out=self._sparse_rows(n))
        self._step_done()

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def compute_item_all(self):
        """The (flushed) item table [I, E] (acf.py compute_item_all); also fills the per-item caches x, x~ [I H, E] that
        encode_last / predict gather from, chunked over items straight from v_feat (no gather)."""
        self._ensure_packed()
        self.sync_table()
        I, H, F, E = self.item_num, self.regions, self.feature_dim, self.embedding_size
        feat = self.v_feat.view(I * H, F)
        xc = torch.empty(I * H, E, dtype=torch.float32, device=feat.device)
        xtc = torch.empty_like(xc)
        step = max(H, self.EVAL_CHUNK_ROWS // H * H)
        for lo in range(0, I * H, step):
            hi = min(I * H, lo + step)
            x = ops.linear_epi(feat[lo:hi], self._p("fd.w"), self._p("fd.b"), ops.EPI_BIAS_RELU,
                               tag="gemm_kernel<KC,KC,EPI_BIAS_RELU> (ACF dim_reductor)")
            xc[lo:hi].copy_(x)
            xtc[lo:hi].copy_(ops.linear_fwd(x, self._p("fx.w"), self._p("fx.b")))
        self._x_cache, self._xt_cache = xc, xtc
        self.store_ifeatures = self._table[1:1 + I]
        return self.store_ifeatures

    @torch.no_grad()
    def encode_last(self, inputs, item_feature=None, use_cache: bool = True):
        """[profile (L) | user id] int64 [B, L + 1] -> (user [B, 1, E], user [B, E]): the user vectors, the queries of the fused
        scoring against the item table.  use_cache=False projects the regions of every history occurrence again (tests)."""
        self._ensure_packed()
        self.sync_table()
        profile, tail = self._split_input(inputs, 1)
        B = profile.shape[0]
        rows, _ = ops.acf_rows(profile, None, tail.view(-1), self.item_num, self.user_num, want_gidx=False)
        if use_cache:
            if self._x_cache is None:
                self.compute_item_all()
            HE = self.regions * self.embedding_size
            ids = profile.view(-1)
            x = ops.embed_gather(self._x_cache.view(self.item_num, HE), ids)
            xt = ops.embed_gather(self._xt_cache.view(self.item_num, HE), ids)
        else:
            _, x, xt = self._features(profile)
        user = self._user_vector(profile, rows, x, xt)["user"]
        return user.view(B, 1, -1), user

    @torch.no_grad()
    def predict(self, inputs, item_feature):
        """scores [B, I] = user item_feature^T (acf.py predict)."""
        feat = item_feature if item_feature is not None else self.store_ifeatures
        if feat is None:
            raise PxrError("ACF: call compute_item_all() before scoring")
        feat = feat if feat.is_contiguous() else feat.contiguous()
        _, u = self.encode_last(inputs, feat)
        return dense_scores(u, feat)
