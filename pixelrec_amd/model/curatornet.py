"""CuratorNet (ViNet) -- drop-in for `REC.model.ViNet.curatornet.CuratorNet` (code/REC/model/ViNet/curatornet.py) on the
hand-written gfx950 kernels of csrc/curator.hip and the library's fp32-operand GEMMs with the SELU epilogue.  With the frozen
features v_feat [I, F] (row 0 zero-filled after loading), E = embedding_size, Hd = hidden_size * E, a sample b with the profile
items i_{b,1..L} (left-padded with 0), the positive p_b and the negative n_b:

    c(i)   = selu(selu_common2(selu(selu_common1(v_feat[i]))))                          the "common" tower, every item alike
    u_b    = selu(selu_pu3(selu(selu_pu2(selu(selu_pu1([max_l c(i_{b,l}) | mean_l c(i_{b,l})]))))))
    loss   = -mean_b log(1e-8 + sigmoid(<u_b, c(p_b)> - <u_b, c(n_b)>))                 (the 1e-8 inside the log, unlike MF's head)

The pooling includes the padded positions, literally as the reference does: AdaptiveMaxPool2d / AdaptiveAvgPool2d((1, E)) on
[B, L, E] pool over all L positions, a padded position is item 0 whose zero feature row gives the constant row c(0) =
selu(selu_common2(selu(selu_common1.bias))), the mean divides by L and not by the number of real items, and `predict` does the same
with item_feature[0].  The max keeps the first of equal positions (torch's rule; the padded rows tie exactly).

No trainable table: every parameter is a dense Linear.  The ten tensors live in one flat buffer under PxrAdamW's single launch;
`embedding.weight` is the frozen feature matrix (requires_grad=False, in the state_dict like the reference's
nn.Embedding.from_pretrained, never given a gradient, never touched by the optimizer).

A step: gather of the B (L + 2) feature rows [profile rows | positive, negative per sample] -> two Linears with the SELU epilogue
(activation and its derivative in one pass) -> pooling kernel, reading the tower's output in place -> three Linears -> pair head (its own forward: the
reference's 1e-8 sits inside the log, so a badly ranked pair saturates; MF's head has it outside).
Backward: MF's pair-head backward on that head's coefficients -> the three profile Linears (the saved derivative multiplied in the input-gradient GEMM's epilogue) -> ONE
pooling-backward launch that writes the whole [B (L + 2), E] gradient of selu_common2's pre-activation (mean path, max path,
head's item gradient, SELU derivative) -> selu_common2's input gradient -> the weight gradients.  selu_common1 gets no input
gradient: the features are frozen.

Evaluation: `compute_item_all()` runs the common tower over the catalogue in chunks (the derivative buffer stays one chunk wide)
and caches the result until train(); `encode_last` pools the gathered rows of that matrix by id (predict's item_feature[user], so
[B, L, E] never exists) and runs the profile tower; the fused top-k scores its output against the matrix.

Contract kept: `input_type = SEQ`; `__init__(config, dataload)` with `embedding_size`, `hidden_size` (a multiplier), `v_feat_path`;
forward([profile (L) | positive | negative] int64 [B, L + 2], or the same as (profile [B, L], target [B, 2])) -> loss;
`compute_item_all() -> [item_num, E]`; `predict(item_seq [B, L], item_feature)`; `state_dict` = the reference's eleven keys in
its order, so reference checkpoints load with strict=True; xavier-uniform weights, nn.Linear's default biases.  The reference
names a training dataset class that does not exist (REC/data/utils.py:39) and ships no yaml: see data.dataset.CuratorTrainBatcher
and configs/ViNet/curatornet.yaml.  One process: the data-parallel exchange is not built for this model.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..lib import PxrError
from ..utils.enum_type import InputType
from .packed import PackedModel, TrainStep, check_width16, dense_scores, linear_names, linear_specs, one_process, split_tail


# flat-buffer key -> the Linear's attribute, in the reference's parameter order (curatornet.py:29-37)
_LINEARS = (("c1", "selu_common1"), ("c2", "selu_common2"), ("p1", "selu_pu1"), ("p2", "selu_pu2"), ("p3", "selu_pu3"))
_COMMON, _TOWER = ("c1", "c2"), ("p1", "p2", "p3")     # the item tower (shared with the profile rows) and the profile tower


class CuratorNet(PackedModel):
    flat_align = 4                     # every tensor starts on a 16-byte boundary
    input_type = InputType.SEQ
    EVAL_CHUNK_ROWS = 1 << 15          # catalogue rows per launch of compute_item_all (its derivative buffers are this wide)

    def __init__(self, config, dataload):
        super().__init__()
        one_process(self)
        self.embedding_size = E = int(config["embedding_size"])
        check_width16(E)
        mult = config["hidden_size"]
        if isinstance(mult, bool) or not isinstance(mult, (int, np.integer)) or mult < 1:
            raise ValueError(f"hidden_size is a multiplier of embedding_size and must be an integer >= 1; got {mult!r}")
        self.hidden_size = Hd = int(mult) * E
        self.max_seq_length = L = int(config["MAX_ITEM_LIST_LENGTH"])
        if not 1 <= L <= 255:
            raise ValueError(f"MAX_ITEM_LIST_LENGTH must lie in 1..255 (the pooling's argmax is stored in a byte); got {L}")
        self.item_num = dataload.item_num
        self.v_feat_path = config["v_feat_path"]
        v = torch.tensor(np.asarray(np.load(self.v_feat_path, allow_pickle=True)), dtype=torch.float)
        if v.dim() != 2 or v.shape[0] != self.item_num:
            raise ValueError(f"v_feat_path {self.v_feat_path}: the feature matrix must be [item_num, F] with item_num = "
                             f"{self.item_num} rows, got shape {tuple(v.shape)}")
        if v.shape[1] % 4:
            raise ValueError(f"v_feat_path {self.v_feat_path}: the feature width F must be a multiple of 4 (16-byte vector "
                             f"accesses), got F = {v.shape[1]}")
        v = v.contiguous()
        v[0].fill_(0)                                      # curatornet.py:21: the padding item's features
        self.feature_dim = F = v.shape[1]
        # the reference's module order (curatornet.py:22-37); the two pooling modules hold no state
        self.embedding = nn.Embedding.from_pretrained(v, freeze=True)
        self.selu_common1 = nn.Linear(F, E)
        self.selu_common2 = nn.Linear(E, E)
        self.selu_pu1 = nn.Linear(2 * E, Hd)
        self.selu_pu2 = nn.Linear(Hd, Hd)
        self.selu_pu3 = nn.Linear(Hd, E)
        for _, attr in _LINEARS:                           # reset_parameters (curatornet.py:43-54): the biases keep nn.Linear's init
            nn.init.xavier_uniform_(getattr(self, attr).weight)
        self.store_ifeatures = None

    # ------------------------------------------------------------------------------------------ packing
    def _linears(self):
        return [(key, attr, getattr(self, attr)) for key, attr in _LINEARS]

    def _flat_specs(self):
        """Flat layout: the ten Linear tensors in the reference's parameter order."""
        return linear_specs(self._linears())

    def rec_parameter_names(self):
        """{reference parameter name: flat-buffer key} of the TRAINABLE parameters in the reference's registration order
        (optim.native_to_torch_state): the reference trainer hands its optimizer the parameters with requires_grad only, so the
        frozen `embedding.weight` is not among them."""
        return linear_names(self._linears())

    def _drop_eval_cache(self):
        self.store_ifeatures = None                        # the catalogue matrix goes when training resumes

    # ------------------------------------------------------------------------------------------ training
    def _split_input(self, input):
        """The reference's single [B, L + 2] tensor, or (profile [B, L], target [B, 2]) -> contiguous (profile, target)."""
        return split_tail(input, 2, "CuratorNet: expected [B, L + 2] ids (profile of 1..255 positions, positive, negative), got profile "
                                    "{profile} and target {tail}", max_len=255)

    def forward(self, input):
        if not self.training:
            raise PxrError("CuratorNet.forward is the training loss (curatornet.py forward); use compute_item_all / predict to score")
        self._ensure_packed()
        profile, target = self._split_input(input)
        return TrainStep.apply(self._anchor, self, profile, target)

    def _profile_tower(self, cat):
        """[B, 2E] pooled profile -> the three SELU Linears: (activations, derivatives); the last activation is the user vector."""
        return self._act_chain(cat, _TOWER, "selu")

    def _forward_train(self, profile, target):
        B, L = profile.shape
        F, R = self.feature_dim, B * L
        n = R + 2 * B
        feat = self.embedding.weight.data
        x = self._buf("x", (n, F))                         # rows: [B L profile | positive, negative per sample]
        ops.embed_gather(feat, profile.view(-1), out=x[:R])
        ops.embed_gather(feat, target.view(-1), out=x[R:])
        (h1, h2), (d1, d2) = self._act_chain(x, _COMMON, "selu")
        cat, arg = ops.curator_pool(h2, B, L, cat=self._buf("cat", (B, 2 * self.embedding_size)),
                                    argmax=self._buf("arg", (B, self.embedding_size), torch.uint8))
        acts, ders = self._profile_tower(cat)
        ie = h2[R:]
        loss, coef = ops.curator_pair_fwd(acts[-1], ie, B, out=self._buf("head", (2 * B + 1,)))
        self._saved = dict(B=B, L=L, x=x, h1=h1, d1=d1, d2=d2, cat=cat, arg=arg, acts=acts, ders=ders, ie=ie, coef=coef)
        return loss

    def _backward_train(self, gsd):
        s = self._take_saved()
        B, L, E = s["B"], s["L"], self.embedding_size
        G = lambda k: self._p(k, grad=True)
        du, di = self._buf("du", (B, E)), self._buf("di", (2 * B, E))
        (a1, a2, u), ders = s["acts"], s["ders"]
        ops.mf_pair_bwd(u, s["ie"], s["coef"], du, di, self.grad_scale, gsd)
        dz3 = ops.mul(du, ders[-1], out=du)                                       # through selu_pu3's SELU
        dz1, dz2, dz3 = self._act_chain_bwd(dz3, _TOWER, ders)
        dcat = ops.linear_bwd_input(dz1, self._p("p1.w"))
        dpre2 = ops.curator_pool_bwd(dcat, s["arg"], di, s["d2"], B, L, out=self._buf("dpre2", (B * (L + 2), E)))
        dpre1 = ops.linear_bwd_input(dpre2, self._p("c2.w"), mul=s["d1"])
        # v_feat is frozen: selu_common1 needs no input gradient.  The two reductions over B (L + 2) rows are launches of their own
        # (their token range may be split); the three over B rows share one grouped launch
        ops.grouped_linear_bwd_weight([(dpre1, s["x"], G("c1.w"), G("c1.b"))])
        ops.grouped_linear_bwd_weight([(dpre2, s["h1"], G("c2.w"), G("c2.b"))])
        ops.grouped_linear_bwd_weight([(dz1, s["cat"], G("p1.w"), G("p1.b")), (dz2, a1, G("p2.w"), G("p2.b")),
                                       (dz3, a2, G("p3.w"), G("p3.b"))])
        self._step_done()

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def compute_item_all(self):
        """[I, E] = the common tower over the whole catalogue (curatornet.py compute_item_all), in chunks of EVAL_CHUNK_ROWS rows;
        cached until train() / load_state_dict()."""
        self._ensure_packed()
        if self.store_ifeatures is not None:
            return self.store_ifeatures
        feat = self.embedding.weight.data
        I = feat.shape[0]
        out = torch.empty(I, self.embedding_size, dtype=torch.float32, device=feat.device)
        for lo in range(0, I, self.EVAL_CHUNK_ROWS):
            hi = min(I, lo + self.EVAL_CHUNK_ROWS)
            out[lo:hi].copy_(self._act_chain(feat[lo:hi], _COMMON, "selu")[0][-1])
        self.store_ifeatures = out
        return out

    def invalidate_item_cache(self):
        """Drop the cached catalogue matrix (after the weights changed outside train() / load_state_dict())."""
        self.store_ifeatures = None

    @torch.no_grad()
    def encode_last(self, item_seq, item_feature=None):
        """item_seq int64 [B, L] -> (u [B, 1, E], u [B, E]): the user vectors, the queries of the fused scoring against
        item_feature (default: compute_item_all()).  item_feature[item_seq] is pooled by id: [B, L, E] never exists."""
        self._ensure_packed()
        feat = item_feature if item_feature is not None else self.compute_item_all()
        feat = feat if feat.is_contiguous() else feat.contiguous()
        item_seq = item_seq.contiguous()
        if item_seq.dim() != 2 or not 1 <= item_seq.shape[1] <= 255:
            raise ValueError(f"CuratorNet: item_seq must be [B, L] with 1 <= L <= 255, got {tuple(item_seq.shape)}")
        B, L = item_seq.shape
        cat, _ = ops.curator_pool(feat, B, L, ids=item_seq, want_argmax=False)
        u = self._profile_tower(cat)[0][-1]
        return u.view(B, 1, -1), u

    @torch.no_grad()
    def predict(self, item_seq, item_feature):
        """scores [B, I] = u item_feature^T (curatornet.py predict)."""
        feat = item_feature if item_feature is not None else self.compute_item_all()
        feat = feat if feat.is_contiguous() else feat.contiguous()
        _, u = self.encode_last(item_seq, feat)
        return dense_scores(u, feat)
