"""LightSANs (IDNet) -- drop-in for `REC.model.IDNet.lightsans.LightSANs` (code/REC/model/IDNet/lightsans.py) on the hand-written
gfx950 kernels: the low-rank interest attention of csrc/lightsans.hip between the library's fp32-operand GEMMs, LayerNorms and
loss head.

    x0 = dropout(LN(e[:, :L]))                                       (no position embedding on the input)
    per layer:  q|k|v = x W + b  (one GEMM);  ctx = lightsans core(q, k, v, thK, thV, A)   (pxr_lightsans_fwd_f32)
                A = softmax over queries of the position scores of pos_ln(P) (pxr_lightsans_pos_fwd_f32, batch-independent)
                a = LN(dropout(dense(ctx)) + x);  y = LN(dropout(dense_2(act(dense_1(a)))) + a)
    loss = mean_b -log(sigmoid(<y[:, -1], e_pos> - <y[:, -1], e_neg>) + 1e-8)

A sibling backbone on SASRec's shell, the way GRU4Rec is: everything around the block is SASRec's machinery, inherited --

  * the item table: occurrence sort of the batch's ids, lazy AdamW catch-up of exactly those rows, sparse table gradient from the
    segment sums, `state_dict` hooks (`model/sasrec.py`);
  * the loss head: SASRec's BPR head (inside-log epsilon) run on the reference's [B, L+2] id rows through its layout arguments:
    position t scores against items[b, 1 + t] / items[b, 2 + t], and masked_index is 1 at t = L-1 only, so the head scores the
    last position against the positive items[b, L] and the negative items[b, L+1], and writes zero coefficients elsewhere;
  * the flat parameter / gradient buffers, PxrAdamW, GraphedTrainStep, the fused scoring + top-k evaluation.

The occurrence sort reads the same rows with layout (L+2, 0, 1, 2): inputs at columns [0, L), the head's windows behind them.
No mask anywhere (layers.py:839-878): padded positions read table row 0 like any other row (row 0 gets no gradient, padding_idx).
`attpooling_{key,value}.theta` start at N(0, 1), identical in every layer (the reference deep-copies one layer), untouched by
_init_weights.  One process: the data-parallel exchange is not built for this model.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..utils.enum_type import InputType
from .packed import TrainStep, one_process
from .sasrec import SASRec
from .seqcore import SeqRecCore, _FeedForwardParams


# ---- parameter containers with the reference's module tree (layers.py:762-932; their forward is never called) -----------------
class _ItemToInterestParams(nn.Module):
    def __init__(self, hidden, k_interests):
        super().__init__()
        self.theta = nn.Parameter(torch.randn([hidden, k_interests]))


class _LightMultiHeadAttentionParams(nn.Module):
    def __init__(self, hidden, k_interests, eps):
        super().__init__()
        self.query = nn.Linear(hidden, hidden)
        self.key = nn.Linear(hidden, hidden)
        self.value = nn.Linear(hidden, hidden)
        self.attpooling_key = _ItemToInterestParams(hidden, k_interests)
        self.attpooling_value = _ItemToInterestParams(hidden, k_interests)
        self.pos_q_linear = nn.Linear(hidden, hidden)
        self.pos_k_linear = nn.Linear(hidden, hidden)
        self.pos_ln = nn.LayerNorm(hidden, eps=eps)
        self.dense = nn.Linear(hidden, hidden)
        self.LayerNorm = nn.LayerNorm(hidden, eps=eps)


class _LightTransformerLayerParams(nn.Module):
    def __init__(self, hidden, k_interests, inner, eps):
        super().__init__()
        self.multi_head_attention = _LightMultiHeadAttentionParams(hidden, k_interests, eps)
        self.feed_forward = _FeedForwardParams(hidden, inner, eps)


class _LightTransformerEncoderParams(nn.Module):
    def __init__(self, n_layers, hidden, k_interests, inner, eps):
        super().__init__()
        self.layer = nn.ModuleList([_LightTransformerLayerParams(hidden, k_interests, inner, eps) for _ in range(n_layers)])


class LightSANsBlock:
    """The LightSANs encoder as a mixin on SASRec's shell: parameters, flat packing, forward and hand-written backward."""

    _causal = False
    _split_catch_up_ok = False    # (the split catch-up reads SASRec's [B, 2, L+1] input window; the plain catch-up serves)

    def _build_lightsans(self, config, dataload):
        self.n_layers = config["n_layers"]
        self.n_heads = config["n_heads"]
        self.hidden_size = config["embedding_size"]
        self.inner_size = config["inner_size"] * self.hidden_size       # a multiplier (lightsans.py:18-22)
        self.k_interests = config["k_interests"]
        self.hidden_dropout_prob = float(config["hidden_dropout_prob"])
        self.attn_dropout_prob = float(config["attn_dropout_prob"])
        self.hidden_act = config["hidden_act"]
        self.layer_norm_eps = float(config["layer_norm_eps"])
        self.initializer_range = config["initializer_range"]
        self.max_seq_length = config["MAX_ITEM_LIST_LENGTH"]
        self.item_num = dataload.item_num
        if self.hidden_act not in ("gelu", "relu", "swish", "tanh", "sigmoid"):     # ACT2FN, layers.py:642-649
            raise ValueError(f"hidden_act must be one of gelu / relu / swish / tanh / sigmoid, got {self.hidden_act!r}")
        if self.hidden_size % self.n_heads != 0:
            raise ValueError("The hidden size (%d) is not a multiple of the number of attention heads (%d)"
                             % (self.hidden_size, self.n_heads))
        err = ops.lightsans_shape_error(self.max_seq_length, self.hidden_size, self.n_heads, self.k_interests)
        if err is not None:
            raise ValueError(f"LightSANs: {err} (the limits of the low-rank attention kernels, csrc/lightsans.hip)")
        if self.inner_size % 4:
            raise ValueError("inner_size * embedding_size must be a multiple of 4 (16-byte vector accesses)")
        # registration order = the reference's (lightsans.py:32-49): item_embedding, position_embedding, trm_encoder, LayerNorm
        self.item_embedding = nn.Embedding(self.item_num, self.hidden_size, padding_idx=0)
        self.position_embedding = nn.Embedding(self.max_seq_length, self.hidden_size)
        self.trm_encoder = _LightTransformerEncoderParams(self.n_layers, self.hidden_size, self.k_interests, self.inner_size,
                                                          self.layer_norm_eps)
        self.LayerNorm = nn.LayerNorm(self.hidden_size, eps=self.layer_norm_eps)
        self.dropout = nn.Dropout(self.hidden_dropout_prob)

    def _copy_first_layer_thetas(self):
        """The reference builds one layer and deep-copies it (layers.py:926-927), and _init_weights skips the bare theta
        Parameters: every layer starts with layer 0's thetas."""
        a0 = self.trm_encoder.layer[0].multi_head_attention
        for lay in self.trm_encoder.layer[1:]:
            a = lay.multi_head_attention
            a.attpooling_key.theta.data.copy_(a0.attpooling_key.theta.data)
            a.attpooling_value.theta.data.copy_(a0.attpooling_value.theta.data)

    # ------------------------------------------------------------------------------------------ flat packing
    def _flat_specs(self):
        """q|k|v adjacent (one GEMM), thK|thV adjacent (one column sum), pos_q|pos_k adjacent (one GEMM)."""
        specs = [("pos", self.position_embedding.weight), ("ln0.w", self.LayerNorm.weight), ("ln0.b", self.LayerNorm.bias)]
        for i, lay in enumerate(self.trm_encoder.layer):
            a, f = lay.multi_head_attention, lay.feed_forward
            specs += [(f"{i}.q.w", a.query.weight), (f"{i}.k.w", a.key.weight), (f"{i}.v.w", a.value.weight),
                      (f"{i}.q.b", a.query.bias), (f"{i}.k.b", a.key.bias), (f"{i}.v.b", a.value.bias),
                      (f"{i}.thK", a.attpooling_key.theta), (f"{i}.thV", a.attpooling_value.theta),
                      (f"{i}.pq.w", a.pos_q_linear.weight), (f"{i}.pk.w", a.pos_k_linear.weight),
                      (f"{i}.pq.b", a.pos_q_linear.bias), (f"{i}.pk.b", a.pos_k_linear.bias),
                      (f"{i}.pln.w", a.pos_ln.weight), (f"{i}.pln.b", a.pos_ln.bias),
                      (f"{i}.o.w", a.dense.weight), (f"{i}.o.b", a.dense.bias),
                      (f"{i}.ln1.w", a.LayerNorm.weight), (f"{i}.ln1.b", a.LayerNorm.bias),
                      (f"{i}.f1.w", f.dense_1.weight), (f"{i}.f1.b", f.dense_1.bias),
                      (f"{i}.f2.w", f.dense_2.weight), (f"{i}.f2.b", f.dense_2.bias),
                      (f"{i}.ln2.w", f.LayerNorm.weight), (f"{i}.ln2.b", f.LayerNorm.bias)]
        return specs

    def _first_flat_parameter(self):
        return self.position_embedding.weight

    def rec_parameter_names(self):
        """{reference parameter name: flat-buffer key} in the reference's registration order (what torch.optim.AdamW numbers its
        state in; optim.reference_rec_parameter_names)."""
        out = {"item_embedding.weight": None, "position_embedding.weight": "pos"}
        for i in range(self.n_layers):
            p = f"trm_encoder.layer.{i}."
            m = p + "multi_head_attention."
            for mod, key in (("query", "q"), ("key", "k"), ("value", "v")):
                out[m + mod + ".weight"], out[m + mod + ".bias"] = f"{i}.{key}.w", f"{i}.{key}.b"
            out[m + "attpooling_key.theta"], out[m + "attpooling_value.theta"] = f"{i}.thK", f"{i}.thV"
            for mod, key in (("pos_q_linear", "pq"), ("pos_k_linear", "pk"), ("pos_ln", "pln"), ("dense", "o"), ("LayerNorm", "ln1")):
                out[m + mod + ".weight"], out[m + mod + ".bias"] = f"{i}.{key}.w", f"{i}.{key}.b"
            f = p + "feed_forward."
            for mod, key in (("dense_1", "f1"), ("dense_2", "f2"), ("LayerNorm", "ln2")):
                out[f + mod + ".weight"], out[f + mod + ".bias"] = f"{i}.{key}.w", f"{i}.{key}.b"
        out["LayerNorm.weight"], out["LayerNorm.bias"] = "ln0.w", "ln0.b"
        return out

    def _planes_on(self) -> bool:          # the block runs on the fp32-operand GEMM entry points
        return False

    def weight_plane_segments(self):
        return None

    def refresh_weight_planes(self):
        return None

    def _zeros_LD(self, device):
        """A persistent [L, D] zero row block: the input LayerNorm's position term (LightSANs adds none) and pos_ln's residual."""
        z = getattr(self, "_zeros", None)
        if z is None or z.device != device:
            z = self._zeros = torch.zeros(self.max_seq_length, self.hidden_size, dtype=torch.float32, device=device)
        return z

    # ------------------------------------------------------------------------------------------ the encoder
    def _train_inputs(self, items, masked_index):
        # the input ids are items[:, :L] of the [B, L+2] rows; the block has no key mask
        return self.max_seq_length + 2, None, 0

    def _position_branch(self, i, train):
        """pe = pos_ln(P), pqk = pe [Wpq; Wpk]^T + [bpq; bpk], A = softmax over the queries (batch-independent)."""
        dev = self._flat.device
        P = self._p("pos")
        pe, pxhat, prstd = ops.ln_residual_fwd(P, self._zeros_LD(dev), self._p(f"{i}.pln.w"), self._p(f"{i}.pln.b"),
                                               self.layer_norm_eps, save=train)
        pqk = ops.linear_fwd(pe, self._p(f"{i}.pq.w", span=2), self._p(f"{i}.pq.b", span=2))
        A = ops.lightsans_pos_fwd(pqk, self.n_heads)
        return A, dict(pe=pe, pxhat=pxhat, prstd=prstd, pqk=pqk, A=A)

    def _encode(self, table, idx, idx_bstride, B, keymask, km_bstride, train: bool, head=None):
        """row ids into `table` -> last-layer states [B, L, D] (lightsans.py:65-82 / :86-99); saves activations when train.
        head = (table, items, masked_index): also run the loss head's forward (results in self._head_out)."""
        L, D, H, K = self.max_seq_length, self.hidden_size, self.n_heads, self.k_interests
        eps = self.layer_norm_eps
        ph = self.hidden_dropout_prob if train else 0.0
        pa = self.attn_dropout_prob if train else 0.0
        seed = (self._drop_seed * 1000003) & 0xFFFFFFFFFFFFFFFF
        sdv = self._drop_dev if train else None
        saved = {"seed": seed, "ph": ph, "pa": pa, "layers": []} if train else None
        h, xhat0, rstd0 = ops.input_ln_fwd(table, idx, idx_bstride, B, L, self._zeros_LD(table.device), self._p("ln0.w"),
                                           self._p("ln0.b"), eps, ph, seed, 0, save=train, step_dev=sdv)
        self._after_input_ln()
        if train:
            saved["xhat0"], saved["rstd0"] = xhat0, rstd0
        for i in range(self.n_layers):
            A, pos = self._position_branch(i, train)
            qkv = ops.linear_fwd(h, self._p(f"{i}.q.w", span=3), self._p(f"{i}.q.b", span=3))
            theta = self._p(f"{i}.thK", span=2)
            ctx, core = ops.lightsans_fwd(qkv, theta, A, B, L, H, K, pa, seed, 1 + 3 * i, step_dev=sdv, save=train)
            ctx = ctx.view(B, L, D)
            a = ops.linear_fwd(ctx, self._p(f"{i}.o.w"), self._p(f"{i}.o.b"))
            h1, xhat1, rstd1 = ops.ln_residual_fwd(a, h, self._p(f"{i}.ln1.w"), self._p(f"{i}.ln1.b"), eps, ph, seed, 2 + 3 * i,
                                                   save=train, step_dev=sdv)
            f, u = ops.linear_fwd(h1, self._p(f"{i}.f1.w"), self._p(f"{i}.f1.b"), gelu=True, save_grad=train, act=self.hidden_act)
            f2 = ops.linear_fwd(f, self._p(f"{i}.f2.w"), self._p(f"{i}.f2.b"))
            if i == self.n_layers - 1 and head is not None:
                self._before_head()
                h2, xhat2, rstd2, *self._head_out = ops.ln_residual_bpr_fwd(
                    f2, h1, self._p(f"{i}.ln2.w"), self._p(f"{i}.ln2.b"), eps, *head, p_drop=ph, seed=seed, stream_id=3 + 3 * i,
                    save=train, step_dev=sdv, layout=self._head_layout)
            else:
                h2, xhat2, rstd2 = ops.ln_residual_fwd(f2, h1, self._p(f"{i}.ln2.w"), self._p(f"{i}.ln2.b"), eps, ph, seed,
                                                       3 + 3 * i, save=train, step_dev=sdv)
            if train:
                saved["layers"].append(dict(h_in=h, qkv=qkv, theta=theta, core=core, pos=pos, ctx=ctx, xhat1=xhat1, rstd1=rstd1,
                                            h1=h1, u=u, f=f, xhat2=xhat2, rstd2=rstd2))
            h = h2
        return h, saved

    def _backward_core(self, gsd, table):
        """Backward of SeqRecCore._forward_core for the LightSANs block: fills the flat gradient buffer, hands the gradient w.r.t.
        the gathered input rows to the table machinery (`_after_input_grads`)."""
        s = self._take_saved()
        B, L, D, H, K = s["B"], self.max_seq_length, self.hidden_size, self.n_heads, self.k_interests
        T = B * L
        seed, ph, pa = s["seed"], s["ph"], s["pa"]
        sdv = self._drop_dev
        g = lambda name, span=1: self._p(name, grad=True, span=span)
        defer = ops.DeferredReductions()
        pend = []
        fused = bool(s.get("fused_head"))
        head_args = (s["pos"], s["neg"], table, s["items"], s["mask"], self.grad_scale, gsd)
        dh = coef = None
        if not fused:
            dh, coef = ops.bpr_loss_bwd(*head_args[:5], D, self.grad_scale, gsd, layout=self._head_layout)
        dpos = None
        for i in reversed(range(self.n_layers)):
            a = s["layers"][i]
            if fused and i == self.n_layers - 1:
                dz2, dxf2, _, coef = ops.bpr_ln_bwd(*head_args, a["xhat2"], a["rstd2"], self._p(f"{i}.ln2.w"), g(f"{i}.ln2.w"),
                                                    g(f"{i}.ln2.b"), p_drop=ph, seed=seed, stream_id=3 + 3 * i, need_dx=ph > 0,
                                                    step_dev=sdv, defer=defer, layout=self._head_layout)
            else:
                dz2, dxf2 = ops.ln_bwd(0, dh, a["xhat2"], a["rstd2"], self._p(f"{i}.ln2.w"), g(f"{i}.ln2.w"), g(f"{i}.ln2.b"), ph,
                                       seed, 3 + 3 * i, need_dx=ph > 0, step_dev=sdv, defer=defer)
            dxf2 = dz2 if dxf2 is None else dxf2
            pend.append((dxf2.view(T, D), a["f"].view(T, -1), g(f"{i}.f2.w"), g(f"{i}.f2.b")))
            du = ops.linear_bwd_input(dxf2, self._p(f"{i}.f2.w"), mul=a["u"])
            pend.append((du.view(T, -1), a["h1"].view(T, D), g(f"{i}.f1.w"), g(f"{i}.f1.b")))
            dh1 = ops.linear_bwd_input(du, self._p(f"{i}.f1.w"), add=dz2)
            dz1, dxa = ops.ln_bwd(0, dh1, a["xhat1"], a["rstd1"], self._p(f"{i}.ln1.w"), g(f"{i}.ln1.w"), g(f"{i}.ln1.b"), ph, seed,
                                  2 + 3 * i, need_dx=ph > 0, step_dev=sdv, defer=defer)
            dxa = dz1 if dxa is None else dxa
            pend.append((dxa.view(T, D), a["ctx"].view(T, D), g(f"{i}.o.w"), g(f"{i}.o.b")))
            dctx = ops.linear_bwd_input(dxa, self._p(f"{i}.o.w"))
            p = a["pos"]
            dqkv, _, dth, dA = ops.lightsans_bwd(dctx, a["qkv"], a["theta"], p["A"], a["core"], B, L, H, K, pa, seed, 1 + 3 * i,
                                                 step_dev=sdv)
            ops.colsum(dth, out=g(f"{i}.thK", span=2).view(-1), defer=defer)
            # the position branch: dA summed over the batch, back through the softmax over queries, pos_q|pos_k and pos_ln
            dpqk = ops.lightsans_pos_bwd(p["pqk"], p["A"], ops.colsum(dA).view(H, L, L))
            pend.append((dpqk, p["pe"], g(f"{i}.pq.w", span=2), g(f"{i}.pq.b", span=2)))
            dpe = ops.linear_bwd_input(dpqk, self._p(f"{i}.pq.w", span=2))
            dP, _ = ops.ln_bwd(0, dpe, p["pxhat"], p["prstd"], self._p(f"{i}.pln.w"), g(f"{i}.pln.w"), g(f"{i}.pln.b"), defer=defer)
            dpos = dP if dpos is None else ops.add(dpos, dP)
            pend.append((dqkv, a["h_in"].view(T, D), g(f"{i}.q.w", 3), g(f"{i}.q.b", 3)))
            dh = ops.linear_bwd_input(dqkv.view(B, L, 3 * D), self._p(f"{i}.q.w", span=3), add=dz1)
        dx0, _ = ops.ln_bwd(1, dh, s["xhat0"], s["rstd0"], self._p("ln0.w"), g("ln0.w"), g("ln0.b"), ph, seed, 0, step_dev=sdv,
                            defer=defer)
        g("pos").copy_(dpos)
        # every dropout-mask consumer of this pass has been issued: the reduction launch also advances the dropout step counter
        bumped = defer.flush(bump=self._drop_dev)
        self._after_input_grads(dx0, coef, s)
        ops.grouped_linear_bwd_weight(pend)        # every weight (and bias) gradient of the step: one launch
        self._step_done(bumped)
        return dx0, coef, s


class LightSANs(LightSANsBlock, SASRec):
    input_type = InputType.AUGSEQ            # every prefix a sample, read as TwoTower rows (data/utils.py SUPPORTED)

    def __init__(self, config, dataload):
        SeqRecCore.__init__(self)
        one_process(self)
        self._build_lightsans(config, dataload)
        self.apply(self._init_weights)       # Linear / Embedding N(0, initializer_range) incl. row 0, LayerNorm (1, 0)
        self._copy_first_layer_thetas()
        self._init_runtime_state(config)
        self._init_table_state()
        L = self.max_seq_length
        self._head_layout = (L + 2, 1, 2)    # position t: target items[b, 1 + t], negative items[b, 2 + t]; only t = L-1 counts
        self._occ_layout = (L + 2, 0, 1, 2)  # + the inputs items[b, t]
        self._last_only = {}

    def _occ_positions(self, items):
        return self.max_seq_length

    def _last_position_mask(self, B, device):
        """masked_index of the loss head: 1 at position L-1, 0 elsewhere (persistent: a captured step replays on it)."""
        m = self._last_only.get((B, device))
        if m is None:
            m = torch.zeros(B, self.max_seq_length, dtype=torch.int64, device=device)
            m[:, -1] = 1
            self._last_only[(B, device)] = m
        return m

    def forward(self, interaction):
        """interaction = items int64 [B, L+2] (the reference's TwoTower rows: history | positive | negative) or the loader's pair
        (history [B, L], target [B, 2]) -> 0-dim loss (lightsans.py:65-85)."""
        L = self.max_seq_length
        if isinstance(interaction, torch.Tensor):
            items = interaction
        else:
            hist, target = interaction
            if hist.dim() != 2 or hist.shape[1] != L or tuple(target.shape) != (hist.shape[0], 2):
                raise ValueError(f"expected (history [B, {L}], target [B, 2]), got {tuple(hist.shape)} / {tuple(target.shape)}")
            items = torch.cat((hist, target), dim=1)
        if items.dim() != 2 or items.shape[1] != L + 2:
            raise ValueError(f"items must be [B, {L + 2}], got {tuple(items.shape)}")
        self._ensure_packed()
        items = items.contiguous()
        return self._forward_dispatch(items, self._last_position_mask(items.shape[0], items.device))

    def _forward_dispatch(self, items, masked_index):
        if torch.is_grad_enabled() and self.training:
            return TrainStep.apply(self._anchor, self, items, masked_index)
        was = self.training
        try:
            self.training = False
            return self._forward_train(items, masked_index).view(())
        finally:
            self.training = was
