"""MOMF (PixelNet) -- drop-in for `REC.model.PixelNet.momf.MOMF` (code/REC/model/PixelNet/momf.py, MLPLayers of layers.py:239-294):
MF of mf.py with the visual encoder's output in the item table's place, on the same kernels (csrc/mf.hip).  With E =
visual_encoder(images) [M, D] -- one row per distinct image of the batch --, user [B] and idx [B, 2] positions into E (positive,
negative):

    u_b = tower_u(user_embedding[user_b])      i_{b,t} = tower_i(E[idx_{b,t}])
    x_b = <u_b, i_{b,0}> - <u_b, i_{b,1}>      loss = -mean_b log sigmoid(x_b)                  (momf.py:59: NO 1e-8)

A tower is MF's MLPLayers([D] + mlp_hidden_size, dropout_prob, 'tanh', bn=True); with `mlp_hidden_size: []` (the shipped config) it
is the identity.  The towers' code is MF's (mf.MfTowers).

MOMF is the one pixel model with a large trainable TABLE next to the encoder: `user_embedding` is a [1 + user_num, D] lazy table
(row 0 a spare, user u at row 1 + u, as in MF) that PxrAdamW updates by rows, and E is a batch-local row space whose gradient
autograd takes dense.  One step: encoder forward -> row list rows[3B] = [1 + user | idx.view(-1)], checked (pxr_table_rows_i64, base
0 for the positions) -> catch_up_ids on the user rows -> head forward with eps = 0 (pxr_mf_pair_fwd_eps_f32, which reads the user
table and E through the one row list: no gather) -> pxr_momf_pair_grad_f32, ONE launch with two sinks: the user rows' gradient as
sparse rows (`sparse_table_grad`, B slots) and d loss / d E as a dense [M, D] block in a fixed summation order, which goes back to
autograd through packed.EncoderRows -> encoder backward.  No float atomic is used.  M changes from batch to batch, so the step runs
eagerly, as the other deduplicating pixel models do.

With towers the item tower runs PER OCCURRENCE: embed_gather(E, idx) gives [2B, D], then MF's tower forward and backward (dropout
included), then the kernel's occ mode.  The reference's BatchNorm1d takes its statistics over the 2B rows of item.flatten(0, 1), so
a repeated image counts once per occurrence; a tower over the distinct rows would change the statistics.  The ENCODER still sees
each image once.  (A count-weighted BatchNorm over distinct rows is not built: DESIGN.md.)  The gradient of a Linear bias is the
exact zero it is in exact arithmetic (the BatchNorm behind every Linear subtracts the batch mean, bias included), not the rounding
noise of its column sums that the reference's float32 autograd leaves there and AdamW turns into steps of about +-lr.

Contract kept: `input_type = PAIR`; `__init__(config, dataload)` with `embedding_size`, `mlp_hidden_size`, `dropout_prob`;
forward((user [B], index [B, 2], images [M, 3, H, W])) -> loss, or the reference's own (user [B], item [B, 2, 3, H, W]);
`loss_from_embeddings(E, user, index)` is the head alone; `compute_item(images)` = the eval-mode item tower over the encoder;
`encode_last` / `predict(user, item_feature)` are MF's on the user table; `modal_inputs(store, data)` turns the batcher's (user,
index, image_ids) into the forward's input; `state_dict` keys and order of the reference (user_mlp_layers.*, item_mlp_layers.* with
the BatchNorm buffers, user_embedding.weight, visual_encoder.*; xavier-normal Linears and embedding, made before the encoder is
loaded), so reference checkpoints load with strict=True.  One process: the data-parallel exchange is not built for this model.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..lib import PxrError
from ..utils.enum_type import InputType
from .mf import MfTowers
from .packed import EncoderRows, LazyTableModel, _Rows, dense_scores, one_process
from .visual import load_model


class MOMF(EncoderRows, MfTowers, LazyTableModel):
    input_type = InputType.PAIR

    def __init__(self, config, dataload):
        super().__init__()
        one_process(self, "MOMF")
        self.user_num = dataload.user_num
        self.item_num = dataload.item_num
        self._build_towers(config)
        self.user_embedding = _Rows(self.user_num, self.embedding_size)
        self._init_linears()                                # momf.py:38 self.apply(_init_weights): the Linears, then the embedding,
        nn.init.xavier_normal_(self.user_embedding.weight)  # before the encoder exists, so it is not touched
        self.visual_encoder = load_model(config=config)

    # ------------------------------------------------------------------------------------------ packing
    def rec_parameter_names(self):
        """{reference parameter name: flat-buffer key} in the reference's registration order (optim.native_to_torch_state): the
        tower tensors, then the user table, which maps to None -- its state is the table's (optim.table_spans)."""
        out = self._tower_parameter_names()
        out["user_embedding.weight"] = None
        return out

    def table_parameter_spans(self):
        """Rows of the table buffer the table parameter occupies (optim.table_spans): row 0 is the spare."""
        return {"user_embedding.weight": (1, 1 + self.user_num)}

    # ------------------------------------------------------------------------------------------ input forms
    @staticmethod
    def modal_inputs(store, data):
        """The batcher's (user, index, image_ids [M]) -> the forward's (user, index, images [M, 3, H, W]): each distinct image of
        the batch is fetched, and later encoded, once."""
        return data[0], data[1], store.batch(data[2])

    @staticmethod
    def _reference_form(user, item):
        """momf.py:50-53's (user [B], item [B, 2, 3, H, W]) -> (user, index, images): one image per position, position t of sample b
        at 2b + t (item.flatten(0, 1))."""
        B = item.shape[0]
        if item.shape[1] != 2 or user.numel() != B:
            raise ValueError(f"MOMF: expected user [B] and item [B, 2, 3, H, W], got {tuple(user.shape)} and {tuple(item.shape)}")
        return user, torch.arange(2 * B, dtype=torch.int64, device=item.device).view(B, 2), item.flatten(0, 1)

    # ------------------------------------------------------------------------------------------ training
    def forward(self, input):
        """input = (user int64 [B], index int64 [B, 2], images fp32 [M, 3, H, W]) -> 0-dim loss (momf.py:50-60); or the
        reference's own (user int64 [B], item fp32 [B, 2, 3, H, W])."""
        if not self.training:
            raise PxrError("MOMF.forward is the training loss (momf.py forward); use compute_item / predict to score")
        self._ensure_packed()                # (raises on a CPU model before the tower runs)
        if len(input) == 2:
            user, item = input
            if not (isinstance(item, torch.Tensor) and item.dim() == 5 and item.is_floating_point()):
                raise ValueError("MOMF: expected (user, index, images) or the reference's (user, item [B, 2, 3, H, W])")
            user, index, images = self._reference_form(user, item)
        else:
            user, index, images = input
        return self.loss_from_embeddings(self.visual_encoder(images), user, index)

    def loss_from_embeddings(self, E, user, index):
        """The head without the encoder: E float32 [M, D] on the HIP device, user int64 [B], index int64 [B, 2] positions into E
        -> 0-dim loss; under autograd its backward leaves d loss / d E [M, D] on E, the user rows' gradient in
        `sparse_table_grad` and the tower gradients in the flat gradient buffer.  A position outside [0, M) or a user outside
        [0, user_num) flags the status word (ops.raise_on_bad_indices: IndexError)."""
        self._check_rows(E, self.embedding_size)
        self._ensure_packed()
        user = user.to(E.device).reshape(-1).contiguous()
        index = index.to(E.device).contiguous()
        if index.dim() != 2 or tuple(index.shape) != (user.numel(), 2):
            raise ValueError(f"MOMF: index must be [B, 2] = [{user.numel()}, 2] (positive, negative), got {tuple(index.shape)}")
        self._check_tower_batch(user.numel())
        table = E.detach().contiguous()
        if torch.is_grad_enabled():
            return self._encoded_step(E, table, user, index)
        loss = self._head_fwd(table, user, index).view(()).clone()
        self._saved = None
        return loss

    def _forward_train(self, user, index):
        return self._head_fwd(self._train_table, user, index)

    def _head_fwd(self, E, user, index):
        B = user.numel()
        rows = ops.momf_pair_rows(user, index, self.user_num, E.shape[0], out=self._buf("rows", (3 * B,), torch.int64))
        if self._table_hooks is not None:
            self._table_hooks.catch_up_ids(rows[:B])      # the step's user rows, current through the last step before they are read
        head = self._buf("head", (2 * B + 1,))
        if not self.mlp_hidden_size:
            loss, coef = ops.mf_pair_fwd(self._table, E, B, rows=rows, out=head, eps=0.0)
            self._saved = dict(B=B, rows=rows, coef=coef)
            return loss
        xu = ops.embed_gather(self._table, rows[:B])                             # [B, D]
        xi = ops.embed_gather(E, rows[B:])                                       # [2B, D]: one row per occurrence, index.view(-1) order
        hu, su = self._tower_fwd("u", self.user_mlp_layers, xu, True, 0)
        hi, si = self._tower_fwd("i", self.item_mlp_layers, xi, True, 64)
        loss, coef = ops.mf_pair_fwd(hu, hi, B, out=head, eps=0.0)
        self._saved = dict(B=B, rows=rows, coef=coef, hu=hu, hi=hi, su=su, si=si)
        return loss

    def _backward_train(self, gsd):
        """-> d loss / d E [M, D] (the bridge's anchor is the encoder's output); leaves `sparse_table_grad`."""
        s, table = self._take_table()                # (backward() without a forward() raises here)
        B, M = s["B"], table.shape[0]
        sp = self._sparse_rows(B)
        if not self.mlp_hidden_size:
            dE = ops.momf_pair_grad(s["rows"], B, sp, M, utable=self._table, E=table, coef=s["coef"], grad_scale=self.grad_scale,
                                    grad_scale_dev=gsd)
        else:
            H = self.out_size
            du, di = self._buf("du", (B, H)), self._buf("di", (2 * B, H))
            ops.mf_pair_bwd(s["hu"], s["hi"], s["coef"], du, di, self.grad_scale, gsd)
            occ = self._buf("occ", (3 * B, self.embedding_size))
            problems = []
            # (a Linear bias in front of a training BatchNorm has a zero gradient: the flat gradient buffer keeps its +0.0 there)
            self._tower_bwd("u", du, s["su"], 0, occ[:B], problems, bias_grad=False)
            self._tower_bwd("i", di, s["si"], 64, occ[B:], problems, bias_grad=False)
            ops.grouped_linear_bwd_weight(problems)
            dE = ops.momf_pair_grad(s["rows"], B, sp, M, occ=occ)
        self.sparse_table_grad = sp
        self._step_done()
        return dE

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def compute_item(self, item):
        """images [N, 3, H, W] -> the eval-mode item tower over the encoder [N, out_size] (momf.py:69-71)."""
        self._ensure_packed()
        feat = self.visual_encoder(item)
        if self.mlp_hidden_size:
            feat, _ = self._tower_fwd("i", self.item_mlp_layers, feat.contiguous(), False, 0)
        return feat

    @torch.no_grad()
    def encode_last(self, user, item_feature=None):
        """user int64 [B] -> (u [B, 1, H], u [B, H]): the eval-mode user tower's output, the query vectors of the fused scoring."""
        self._ensure_packed()
        self.sync_table()
        rows = ops.mf_pair_rows(user.reshape(-1).contiguous(), None, self.user_num, 0)
        u = ops.embed_gather(self._table, rows)
        if self.mlp_hidden_size:
            u, _ = self._tower_fwd("u", self.user_mlp_layers, u, False, 0)
        return u.view(u.shape[0], 1, -1), u

    @torch.no_grad()
    def predict(self, user, item_feature):
        """scores [B, N] = u item_feature^T (momf.py:62-67)."""
        feat = item_feature if item_feature.is_contiguous() else item_feature.contiguous()
        _, u = self.encode_last(user, feat)
        return dense_scores(u, feat)
