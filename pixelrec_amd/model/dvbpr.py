"""DVBPR (PixelNet) -- drop-in for `REC.model.PixelNet.dvbpr.DVBPR` (code/REC/model/PixelNet/dvbpr.py:11-143): visual BPR whose
image encoder, a CNN-F (model/cnnf.py), is trained from pixels.  With Dh = embedding_size // 2, E = CNNF(images) [M, Dh] -- one row per
DISTINCT image of the batch --, user [B], item_id [B, 2] and index [B, 2] positions into E (positive, negative):

    x_b  = <gamma_u[user_b], gamma_i[item_b,0] - gamma_i[item_b,1]> + <theta_u[user_b], E[p_b] - E[n_b]>
    loss = -mean_b log sigmoid(x_b)                                                                  (dvbpr.py:61: NO 1e-8)

The tables: theta_users [U, Dh], gamma_users [U, Dh], gamma_items [I, Dh] (uniform_(0, 1), dvbpr.py:44-46) are views of ONE lazy
[1 + U + U + I, Dh] buffer in the reference's registration order, row 0 a spare (optim.table_spans, as VBPR's three).  One step:
encoder forward -> rows[6B] = [gamma row of user | theta row of user | gamma rows of item_id.view(-1) | index.view(-1)], checked
(pxr_table_rows_i64) -> catch_up_ids on the 4B table rows -> head forward (pxr_dvbpr_pair_fwd_f32: VBPR's head without the bias
term, csrc/dvbpr.hip on pair_head.cuh) -> head backward, ONE launch with two sinks: the tables' gradient as sparse rows
(`sparse_table_grad`, 4B slots) and d loss / d E as a dense [M, Dh] block, a fixed-order segment sum of the per-occurrence +-c_b theta_u
over the positions -- position 0 is a real image and keeps its gradient -- which goes back to autograd through packed.EncoderRows ->
CNN-F backward.  No float atomic is used.  M changes from batch to batch, so the step runs eagerly.

Three facts about the reference:
  1. its dataset does not match it: REC/data/utils.py:40 maps DVBPR to MOPairTrainDataset, which returns (user, item_modal), while
     forward unpacks (user, item_id, item_modal) (dvbpr.py:50) -- the pair does not run as shipped.  Here the batcher carries the
     ids: MoPairTrainBatcher's image_ids [M] are item ids, so item_id = image_ids[index] (`batch_ids`);
  2. it ships no yaml for the model (configs/PixelNet/dvbpr.yaml is this project's);
  3. it encodes 2B images a step.  Here each distinct image of a batch is encoded once and the gradients of its copies are summed
     into it (as MOMF).  With dropout_prob > 0 the encoder is not a pure per-image function: an image that occurs twice in a batch
     gets ONE mask here where the reference would draw two.  The dedup is kept.

Evaluation: `compute_item(images)` is the eval-mode CNN-F (no dropout).  The score gamma_u gamma_i^T + theta_u item_feature^T is one
inner product of [gamma_u | theta_u | 1 | 0...] with [gamma_i | item_feature | 0 | 0...] -- VBPR's packing with a zero bias column
(pxr_vbpr_pack_f32) -- so `scoring_item_matrix()` / `encode_last` feed the Trainer's fused top-k unchanged; `predict` is the
reference's literal formula (dvbpr.py:66-75) and what `eval_fused_topk: False` goes through.

Contract kept: `input_type = PAIR`; `__init__(config, dataload)` with `embedding_size`, `dropout_prob` (and this build's
`conv_workspace_mb`); forward((user [B], index [B, 2], images [M, 3, 224, 224], image_ids [M])) -> loss -- what
`modal_inputs(store, data)` makes of a batch --, or the reference's own (user [B], item_id [B, 2], item_modal [B, 2, 3, 224, 224]),
recognised by the 5-D tensor and mapped to one row per position; `loss_from_embeddings(E, user, item_id, index)` is the head alone;
`state_dict` keys and order of the reference (visual_encoder.*, theta_users, gamma_users, gamma_items), so reference checkpoints load
with strict=True.  Under four optim_args the optimizer is OptimizerGroup(VisualAdamW over the encoder's 16 tensors, PxrAdamW over
the three tables), the torch-layout state has the reference's two groups; under two keys the Trainer builds what it builds for the
other pixel models with a table.  One process: the data-parallel exchange is not built for this model.
"""
from __future__ import annotations

import torch

from .. import ops
from ..lib import PxrError
from ..utils.enum_type import InputType
from .cnnf import CNNF
from .packed import EncoderRows, LazyTableModel, _Rows, dense_gemm, one_process


class DVBPR(EncoderRows, LazyTableModel):
    input_type = InputType.PAIR

    def __init__(self, config, dataload):
        super().__init__()
        one_process(self, "DVBPR")
        self.dropout_prob = float(config["dropout_prob"] or 0.0)
        self.embedding_size = int(config["embedding_size"]) // 2
        Dh = self.embedding_size
        if Dh <= 0 or Dh % 4 or Dh > 4096:
            raise ValueError(f"embedding_size // 2 must be a positive multiple of 4, at most 4096 (16-byte vector accesses); "
                             f"got embedding_size // 2 = {Dh}")
        self.user_num = dataload.user_num
        self.item_num = dataload.item_num
        mb = config["conv_workspace_mb"] if "conv_workspace_mb" in config else None
        s = config["seed"] if "seed" in config else None
        # the reference's module order (dvbpr.py:25-32)
        self.visual_encoder = CNNF(hidden_dim=Dh, dropout=self.dropout_prob, conv_workspace_mb=1024 if mb is None else mb,
                                   seed=int(s) if s is not None else 2020)
        self.theta_users = _Rows(self.user_num, Dh)
        self.gamma_users = _Rows(self.user_num, Dh)
        self.gamma_items = _Rows(self.item_num, Dh)
        for mod in (self.theta_users, self.gamma_users, self.gamma_items):       # dvbpr.py:44-46 (CNNF has reset itself)
            torch.nn.init.uniform_(mod.weight)
        self._item_feature = None

    # ------------------------------------------------------------------------------------------ packing
    def _flat_specs(self):
        """No flat parameter: everything outside the encoder is a table."""
        return []

    def rec_parameter_names(self):
        """{reference parameter name: flat-buffer key} of the rec group in the reference's registration order; the tables map to None
        -- their state is the table's (optim.table_spans)."""
        return {"theta_users.weight": None, "gamma_users.weight": None, "gamma_items.weight": None}

    def table_parameter_spans(self):
        """Rows of the table buffer each table parameter occupies (optim.table_spans), in the reference's order; row 0 is the spare."""
        U, I = self.user_num, self.item_num
        return {"theta_users.weight": (1, 1 + U), "gamma_users.weight": (1 + U, 1 + 2 * U),
                "gamma_items.weight": (1 + 2 * U, 1 + 2 * U + I)}

    def _drop_eval_cache(self):
        self._item_feature = None

    # ------------------------------------------------------------------------------------------ input forms
    @staticmethod
    def batch_ids(data):
        """The batcher's (user, index [B, 2], image_ids [M]) -> (user, item_id [B, 2], index): the distinct images of a batch ARE its
        distinct items, so the item ids the reference's forward wants (dvbpr.py:50) are image_ids[index]."""
        user, index, image_ids = data[0], data[1], data[2]
        return user, image_ids[index], index

    @staticmethod
    def modal_inputs(store, data):
        """The batcher's (user, index, image_ids [M]) -> the forward's (user, index, images [M, 3, 224, 224], image_ids): each distinct
        image of the batch is fetched, and later encoded, once."""
        return data[0], data[1], store.batch(data[2]), data[2]

    @staticmethod
    def _reference_form(user, item_id, item_modal):
        """dvbpr.py:50's (user [B], item_id [B, 2], item_modal [B, 2, 3, 224, 224]) -> (user, item_id, index, images): one image per
        position, position t of sample b at 2b + t."""
        B = item_modal.shape[0]
        if item_modal.shape[1] != 2 or user.numel() != B or item_id.numel() != 2 * B:
            raise ValueError(f"DVBPR: expected user [B], item_id [B, 2] and item_modal [B, 2, 3, 224, 224], got {tuple(user.shape)}, "
                             f"{tuple(item_id.shape)} and {tuple(item_modal.shape)}")
        index = torch.arange(2 * B, dtype=torch.int64, device=item_modal.device).view(B, 2)
        return user, item_id.reshape(B, 2), index, item_modal.flatten(0, 1)

    # ------------------------------------------------------------------------------------------ training
    def forward(self, input):
        """input = (user int64 [B], index int64 [B, 2], images fp32 [M, 3, 224, 224], image_ids int64 [M]) -> 0-dim loss
        (dvbpr.py:49-62); or the reference's own (user, item_id int64 [B, 2], item_modal fp32 [B, 2, 3, 224, 224])."""
        if not self.training:
            raise PxrError("DVBPR.forward is the training loss (dvbpr.py forward); use compute_item / predict to score")
        if len(input) == 3 and isinstance(input[2], torch.Tensor) and input[2].dim() == 5 and input[2].is_floating_point():
            user, item_id, index, images = self._reference_form(*input)
        elif len(input) == 4:
            user, index, images, image_ids = input
            index = index.to(images.device)
            item_id = image_ids.to(images.device)[index]
        else:
            raise ValueError("DVBPR: expected (user, index, images, image_ids) or the reference's (user, item_id, item_modal "
                             "[B, 2, 3, 224, 224])")
        if isinstance(images, torch.Tensor) and images.device.type == "cuda":
            self._ensure_packed()            # (a CPU model raises here, before the encoder runs)
        return self.loss_from_embeddings(self.visual_encoder(images), user, item_id, index)

    def loss_from_embeddings(self, E, user, item_id, index):
        """The head without the encoder: E float32 [M, Dh] on the HIP device, user int64 [B], item_id int64 [B, 2], index int64 [B, 2]
        positions into E -> 0-dim loss; under autograd its backward leaves d loss / d E [M, Dh] on E and the tables' gradient in
        `sparse_table_grad`.  A position outside [0, M), a user outside [0, user_num) or an item outside [0, item_num) flags the
        status word (ops.raise_on_bad_indices: IndexError)."""
        self._check_rows(E, self.embedding_size)
        self._ensure_packed()
        user = user.to(E.device).reshape(-1).contiguous()
        B = user.numel()
        item_id, index = item_id.to(E.device).contiguous(), index.to(E.device).contiguous()
        for name, t in (("item_id", item_id), ("index", index)):
            if t.dim() != 2 or tuple(t.shape) != (B, 2):
                raise ValueError(f"DVBPR: {name} must be [B, 2] = [{B}, 2] (positive, negative), got {tuple(t.shape)}")
        table = E.detach().contiguous()
        if torch.is_grad_enabled():
            return self._encoded_step(E, table, user, item_id, index)
        loss = self._head_fwd(table, user, item_id, index).view(()).clone()
        self._saved = None
        return loss

    def _forward_train(self, user, item_id, index):
        return self._head_fwd(self._train_table, user, item_id, index)

    def _head_fwd(self, E, user, item_id, index):
        B = user.numel()
        rows = ops.dvbpr_rows(user, item_id, index, self.user_num, self.item_num, E.shape[0], out=self._buf("rows", (6 * B,), torch.int64))
        if self._table_hooks is not None:
            self._table_hooks.catch_up_ids(rows[:4 * B])   # the step's table rows, current through the last step before they are read
        loss, coef = ops.dvbpr_pair_fwd(self._table, rows, E, B, out=self._buf("head", (2 * B + 1,)))
        self._saved = dict(B=B, rows=rows, coef=coef)
        return loss

    def _backward_train(self, gsd):
        """-> d loss / d E [M, Dh] (the bridge's anchor is the encoder's output); leaves `sparse_table_grad`."""
        s, table = self._take_table()                # (backward() without a forward() raises here)
        sp = self._sparse_rows(4 * s["B"])
        dE = ops.dvbpr_pair_bwd(self._table, s["rows"], table, s["coef"], s["B"], sp, self.grad_scale, gsd)
        self.sparse_table_grad = sp
        self._step_done()
        return dE

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def compute_item(self, item):
        """images [N, 3, 224, 224] -> the eval-mode CNN-F [N, Dh], no dropout (dvbpr.py:77-79)."""
        return self.visual_encoder.encode(item, train=False)

    def set_item_feature(self, item_feature):
        """The encoded catalogue [item_num, Dh] of this evaluation: what scoring_item_matrix() packs."""
        self._item_feature = item_feature

    def _user_rows(self, user):
        self._ensure_packed()
        self.sync_table()
        user = user.reshape(-1).contiguous()
        return user.numel(), ops.dvbpr_rows(user, None, None, self.user_num, self.item_num, 0)    # [gamma rows | theta rows]

    @torch.no_grad()
    def scoring_item_matrix(self):
        """[I, P] = [gamma_items row | item feature | 0 | 0...]: the item side of the score as one inner product -- VBPR's packing
        with a zero bias column (the Trainer's fused top-k reads it in place of the item feature)."""
        feat = self._item_feature
        if feat is None:
            raise PxrError("DVBPR: call set_item_feature(compute_item(...)) before scoring")
        self._ensure_packed()
        self.sync_table()
        lo, hi = self.table_parameter_spans()["gamma_items.weight"]
        if feat.shape[0] != hi - lo:
            raise PxrError(f"DVBPR: the item feature has {feat.shape[0]} rows, the catalogue {hi - lo} items")
        zero = torch.zeros(hi - lo, dtype=torch.float32, device=feat.device)
        return ops.vbpr_pack(self._table[lo:hi], feat.contiguous(), zero)

    @torch.no_grad()
    def encode_last(self, user, item_feature=None):
        """user int64 [B] -> (q [B, 1, P], q [B, P]): [gamma_users row | theta_users row | 1 | 0...], the query side of the fused
        scoring against scoring_item_matrix()."""
        B, rows = self._user_rows(user)
        q = ops.vbpr_pack(self._table, self._table, None, rows[:B], rows[B:])
        return q.view(B, 1, -1), q

    @torch.no_grad()
    def predict(self, user, item_feature):
        """scores [B, I] = gamma_u gamma_i^T + theta_u item_feature^T (dvbpr.py:66-75)."""
        B, rows = self._user_rows(user)
        feat = item_feature if item_feature.is_contiguous() else item_feature.contiguous()
        u = ops.embed_gather(self._table, rows)                                    # [2B, Dh]: gamma rows | theta rows
        lo, hi = self.table_parameter_spans()["gamma_items.weight"]
        s_id, s_mo = dense_gemm(u[:B], self._table[lo:hi]), dense_gemm(u[B:], feat)
        ops.raise_on_bad_indices(u.device)     # a user id outside the table raises, like the reference's indexing
        return s_id.add_(s_mo)
