"""MODSSM and MOFM (PixelNet) -- drop-ins for `REC.model.PixelNet.modssm.MODSSM` and `REC.model.PixelNet.mofm.MOFM`
(code/REC/model/PixelNet/modssm.py, mofm.py): DSSM and FM of pooled.py with the visual encoder's output in the item table's place,
on the same kernels (csrc/pool.hip, MODE_POOL of csrc/embed_grad.hip).  With E = visual_encoder(all_item_modal) [M, D] -- one row
per distinct image of the batch, row 0 the zero image's encoding (which is not zero) -- and idx positions into E, 0 = "no item":

    MODSSM:  U_s = (sum_l [idx_sl != 0] E[idx_sl]) / (cnt + 1e-8)        (an fp32 division; cnt = 0 gives exactly 0)
    MOFM:    U_s = H_s = sum_l [idx_sl != 0] E[idx_sl]
    x_s = <U_s, E[p_s]> - <U_s, E[n_s]>                 loss = -mean_s log(1e-8 + sigmoid(x_s))   over EVERY row s

MODSSM reads `mlp_hidden_size` and `dropout_prob` and builds no MLP, as the reference.  MOFM's reference runs
BaseFactorizationMachine over [profile | p] and [profile | n] and subtracts; the history-history terms cancel exactly and leave the
factored form above, which is what the kernels compute (pooled.py's docstring has the argument, tests/pool_restate.py both forms).
Neither reference forward has the `inputs[0]` leftover of the ID versions: every row counts there as well.

What differs from pooled.py is where the rows live.  One encoder row is read by many occurrences -- the history of several
samples, the target of another -- so the gradient with respect to E is a segment sum over a batch-local row space, and it has to
come out DENSE ([M, D]: autograd hands it to the native tower) and in a fixed order: pxr_pool_dense_grad_f32, the MODE_POOL sums
through a third sink.  Row 0 and every row no sample points at get exactly +0.0.  A step: encoder forward -> pooling fused with
the pair head (one launch) -> the compact block G [3S, D] -> stable sort + segment sum into dE -> encoder backward; E reaches the
step, and dE autograd, through packed.EncoderRows.  No
[S (L + 2), D] buffer is written and no float atomic is used.  A target position equal to 0 does not occur in the batcher's
output (targets are real items); its gradient would be dropped like padding's.

Neither model has a parameter outside `visual_encoder.*`: the state_dict is the encoder's, so a reference checkpoint loads with
strict=True, and the optimizer is the visual-encoder group alone (Trainer._build_optimizer).

Contract kept: `input_type = SEQ`; `__init__(config, dataload)`; forward((index, all_item_modal)) -> loss with `index` the
reference's tensor (MODSSM [S, L + 2] = [profile | p | n]; MOFM [S, 2, L + 1], plane 0 = [profile | p], plane 1 = [profile | n];
both also take the batcher's [S, L + 2]); `loss_from_embeddings(E, profile_idx, target_idx)` is the head alone; `predict(item_seq,
item_feature)` = pooled window times item_feature^T; `compute_item(images)` = the encoder; `modal_inputs(store, data)` turns the
batcher's (index, image_ids) into the forward's input.  One process: the data-parallel exchange is not built for these models.
"""
from __future__ import annotations

import torch

from .. import ops
from ..utils.enum_type import InputType
from .basemodel import BaseModel
from .packed import EncoderRows, check_width16, dense_scores, one_process, split_planes, split_tail, store_modal_inputs
from .pooled import pool_queries
from .visual import load_model


class _MoPooledPair(EncoderRows, BaseModel):
    """What MODSSM and MOFM share: the encoder, the pooled pair step over its output (handed over through packed.EncoderRows) and
    the evaluation.  No flat buffer: the encoder's parameters are all there is."""

    input_type = InputType.SEQ
    pool_mean = False                  # MODSSM: masked mean; MOFM: masked sum

    def __init__(self, config, dataload):
        super().__init__()
        one_process(self)
        self.embedding_size = int(config["embedding_size"])
        check_width16(self.embedding_size)
        self.mlp_hidden_size = config["mlp_hidden_size"] if "mlp_hidden_size" in config else []      # read, never used
        self.dropout_prob = config["dropout_prob"] if "dropout_prob" in config else 0.0              # (modssm.py:15-16, mofm.py:17-18)
        L = config["MAX_ITEM_LIST_LENGTH"] if "MAX_ITEM_LIST_LENGTH" in config else None
        self.max_seq_length = int(L) if L else None
        self.item_num = dataload.item_num
        self.pretrain_weights = config["pretrain_path"] if "pretrain_path" in config else None
        self.visual_encoder = load_model(config=config)
        if self.pretrain_weights:
            self.load_weights(self.pretrain_weights)
        self.grad_scale = 1.0
        self._bufs = {}
        self._saved = None

    # ------------------------------------------------------------------------------------------ input forms
    def _split_index(self, index):
        """[S, L + 2] positions = [profile | positive | negative], or (profile [S, L], target [S, 2]) -> contiguous pair, L >= 1."""
        return split_tail(index, 2, self._pair_text())

    def _pair_text(self):
        return (f"{type(self).__name__}: expected [S, L + 2] positions (profile, positive, negative) or a profile [S, L] (L >= 1) and "
                "targets [S, 2], got profile {profile} and target {tail}")

    modal_inputs = staticmethod(store_modal_inputs)

    # ------------------------------------------------------------------------------------------ training
    def forward(self, interaction):
        """interaction = (index, all_item_modal fp32 [M, 3, H, W]) -> 0-dim loss (modssm.py:45-56, mofm.py:40-50)."""
        index, all_item_modal = interaction
        profile, target = self._split_index(index)
        E = self.visual_encoder(all_item_modal)
        return self.loss_from_embeddings(E, profile, target)

    def _buf(self, name, shape, device, dtype=torch.float32):
        b = self._bufs.get(name)
        if b is None or tuple(b.shape) != tuple(shape) or b.dtype != dtype or b.device != device:
            b = self._bufs[name] = torch.empty(*shape, dtype=dtype, device=device)
        return b

    def loss_from_embeddings(self, E, profile_idx, target_idx):
        """The head without the tower: E float32 [M, D] on the HIP device, profile_idx int64 [S, L] and target_idx int64 [S, 2]
        positions into E (0 = no item) -> 0-dim loss; under autograd its backward leaves d loss / d E [M, D] on E."""
        self._check_rows(E, self.embedding_size)
        profile, target = split_tail((profile_idx.to(E.device), target_idx.to(E.device)), 2, self._pair_text())
        table = E.detach().contiguous()
        if torch.is_grad_enabled():
            return self._encoded_step(E, table, profile, target)
        loss = self._pair_fwd(table, profile, target).view(()).clone()
        self._saved = None
        return loss

    def _forward_train(self, profile, target):
        return self._pair_fwd(self._train_table, profile, target)

    def _pair_fwd(self, table, profile, target):
        S, L = profile.shape
        D, dev = table.shape[1], table.device
        rows = torch.cat((profile.flatten(), target.flatten()))       # history [S L] | targets [2 S]: also the gradient's row list
        U, w, head = self._buf("U", (S, D), dev), self._buf("w", (S,), dev), self._buf("head", (2 * S + 1,), dev)
        loss, coef, _, _, _ = ops.pool_pair_fwd(table, rows, S, L, self.pool_mean, pad_row=0, U=U, w=w, out=head)
        self._saved = dict(S=S, L=L, rows=rows, U=U, w=w, coef=coef)
        return loss

    def _backward_train(self, gsd):
        """-> d loss / d E [M, D] (the bridge's anchor is the encoder's output)."""
        s, table = self._take_table()                # (backward() without a forward() raises here)
        S, L = s["S"], s["L"]
        M, D = table.shape
        G = self._buf("G", (3 * S, D), table.device)
        ops.pool_pair_bwd(table, s["rows"], S, L, s["U"], s["coef"], self.grad_scale, gsd, G=G)
        dE = ops.pool_dense_grad(s["rows"], S, L, G, s["w"], M)
        self._saved = None
        return dE

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def encode_last(self, item_seq, item_feature):
        """item_seq int64 [B, L] left-padded with 0 -> (q [B, 1, D], q [B, D]): the pooled rows of item_feature, the queries of
        the fused scoring (pooled.pool_queries: DSSM's and FM's)."""
        feat = (item_feature if item_feature.is_contiguous() else item_feature.contiguous()).data
        q = pool_queries(type(self).__name__, feat, item_seq, self.pool_mean)
        return q.view(q.shape[0], 1, -1), q

    @torch.no_grad()
    def predict(self, item_seq, item_feature):
        """scores [B, N] = q item_feature^T (predict of modssm.py / mofm.py); an all-padding window pools to exactly 0."""
        feat = (item_feature if item_feature.is_contiguous() else item_feature.contiguous()).data
        _, q = self.encode_last(item_seq, feat)
        return dense_scores(q, feat)


class MODSSM(_MoPooledPair):
    """modssm.py: masked-mean pooling of encoder rows -> pair head.  index: [S, L + 2] = [profile | positive | negative], or
    (profile [S, L], target [S, 2])."""

    pool_mean = True


class MOFM(_MoPooledPair):
    """mofm.py: x = FM([profile | p]) - FM([profile | n]) = <H, E[p]> - <H, E[n]> with H the masked sum.  index: the reference's
    [S, 2, L + 1] -- plane 0 = [profile | positive], plane 1 = [profile | negative] --, the batcher's [S, L + 2], or (profile
    [S, L], target [S, 2])."""

    pool_mean = False

    def _split_index(self, index):
        if isinstance(index, torch.Tensor) and index.dim() >= 3:
            return split_planes(index, "MOFM", self._pair_text())
        return super()._split_index(index)
