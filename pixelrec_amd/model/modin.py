"""MODIN (PixelNet) -- drop-in for `REC.model.PixelNet.modin.MODIN` (code/REC/model/PixelNet/modin.py, with SequenceAttLayer of
code/REC/model/layers.py:460-514): DIN of din.py with the visual encoder's output in the item table's place, on the same kernels
(csrc/din.hip, MODE_ROWS of csrc/embed_grad.hip through the dense sink).  With E = visual_encoder(all_item_modal) [M, D] -- one row
per distinct image of the batch, row 0 the zero image's encoding (which is not zero) -- idx positions into E (0 = "no item"),
k_l = E[idx_{s,l}] and a candidate q:

    s_l(q)   = dense(sigmoid(... sigmoid(W1 [q | k_l | q - k_l | q * k_l] + b1) ...))     0 where idx_{s,l} == 0, then / sqrt(D)
    score(q) = sum_l s_l(q) <k_l, q>                                       (softmax_stag=False: the weights are NOT normalised)
    loss     = -mean_s log(sigmoid(score(E[p_s]) - score(E[n_s])) + 1e-8)                  (modin.py:61: NO regulariser)

A padded position reads E[0] under the mask and receives no gradient, as in the reference (its zero image is encoded like any
other and masked afterwards).

What differs from din.py is where the rows live.  One encoder row is read by many occurrences, so the gradient with respect to E
is a segment sum over a batch-local row space and has to come out DENSE ([M, D]: autograd hands it to the native tower) and in a
fixed order: pxr_embed_grad_dense_f32, the sums of DIN's sparse table gradient through the dense sink.  Row 0 and every row no
sample points at get exactly +0.0.  A step: encoder forward -> position check (pxr_table_rows_i64, base 0) -> attention-input
kernel -> the MLP Linears with the sigmoid epilogue -> head forward with reg = 0 (pxr_din_head_fwd_reg_f32) -> head backward ->
the MLP's input-gradient GEMMs -> fold kernel (one gradient row per occurrence; head[1] == 0 adds an exact zero) -> stable sort +
segment sum into dE -> encoder backward; the weight gradients in DIN's grouped launches.  No float atomic is used.

The reference's dataset (MOTwoTowerTrainDataset, REC/data/utils.py:44) returns the images alone while forward unpacks
(items_modal, items): the mapped pair does not run as shipped.  Here the batcher carries the ids (data.MoTowerTrainBatcher), each
distinct image of a batch is encoded ONCE and the gradients of its occurrences are summed into it -- the same parameter
gradients as the reference's one image per position, which `forward` also accepts.

The step between the row list and the occurrence rows is DIN's code (din.DinStep); E reaches it through packed.EncoderRows
(`_train_table`, the autograd bridge anchored at E).  The evaluation is DIN's as well (din.DinEval), on the encoded catalogue: `set_item_feature(feat)` hands the [item_num, D] matrix over, and
`fused_topk_batch` scores and ranks a batch of users in one launch of pxr_din_topk_f32; A q + b1 is made once per evaluation and
cached until train(), load_state_dict or a new set_item_feature.  `predict` takes the reference's [B, item_num, L + 1] id tensor or
[B, L] windows, in candidate chunks.

Contract kept: `input_type = SEQ`; `__init__(config, dataload)` with `embedding_size`, `mlp_hidden_size`, `dropout_prob` (read and
ignored, as in the reference); forward((index, all_item_modal)) -> loss; `loss_from_embeddings(E, profile_idx, target_idx)` is the
head alone; `compute_item(images)` = the encoder; `modal_inputs(store, data)` turns the batcher's (index, image_ids) into the
forward's input; `state_dict` keys and order of the reference (attention.*, then visual_encoder.*; xavier-normal attention weights,
zero biases), so reference checkpoints load with strict=True.  One process: the data-parallel exchange is not built for this model.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..lib import PxrError
from ..utils.enum_type import InputType
from .din import DinEval, DinStep
from .packed import EncoderRows, PackedModel, linear_names, split_tail, store_modal_inputs
from .visual import load_model


class MODIN(EncoderRows, DinStep, DinEval, PackedModel):
    input_type = InputType.SEQ

    def __init__(self, config, dataload):
        super().__init__()
        self._build_attention(config, dataload)
        for mod in self.modules():                       # modin.py:30,36-42: before the encoder exists, so it is not touched
            if isinstance(mod, nn.Linear):
                nn.init.xavier_normal_(mod.weight.data)
                nn.init.zeros_(mod.bias.data)
        self.visual_encoder = load_model(config=config)
        self._item_feature = None

    # ------------------------------------------------------------------------------------------ packing
    def rec_parameter_names(self):
        """{reference parameter name: flat-buffer key} in the reference's registration order (optim.native_to_torch_state): the
        attention tensors; there is no table."""
        return linear_names(self._linears())

    # ------------------------------------------------------------------------------------------ input forms
    def _split_index(self, index):
        """[S, L + 2] positions = [profile | positive | negative], or (profile [S, L], target [S, 2]) -> contiguous pair."""
        return split_tail(index, 2, "MODIN: expected [S, L + 2] positions (profile, positive, negative), got profile {profile} and "
                                    "target {tail}")

    modal_inputs = staticmethod(store_modal_inputs)

    @staticmethod
    def _reference_form(items_modal, items):
        """modin.py:44-48's (items_modal [B, L + 2, 3, H, W], items [B, L + 2]) -> (index, all_item_modal): the zero image in
        front, position j of sample b at 1 + b (L + 2) + j where items != 0 and at 0 elsewhere."""
        B, W = items_modal.shape[:2]
        if tuple(items.shape) != (B, W):
            raise ValueError(f"MODIN: items must be [B, L + 2] = [{B}, {W}] next to items_modal {tuple(items_modal.shape)}, got "
                             f"{tuple(items.shape)}")
        flat = items_modal.flatten(0, 1)
        images = torch.cat((torch.zeros_like(flat[:1]), flat))
        pos = 1 + torch.arange(B * W, dtype=torch.int64, device=items.device).view(B, W)
        return torch.where(items != 0, pos, torch.zeros_like(pos)), images

    # ------------------------------------------------------------------------------------------ training
    def forward(self, interaction):
        """interaction = (index, all_item_modal fp32 [M, 3, H, W]) -> 0-dim loss (modin.py:44-62); or the reference's own
        (items_modal fp32 [B, L + 2, 3, H, W], items int64 [B, L + 2])."""
        first, second = interaction
        if isinstance(first, torch.Tensor) and first.dim() == 5 and first.is_floating_point():
            first, second = self._reference_form(first, second)
        profile, target = self._split_index(first)
        E = self.visual_encoder(second)
        return self.loss_from_embeddings(E, profile, target)

    def loss_from_embeddings(self, E, profile_idx, target_idx):
        """The head without the tower: E float32 [M, D] on the HIP device, profile_idx int64 [S, L] and target_idx int64 [S, 2]
        positions into E (0 = no item) -> 0-dim loss; under autograd its backward leaves d loss / d E [M, D] on E and the
        attention gradients in the flat gradient buffer."""
        self._check_rows(E, self.embedding_size)
        self._ensure_packed()
        profile, target = self._split_index((profile_idx.to(E.device), target_idx.to(E.device)))
        table = E.detach().contiguous()
        if torch.is_grad_enabled():
            return self._encoded_step(E, table, profile, target)
        loss = self._head_fwd(table, profile, target).view(()).clone()
        self._saved = None
        return loss

    def _forward_train(self, profile, target):
        return self._head_fwd(self._train_table, profile, target)

    def _head_fwd(self, E, profile, target):
        rows, gidx = ops.din_positions(profile, target, E.shape[0], out=self._buf("rows", (2, profile.numel() + target.numel()), torch.int64))
        return self._attention_fwd(E, rows, gidx, profile, 0.0)      # modin.py:61: no regulariser

    def _backward_train(self, gsd):
        """-> d loss / d E [M, D] (the bridge's anchor is the encoder's output)."""
        _, table = self._take_table()                # (backward() without a forward() raises here)
        gidx, occ = self._attention_bwd(gsd)
        # the gradient of E: stable sort of the occurrence rows + segmented sum into a dense block (position 0: dropped)
        dE = ops.embed_grad_dense(gidx, occ, table.shape[0])
        self._step_done()
        return dE

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def set_item_feature(self, feat):
        """The encoded catalogue [item_num, D] the fused scoring reads (Trainer.compute_item_feature hands it over); what the
        last one left in the evaluation cache goes."""
        if feat.dim() != 2 or feat.dtype != torch.float32 or feat.shape[1] != self.embedding_size:
            raise ValueError(f"MODIN: item_feature must be float32 [N, {self.embedding_size}], got {tuple(feat.shape)} {feat.dtype}")
        self._item_feature = feat.detach().contiguous()
        self._drop_eval_cache()

    def _item_rows(self):
        if self._item_feature is None:
            raise PxrError("MODIN: no item_feature yet -- call set_item_feature(compute_item(images of the catalogue)) first "
                           "(Trainer.compute_item_feature does)")
        return self._item_feature
