"""MOBERT4Rec (PixelNet) -- drop-in for `REC.model.PixelNet.mobert4rec.MOBERT4Rec` (code/REC/model/PixelNet/mobert4rec.py):
BERT4Rec's bidirectional block and masked-item head with the visual encoder's output in the item table's place.  With
E = visual_encoder(images) [M, D] and idx [B, 3, P] positions into E (P = MAX_ITEM_LIST_LENGTH + 1; plane 0 the masked input
sequence, plane 1 the original sequence, plane 2 the negatives):

    x_t  = LayerNorm(E[idx[b,0,t]] + position_embedding[t]) -> dropout -> TransformerEncoder, key padding only: a key is real
           where idx[b,0,t] != 0 (mobert4rec.py:87-97,138-143)
    loss = sum over masked_index != 0 of -log(1e-8 + sigmoid(<out_t, E[idx[b,1,t]]> - <out_t, E[idx[b,2,t]]>)) / B   (:99-111)

Row 0 of E is the zero image's encoding ("no item"; it is not zero), row 1 the mask image's (all ones after normalisation), rows
2.. the batch's distinct item images.  That is bert4rec.BERT4Rec's arithmetic on E, so the model is a composition: the id layout,
the uncausal attention and the P positions are BERT4Rec's, and E reaches the block through packed.EncoderRows (`_train_table`, the
autograd bridge anchored at E).  One step closes it: each image is encoded ONCE and read by many positions, so the gradient
with respect to E is a segment sum over a batch-local row space that has to come out DENSE ([M, D]: autograd hands it to the
native tower) and in a fixed order -- pxr_seq_occ_dense_f32, the sums of BERT4Rec's sparse table gradient (dx0[r], +coef[r] out[r],
-coef[r] out[r]) through the dense sink.  Row 0 and every row nobody reads get exactly +0.0; no float atomic is used.

Padded input positions: the reference feeds the ones image there (trainset.py:907), masks them as keys and keeps their outputs
out of the loss, so they are inert; here they hold position 0 and the segment sum drops them.  Padded positive / negative positions
hold 0 as well (the reference's zero image; coef is 0 there).

Contract kept: `input_type = SEQ`; `__init__(config, dataload)`; forward((index [B, 3, P], images [M, 3, H, W], masked_index
[B, P])) -> loss, or the reference's own (input_ids [B, P], items_modal [B, 3 P, 3, H, W], masked_index), recognised by the 5-D
tensor; `loss_from_embeddings(E, index, masked_index)` is the head without the tower; `modal_inputs(store, data)` turns the
batcher's (index, masked_index, image_ids) into the forward's input; `compute_item(images)` = the encoder;
`extra_item_images(H, W, device)` is the ones image the Trainer appends to the catalogue, so item_feature is [item_num + 1, D]
with the mask row last; `predict(item_seq, item_feature)` appends the mask row to the window and scores the last of the P
positions against item_feature[:item_num] (mobert4rec.py:113-132); `scoring_item_matrix()` is that slice, so the fused top-k never
ranks the mask row.  `state_dict` keeps the reference's keys and order (visual_encoder.*, position_embedding, trm_encoder.*,
LayerNorm), so reference checkpoints load with strict=True.  M changes from batch to batch: the step runs eagerly, on one process.
"""
from __future__ import annotations

import torch

from .. import ops
from ..lib import PxrError
from ..utils.enum_type import InputType
from .bert4rec import _WithPositions
from .packed import EncoderRows, dense_scores, one_process
from .seqcore import SeqRecCore
from .visual import load_model


class MOBERT4Rec(EncoderRows, SeqRecCore):
    input_type = InputType.SEQ
    # BERT4Rec's bidirectional mask (key padding only)
    _causal = False

    def __init__(self, config, dataload):
        super().__init__()
        one_process(self, "MOBERT4Rec")
        self.item_num = dataload.item_num
        self.mask_token = self.item_num
        self.mask_ratio = float(config["mask_ratio"])
        self.max_item_list_length = int(config["MAX_ITEM_LIST_LENGTH"])
        self.embedding_size = config["embedding_size"]
        P = self.max_item_list_length + 1
        self.visual_encoder = load_model(config=config)
        self._build_core(_WithPositions(config, P))       # position_embedding has P rows (mobert4rec.py:35)
        # mobert4rec.py:51-54: position table N(0, init_range); encoder block through _init_weights; LayerNorm (1, 0)
        self.position_embedding.weight.data.normal_(mean=0.0, std=self.initializer_range)
        self.trm_encoder.apply(self._init_weights)
        self.LayerNorm.bias.data.zero_()
        self.LayerNorm.weight.data.fill_(1.0)
        self._head_layout = (3 * P, P, 2 * P)       # targets = idx[:, 1, t], negatives = idx[:, 2, t]
        self._occ_layout = (3 * P, 0, P, 2 * P)     # + the inputs idx[:, 0, t]
        self._item_feature = None

    def rec_parameter_names(self):
        """{reference parameter name: flat-buffer key} in the reference's registration order (mobert4rec.py:35-47:
        position_embedding, trm_encoder, LayerNorm; optim.native_to_torch_state)."""
        from ..optim import _layer_names, _short_name

        names = (["position_embedding.weight"] + [n for i in range(self.n_layers) for n in _layer_names(i)]
                 + ["LayerNorm.weight", "LayerNorm.bias"])
        return {n: _short_name(n) for n in names}

    def _train_inputs(self, items, masked_index):
        # input positions = plane 0; its nonzero entries are the attention's real keys (mobert4rec.py:94,138-143)
        P = self.max_seq_length
        return 3 * P, items, 3 * P

    # ------------------------------------------------------------------------------------------ input forms
    def modal_inputs(self, store, data):
        """The batcher's (index [B, 3, P], masked_index [B, P], image_ids [M]) -> the forward's (index, images [M, 3, H, W],
        masked_index): each distinct image of the batch is fetched, and later encoded, once.  The mask token's row is the ones
        image (trainset.py:849; a store pixel of 255 also normalises to 1.0, but the store has no such row)."""
        index, masked_index, image_ids = data
        images = store.batch(torch.where(image_ids == self.mask_token, torch.zeros_like(image_ids), image_ids))
        images[1].fill_(1.0)
        return index, images, masked_index

    @staticmethod
    def reference_positions(input_ids, masked_index):
        """The reference's one image per (position, input | positive | negative), behind a zero image: input (b, t) at
        1 + 3 (b P + t) where input_ids != 0, its positive and negative at + 1 / + 2 where masked_index != 0, 0 elsewhere
        -> index int64 [B, 3, P]."""
        B, P = input_ids.shape
        if tuple(masked_index.shape) != (B, P):
            raise ValueError(f"MOBERT4Rec: masked_index must be [B, P] = [{B}, {P}] next to input_ids, got {tuple(masked_index.shape)}")
        base = 1 + 3 * torch.arange(B * P, dtype=torch.int64, device=input_ids.device).view(B, P)
        zero = torch.zeros_like(base)
        m = masked_index != 0
        return torch.stack((torch.where(input_ids != 0, base, zero), torch.where(m, base + 1, zero), torch.where(m, base + 2, zero)),
                           dim=1)

    def _reference_form(self, input_ids, items_modal, masked_index):
        B, P = input_ids.shape
        if items_modal.shape[0] != B or items_modal.shape[1] != 3 * P:
            raise ValueError(f"MOBERT4Rec: items_modal must be [B, 3 P, 3, H, W] = [{B}, {3 * P}, ...] next to input_ids "
                             f"{tuple(input_ids.shape)}, got {tuple(items_modal.shape)}")
        flat = items_modal.flatten(0, 1)
        return self.reference_positions(input_ids, masked_index), torch.cat((torch.zeros_like(flat[:1]), flat))

    # ------------------------------------------------------------------------------------------ training
    def forward(self, interaction):
        """interaction = (index int64 [B, 3, P], images fp32 [M, 3, H, W], masked_index int64 [B, P]) -> 0-dim loss
        (mobert4rec.py:78-111); or the reference's own (input_ids [B, P], items_modal fp32 [B, 3 P, 3, H, W], masked_index)."""
        index, images, masked_index = interaction
        self._ensure_packed()                # (raises on a CPU model before the tower runs)
        if images.dim() == 5:
            index, images = self._reference_form(index, images, masked_index)
        return self.loss_from_embeddings(self.visual_encoder(images), index, masked_index)

    def loss_from_embeddings(self, E, index, masked_index):
        """The head without the tower: E float32 [M, D] on the HIP device, index int64 [B, 3, P] positions into E (0 = no item),
        masked_index int64 [B, P] -> 0-dim loss; under autograd its backward leaves d loss / d E [M, D] on E and the block's
        gradients in the flat gradient buffer."""
        P = self.max_seq_length
        self._check_rows(E, self.hidden_size)
        if index.dim() != 3 or index.shape[1] != 3 or index.shape[2] != P:
            raise ValueError(f"MOBERT4Rec: index must be [B, 3, {P}], got {tuple(index.shape)}")
        if tuple(masked_index.shape) != (index.shape[0], P):
            raise ValueError(f"MOBERT4Rec: masked_index must be [B, {P}], got {tuple(masked_index.shape)}")
        self._ensure_packed()
        index = index.to(E.device).contiguous()
        masked_index = masked_index.to(E.device).contiguous()
        table = E.detach().contiguous()
        if torch.is_grad_enabled() and self.training:
            return self._encoded_step(E, table, index, masked_index)
        return self._forward_core(table, index, masked_index, train=False).view(())

    def _forward_train(self, index, masked_index):
        return self._forward_core(self._train_table, index, masked_index, train=True)

    def _backward_train(self, gsd):
        """-> d loss / d E [M, D] (the bridge's anchor is the encoder's output)."""
        _, table = self._take_table()                # (backward() without a forward() raises here)
        dx0, coef, s = self._backward_core(gsd, table)
        # the gradient of E: stable sort of the 3 B P occurrences + segmented sum into a dense block (position 0: dropped)
        return ops.seq_occ_dense_grad(s["items"], self._occ_layout, dx0.view_as(s["out"]), s["out"], coef, table.shape[0])

    # ------------------------------------------------------------------------------------------ evaluation
    @staticmethod
    def extra_item_images(H, W, device):
        """What the catalogue holds behind the store's rows (reference BatchDataset: item_num + 1 entries for the BERT4Rec
        models, the last one the ones image) -> fp32 [1, 3, H, W]."""
        return torch.ones(1, 3, H, W, dtype=torch.float32, device=device)

    def _check_feature(self, item_feature):
        if item_feature.dim() != 2 or item_feature.shape != (self.item_num + 1, self.hidden_size):
            raise ValueError(f"MOBERT4Rec: item_feature must be [item_num + 1, D] = [{self.item_num + 1}, {self.hidden_size}] with the "
                             f"mask image's row last (Trainer.compute_item_feature appends extra_item_images), got "
                             f"{tuple(item_feature.shape)}")

    @torch.no_grad()
    def set_item_feature(self, feat):
        """The encoded catalogue [item_num + 1, D] (Trainer.compute_item_feature hands it over)."""
        self._check_feature(feat)
        self._item_feature = feat.detach().contiguous()

    def scoring_item_matrix(self):
        """What the fused top-k ranks: the catalogue without the mask row."""
        if self._item_feature is None:
            raise PxrError("MOBERT4Rec: no item_feature yet -- call set_item_feature first (Trainer.compute_item_feature does)")
        return self._item_feature[:self.item_num]

    def reconstruct_test_data(self, item_seq):
        """item_seq [B, L] -> [B, L+1] with the mask token appended (mobert4rec.py:68-73)."""
        pad = torch.full((item_seq.shape[0], 1), self.mask_token, dtype=item_seq.dtype, device=item_seq.device)
        return torch.cat((item_seq, pad), dim=-1)

    @torch.no_grad()
    def encode_last(self, item_seq, item_feature):
        """item_seq int64 [B, L], item_feature [item_num + 1, D] -> (states [B, L+1, D], view of the appended mask position)."""
        self._check_feature(item_feature)
        self._ensure_packed()
        B, L = item_seq.shape
        if L != self.max_item_list_length:
            raise ValueError(f"item_seq must have MAX_ITEM_LIST_LENGTH={self.max_item_list_length} columns, got {L}")
        seq = self.reconstruct_test_data(item_seq).contiguous()
        P = self.max_seq_length
        feat = item_feature if item_feature.is_contiguous() else item_feature.contiguous()
        out, _ = self._encode(feat, seq, P, B, seq, P, train=False)                   # mobert4rec.py:115-128
        return out, out[:, -1]

    @torch.no_grad()
    def predict(self, item_seq, item_feature):
        """scores [B, item_num] = state of the appended mask position x item_feature[:item_num]^T (mobert4rec.py:113-132)."""
        out, last = self.encode_last(item_seq, item_feature)
        B, P, D = out.shape
        return dense_scores(last, item_feature[:self.item_num].contiguous(), ldq=P * D)
