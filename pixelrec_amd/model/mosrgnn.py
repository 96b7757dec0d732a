"""MOSRGNN (PixelNet) -- drop-in for `REC.model.PixelNet.mosrgnn.MOSRGNN` (code/REC/model/PixelNet/mosrgnn.py): SRGNN's session
graph, gated cells, attention readout and pair head with the visual encoder's output in the item table's place.  With
E = visual_encoder(images) [M, D] and idx [B, L + 2] = [item_seq (right-padded) | positive | negative] positions into E (0 = no item):

    session graph of idx[:, :L] at a fixed L nodes;  H_0 = E[nodes];  `step` gated-GNN cells (srgnn.py's arithmetic)
    readout with mask = idx[:, :L] != 0;  out = linear_transform([a | ht])
    loss = -mean(1e-8 + log sigmoid(<out, E[p]> - <out, E[n]>))                                   (mosrgnn.py:64-74)

The step between the graph and the node gradients is SRGNN's code (srgnn.SrgnnStep), launch for launch; E reaches it through
packed.EncoderRows (`_train_table`, the autograd bridge anchored at E).  What closes it is the gradient of E: one encoder row is
read by many nodes and targets, so it is a segment sum over a batch-local row space that comes out DENSE ([M, D]: autograd hands
it to the native tower) and in a fixed order -- pxr_seq_occ_dense_f32 over the id rows [B, 3L] = nodes | target | negative that the
graph build writes, the sums of SRGNN's sparse table gradient through the dense sink.  No float atomic is used.

Row 0 of E is the zero image's encoding (it is not zero).  A padding node reads it, has no edges, and every position that aliases
it is masked in the readout: the loss does not depend on it and the gradient that reaches it is exactly +0.0, which is what the
dense sink writes to row 0 and to every row nobody reads.

The reference's collate stacks one image per node slot and target -- B (n + 2) a step, n the batch's largest node count, pad
images included; the batcher here (data.MoGraphTrainBatcher) lists each distinct image of the batch once.  The CLIP tower is a
per-image function without batch statistics or dropout, so an image encoded once receives the sum of the gradients its copies
would have received: the same parameter gradients.  `forward` also takes the reference's own 4-tuple.

Contract kept: `input_type = AUGSEQ`; `__init__(config, dataload)` with `embedding_size`, `step`; forward((index [B, L + 2],
images [M, 3, H, W])) -> loss, or the reference's (alias_inputs [B, L], A [B, n, 2n], mask [B, L], items_all [B (n + 2), 3, H, W]),
recognised by its length; `loss_from_embeddings(E, item_idx, target_idx)` is the head without the tower; `modal_inputs(store,
data)` turns the batcher's (index, image_ids) into the forward's input; `compute_item(images)` = the encoder; `encode_last` /
`predict(item_seq, item_feature)` read the node rows from item_feature (mosrgnn.py:78-83).  `state_dict` keeps the reference's
keys and order (visual_encoder.*, gnn.*, linear_{one,two,three,transform}), so reference checkpoints load with strict=True;
`gnn.linear_edge_f` is read by nothing and never changes.  M changes from batch to batch: the step runs eagerly, on one process.
"""
from __future__ import annotations

import math

import torch

from .. import ops
from ..utils.enum_type import InputType
from .packed import EncoderRows, PackedModel, dense_scores, one_process, split_tail, store_modal_inputs
from .srgnn import SrgnnStep
from .visual import load_model


class MOSRGNN(EncoderRows, SrgnnStep, PackedModel):
    input_type = InputType.AUGSEQ

    def __init__(self, config, dataload):
        super().__init__()
        one_process(self, "MOSRGNN")
        self.item_num = dataload.item_num
        self.visual_encoder = load_model(config=config)
        self._build_gnn(config)
        # mosrgnn.py:33-44,113-116: gnn.* and the four Linears' weights uniform(-stdv, stdv), their biases nn.Linear's default;
        # then the encoder's rec_fc
        stdv = 1.0 / math.sqrt(self.hidden_size)
        for w in self.gnn.parameters():
            w.data.uniform_(-stdv, stdv)
        for lin in (self.linear_one, self.linear_two, self.linear_three, self.linear_transform):
            lin.weight.data.uniform_(-stdv, stdv)
        for w in self.visual_encoder.rec_fc.parameters():
            w.data.uniform_(-stdv, stdv)

    def rec_parameter_names(self):
        """{reference parameter name: flat-buffer key} in the reference's registration order (optim.native_to_torch_state):
        there is no table, and linear_edge_f (no gradient, no optimizer state) maps to None."""
        return self._gnn_parameter_names()

    def _occ_layout(self):
        L = self.max_seq_length
        return 3 * L, 0, L, 2 * L       # the id rows of pxr_srgnn_graph_i64: nodes | target, 0.. | negative, 0..

    # ------------------------------------------------------------------------------------------ input forms
    def _split_index(self, index):
        """[B, L + 2] positions = [item_seq | positive | negative], or (item_seq [B, L], target [B, 2]) -> contiguous pair."""
        L = self.max_seq_length
        seq, target = split_tail(index, 2, "MOSRGNN: expected [B, L + 2] positions (item_seq, positive, negative), got item_seq "
                                           "{profile} and target {tail}", max_len=L)
        if seq.shape[1] != L:
            raise ValueError(f"MOSRGNN: item_seq must be [B, {L}], got {tuple(seq.shape)}")
        return seq, target

    modal_inputs = staticmethod(store_modal_inputs)

    def _reference_form(self, alias_inputs, A, mask, items_all):
        """mosrgnn.py:64-70's input -> (graph dict at L nodes, mask, target [B, 2], images): a zero image goes in front, node slot
        k of sample b reads row 1 + b (n + 2) + k and its two targets rows + n and + n + 1; the given alias and A are padded from
        n to L nodes (the [:, :n, :n] and [:, :n, L:L + n] blocks), and the extra node slots read row 0."""
        L = self.max_seq_length
        B = mask.shape[0]
        n = A.shape[1] if A.dim() == 3 else -1
        if tuple(alias_inputs.shape) != (B, L) or tuple(mask.shape) != (B, L) or not 1 <= n <= L or tuple(A.shape) != (B, n, 2 * n):
            raise ValueError(f"MOSRGNN: expected alias_inputs [B, {L}], A [B, n, 2n] with n <= {L} and mask [B, {L}], got "
                             f"{tuple(alias_inputs.shape)}, {tuple(A.shape)}, {tuple(mask.shape)}")
        if items_all.dim() != 4 or items_all.shape[0] != B * (n + 2):
            raise ValueError(f"MOSRGNN: items_all must be [B (n + 2), 3, H, W] = [{B * (n + 2)}, ...], got {tuple(items_all.shape)}")
        dev = items_all.device
        first = 1 + (n + 2) * torch.arange(B, dtype=torch.int64, device=dev)[:, None]           # [B, 1]
        k = torch.arange(L, dtype=torch.int64, device=dev)[None, :]
        nodes = torch.where(k < n, first + k, torch.zeros_like(k))                               # [B, L]
        target = torch.cat((first + n, first + n + 1), dim=1)
        zeros = torch.zeros(B, L - 1, dtype=torch.int64, device=dev)
        occ = torch.cat((nodes, target[:, :1], zeros, target[:, 1:], zeros), dim=1)
        A = A.to(device=dev, dtype=torch.float32)
        Ap = torch.zeros(B, L, 2 * L, dtype=torch.float32, device=dev)
        Ap[:, :n, :n] = A[:, :, :n]
        Ap[:, :n, L:L + n] = A[:, :, n:]
        g = dict(nodes=nodes.contiguous(), alias=alias_inputs.to(device=dev, dtype=torch.int32).contiguous(), A=Ap,
                 occ=occ.contiguous(), mask=None)
        images = torch.cat((torch.zeros_like(items_all[:1]), items_all))
        return g, mask.to(device=dev, dtype=torch.int64).contiguous(), target.contiguous(), images

    # ------------------------------------------------------------------------------------------ training
    def forward(self, interaction):
        """interaction = (index int64 [B, L + 2], images fp32 [M, 3, H, W]) -> 0-dim loss (mosrgnn.py:64-74); or the reference's
        own (alias_inputs int64 [B, L], A fp32 [B, n, 2n], mask int64 [B, L], items_all fp32 [B (n + 2), 3, H, W])."""
        self._ensure_packed()                # (raises on a CPU model before the tower runs)
        if len(interaction) == 4:
            g, mask, target, images = self._reference_form(*interaction)
            return self._loss_from_graph(self.visual_encoder(images), g, mask, target)
        index, images = interaction
        item_idx, target_idx = self._split_index(index)
        return self.loss_from_embeddings(self.visual_encoder(images), item_idx, target_idx)

    def loss_from_embeddings(self, E, item_idx, target_idx):
        """The head without the tower: E float32 [M, D] on the HIP device, item_idx int64 [B, L] (right-padded) and target_idx
        int64 [B, 2] positions into E (0 = no item) -> 0-dim loss; under autograd its backward leaves d loss / d E [M, D] on E and
        the 17 gradients of the block in the flat gradient buffer.  A position outside [0, M) flags the status word."""
        self._check_rows(E, self.hidden_size)
        self._ensure_packed()
        item_idx, target_idx = self._split_index((item_idx.to(E.device), target_idx.to(E.device)))
        g = ops.srgnn_graph(item_idx, E.shape[0], target_idx, want_occ=True, want_mask=True, out=self._gbufs)
        return self._loss_from_graph(E, g, g["mask"], target_idx)

    def _loss_from_graph(self, E, g, mask, target):
        self._check_rows(E, self.hidden_size)
        table = E.detach().contiguous()
        if torch.is_grad_enabled() and self.training:
            return self._encoded_step(E, table, g, mask, target)
        was = self.training
        try:
            self.training = False        # (nothing is saved for a backward)
            return self._step_forward(table, g, mask, target).view(()).clone()
        finally:
            self.training = was

    def _forward_train(self, g, mask, target):
        return self._step_forward(self._train_table, g, mask, target)

    def _backward_train(self, gsd):
        """-> d loss / d E [M, D] (the bridge's anchor is the encoder's output)."""
        s, table = self._take_table()                # (backward() without a forward() raises here)
        B, L, D = s["B"], self.max_seq_length, self.hidden_size
        dH, coef_pad = self._step_backward(gsd, table, s)
        # the gradient of E: stable sort of the 3 B L occurrences + segmented sum into a dense block (position 0: dropped)
        dE = ops.seq_occ_dense_grad(s["g"]["occ"], self._occ_layout(), dH.view(B, L, D), s["out_pad"], coef_pad, table.shape[0])
        self._step_done()
        return dE

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def encode_last(self, item_seq, item_feature):
        """item_seq int64 [B, L] (right-padded; mask = item_seq != 0), item_feature [N, D] -> (out [B, 1, D], out [B, D]): the
        query vectors of the fused scoring, H_0 = item_feature[nodes] (mosrgnn.py:80)."""
        self._ensure_packed()
        self._check_rows(item_feature, self.hidden_size)
        out = self._encode(item_seq, item_feature.contiguous())
        return out.view(out.shape[0], 1, -1), out

    @torch.no_grad()
    def predict(self, item_seq, item_feature):
        """scores [B, N] = seq_output item_feature^T (mosrgnn.py:77-83)."""
        feat = item_feature if item_feature.is_contiguous() else item_feature.contiguous()
        _, out = self.encode_last(item_seq, feat)
        return dense_scores(out, feat)
