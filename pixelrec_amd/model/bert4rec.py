"""BERT4Rec (IDNet) on the MI355X-native kernels -- drop-in for the reference class
`REC.model.IDNet.bert4rec.BERT4Rec` (code/REC/model/IDNet/bert4rec.py).

The bidirectional counterpart of SASRec on the same TransformerEncoder, so everything below the model contract is the
SASRec machinery (seqcore.SeqRecCore through sasrec.SASRec: flat parameter buffer, GEMM family, h2 planes, the sparse
table gradient and the lazy / series-replay AdamW, hipGraph capture).  What differs, and how it reaches the kernels:
  * positions: the encoder runs on P = MAX_ITEM_LIST_LENGTH + 1 positions (bert4rec.py:34; trainset.py:427), and the table
    has item_num + 1 rows -- row item_num is the mask token (bert4rec.py:29-33), an ordinary row for the optimizer;
  * attention: key padding only, no causal term (get_attention_mask, bert4rec.py:150-155): the CAUSAL = false instantiations
    of every attention family (pxr_attn_fwd_f32 / pxr_attn_rows_fwd_f32 with causal = 0); the mask is built from the masked
    sequence items[:, 0], whose mask tokens are real keys;
  * loss head: the batch is items [B, 3, P] = (masked sequence | original sequence | negatives) with masked_index [B, P]
    (trainset.py:470-478); targets are aligned with the output position (no shift): the head kernels and the occurrence
    sort of the table gradient take that id layout as arguments (id_bstride and offsets in include/pxr.h).  The loss
    sum_masked -log(1e-8 + sigmoid(pos - neg)) / B (bert4rec.py:98-111) is the SASRec head's arithmetic on this layout;
  * predict: a mask-token column is appended to item_seq [B, L] and the last of the P positions is scored
    (reconstruct_test_data, bert4rec.py:61-66,116-135); compute_item_all() is weight[:item_num] (bert4rec.py:138-140).
The state_dict keys are the reference's, so checkpoints interchange.
"""
from __future__ import annotations

import torch

from .. import ops
from .packed import TrainStep
from .sasrec import SASRec


class _WithPositions:
    """The model config with MAX_ITEM_LIST_LENGTH read as the encoder's position count (L + 1)."""

    def __init__(self, config, positions):
        self._config, self._positions = config, positions

    def __getitem__(self, key):
        return self._positions if key == "MAX_ITEM_LIST_LENGTH" else self._config[key]


class BERT4Rec(SASRec):
    # the bidirectional mask and the aligned [B, 3, P] id layout
    _causal = False
    _split_catch_up_ok = False   # (the split catch-up reads SASRec's [B, 2, L+1] input window; the plain catch-up serves)
    _tail_carrier = False        # the closing reductions of its backward stay launches of their own

    def __init__(self, config, dataload):
        # SASRec.__init__ with the table and position counts of BERT4Rec (bert4rec.py:29-35)
        super(SASRec, self).__init__()
        self.item_num = dataload.item_num
        self.mask_token = self.item_num
        self.mask_ratio = float(config["mask_ratio"])
        self.max_item_list_length = int(config["MAX_ITEM_LIST_LENGTH"])
        P = self.max_item_list_length + 1
        self._build_core(_WithPositions(config, P))
        self.item_embedding = torch.nn.Embedding(self.item_num + 1, self.hidden_size, padding_idx=0)
        self.apply(self._init_weights)   # incl. table row 0 (bert4rec.py:47,53)
        self._init_table_state()
        self._head_layout = (3 * P, P, 2 * P)       # targets = items[:, 1, t], negatives = items[:, 2, t]
        self._occ_layout = (3 * P, 0, P, 2 * P)     # + the inputs items[:, 0, t]

    # ---- the id layout as the table gradient sees it
    def _occ_positions(self, items):
        return items.shape[2]

    def _table_rows(self):
        return self.item_num + 1

    def _train_inputs(self, items, masked_index):
        # input ids = the masked sequence items[:, 0]; its nonzero entries are the attention's real keys (bert4rec.py:75,86)
        P = self.max_seq_length
        return 3 * P, items, 3 * P

    def forward(self, interaction):
        """interaction = (items int64 [B,3,L+1], masked_index int64 [B,L+1]) -> 0-dim loss (bert4rec.py:70-113)."""
        items, masked_index = interaction
        P = self.max_seq_length
        if items.dim() != 3 or items.shape[1] != 3 or items.shape[2] != P:
            raise ValueError(f"items must be [B, 3, {P}], got {tuple(items.shape)}")
        if masked_index.shape != (items.shape[0], P):
            raise ValueError(f"masked_index must be [B, {P}], got {tuple(masked_index.shape)}")
        return self._forward_dispatch(items, masked_index)

    def _forward_dispatch(self, items, masked_index):
        self._ensure_packed()
        items = items.contiguous()
        masked_index = masked_index.contiguous()
        if torch.is_grad_enabled() and self.training:
            return TrainStep.apply(self._anchor, self, items, masked_index)
        was = self.training
        try:
            self.training = False
            return self._forward_train(items, masked_index).view(())
        finally:
            self.training = was

    # ------------------------------------------------------------------------------------------ inference
    def reconstruct_test_data(self, item_seq):
        """item_seq [B, L] -> [B, L+1] with the mask token appended (bert4rec.py:61-66)."""
        pad = torch.full((item_seq.shape[0], 1), self.mask_token, dtype=item_seq.dtype, device=item_seq.device)
        return torch.cat((item_seq, pad), dim=-1)

    @torch.no_grad()
    def encode_last(self, item_seq):
        """item_seq int64 [B, L] -> (states [B, L+1, D], view of the appended mask position [B, D], row stride (L+1)*D)."""
        self._ensure_packed()
        self.sync_table()
        B, L = item_seq.shape
        if L != self.max_item_list_length:
            raise ValueError(f"item_seq must have MAX_ITEM_LIST_LENGTH={self.max_item_list_length} columns, got {L}")
        seq = self.reconstruct_test_data(item_seq).contiguous()
        P = self.max_seq_length
        out, _ = self._encode(self.item_embedding.weight.data, seq, P, B, seq, P, train=False)
        return out, out[:, -1]

    @torch.no_grad()
    def predict(self, item_seq, item_feature):
        """scores [B, N] = state of the appended mask position x item_feature^T (bert4rec.py:115-135)."""
        out, last = self.encode_last(item_seq)
        B, P, D = out.shape
        feat = item_feature if item_feature.is_contiguous() else item_feature.contiguous()
        N = feat.shape[0]
        scores = torch.empty(B, N, dtype=torch.float32, device=out.device)
        ops.gemm(True, True, B, N, D, last, P * D, feat, D, scores, N, ops.EPI_NONE, use_ws=False)
        ops.raise_on_bad_indices(out.device)
        return scores

    @torch.no_grad()
    def compute_item_all(self):
        """The catalogue without the mask-token row (bert4rec.py:138-140)."""
        self.sync_table()
        return self.item_embedding.weight[:self.item_num]
