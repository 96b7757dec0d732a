"""SASRec (IDNet) on the MI355X-native kernels -- drop-in for the reference class
`REC.model.IDNet.sasrec.SASRec` (code/REC/model/IDNet/sasrec.py:9-126).

Contract kept: class attr `input_type`; `__init__(config, dataload)`; `forward(interaction) ->
0-dim loss` usable with `loss.backward()`; `predict(item_seq, item_feature) -> [B, N]`; `compute_item_all()`;
an nn.Module whose `state_dict()` keys are exactly the reference's, so checkpoints interchange.

The sequence block itself lives in seqcore.SeqRecCore; this class adds the item-embedding table:
  * the table gradient is never dense: backward leaves `(uniq_idx, uniq_rows, n)` in `self.sparse_table_grad` for
    pixelrec_amd.optim.PxrAdamW (dense AdamW semantics, sparse gradient);
  * the occurrence sort that de-duplicates the batch's ids runs BEFORE the forward pass, so that a lazy optimizer can
    bring exactly those rows up to date before they are read.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from .. import ops
from ..utils.enum_type import InputType
from .packed import TableHooks, TrainStep
from ..lib import PxrError
from .seqcore import SeqRecCore


class SASRec(TableHooks, SeqRecCore):
    input_type = InputType.SEQ

    def __init__(self, config, dataload):
        super().__init__()
        self.item_num = dataload.item_num
        self._build_core(config)
        self.item_embedding = nn.Embedding(self.item_num, self.hidden_size, padding_idx=0)
        self.apply(self._init_weights)   # incl. table row 0 (sasrec.py:49,56)
        self._init_table_state()

    def _init_table_state(self):
        """Bookkeeping of the sparsely updated item table (shared with the sibling ID backbones)."""
        self._local_sparse = None       # reusable output buffer of this rank's backward (-> sparse_table_grad, local or merged)
        self._occ_ws = None             # persistent workspace carrying the sorted occurrences fwd -> bwd
        self._occ_ws2 = None            # second workspace of the split segment sums (big batches; zero-initialised cursor)
        # look-ahead for a lazy table optimizer: the ids of the NEXT batch (set_next_batch).  Their rows are brought up to
        # date on a side stream while this step's GEMMs run (MFMA pipe) instead of at the head of the next step
        self._next_items = None
        self._next_sparse = None        # unique ids of the next batch (own buffers: the current batch's are in use)
        self._next_ws = None
        self._prefetched = None         # (SparseRows of the next batch) the optimizer advances through the current step
        self._prefetch_stream = None
        self._sort_stream = None        # the batch's id sort runs beside the forward pass (lazy table optimizer)
        self._sort_pending = False
        self._fork = None
        # split catch-up (see _forward_train): opt-in for loops that issue the step as a captured graph, where the fork / join
        # are graph edges; PXR_CATCHUP_SPLIT=0/1 overrides
        env = os.environ.get("PXR_CATCHUP_SPLIT")
        self.split_catch_up = (env == "1")
        self._split_env = env

    # state_dict key order of the reference: item_embedding first (sasrec.py:31-45); register order above differs only
    # in position, which load_state_dict does not care about.

    def set_next_batch(self, items_next):
        """Optional look-ahead (lazy table optimizer only): `items_next` int64 [B,2,L+1] on the device = the batch the
        NEXT forward will see.  Consumed by the next training forward.  Purely a schedule hint: the step computes the
        same bits with or without it (rows are caught up exactly either way; tested).
        OFF by default everywhere (GraphedTrainStep(lookahead=False), Trainer `lookahead_rows`, bench --lookahead):
        measured on MI355X it takes the replay (69 -> 11 us) off the head of the step but the replay kernel running
        beside the forward GEMMs slows them by more than that (1.205 -> 1.247 ms/step; thin grids and a low-priority
        stream do not change it) -- see DESIGN.md "dead ends"."""
        self._next_items = items_next

    # ---- the id layout of a training batch, as the table-gradient sort sees it (BERT4Rec overrides these four)
    # the split catch-up claims the input rows from the raw window items[:, 0, :L] of SASRec's [B, 2, L+1] layout
    _split_catch_up_ok = True
    # (id_bstride, in_off, pos_off, neg_off) of the input / target / negative ids in `items`; None = SASRec's shifted windows
    _occ_layout = None

    def _occ_positions(self, items):
        """Positions per sequence of a batch `items` [B, 2, L+1]: L."""
        return items.shape[2] - 1

    def _table_rows(self):
        """Rows of the item table the batch's ids index (the n_table of the occurrence sort and its segment sums)."""
        return self.item_num

    def _occ_sort(self, items, sp, ws):
        """Phase 1 of the table gradient: the batch's unique ids into `sp`, the sorted occurrences into `ws`."""
        ops.occ_sort(items, self._occ_positions(items), self._occ_layout, self._table_rows(), sp, ws)

    def _start_prefetch(self, items_next):
        """Sort the next batch's ids and replay their rows' missed steps on a side stream (must be issued AFTER this
        batch's own catch-up: a row in both batches is then already current and is skipped, not raced for)."""
        B = items_next.shape[0]
        L = self._occ_positions(items_next)
        cap = B * (2 * L + 1)
        sp = self._next_sparse
        if sp is None or sp.cap != cap or sp.idx.device != items_next.device:
            sp = self._next_sparse = ops.SparseRows(cap, 1, items_next.device)   # ids + count only (rows unused)
        need = ops.occ_ws_bytes(B, L)
        if self._next_ws is None or self._next_ws.numel() < need or self._next_ws.device != items_next.device:
            self._next_ws = torch.empty(need, dtype=torch.uint8, device=items_next.device)
        main = torch.cuda.current_stream()
        side = self._prefetch_stream
        if side is None or side.device != main.device:
            # lowest priority the device offers: the GEMM workgroups of the step are dispatched ahead of this stream's
            lo = int(os.environ.get("PXR_PREFETCH_PRIO", "1"))
            try:
                side = torch.cuda.Stream(device=main.device, priority=lo)
            except Exception:  # noqa: BLE001 - priority outside the runtime's range
                side = torch.cuda.Stream(device=main.device)
            self._prefetch_stream = side
        side.wait_stream(main)
        with torch.cuda.stream(side):
            self._occ_sort(items_next, sp, self._next_ws)
            # a THIN launch (PXR_PREFETCH_BLOCKS workgroups, default one per CU): the replay is pure VALU work with a
            # whole forward + backward pass of time to finish in; it must not take the CUs' wave slots from the GEMMs
            self._table_hooks.catch_up_rows(sp.idx, sp.n, sp.cap, max_blocks=int(os.environ.get("PXR_PREFETCH_BLOCKS", "256")))
        self._prefetched = sp

    def join_prefetch(self):
        """Order the current stream behind the look-ahead catch-up (the optimizer calls this before it touches rows)."""
        if self._prefetched is not None and self._prefetch_stream is not None:
            torch.cuda.current_stream().wait_stream(self._prefetch_stream)

    def _forward_train(self, items, masked_index):
        B = items.shape[0]
        L = self.max_seq_length
        D = self.hidden_size
        if self.training:
            # phase 1 of the table gradient runs first: the unique ids of the batch are what a lazy optimizer must
            # bring up to date before the forward pass reads those rows
            # a batch touches at most B*(L+1) positive + B*L negative distinct ids: that bounds the unique rows (and the
            # per-rank payload of the data-parallel row exchange), not the 3*B*L occurrences
            cap = B * (2 * L + 1)
            sp = self._local_sparse
            if sp is None or sp.cap != cap or sp.rows.shape[1] != D or sp.rows.device != items.device:
                sp = self._local_sparse = ops.SparseRows(cap, D, items.device, packed=True)
            need = ops.occ_ws_bytes(B, L)
            if self._occ_ws is None or self._occ_ws.numel() < need or self._occ_ws.device != items.device:
                self._occ_ws = torch.empty(need, dtype=torch.uint8, device=items.device)
            # big batches: the segment sums cut very long segments (a popular item's thousands of occurrences) into parts for
            # many workgroups -- two more launches, worth it from ~30 000 occurrences (PXR_SEGSUM_SPLIT=0 | 1 overrides)
            env = os.environ.get("PXR_SEGSUM_SPLIT", "auto")
            need2 = ops.occ_split_ws_bytes(B, L, D) if (env == "1" or (env != "0" and 3 * B * L >= 30000)) else 0
            if need2 == 0:
                self._occ_ws2 = None
            elif self._occ_ws2 is None or self._occ_ws2.numel() != need2 or self._occ_ws2.device != items.device:
                self._occ_ws2 = torch.zeros(need2, dtype=torch.uint8, device=items.device)
            hooks = self._table_hooks
            if (hooks is not None and getattr(hooks, "table_update", None) == "lazy" and hasattr(hooks, "catch_up_input_ids")
                    and self.split_catch_up and self._split_catch_up_ok and self._next_items is None):
                # SPLIT catch-up (round 5; graph.GraphedTrainStep turns it on): only the INPUT rows stand between the batch and
                # the first LayerNorm -- they are claimed from the raw id window items[:, 0, :L] (no sort needed).  Everything
                # else the step does with the ids before the loss head -- the catch-up of the target / negative rows (the long
                # replays: uniformly drawn negatives return after ~120 steps) and the sort + segments that only the backward's
                # segment sums read -- runs on a second stream beside the encoder and is joined in _before_head().  The side
                # stream starts AFTER the input catch-up: a row it claimed first would be read by the forward mid-replay.
                main = torch.cuda.current_stream()
                side = self._sort_stream
                if side is None or side.device != main.device:
                    side = self._sort_stream = torch.cuda.Stream(device=main.device)
                hooks.catch_up_input_ids(items)
                # the side branch is ISSUED after the encoder's first launch (_after_input_ln): in a captured graph the branch
                # created first keeps the queue of the node it forks from, and that should be the critical chain
                ev = torch.cuda.Event()
                ev.record(main)
                self._fork = (ev, hooks, items, sp)
            elif (hooks is not None and getattr(hooks, "table_update", None) == "lazy" and hasattr(hooks, "catch_up_ids")
                    and os.environ.get("PXR_SORT_OVERLAP", "0") == "1"):
                # OPT-IN schedule (PXR_SORT_OVERLAP=1).  The sorted unique list is first needed by the table-gradient segment
                # sums in backward: only the catch-up stands between the batch and the forward pass, and it can take the raw
                # id tensor (rows are claimed, duplicates drop out), so the sort / segment launches run beside it and the
                # forward pass on a second stream; _after_input_grads joins it.  Measured on MI355X (profiles/r03, step
                # timelines): the forward pass starts 16-20 us earlier, the cross-stream join in front of the segment sums
                # costs ~11 us and the catch-up runs ~5 us longer beside the sort -- 0.965 ms/step either way.  Off by default.
                main = torch.cuda.current_stream()
                side = self._sort_stream
                if side is None or side.device != main.device:
                    side = self._sort_stream = torch.cuda.Stream(device=main.device)
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    self._occ_sort(items, sp, self._occ_ws)
                self._sort_pending = True
                if not hooks.catch_up_ids(items):
                    self._join_sort()
            else:
                self._occ_sort(items, sp, self._occ_ws)
            if hooks is not None:
                if not self._sort_pending and self._fork is None:
                    hooks.catch_up_rows(sp.idx, sp.n, sp.cap)
                nxt, self._next_items = self._next_items, None
                if nxt is not None and getattr(self._table_hooks, "table_update", None) == "lazy":
                    self._start_prefetch(nxt.contiguous())
        elif self._table_hooks is not None:
            self.sync_table()
        return self._forward_core(self.item_embedding.weight.data, items, masked_index, self.training)

    def forward(self, interaction):
        """interaction = (items int64 [B,2,L+1], masked_index int64 [B,L]) -> 0-dim loss (sasrec.py:65-92)."""
        items, masked_index = interaction
        if items.dim() != 3 or items.shape[1] != 2 or items.shape[2] != self.max_seq_length + 1:
            raise ValueError(f"items must be [B, 2, {self.max_seq_length + 1}], got {tuple(items.shape)}")
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

    def _join_sort(self):
        """Order the current stream behind the id sort that runs beside the forward pass (no-op when there is none)."""
        if self._sort_pending:
            torch.cuda.current_stream().wait_stream(self._sort_stream)
            self._sort_pending = False

    def _after_input_ln(self):
        self._issue_fork()

    def _issue_fork(self):
        """Split catch-up: everything the step does with the ids before the loss head except the input rows' catch-up, on the
        side stream, ordered behind that catch-up (the event recorded right after it)."""
        fk, self._fork = self._fork, None
        if fk is None:
            return
        ev, hooks, items, sp = fk
        side = self._sort_stream
        side.wait_event(ev)
        with torch.cuda.stream(side):
            hooks.catch_up_ids(items)
            self._occ_sort(items, sp, self._occ_ws)
        self._sort_pending = True

    def _before_head(self):
        self._issue_fork()       # (an encoder without the _after_input_ln hook: issue now, no overlap)
        self._join_sort()        # split catch-up: the loss head reads the target / negative rows the side stream brought current

    # the phase-2 launch of the table gradient carries the backward's closing reductions (ops.TailRider) on its single-launch routes
    _tail_carrier = True

    def _tail_has_carrier(self):
        """Whether this step's _after_input_grads is ONE segment-sum launch (rows_apply_handle's, or the plain route without the
        split workspace of big batches): known once _forward_train has sized the workspaces.  Not in a step with collectives (a
        row exchange hooked behind the segment sums, parallel.GradSync): it keeps the launches it had."""
        return (self._tail_carrier and not getattr(self, "_sharded", False) and self._occ_ws2 is None
                and getattr(self, "_sparse_ready_hook", None) is None)

    def _after_input_grads(self, dx0, coef, s):
        sp = self._local_sparse
        self._join_sort()
        rider, self._tail_rider = self._tail_rider, None      # (the join above now also precedes these reductions)
        if rider is not None and self._occ_ws2 is not None:
            raise PxrError("a tail rider was prepared for a step whose segment sums take the split route")
        # one rank, lazy table update, every backward followed by the optimizer's step (PxrAdamW.rows_apply_handle): the rows take
        # this step's update inside the segment-sum launch.  Not with the split route of big batches (the long rows' sums are
        # finished by later launches) and not beside a look-ahead catch-up that may still be reading rows on its side stream
        hooks = self._table_hooks
        apply_rows = (hooks.rows_apply_handle() if (hasattr(hooks, "rows_apply_handle") and self._occ_ws2 is None
                                                    and self._prefetched is None) else None)
        if apply_rows is not None:
            apply_rows(self._occ_ws, dx0, s["out"], coef, self._table_rows(), sp, **({"rider": rider} if rider is not None else {}))
        else:
            sp.applied = False
            ops.sasrec_occ_segsum(self._occ_ws, dx0, s["out"], coef, self._table_rows(), sp, 1.0, ws2=self._occ_ws2, rider=rider)
        self.sparse_table_grad = sp
        hook = getattr(self, "_sparse_ready_hook", None)
        if hook is not None:
            hook()

    def _backward_train(self, gsd):
        self._backward_core(gsd, self.item_embedding.weight.data)

    # ------------------------------------------------------------------------------------------ inference
    @torch.no_grad()
    def encode_last(self, item_seq):
        """item_seq int64 [B, L] -> (states [B, L, D], view of the last position [B, D] with row stride L*D)."""
        self._ensure_packed()
        self.sync_table()
        item_seq = item_seq.contiguous()
        B, L = item_seq.shape
        if L != self.max_seq_length:
            raise ValueError(f"item_seq must have MAX_ITEM_LIST_LENGTH={self.max_seq_length} columns, got {L}")
        out, _ = self._encode(self.item_embedding.weight.data, item_seq, L, B, item_seq, L, train=False)
        return out, out[:, -1]

    @torch.no_grad()
    def predict(self, item_seq, item_feature):
        """scores [B, N] = last-position state x item_feature^T (sasrec.py:94-113)."""
        out, last = self.encode_last(item_seq)
        B, L, D = out.shape
        feat = item_feature if item_feature.is_contiguous() else item_feature.contiguous()
        N = feat.shape[0]
        scores = torch.empty(B, N, dtype=torch.float32, device=out.device)
        ops.gemm(True, True, B, N, D, last, L * D, feat, D, scores, N, ops.EPI_NONE, use_ws=False)
        ops.raise_on_bad_indices(out.device)     # an id outside the catalogue raises, like nn.Embedding (sasrec.py:101)
        return scores

    @torch.no_grad()
    def compute_item_all(self):
        self.sync_table()
        return self.item_embedding.weight
