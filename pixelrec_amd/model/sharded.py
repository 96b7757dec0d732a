"""Row-sharded item-embedding table for SASRec -- north_star "embedding table optionally row-sharded with an all-gather
of hit rows", BASELINE.json configs[3] (emb 4096).  The reference has no such mode (it replicates the table under DDP,
code/run.py:40); this is the build's design for catalogues whose table + moments outgrow one GPU (DESIGN.md §6 argues
it is NOT needed for configs[3] on 288 GB parts; it exists for completeness and is exactly equivalent to the replicated
data-parallel step -- tested bit for bit).

Layout: owner(id) = id % W; the owner keeps row id at local row id // W + 1 of a [ceil(N/W) + 1, D] shard whose row 0 is
an all-zero dummy ("index 0 = not mine / contributes zeros").  AdamW moments and the lazy `last[]` exist for the local
rows only (PxrAdamW sizes itself from `item_embedding.weight`).  Per training step and rank:

  1. occurrence sort of the batch -> this rank's ascending unique ids U_r (padded to a fixed capacity);
  2. the hit rows are fetched from their owners by an ALL-TO-ALL pair (`row_exchange = "alltoall"`, default): U_r is split
     by owner into W request lists of `pair_cap` slots (`pxr_shard_bucket_ids_i64`), all-to-all of the requests, every rank
     brings the requested rows it owns up to date (lazy AdamW catch-up) and gathers them, all-to-all of the rows back,
     `pxr_scatter_rows_f32` puts them at their place in the compact block.  Per rank and step ~ |U_r| rows cross the fabric
     (pair_cap = |U_r| / W x slack per pair), against W x cap rows for
  3. the older `row_exchange = "reduce_scatter"`: all-gather of the W full id lists, every rank serves a [W, cap, D] block that
     is zero wherever it is not the owner, reduce-scatter(SUM) -- exactly one non-zero contribution per slot, so the sum is
     exact.  Kept as the fallback without a capacity bound.  A batch whose hits pile up on one owner beyond pair_cap is caught
     INSIDE the step (`shard_overflow_check = "step"`, default): every rank's largest bucket count rides in one extra slot of
     the request all-to-all, so after it all ranks hold the same W figures; one host read of them (the step's only host
     synchronisation -- this mode issues its collectives eagerly anyway) and, if any exceeds pair_cap, ALL ranks serve that
     batch through the reduce-scatter exchange instead (`overflow_fallbacks` counts them) -- no zero embedding is ever served.
     `shard_overflow_check = "epoch"` keeps the sync-free behaviour of earlier rounds for loops that cannot afford the read:
     the surplus rows are served as ZERO embeddings, PXR_STATUS_SHARD_OVERFLOW is set and `ops.raise_on_bad_indices` /
     `check_overflow()` raises at the caller's next host check (the Trainer's is once per epoch).
     Either way the forward / backward kernels then run on the [cap + 1, D] block with the batch re-indexed onto it
     (`pxr_ids_to_compact_i64`): same kernels, same arithmetic as the replicated model;
  4. the sparse gradient (global ids, rows) is exchanged and merged exactly as in the replicated mode
     (pixelrec_amd.parallel.GradSync); each rank then keeps only the rows it owns (`pxr_shard_local_rows_i64`) and its
     AdamW touches its shard only.
Evaluation / checkpoints all-gather the shards into a full [N, D] table (cached until the next training step), so
`state_dict()` keys and shapes stay the reference's.
"""
from __future__ import annotations

import torch
import torch.distributed as dist
import torch.nn as nn

from .. import ops
from ..parallel import PAD_ID, DataParallel, GradSync, world_info
from .sasrec import SASRec


class ShardedSASRec(SASRec):
    def __init__(self, config, dataload):
        super().__init__(config, dataload)
        self._shard_rank, self._shard_world = 0, 1
        self._sharded = False
        self._full_cache = None
        self._group = None
        self._force_collectives = False     # tests: run the collectives even in a world of one (1-rank RCCL group)
        cfg = lambda key, default: config[key] if (key in config and config[key] is not None) else default
        self.row_exchange = str(cfg("shard_row_exchange", "alltoall"))       # YAML keys of this build (no reference analogue)
        self.pair_slack = float(cfg("shard_pair_slack", 1.5))
        self.overflow_check = str(cfg("shard_overflow_check", "step"))
        self.overflow_fallbacks = 0          # batches served through the reduce-scatter exchange because a pair list overflowed
        if self.overflow_check not in ("step", "epoch"):
            raise ValueError(f"shard_overflow_check must be 'step' or 'epoch', got {self.overflow_check!r}")
        if self.row_exchange not in ("alltoall", "reduce_scatter"):
            raise ValueError(f"shard_row_exchange must be 'alltoall' or 'reduce_scatter', got {self.row_exchange!r}")

    # ------------------------------------------------------------------------------------------ (re)sharding
    def shard(self, rank: int | None = None, world: int | None = None, group=None):
        """Replace the full [N, D] table (identical on every rank at this point) by this rank's shard."""
        r, w = world_info()
        rank = r if rank is None else rank
        world = w if world is None else world
        full = self.item_embedding.weight.data
        assert not self._sharded and full.shape[0] == self.item_num
        self._install_shard(full, rank, world)
        self._group = group
        return self

    def _install_shard(self, full, rank, world):
        self._shard_rank, self._shard_world, self._sharded = rank, world, True
        local = self.scatter_rows(full)
        emb = nn.Embedding(local.shape[0], full.shape[1], padding_idx=0, device=full.device)
        emb.weight.data = local
        self.item_embedding = emb
        self._full_cache = None

    def gather_rows(self, local: torch.Tensor) -> torch.Tensor:
        """[n_local + 1, D] per-rank rows (table, AdamW moments, ...) -> the full [N, D] tensor on every rank.
        Collective: every rank must call it."""
        W, N, D = self._shard_world, self.item_num, local.shape[1]
        rows_max = (N + W - 1) // W + 1
        mine = torch.zeros(rows_max, D, dtype=local.dtype, device=local.device)
        mine[:local.shape[0]] = local
        if W > 1 or self._force_collectives:
            parts = [torch.empty_like(mine) for _ in range(W)]
            dist.all_gather(parts, mine, group=self._group)
        else:
            parts = [mine]
        full = torch.empty(N, D, dtype=local.dtype, device=local.device)
        for r in range(W):
            cnt = (N - r + W - 1) // W
            full[r::W] = parts[r][1:1 + cnt]
        return full

    def scatter_rows(self, full: torch.Tensor) -> torch.Tensor:
        """The inverse of gather_rows for this rank: [N, D] -> [n_local + 1, D] (row 0 = the all-zero dummy)."""
        mine = full[self._shard_rank::self._shard_world]
        local = torch.zeros(mine.shape[0] + 1, full.shape[1], dtype=full.dtype, device=full.device)
        local[1:] = mine
        return local

    def _full_table(self):
        """All shards -> [N, D] (every rank gets the whole table; cached until the next training forward)."""
        if not self._sharded:
            return self.item_embedding.weight.data
        if self._full_cache is None:
            self.sync_table()
            self._full_cache = self.gather_rows(self.item_embedding.weight.data)
        return self._full_cache

    # ------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self, *args, **kwargs):
        sd = super().state_dict(*args, **kwargs)
        if self._sharded:
            key = [k for k in sd if k.endswith("item_embedding.weight")][0]
            sd[key] = self._full_table()
        return sd

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        self.sync_table()       # owed lazy updates land on the shard being replaced, not on the loaded one
        if self._sharded and "item_embedding.weight" in state_dict and state_dict["item_embedding.weight"].shape[0] == self.item_num:
            full = state_dict["item_embedding.weight"].to(self.item_embedding.weight.device)
            state_dict = dict(state_dict)
            self._install_shard(full, self._shard_rank, self._shard_world)
            state_dict["item_embedding.weight"] = self.item_embedding.weight.data
        return super().load_state_dict(state_dict, strict=strict, **kwargs)

    # ------------------------------------------------------------------------------------------ training step
    def _forward_train(self, items, masked_index):
        if not self._sharded:
            return super()._forward_train(items, masked_index)
        if not self.training:
            return self._forward_core(self._full_table(), items, masked_index, False)
        self._full_cache = None
        B, L, D = items.shape[0], self.max_seq_length, self.hidden_size
        W, rank = self._shard_world, self._shard_rank
        cap = B * (2 * L + 1)
        sp = self._local_sparse
        if sp is None or sp.cap != cap or sp.rows.shape[1] != D or sp.rows.device != items.device:
            sp = self._local_sparse = ops.SparseRows(cap, D, items.device, packed=True)
        need = ops.occ_ws_bytes(B, L)
        if self._occ_ws is None or self._occ_ws.numel() < need or self._occ_ws.device != items.device:
            self._occ_ws = torch.empty(need, dtype=torch.uint8, device=items.device)
        ops.occ_sort(items, L, None, self.item_num, sp, self._occ_ws)                     # 1. U_r
        if self.row_exchange == "alltoall":
            block = self._fetch_rows_alltoall(sp, cap, D)
        else:
            block = self._fetch_rows_reduce_scatter(sp, cap, D)
        items_c = ops.ids_to_compact(items, sp.idx, sp.n)
        self._block = block
        return self._forward_core(block, items_c, masked_index, True)

    def pair_cap(self, cap: int) -> int:
        """Slots of one (requester, owner) pair: the expected cap / W hits of a pair x pair_slack + 64, never more than cap."""
        W = self._shard_world
        if W == 1:
            return cap
        return min(cap, (int(cap / W * self.pair_slack) + 64 + 63) // 64 * 64)

    def check_overflow(self):
        """Host check (synchronises) of the status word: raises if a pair of the all-to-all row exchange overflowed since the last
        check.  The Trainer's once-per-epoch `ops.raise_on_bad_indices` is the same check; call this where a custom loop syncs."""
        ops.raise_on_bad_indices(self.item_embedding.weight.device)

    def _all_to_all(self, send: torch.Tensor) -> torch.Tensor:
        """send[o] goes to rank o; returns recv with recv[q] = what rank q sent here.  send: [W, ...] contiguous."""
        W, rank = self._shard_world, self._shard_rank
        if not (W > 1 or self._force_collectives):
            return send
        if dist.get_backend(self._group) == "nccl":
            recv = torch.empty_like(send)
            dist.all_to_all_single(recv, send, group=self._group)
            return recv
        parts = [torch.empty_like(send) for _ in range(W)]      # gloo (tests): all-gather everything, keep what is addressed here
        dist.all_gather(parts, send, group=self._group)
        return torch.stack([p[rank] for p in parts])

    def _fetch_rows_alltoall(self, sp, cap, D):
        """Step 2 of the module docstring: [cap + 1, D] block with row 1 + j = the table row of U_r[j]."""
        W, rank, dev = self._shard_world, self._shard_rank, sp.idx.device
        pp = self.pair_cap(cap)
        req, pos, counts = ops.shard_bucket_ids(sp.idx, sp.n, W, self.item_num, pp, PAD_ID)
        if getattr(self, "overflow_check", "step") == "step" and pp < cap:
            # this rank's largest bucket travels with every request list (slot pp): after the all-to-all all ranks hold the same
            # W figures and take the same branch -- an overflowing batch goes through the unbounded exchange instead
            worst = counts.max().to(torch.int64).reshape(1, 1).expand(W, 1)
            got_x = self._all_to_all(torch.cat([req, worst], dim=1))
            if int(got_x[:, pp].max().item()) > pp:                                       # host read (the step's only one)
                ops.clear_status_bits(dev, ops.STATUS_SHARD_OVERFLOW)                     # handled here, nothing was served
                self.overflow_fallbacks = getattr(self, "overflow_fallbacks", 0) + 1
                return self._fetch_rows_reduce_scatter(sp, cap, D)
            got = got_x[:, :pp].contiguous()
        else:
            got = self._all_to_all(req)                                                   # [W, pp]: what each rank wants from me
        flat = got.view(-1)
        loc = ops.shard_local_rows(flat, W, rank, self.item_num)
        if self._table_hooks is not None:                                                 # owned rows up to date
            # an id requested by several ranks must be replayed by ONE wave: work list = first request only
            first = ops.shard_first_rows(flat, W, rank, self.item_num) if W > 1 else loc
            n_all = torch.full((1,), W * pp, dtype=torch.int32, device=dev)
            self._table_hooks.catch_up_rows(first, n_all, W * pp)
        serve = ops.embed_gather(self.item_embedding.weight.data, loc).view(W, pp, D)     # zero rows where padded
        recv = self._all_to_all(serve)                                                    # [W, pp, D]: my rows, by owner
        block = torch.zeros(cap + 1, D, dtype=torch.float32, device=dev)
        ops.scatter_rows(recv.view(W * pp, D), pos.view(-1), block, row_offset=1)
        return block

    def _fetch_rows_reduce_scatter(self, sp, cap, D):
        """Step 3 of the module docstring (no capacity bound; W x the traffic)."""
        W, rank, dev = self._shard_world, self._shard_rank, sp.idx.device
        ar = torch.arange(cap, device=dev, dtype=torch.int32)
        ids_mine = torch.where(ar < sp.n, sp.idx, PAD_ID)
        comm = W > 1 or self._force_collectives
        if comm:                                                                          # 2. who needs what
            ids_all = torch.empty(W * cap, dtype=torch.int64, device=dev)
            if dist.get_backend(self._group) == "nccl":
                dist.all_gather_into_tensor(ids_all, ids_mine, group=self._group)
            else:   # gloo (tests)
                dist.all_gather(list(ids_all.chunk(W)), ids_mine, group=self._group)
        else:
            ids_all = ids_mine
        loc = ops.shard_local_rows(ids_all, W, rank, self.item_num)
        if self._table_hooks is not None:                                                 #    owned rows up to date
            # an id requested by several ranks must be replayed by ONE wave: work list = first request only
            first = ops.shard_first_rows(ids_all, W, rank, self.item_num) if W > 1 else loc
            n_all = torch.full((1,), W * cap, dtype=torch.int32, device=dev)
            self._table_hooks.catch_up_rows(first, n_all, W * cap)
        serve = ops.embed_gather(self.item_embedding.weight.data, loc)                    #    zeros where not the owner
        if comm:                                                                          # 3. rows of U_r arrive
            if dist.get_backend(self._group) == "nccl":
                mine = torch.empty(cap, D, dtype=torch.float32, device=dev)
                dist.reduce_scatter_tensor(mine, serve, op=dist.ReduceOp.SUM, group=self._group)
            else:   # gloo (tests): no reduce-scatter -> all-reduce and keep this rank's slice
                dist.all_reduce(serve, op=dist.ReduceOp.SUM, group=self._group)
                mine = serve.view(W, cap, D)[rank]
        else:
            mine = serve
        block = torch.zeros(cap + 1, D, dtype=torch.float32, device=dev)
        block[1:] = mine
        return block

    def _backward_train(self, gsd):
        if not self._sharded:
            return super()._backward_train(gsd)
        self._backward_core(gsd, self._block)
        self._block = None

    # ------------------------------------------------------------------------------------------ inference
    @torch.no_grad()
    def encode_last(self, item_seq):
        if not self._sharded:
            return super().encode_last(item_seq)
        self._ensure_packed()
        item_seq = item_seq.contiguous()
        B, L = item_seq.shape
        out, _ = self._encode(self._full_table(), item_seq, L, B, item_seq, L, train=False)
        return out, out[:, -1]

    @torch.no_grad()
    def compute_item_all(self):
        return self._full_table() if self._sharded else super().compute_item_all()


class ShardedGradSync(GradSync):
    """GradSync + ownership filter: after the (unchanged) exchange and merge, the merged list keeps only the rows
    this rank owns, re-indexed to its shard, so the optimizer applies them to the local table."""

    def __init__(self, model, group=None):
        super().__init__(model, group=group, force=True if (dist.is_available() and dist.is_initialized()) else False)
        self._local_view = None

    def sync(self, defer_flat: bool = False):
        m = self.model
        if self.active:
            super().sync(defer_flat=defer_flat)
        sp = m.sparse_table_grad
        loc = ops.shard_local_rows(sp.idx, m._shard_world, m._shard_rank, m.item_num)
        view = self._local_view
        if view is None or view.cap != sp.cap:
            view = self._local_view = ops.SparseRows.__new__(ops.SparseRows)
            view.cap = sp.cap
        view.idx, view.rows, view.n = loc, sp.rows, sp.n
        # the merged GLOBAL ids: what is "live" in the dense gradient the reference clips (clip_grad_norm_ must see the
        # same rows on every rank, not only the owned ones)
        view.gidx = sp.idx
        if not self.active:                   # single rank: slots beyond n hold stale ids -> make them skip
            ar = torch.arange(sp.cap, device=loc.device, dtype=torch.int32)
            view.idx = torch.where(ar < sp.n, loc, 0)
        m.sparse_table_grad = view


class ShardedDataParallel(DataParallel):
    """DataParallel for a ShardedSASRec: broadcast the replicated initial state, THEN cut the table into shards."""

    def __init__(self, module: ShardedSASRec, group=None, force_collectives: bool = False):
        torch.nn.Module.__init__(self)
        self.module = module
        module._force_collectives = bool(force_collectives) and dist.is_available() and dist.is_initialized()
        boot = GradSync(module, group=group)
        boot.broadcast_parameters(0)
        module._sparse_ready_hook = None
        rank, world = world_info()
        module.shard(rank, world, group)
        self.grad_sync = ShardedGradSync(module, group=group)


def optimizer_state_full(opt, model: ShardedSASRec) -> dict:
    """PxrAdamW.state_dict() with the per-rank table moments gathered to the reference-shaped [N, D] (collective)."""
    sd = dict(opt.state_dict())
    for k in ("table_m", "table_v"):
        if k in sd:
            sd[k] = model.gather_rows(sd[k])
    return sd


def load_optimizer_state_full(opt, model: ShardedSASRec, sd: dict):
    """Inverse of optimizer_state_full: keeps this rank's rows of the full moments."""
    from ..optim import is_torch_adamw_state, torch_to_native_state

    if is_torch_adamw_state(sd):          # a reference-layout checkpoint: per-parameter state -> flat buffers first
        sd = torch_to_native_state(sd, model)
    sd = dict(sd)
    dev = model.item_embedding.weight.device
    for k in ("table_m", "table_v"):
        if k in sd and sd[k].shape[0] == model.item_num:
            sd[k] = model.scatter_rows(sd[k].to(dev))
    opt.load_state_dict(sd)
