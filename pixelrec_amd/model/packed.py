"""What every model on the flat-buffer / hand-written-backward machinery shares (DESIGN.md "The packed-parameter base"):

  * `_Rows`, the parameter container with nn.Embedding's `weight` name;
  * `TrainStep`, the one autograd bridge from `loss.backward()` to a model's `_backward_train`;
  * `flat_layout` (pure) and `pack_flat`: the layout of the flat parameter buffer and the allocate / copy / re-point loop;
  * `PackedModel`: a model that owns a flat buffer -- private state, `_ensure_packed`, `flat_parameters`, `_p`, `_buf`;
  * `TableHooks` and `LazyTableModel`: the surface a lazy table optimizer (optim.PxrAdamW) drives, and the ONE
    [1 + rows, D] table buffer built from `table_parameter_spans()`.

None of these registers a parameter, a buffer or a submodule, and none defines a member the surrounding code probes for by
attribute (`table_parameter_spans`, `rec_parameter_names`, `running_state_buffers`, `split_flat_table_groups`,
`item_table_attr`): a model has those exactly when it writes them itself.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .. import ops
from ..lib import PxrError
from .basemodel import BaseModel


class _Rows(nn.Module):
    """Parameter container with nn.Embedding's `weight` name (state_dict keys of the reference); never called."""

    def __init__(self, n, d):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(n, d))


class TrainStep(torch.autograd.Function):
    """Bridges `loss.backward()` to the hand-written backward chain: apply(anchor, model, *inputs).  The anchor is what makes
    the loss require a gradient; it receives whatever `_backward_train` returns -- None, except for the pixel model, whose
    anchor is the visual encoder's output."""

    @staticmethod
    def forward(ctx, anchor, model, *inputs):
        ctx.model, ctx.n_inputs = model, len(inputs)
        return model._forward_train(*inputs).view(())

    @staticmethod
    def backward(ctx, grad_out):
        return (ctx.model._backward_train(grad_out),) + (None,) * (1 + ctx.n_inputs)


def flat_layout(specs, align=1):
    """[(name, shape)] -> ({name: (offset, numel, shape)}, total), in elements.  Every tensor starts on a multiple of `align`:
    1 packs densely, 4 puts every start on a 16-byte boundary (the gap after a tensor whose numel is no multiple of 4 is
    padding that belongs to nobody)."""
    views, off = {}, 0
    for name, shape in specs:
        n = math.prod(shape)
        views[name] = (off, n, tuple(shape))
        off += -(-n // align) * align
    return views, off


def pack_flat(specs, dev, align=1):
    """[(name, parameter)] -> (flat, gflat, views): copies every parameter into one zero-filled fp32 buffer laid out by
    flat_layout and re-points its .data and .grad at its slices of `flat` and of the gradient twin `gflat`.  Zero-filled because
    the optimizer's flat launch runs over the padding too; never shorter than 4 elements because that launch takes real pointers
    (MF without towers has no flat parameter at all)."""
    views, total = flat_layout([(name, p.shape) for name, p in specs], align)
    flat = torch.zeros(max(4, total), dtype=torch.float32, device=dev)
    gflat = torch.zeros_like(flat)
    for name, p in specs:
        off, n, _ = views[name]
        flat[off:off + n].copy_(p.data.reshape(-1))
        p.data = flat[off:off + n].view(p.shape)
        p.grad = gflat[off:off + n].view(p.shape)
    return flat, gflat, views


class PackedModel(BaseModel):
    """A model whose trainable non-table parameters live in ONE flat fp32 buffer with a gradient twin (PxrAdamW's one launch).
    A subclass supplies `_flat_specs()` -> [(flat-buffer key, parameter)] and, where it needs them, `flat_align`,
    `_first_flat_parameter()`, `_pack_tables(dev)` and `_after_pack(dev)`."""

    flat_align = 1          # elements every tensor's start is rounded up to (flat_layout)

    def __init__(self):
        super().__init__()
        self._flat = None               # packed non-table parameters
        self._gflat = None              # packed gradients (same layout)
        self._views = {}                # flat-buffer key -> (offset, numel, shape)
        self._bufs = {}                 # persistent work buffers (_buf)
        self._anchor = None
        self._saved = None              # what the forward leaves for the backward
        self._step_counter = 0          # completed backward passes: host mirror ...
        self._drop_dev = None           # ... and device counter (dropout seed offset; graph.py keeps both)
        self.grad_scale = 1.0           # 1/world_size under data parallelism (sum-all-reduce == DDP's mean)

    def _first_flat_parameter(self):
        """The parameter at offset 0 of the flat buffer (its address tells whether the buffer is still the packed one)."""
        return self._flat_specs()[0][1]

    def _pack_probe(self):
        """(a packed parameter, the tensor whose address it has while the buffers are the packed ones | None)."""
        return self._first_flat_parameter(), self._flat

    def _pack_tables(self, dev):
        """Hook: runs before the flat buffer is packed (LazyTableModel builds its table buffer here)."""

    def _after_pack(self, dev):
        """Hook: runs after every (re)pack -- whatever else follows the parameters to their device or goes stale with them."""

    def _ensure_packed(self):
        """(Re)build the buffers when the parameters moved (e.g. after .to(device))."""
        p, at = self._pack_probe()
        if at is not None and at.device == p.device and p.data_ptr() == at.data_ptr():
            return
        dev = p.device
        if dev.type != "cuda":
            raise PxrError("pixelrec_amd models run on a HIP device only (no CPU fallback); move the model with .to('cuda') first")
        self._pack_tables(dev)
        self._flat, self._gflat, self._views = pack_flat(self._flat_specs(), dev, self.flat_align)
        self._anchor = torch.zeros((), dtype=torch.float32, device=dev, requires_grad=True)
        self._drop_dev = torch.full((1,), self._step_counter, dtype=torch.int64, device=dev)
        self._bufs = {}
        self._after_pack(dev)

    def flat_parameters(self):
        self._ensure_packed()
        return self._flat, self._gflat

    def _p(self, name, grad=False, span=1):
        """View of parameter `name` (or of `span` adjacent ones fused along dim 0) in the flat (grad) buffer."""
        off, n, shape = self._views[name]
        buf = self._gflat if grad else self._flat
        if span == 1:
            return buf[off:off + n].view(shape)
        return buf[off:off + span * n].view((span * shape[0],) + tuple(shape[1:]))

    def _buf(self, name, shape, dtype=torch.float32, zero=False):
        """Persistent work buffers (stable addresses: a captured step replays on them)."""
        b = self._bufs.get(name)
        if b is None or tuple(b.shape) != tuple(shape) or b.dtype != dtype:
            b = self._bufs[name] = (torch.zeros if zero else torch.empty)(*shape, dtype=dtype, device=self._flat.device)
        return b


class TableHooks:
    """Mixin: the surface of a model whose table a lazy optimizer updates (rows are brought up to date before they are read)."""

    sparse_table_grad = None    # the table gradient of the last backward, as sparse rows
    _table_hooks = None         # the lazy optimizer (catch_up_* / flush) when one is attached
    # False: something reads the step's gradient rows between backward() and the optimizer's step() (gradient clipping), so the
    # backward must not apply them to the table itself (PxrAdamW.rows_apply_handle)
    fuse_row_update = True

    def register_table_hooks(self, opt):
        """Attach a lazy table optimizer: it is asked to bring rows up to date before they are read."""
        self._table_hooks = opt

    def join_prefetch(self):
        return None

    def sync_table(self):
        """Make every table row current (no-op without a lazy optimizer).  Called before the table is read as a whole:
        predict / compute_item_all / state_dict."""
        if self._table_hooks is not None:
            self._table_hooks.flush()

    def state_dict(self, *args, **kwargs):
        self.sync_table()
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        # updates a lazy optimizer still owes belong to the rows being REPLACED: apply them first, so that none is left
        # to land on the loaded weights (the reference's dense AdamW has applied them by the time it loads)
        self.sync_table()
        return super().load_state_dict(state_dict, strict=strict, **kwargs)


class LazyTableModel(TableHooks, PackedModel):
    """A PackedModel whose table parameters are views of ONE [1 + rows, D] buffer that PxrAdamW updates lazily
    (optim.table_spans).  The subclass supplies `table_parameter_spans()` -> {parameter name: (first row, end row)} in the
    reference's order; row 0 is a spare nothing reads (the sparse-row kernels treat id 0 as padding / an empty slot)."""

    def __init__(self):
        super().__init__()
        self._table = None
        self._table_params = None
        self._sparse = None

    def _pack_probe(self):
        if self._table_params is None:
            self._table_params = [self.get_parameter(name) for name in self.table_parameter_spans()]
        return self._table_params[0], (None if self._table is None else self._table[1])

    def _pack_tables(self, dev):
        spans = list(self.table_parameter_spans().values())
        table = torch.zeros(spans[-1][1], self._table_params[0].shape[1], dtype=torch.float32, device=dev)
        for p, (lo, hi) in zip(self._table_params, spans):
            table[lo:hi].copy_(p.data)
            p.data = table[lo:hi]
        self._table = table

    def lazy_table(self):
        self._ensure_packed()
        return self._table

    def _sparse_rows(self, n):
        """The reusable sparse-row buffer (n slots) that the backward leaves the table gradient in."""
        sp = self._sparse
        if sp is None or sp.cap != n or sp.rows.device != self._table.device:
            sp = self._sparse = ops.SparseRows(n, self._table.shape[1], self._table.device)
        return sp
