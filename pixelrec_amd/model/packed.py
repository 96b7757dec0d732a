"""What every model on the flat-buffer / hand-written-backward machinery shares (DESIGN.md "The packed-parameter base"):

  * `_Rows`, the parameter container with nn.Embedding's `weight` name;
  * `_ActMLP`, the reference's MLPLayers parameter layout, and `linear_specs` / `linear_names` over a model's `_linears()`;
  * `TrainStep`, the one autograd bridge from `loss.backward()` to a model's `_backward_train`, and `EncoderRows`, what the pixel
    models put between the visual encoder's output and it (`store_modal_inputs` is their batcher-to-forward input form);
  * `split_tail` / `split_planes` (the two input forms of the pair models), `dense_gemm` / `dense_scores` (the predict tail), `take_saved` and the
    constructor checks `one_process`, `check_width16`, `hidden_sizes`;
  * `flat_layout` (pure) and `pack_flat`: the layout of the flat parameter buffer and the allocate / copy / re-point loop;
  * `PackedModel`: a model that owns a flat buffer -- private state, `_ensure_packed`, `flat_parameters`, `_p`, `_buf`, the
    step bracket (`_take_saved`, `_step_done`), the activation-epilogue Linear chain and the evaluation-cache hook;
  * `TableHooks` and `LazyTableModel`: the surface a lazy table optimizer (optim.PxrAdamW) drives, and the ONE
    [1 + rows, D] table buffer built from `table_parameter_spans()`.

None of these registers a parameter, a buffer or a submodule, and none defines a member the surrounding code probes for by
attribute (`table_parameter_spans`, `rec_parameter_names`, `running_state_buffers`, `split_flat_table_groups`,
`item_table_attr`, `modal_inputs`, `set_item_feature`, `scoring_item_matrix`, `extra_item_images`): a model has those exactly
when it writes them itself.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .. import ops
from ..lib import PxrError
from ..parallel import world_info
from .basemodel import BaseModel


class _Rows(nn.Module):
    """Parameter container with nn.Embedding's `weight` name (state_dict keys of the reference); never called."""

    def __init__(self, n, d):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(n, d))


class _ActMLP(nn.Module):
    """MLPLayers(sizes, dropout, activation, bn=False) with the reference's module layout (mlp_layers.{3k: Dropout, 3k + 1:
    Linear, 3k + 2: act_cls}); never called -- the kernels read its parameters."""

    def __init__(self, sizes, act_cls, dropout=0.0):
        super().__init__()
        mods = []
        for i, o in zip(sizes[:-1], sizes[1:]):
            mods += [nn.Dropout(p=dropout), nn.Linear(i, o), act_cls()]
        self.mlp_layers = nn.Sequential(*mods)


def linear_specs(linears):
    """[(flat-buffer key, reference path, Linear)] -> the `_flat_specs()` entries [(key.w, weight), (key.b, bias)]."""
    return [spec for key, _, lin in linears for spec in ((key + ".w", lin.weight), (key + ".b", lin.bias))]


def linear_names(linears):
    """[(flat-buffer key, reference path, Linear)] -> the `rec_parameter_names()` entries {path.weight: key.w, path.bias: key.b}."""
    out = {}
    for key, path, _ in linears:
        out[path + ".weight"] = key + ".w"
        out[path + ".bias"] = key + ".b"
    return out


def one_process(model, what="this model"):
    """The constructor guard of a model whose data-parallel exchange is not built."""
    if world_info()[1] > 1:
        raise NotImplementedError(f"{type(model).__name__} runs on one process: data parallelism is not built for {what}")


def check_width16(D):
    """embedding_size of a model whose kernels read rows in 16-byte vectors."""
    if D <= 0 or D % 4 or D > 4096:
        raise ValueError(f"embedding_size must be a positive multiple of 4, at most 4096 (16-byte vector accesses); got {D}")


def hidden_sizes(hidden):
    """config's `mlp_hidden_size` -> a list of ints: an int is a one-entry list, None is []."""
    if isinstance(hidden, int):
        hidden = [hidden]
    return [int(h) for h in (hidden or [])]


def _split_checked(profile, tail, n_tail, min_len, max_len, text):
    if profile.dim() != 2 or tail.dim() != 2 or tail.shape != (profile.shape[0], n_tail) or not min_len <= profile.shape[1] <= max_len:
        raise ValueError(text.format(profile=tuple(profile.shape), tail=tuple(tail.shape)))
    return profile.contiguous(), tail.contiguous()


def split_tail(input, n_tail, text, max_len=math.inf):
    """The reference's single [B, L + n_tail] id tensor, or (profile [B, L], tail [B, n_tail]) -> contiguous (profile, tail),
    1 <= L <= max_len.  `text` is the caller's own error text, with {profile} and {tail} where the two shapes go."""
    if isinstance(input, (tuple, list)):
        profile, tail = input
        tail = tail.reshape(profile.shape[0], -1)
    else:
        if input.dim() < 2:
            raise ValueError(text.format(profile=tuple(input.shape), tail=()))
        profile, tail = input[:, :-n_tail], input[:, -n_tail:]
    return _split_checked(profile, tail, n_tail, 1, max_len, text)


def split_planes(input, name, pair_text, min_len=1):
    """The reference's [B, 2, L + 1] id tensor -- plane 0 = [profile | positive], plane 1 = [profile | negative], the same profile
    in both -- or (profile [B, L], target [B, 2]) -> contiguous (profile, target), L >= min_len.  `pair_text` is the caller's own
    error text for a pair of the wrong shapes, with {profile} and {tail} where the shapes go."""
    if isinstance(input, (tuple, list)):
        profile, target = input
        target = target.reshape(profile.shape[0], -1)
    else:
        if input.dim() != 3 or input.shape[1] != 2 or input.shape[2] < 2:
            raise ValueError(f"{name}: expected [B, 2, L + 1] ids ([profile | positive], [profile | negative]), got {tuple(input.shape)}")
        if not torch.equal(input[:, 0, :-1], input[:, 1, :-1]):
            raise ValueError(f"{name}: the two planes of the [B, 2, L + 1] input must hold the same profile in their first L columns")
        profile, target = input[:, 0, :-1], input[:, :, -1]
    return _split_checked(profile, target, 2, min_len, math.inf, pair_text)


def dense_gemm(q, feat, ldq=None):
    """scores [B, N] = q feat^T in the library GEMM.  `ldq` is the row stride of q in elements (default: its width) -- the last
    position of a [B, L, D] block of states is a [B, D] view with stride L D."""
    B, D = q.shape
    N = feat.shape[0]
    scores = torch.empty(B, N, dtype=torch.float32, device=q.device)
    ops.gemm(True, True, B, N, D, q, D if ldq is None else ldq, feat, D, scores, N, ops.EPI_NONE, use_ws=False)
    return scores


def dense_scores(q, feat, ldq=None):
    """The tail of `predict`: scores [B, N] = q feat^T, then the bad-index flag -- an id outside the catalogue raises, like the
    reference's indexing."""
    scores = dense_gemm(q, feat, ldq)
    ops.raise_on_bad_indices(q.device)
    return scores


def take_saved(model, *also):
    """What the training forward left in `model._saved` for this backward (`also`: what else it must have left)."""
    if model._saved is None or any(x is None for x in also):
        raise PxrError("backward() without a training-mode forward()")
    return model._saved


class TrainStep(torch.autograd.Function):
    """Bridges `loss.backward()` to the hand-written backward chain: apply(anchor, model, *inputs).  The anchor is what makes
    the loss require a gradient; it receives whatever `_backward_train` returns -- None, except for the pixel model, whose
    anchor is the visual encoder's output.  `_backward_train` gets the upstream gradient as the [1] fp32 tensor the kernels read."""

    @staticmethod
    def forward(ctx, anchor, model, *inputs):
        ctx.model, ctx.n_inputs = model, len(inputs)
        return model._forward_train(*inputs).view(())

    @staticmethod
    def backward(ctx, grad_out):
        gsd = grad_out.reshape(1).to(torch.float32).contiguous()
        return (ctx.model._backward_train(gsd),) + (None,) * (1 + ctx.n_inputs)


def store_modal_inputs(store, data):
    """The batcher's (index, image_ids [M]) -> the forward's (index, images [M, 3, H, W]): each distinct image of the batch is
    fetched, and later encoded, once.  A pixel model takes it with `modal_inputs = staticmethod(store_modal_inputs)`."""
    return data[0], store.batch(data[1])


class EncoderRows:
    """Mixin of the models trained from pixels: what lies between the visual encoder's output E [M, D] and the native step.  The
    training branch of a model is `_encoded_step(E, E.detach().contiguous(), *inputs)`; its `_forward_train(*inputs)` reads
    `self._train_table`; its `_backward_train(gsd)` opens with `_take_table()` and returns d loss / d E, which TrainStep hands to
    autograd as the gradient of E.  Which calls take the training branch, and what the other branch does, is the model's own."""

    _train_table = None     # E, detached, between a training forward and its backward

    def _check_rows(self, E, width):
        if E.dim() != 2 or E.dtype != torch.float32 or E.shape[1] != width:
            raise ValueError(f"{type(self).__name__}: E must be float32 [M, {width}], got {tuple(E.shape)} {E.dtype}")
        if E.device.type != "cuda":
            raise PxrError("pixelrec_amd models run on a HIP device only (no CPU fallback); move the model with .to('cuda') first")

    def _encoded_step(self, E, table, *inputs):
        """-> 0-dim loss of `_forward_train(*inputs)` over `table`, with `_backward_train`'s return as the gradient of E."""
        if not E.requires_grad:      # fully frozen encoder (or a plain tensor): still drive the backward of the step
            anchor = getattr(self, "_anchor", None)
            if anchor is None or anchor.device != E.device:
                anchor = self._anchor = torch.zeros((), dtype=torch.float32, device=E.device, requires_grad=True)
            E = E + anchor * 0
        self._train_table = table
        return TrainStep.apply(E, self, *inputs)

    def _take_table(self, *also):
        """-> (what the training forward left in `_saved`, its table); a backward() without a forward() raises here."""
        saved = take_saved(self, self._train_table, *also)
        table, self._train_table = self._train_table, None
        return saved, table

    @torch.no_grad()
    def compute_item(self, item):
        return self.visual_encoder(item)


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
    `_first_flat_parameter()`, `_pack_tables(dev)`, `_after_pack(dev)` and `_drop_eval_cache()`.  Its `_forward_train` leaves
    `_saved`; its `_backward_train(gsd)` opens with `_take_saved()` and closes with `_step_done()`."""

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

    def _drop_eval_cache(self):
        """Hook: drop what evaluation derived from the parameters -- after a repack, on train(True), before load_state_dict."""

    def train(self, mode: bool = True):
        if mode:
            self._drop_eval_cache()
        return super().train(mode)

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        self._drop_eval_cache()
        return super().load_state_dict(state_dict, strict=strict, **kwargs)

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
        self._drop_eval_cache()

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

    # ---- the step bracket: the two counters are what graph.py snapshots and what seeds the dropout masks
    def _take_saved(self):
        """What the training forward left for this backward."""
        return take_saved(self)

    def _step_done(self, bumped=False):
        """Close a backward pass: the device counter advances here unless a launch of the step already carried it (`bumped`)."""
        self._saved = None
        if not bumped:
            ops.counter_add(self._drop_dev, 1)
        self._step_counter += 1

    # ---- Linears with an activation epilogue (activation and derivative in one pass), chained
    def _act_chain(self, x, keys, act):
        """x -> (activations, derivatives) of Linear `k` + `act` for k in keys, each reading the one before."""
        acts, ders = [], []
        for k in keys:
            x, d = ops.linear_fwd(x, self._p(k + ".w"), self._p(k + ".b"), act=act)
            acts.append(x)
            ders.append(d)
        return acts, ders

    def _act_chain_bwd(self, dz_last, keys, ders):
        """The gradient at the last Linear's output (before its activation) -> the same for every Linear of `keys`:
        dz[i - 1] = (dz[i] W_i) * ders[i - 1].  The first Linear's input gradient is the caller's."""
        dzs = [None] * len(keys)
        dzs[-1] = dz_last
        for i in range(len(keys) - 1, 0, -1):
            dzs[i - 1] = ops.linear_bwd_input(dzs[i], self._p(keys[i] + ".w"), mul=ders[i - 1])
        return dzs


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
