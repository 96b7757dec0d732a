"""MF (IDNet) -- drop-in for `REC.model.IDNet.mf.MF` (code/REC/model/IDNet/mf.py, MLPLayers of layers.py:239-294) on the
hand-written gfx950 kernels of csrc/mf.hip and the library's fp32-operand GEMMs.

    u_b = tower_u(user_embedding[user_b])      i_{b,t} = tower_i(item_embedding[item_{b,t}])      (t = positive, negative)
    x_b = <u_b, i+_b> - <u_b, i-_b>            loss = -mean(1e-8 + log sigmoid(x_b))

A tower is MLPLayers([D] + mlp_hidden_size, dropout_prob, 'tanh', bn=True): per layer Dropout -> Linear -> BatchNorm1d -> Tanh.
With `mlp_hidden_size: []` (the shipped config) the towers are the identity and the head reads the table rows directly.  In
training a BatchNorm normalises with its batch's statistics (the user tower's B rows, the item tower's 2B rows in item.view(-1)
order) and updates its running statistics and num_batches_tracked on the device, so a replayed step does too.

The tables: both are views of ONE [1 + U + I, D] buffer -- user u at row 1 + u, item i at row 1 + U + i, row 0 a spare nothing
reads (MF has no padding id, and the sparse-row kernels treat id 0 as padding / an empty slot).  PxrAdamW updates that buffer
lazily (optim.table_spans): the step's user, positive and negative rows are caught up before the forward reads them, the backward
leaves the table gradient as sparse rows (`sparse_table_grad`, one slot per occurrence, deterministic) and only those rows are
updated -- O(B D) per step instead of the reference's dense AdamW over every row of both tables.  Every other parameter (the
towers) lives in the flat buffer of PxrAdamW's one launch; the towers' weight gradients are one grouped launch.

Contract kept: `input_type = PAIR`; `__init__(config, dataload)` with `embedding_size`, `mlp_hidden_size`, `dropout_prob`;
forward((user [B], item [B, 2])) -> loss; `compute_item_all` (the eval-mode item tower over the item table) and `predict(user,
item_feature)`; `state_dict` keys and order of the reference (user_mlp_layers.*, item_mlp_layers.* with the BatchNorm buffers,
user_embedding.weight, item_embedding.weight; xavier-normal init), so reference checkpoints load with strict=True.
Hidden sizes must be multiples of 4 (16-byte vector accesses of the kernels and GEMMs).  One process: the data-parallel exchange
is not built for this model.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..lib import PxrError
from ..utils.enum_type import InputType
from .packed import LazyTableModel, TrainStep, _Rows, dense_scores, hidden_sizes, one_process


class _MLP(nn.Module):
    """MLPLayers(sizes, dropout, 'tanh', bn=True) with the reference's module layout (mlp_layers.{4k: Dropout, 4k+1: Linear,
    4k+2: BatchNorm1d, 4k+3: Tanh}); never called -- the kernels read its parameters and buffers."""

    def __init__(self, sizes, dropout):
        super().__init__()
        mods = []
        for i, o in zip(sizes[:-1], sizes[1:]):
            mods += [nn.Dropout(p=dropout), nn.Linear(i, o), nn.BatchNorm1d(num_features=o), nn.Tanh()]
        self.mlp_layers = nn.Sequential(*mods)

    def layers(self):
        """[(Linear, BatchNorm1d)] per layer."""
        m = list(self.mlp_layers)
        return [(m[4 * k + 1], m[4 * k + 2]) for k in range(len(m) // 4)]


class MfTowers:
    """Mixin: the two MLPLayers towers of the pair models on a lazy table (MF, and MOMF of momf.py) -- their construction and
    init, their tensors in PxrAdamW's flat buffer, the BatchNorm buffers a step advances, and the tower forward and backward on
    the kernels of csrc/mf.hip.  The host class is a PackedModel; its tables, head and step are its own."""

    def _build_towers(self, config):
        """The config's three keys, the width checks and the two `_MLP`s (registered in the reference's order: user, item)."""
        self.embedding_size = int(config["embedding_size"])
        self.mlp_hidden_size = hidden_sizes(config["mlp_hidden_size"])
        self.dropout_prob = float(config["dropout_prob"] or 0.0)
        D = self.embedding_size
        if D % 4 or D > 4096:
            raise ValueError("embedding_size must be a multiple of 4 and at most 4096 (16-byte vector accesses)")
        if any(h % 4 or h <= 0 or h > 4096 for h in self.mlp_hidden_size):
            raise ValueError("every mlp_hidden_size entry must be a positive multiple of 4, at most 4096 (16-byte vector accesses)")
        self.out_size = self.mlp_hidden_size[-1] if self.mlp_hidden_size else D
        sizes = [D] + self.mlp_hidden_size
        self.user_mlp_layers = _MLP(sizes, self.dropout_prob)
        self.item_mlp_layers = _MLP(sizes, self.dropout_prob)
        s = config["seed"] if "seed" in config else None
        self._drop_seed = int(s) if s is not None else 2020

    def _init_linears(self):
        """_init_weights on the Linears, in module order (xavier-normal weights, zero biases)."""
        for mod in self.modules():
            if isinstance(mod, nn.Linear):
                nn.init.xavier_normal_(mod.weight.data)
                nn.init.constant_(mod.bias.data, 0)

    def _check_tower_batch(self, B):
        """BatchNorm1d's own refusal of a one-row training batch."""
        if self.mlp_hidden_size and B == 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size torch.Size([1, %d])"
                             % self.mlp_hidden_size[0])

    # ------------------------------------------------------------------------------------------ packing
    def _flat_specs(self):
        """Flat layout (tower parameters, the reference's parameter order): per tower, per layer Linear w, b, BatchNorm w, b."""
        out = []
        for tag, mlp in (("u", self.user_mlp_layers), ("i", self.item_mlp_layers)):
            for k, (lin, bn) in enumerate(mlp.layers()):
                out += [(f"{tag}{k}.w", lin.weight), (f"{tag}{k}.b", lin.bias), (f"{tag}{k}.g", bn.weight), (f"{tag}{k}.beta", bn.bias)]
        return out

    def _tower_parameter_names(self):
        """{reference parameter name: flat-buffer key} of the tower tensors in the reference's registration order."""
        out = {}
        for tag, pre in (("u", "user_mlp_layers.mlp_layers."), ("i", "item_mlp_layers.mlp_layers.")):
            for k in range(len(self.mlp_hidden_size)):
                out[f"{pre}{4 * k + 1}.weight"] = f"{tag}{k}.w"
                out[f"{pre}{4 * k + 1}.bias"] = f"{tag}{k}.b"
                out[f"{pre}{4 * k + 2}.weight"] = f"{tag}{k}.g"
                out[f"{pre}{4 * k + 2}.bias"] = f"{tag}{k}.beta"
        return out

    def running_state_buffers(self):
        """The BatchNorm buffers a training step advances on the device (GraphedTrainStep's dry run restores them)."""
        return [b for mlp in (self.user_mlp_layers, self.item_mlp_layers) for _, bn in mlp.layers()
                for b in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]

    # ------------------------------------------------------------------------------------------ towers
    def _tower_fwd(self, tag, mlp, x, train, sid0):
        """x [R, D] -> (out [R, H], saved per layer (input, z, y, mean, rstd)) -- Dropout -> Linear -> BN -> Tanh per layer."""
        saved = []
        p = self.dropout_prob
        for k, (_, bn) in enumerate(mlp.layers()):
            xin = ops.dropout(x, p, self._drop_seed, sid0 + k, step_dev=self._drop_dev) if (train and p > 0) else x
            z = ops.linear_fwd(xin, self._p(f"{tag}{k}.w"), self._p(f"{tag}{k}.b"))
            g, b = self._p(f"{tag}{k}.g"), self._p(f"{tag}{k}.beta")
            if train:
                y, mean, rstd = ops.mf_bn_tanh_fwd(z, g, b, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                                   eps=bn.eps, momentum=bn.momentum)
                saved.append((xin, z, y, mean, rstd))
            else:
                y = ops.mf_bn_tanh_eval(z, g, b, bn.running_mean, bn.running_var, eps=bn.eps)
            x = y
        return x, saved

    def _tower_bwd(self, tag, dy, saved, sid0, dx_out, problems, bias_grad=True):
        """Backward of _tower_fwd from dy [R, H]: the input gradient goes to dx_out [R, D]; the weight gradients are appended to
        `problems` (one grouped launch for both towers).  bias_grad=False leaves the Linear biases' gradient at the exact zero it
        is in exact arithmetic -- the batch mean of the BatchNorm behind every Linear removes the bias -- instead of the column sums'
        rounding noise (MF keeps the sums: its trajectories are pinned bit for bit)."""
        p = self.dropout_prob
        for k in reversed(range(len(saved))):
            xin, z, y, mean, rstd = saved[k]
            dz = ops.mf_bn_tanh_bwd(dy, z, y, mean, rstd, self._p(f"{tag}{k}.g"), self._p(f"{tag}{k}.g", grad=True),
                                    self._p(f"{tag}{k}.beta", grad=True))
            problems.append((dz, xin, self._p(f"{tag}{k}.w", grad=True), self._p(f"{tag}{k}.b", grad=True) if bias_grad else None))
            W = self._p(f"{tag}{k}.w")
            if k == 0 and p == 0:
                ops.linear_bwd_input(dz, W, out=dx_out)
                return
            dx = ops.linear_bwd_input(dz, W)
            if p > 0:
                dx = ops.dropout(dx, p, self._drop_seed, sid0 + k, step_dev=self._drop_dev)     # the mask's backward is itself
            if k == 0:
                dx_out.copy_(dx)
                return
            dy = dx


class MF(MfTowers, LazyTableModel):
    input_type = InputType.PAIR

    def __init__(self, config, dataload):
        super().__init__()
        one_process(self)
        self.user_num = dataload.user_num
        self.item_num = dataload.item_num
        self._build_towers(config)
        D = self.embedding_size
        self.user_embedding = _Rows(self.user_num, D)
        self.item_embedding = _Rows(self.item_num, D)
        self._init_linears()                                # mf.py _init_weights, in module order
        nn.init.xavier_normal_(self.user_embedding.weight)
        nn.init.xavier_normal_(self.item_embedding.weight)
        self.store_ifeatures = None

    # ------------------------------------------------------------------------------------------ packing
    def rec_parameter_names(self):
        """{reference parameter name: flat-buffer key} in the reference's registration order (optim.native_to_torch_state); the
        tables map to None -- their state is the table's (optim.table_spans)."""
        out = self._tower_parameter_names()
        out["user_embedding.weight"] = None
        out["item_embedding.weight"] = None
        return out

    def table_parameter_spans(self):
        """Rows of the table buffer each table parameter occupies (optim.table_spans), in the reference's order."""
        U = self.user_num
        return {"user_embedding.weight": (1, 1 + U), "item_embedding.weight": (1 + U, 1 + U + self.item_num)}

    # ------------------------------------------------------------------------------------------ training
    def forward(self, input):
        user, item = input
        if not self.training:
            raise PxrError("MF.forward is the training loss (mf.py forward); use compute_item_all / predict to score")
        self._ensure_packed()
        user, item = user.reshape(-1).contiguous(), item.contiguous()
        self._check_tower_batch(user.numel())
        return TrainStep.apply(self._anchor, self, user, item)

    def _forward_train(self, user, item):
        B, D = user.numel(), self.embedding_size
        rows = ops.mf_pair_rows(user, item, self.user_num, self.item_num, out=self._buf("rows", (3 * B,), torch.int64))
        if self._table_hooks is not None:
            self._table_hooks.catch_up_ids(rows)          # the step's rows, current through the last step before anything reads them
        head = self._buf("head", (2 * B + 1,))
        if not self.mlp_hidden_size:
            loss, coef = ops.mf_pair_fwd(self._table, self._table, B, rows=rows, out=head)
            self._saved = dict(B=B, rows=rows, coef=coef)
            return loss
        x = ops.embed_gather(self._table, rows)                                  # [3B, D]: users | items in item.view(-1) order
        hu, su = self._tower_fwd("u", self.user_mlp_layers, x[:B], True, 0)
        hi, si = self._tower_fwd("i", self.item_mlp_layers, x[B:], True, 64)
        loss, coef = ops.mf_pair_fwd(hu, hi, B, out=head)
        self._saved = dict(B=B, rows=rows, coef=coef, hu=hu, hi=hi, su=su, si=si)
        return loss

    def _backward_train(self, gsd):
        s = self._take_saved()
        B = s["B"]
        sp = self._sparse_rows(3 * B)
        if not self.mlp_hidden_size:
            ops.mf_table_grad(s["rows"], B, sp, table=self._table, coef=s["coef"], grad_scale=self.grad_scale, grad_scale_dev=gsd)
        else:
            H = self.out_size
            du, di = self._buf("du", (B, H)), self._buf("di", (2 * B, H))
            ops.mf_pair_bwd(s["hu"], s["hi"], s["coef"], du, di, self.grad_scale, gsd)
            occ = self._buf("occ", (3 * B, self.embedding_size))
            problems = []
            self._tower_bwd("u", du, s["su"], 0, occ[:B], problems)
            self._tower_bwd("i", di, s["si"], 64, occ[B:], problems)
            ops.grouped_linear_bwd_weight(problems)
            ops.mf_table_grad(s["rows"], B, sp, occ=occ)
        self.sparse_table_grad = sp
        self._step_done()

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def compute_item_all(self):
        """The eval-mode item tower over the (flushed) item table [I, out_size] (mf.py compute_item_all)."""
        self._ensure_packed()
        self.sync_table()
        items = self._table[1 + self.user_num:]
        if self.mlp_hidden_size:
            items, _ = self._tower_fwd("i", self.item_mlp_layers, items, False, 0)
        self.store_ifeatures = items
        return items

    @torch.no_grad()
    def encode_last(self, user, item_feature=None):
        """user int64 [B] -> (u [B, 1, H], u [B, H]): the eval-mode user tower's output, the query vectors of the fused scoring."""
        self._ensure_packed()
        self.sync_table()
        user = user.reshape(-1).contiguous()
        rows = ops.mf_pair_rows(user, None, self.user_num, self.item_num)
        u = ops.embed_gather(self._table, rows)
        if self.mlp_hidden_size:
            u, _ = self._tower_fwd("u", self.user_mlp_layers, u, False, 0)
        return u.view(u.shape[0], 1, -1), u

    @torch.no_grad()
    def predict(self, user, item_feature):
        """scores [B, I] = u item_feature^T (mf.py predict)."""
        feat = item_feature if item_feature is not None else self.store_ifeatures
        if feat is None:
            raise PxrError("MF: call compute_item_all() before scoring")
        feat = feat if feat.is_contiguous() else feat.contiguous()
        _, u = self.encode_last(user, feat)
        return dense_scores(u, feat)
