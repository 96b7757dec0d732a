"""LightGCN (IDNet) -- drop-in for `REC.model.IDNet.lightgcn.LightGCN` (code/REC/model/IDNet/lightgcn.py, layers.py:13-22) on
the hand-written gfx950 kernels of csrc/lightgcn.hip.

    E_0 = [user_embedding; item_embedding]        E_{k+1} = A E_k        E_final = mean(E_0 .. E_K)
    x_b = <u_b, i+_b> - <u_b, i-_b>               loss = -mean(1e-8 + log sigmoid(x_b))

with A the symmetric normalised user-item graph of the training interactions (dataload.norm_adj_csr).  Propagation: K CSR SpMM
launches whose epilogue accumulates the layer mean (the last one writes E_final; K = 1 is one launch for (E_0 + A E_0) / 2).
Backward: A is symmetric and the propagation linear, so d E_0 = (1/(K+1)) sum_k A^k G_final, by Horner's rule in K more SpMM
launches of the same kernel; nothing of the forward is saved but E_final.  The pair head writes G_final's touched rows in a fixed
order.  Every launch is deterministic and the batch stays on the device: the whole step is one hipGraph chain (graph.py).

Contract kept: `input_type = PAIR`; `__init__(config, dataload)` with `embedding_size`, `n_layers`; forward((user [B], item [B, 2]))
-> loss; `compute_item_all` (runs the propagation once, keeps the user part) and `predict(user, item_feature)`; `state_dict` keys
`user_embedding.weight`, `item_embedding.weight` (xavier-normal init), so reference checkpoints load with strict=True.  Both are
views of ONE contiguous [U + I, D] buffer -- the propagation's E_0 and the flat buffer of PxrAdamW, which updates every row every
step (the reference's dense torch.optim.AdamW).  One process: the data-parallel exchange is not built for this model.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..lib import PxrError
from ..utils.enum_type import InputType
from .packed import PackedModel, TrainStep, _Rows, dense_scores, one_process


class LightGCN(PackedModel):
    input_type = InputType.PAIR

    def __init__(self, config, dataload):
        super().__init__()
        one_process(self, "the graph models")
        self.latent_dim = config["embedding_size"]
        self.n_layers = int(config["n_layers"])
        if self.latent_dim % 4:
            raise ValueError("embedding_size must be a multiple of 4 (16-byte vector accesses)")
        if self.n_layers < 1:
            raise ValueError("n_layers must be >= 1")
        self.user_num = dataload.user_num
        self.item_num = dataload.item_num
        self._csr = dataload.get_norm_adj_csr()           # host CSR, moved to the device with the parameters
        self.user_embedding = _Rows(self.user_num, self.latent_dim)
        self.item_embedding = _Rows(self.item_num, self.latent_dim)
        nn.init.xavier_normal_(self.user_embedding.weight)
        nn.init.xavier_normal_(self.item_embedding.weight)
        self._graph = None
        self.store_ufeatures = self.store_ifeatures = None

    # ------------------------------------------------------------------------------------------ flat packing
    def rec_parameter_names(self):
        """{reference parameter name: flat-buffer key} in the reference's registration order (optim.native_to_torch_state)."""
        return {"user_embedding.weight": "user", "item_embedding.weight": "item"}

    def _flat_specs(self):
        """Flat layout: users, then items -- the buffer IS the propagation's E_0 [U + I, D]."""
        return [("user", self.user_embedding.weight), ("item", self.item_embedding.weight)]

    def _after_pack(self, dev):
        if self._graph is None or self._graph.device != dev:
            self._graph = ops.LgcnGraph(*self._csr, device=dev)

    def _table(self, flat):
        return flat.view(self.user_num + self.item_num, self.latent_dim)

    def _work(self, name):
        """Persistent [U + I, D] work buffers."""
        return self._buf(name, (self.user_num + self.item_num, self.latent_dim))

    # ------------------------------------------------------------------------------------------ propagation
    def propagate(self, e0, out):
        """out = mean(E_0 .. E_K), E_{k+1} = A E_k (layers.py:13-22, lightgcn.py:55-68): K launches, the running sum in `out`."""
        K, g = self.n_layers, self._graph
        x = e0
        for k in range(1, K + 1):
            last = k == K
            y = None if last else self._work("t%d" % (k % 2))
            g.spmm(x, y=y, acc_in=e0 if k == 1 else out, acc_out=out, scale=1.0 / (K + 1) if last else 1.0)
            x = y
        return out

    def propagate_grad(self, gfin, out):
        """out = (1/(K+1)) sum_k A^k gfin by Horner's rule: H <- gfin + A H, K times (A symmetric: the same SpMM)."""
        K, g = self.n_layers, self._graph
        h = gfin
        for k in range(1, K + 1):
            last = k == K
            dst = out if last else self._work("h%d" % (k % 2))
            g.spmm(h, acc_in=gfin, acc_out=dst, scale=1.0 / (K + 1) if last else 1.0)
            h = dst
        return out

    def computer(self):
        """(E_final users [U, D], E_final items [I, D]) -- lightgcn.py:55-68."""
        self._ensure_packed()
        ef = torch.empty(self.user_num + self.item_num, self.latent_dim, dtype=torch.float32, device=self._flat.device)
        self.propagate(self._table(self._flat), ef)
        return ef[:self.user_num], ef[self.user_num:]

    # ------------------------------------------------------------------------------------------ training
    def forward(self, input):
        user, item = input
        if not self.training:
            raise PxrError("LightGCN.forward is the training loss (lightgcn.py:70-78); use compute_item_all / predict to score")
        self._ensure_packed()
        return TrainStep.apply(self._anchor, self, user.contiguous(), item.contiguous())

    def _forward_train(self, user, item):
        ef = self._work("ef")
        self.propagate(self._table(self._flat), ef)
        loss, diff, coef, nodes = ops.lgcn_pair_fwd(ef, self.user_num, self.item_num, user, item)
        self._saved = (ef, coef, nodes)
        return loss

    def _backward_train(self, gsd):
        ef, coef, nodes = self._take_saved()
        gfin = ops.lgcn_pair_bwd(ef, nodes, coef, self._work("gf"), self.grad_scale, gsd)
        self.propagate_grad(gfin, self._table(self._gflat))
        self._step_done()

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def compute_item_all(self):
        """Runs the propagation once (lightgcn.py:88-90) and keeps the user part; returns the item part [I, D] -- what the
        trainer's fused scoring reads (the reference returns None and reads its own copy in predict)."""
        self.store_ufeatures, self.store_ifeatures = self.computer()
        return self.store_ifeatures

    @torch.no_grad()
    def encode_last(self, user, item_feature=None):
        """user int64 [B] -> (E_final rows [B, 1, D], the same as [B, D]): the query vectors of the fused scoring."""
        if self.store_ufeatures is None:
            raise PxrError("LightGCN: call compute_item_all() before scoring")
        rows = ops.embed_gather(self.store_ufeatures, user.reshape(-1).contiguous())
        return rows.view(rows.shape[0], 1, -1), rows

    @torch.no_grad()
    def predict(self, user, item_feature=None):
        """scores [B, I] = E_final_u[user] E_final_i^T (lightgcn.py:82-86)."""
        _, rows = self.encode_last(user)
        return dense_scores(rows, self.store_ifeatures)
