"""Generates tests/golden/lightgcn_tiny.npz by running the REFERENCE's LightGCN (REC/model/IDNet/lightgcn.py) and its
get_norm_adj_mat (REC/data/dataload.py:318-339) unmodified, imported through oracle/ref_shim.py.  Run where the reference is
present:   python tools/make_golden_lightgcn.py

torch_geometric is not installed here, so a minimal stand-in with PyG's documented semantics is registered BEFORE
ref_shim.install_stubs() (which leaves an existing module alone): MessagePassing(aggr='add').propagate(edge_index, x=..., **kw)
= zeros.index_add_(0, edge_index[1], message(x[edge_index[0]], **kw)) (source -> target), and degree(index, num_nodes) = the
float32 bincount of index.

Tiny graph: user_num = 7 (user 0 = [PAD] and user 6 have no edge), item_num = 9 (item 0 = [PAD] and item 8 have no edge),
D = 8, with duplicate interactions.  Batches of B = 6 repeat users and items (one item is the positive of one sample and the
negative of another).  Stored for K = 1 and K = 3 (prefix k1. / k3.): state_dict, loss, both table gradients, predict scores,
and a 4-step torch.optim.AdamW trajectory (lr 1e-3, weight decay 0.1): losses + final tables.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

C = dict(user_num=7, item_num=9, D=8, B=6, seed=17, lr=1e-3, wd=0.1)
TRAIN_U = np.array([1, 1, 1, 2, 2, 3, 3, 3, 3, 4, 5, 5, 1, 2], dtype=np.int64)
TRAIN_I = np.array([3, 3, 4, 1, 5, 2, 3, 7, 7, 6, 1, 2, 6, 5], dtype=np.int64)


def install_pyg_standin():
    class MessagePassing(torch.nn.Module):
        def __init__(self, aggr="add", **kw):
            super().__init__()
            assert aggr == "add"

        def propagate(self, edge_index, x, **kw):
            msg = self.message(x[edge_index[0]], **kw)
            return torch.zeros_like(x).index_add_(0, edge_index[1], msg)

    def degree(index, num_nodes=None, dtype=None):
        n = int(num_nodes) if num_nodes is not None else int(index.max()) + 1
        return torch.bincount(index, minlength=n).to(dtype or torch.get_default_dtype())

    tg = types.ModuleType("torch_geometric")
    tg.nn = types.ModuleType("torch_geometric.nn")
    tg.nn.MessagePassing = MessagePassing
    tg.utils = types.ModuleType("torch_geometric.utils")
    tg.utils.degree = degree
    tg.utils.add_self_loops = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("not used by LightGCN"))
    sys.modules.update({"torch_geometric": tg, "torch_geometric.nn": tg.nn, "torch_geometric.utils": tg.utils})


class FakeData:
    """What LightGCN.__init__ reads from the reference's Data, with the reference's own get_norm_adj_mat bound to it."""

    def __init__(self, Data):
        self.user_num, self.item_num = C["user_num"], C["item_num"]
        self.uid_field, self.iid_field = "user_id", "item_id"
        self.train_feat = {"user_id": TRAIN_U, "item_id": TRAIN_I}
        self.get_norm_adj_mat = types.MethodType(Data.get_norm_adj_mat, self)


def batch(rng):
    B = C["B"]
    user = rng.integers(1, 6, size=B)
    user[1] = user[0]                                     # a repeated user
    pos = rng.integers(1, 8, size=B)
    neg = rng.integers(1, 9, size=B)
    neg[2] = pos[0]                                       # an item that is a positive of one sample and a negative of another
    pos[3] = pos[0]
    return user.astype(np.int64), np.stack([pos, neg], axis=1).astype(np.int64)


def main():
    install_pyg_standin()
    ref_shim.import_reference()
    from REC.data.dataload import Data
    from REC.model.IDNet.lightgcn import LightGCN

    rng = np.random.default_rng(C["seed"])
    data = FakeData(Data)
    ei, ew = data.get_norm_adj_mat()
    store = {"meta": np.array([C[k] for k in ("user_num", "item_num", "D", "B", "seed")]), "lr_wd": np.array([C["lr"], C["wd"]]),
             "train_u": TRAIN_U, "train_i": TRAIN_I, "edge_index": ei.numpy(), "edge_weight": ew.numpy()}
    g = torch.Generator().manual_seed(C["seed"])
    sd0 = {"user_embedding.weight": torch.randn(C["user_num"], C["D"], generator=g) * 0.5,
           "item_embedding.weight": torch.randn(C["item_num"], C["D"], generator=g) * 0.5}
    for k, v in sd0.items():
        store["sd." + k] = v.numpy().copy()
    batches = [batch(rng) for _ in range(4)]
    store["users"] = np.stack([b[0] for b in batches])
    store["items"] = np.stack([b[1] for b in batches])
    store["eval.users"] = np.array([1, 2, 3, 4, 5, 6, 0, 3], dtype=np.int64)
    for K in (1, 3):
        cfg = {"embedding_size": C["D"], "n_layers": K, "device": "cpu"}
        model = LightGCN(cfg, data)
        res = model.load_state_dict(sd0, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        p = f"k{K}."
        user, item = (torch.from_numpy(x) for x in batches[0])
        model.zero_grad()
        loss = model((user, item))
        loss.backward()
        store[p + "loss"] = np.array(loss.item(), dtype=np.float32)
        for k, v in model.named_parameters():
            store[p + "grad." + k] = v.grad.numpy().copy()
        with torch.no_grad():
            model.compute_item_all()
            store[p + "eval.scores"] = model.predict(torch.from_numpy(store["eval.users"]), None).numpy()
        opt = torch.optim.AdamW(model.parameters(), lr=C["lr"], weight_decay=C["wd"])
        for s, (u, it) in enumerate(batches):
            opt.zero_grad()
            l = model((torch.from_numpy(u), torch.from_numpy(it)))
            l.backward()
            opt.step()
            store[p + f"adamw.loss{s}"] = np.array(l.item(), dtype=np.float32)
        for k, v in model.state_dict().items():
            store[p + "adamw.final." + k] = v.numpy().copy()
    path = os.path.join(ROOT, "tests", "golden", "lightgcn_tiny.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB), loss k1={float(store['k1.loss']):.6f} k3={float(store['k3.loss']):.6f}")


if __name__ == "__main__":
    main()
