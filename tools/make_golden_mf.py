"""Generates tests/golden/mf_tiny.npz by running the REFERENCE's MF (REC/model/IDNet/mf.py with MLPLayers, layers.py:239-294)
unmodified, imported through oracle/ref_shim.py.  Run where the reference is present:   python tools/make_golden_mf.py

Tiny shape: user_num = 7, item_num = 9, D = 8, B = 6.  The batches repeat users and items, include user 0 and item 0 (ordinary
trainable rows in MF: no padding id), and one item is the positive of one sample and the negative of another.  Two configs
(prefix c0. / c1.): mlp_hidden_size [] (identity towers, the shipped config) and [8, 4] (two Dropout -> Linear -> BatchNorm1d ->
Tanh layers per tower; hidden sizes are multiples of 4, what the native kernels take).  The initial state has random BatchNorm
affine parameters and running statistics.  Stored per config: the initial state_dict, the loss and every gradient of one
training step, the eval-mode predict scores after compute_item_all (running statistics as that step left them), and a 4-step
torch.optim.AdamW trajectory (lr 1e-3, weight decay 0.1) from the initial state: losses, final state_dict (BatchNorm buffers
included).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

C = dict(user_num=7, item_num=9, D=8, B=6, seed=23, lr=1e-3, wd=0.1)
CONFIGS = {"c0": [], "c1": [8, 4]}


class FakeData:
    user_num, item_num = C["user_num"], C["item_num"]


def batch(rng):
    B = C["B"]
    user = rng.integers(0, C["user_num"], size=B)
    user[1] = user[0]                                     # a repeated user
    user[4] = 0                                           # user 0 is an ordinary row
    pos = rng.integers(0, C["item_num"], size=B)
    neg = rng.integers(0, C["item_num"], size=B)
    neg[2] = pos[0]                                       # the positive of one sample is the negative of another
    pos[3] = pos[0]
    pos[5] = 0                                            # item 0 is an ordinary row
    return user.astype(np.int64), np.stack([pos, neg], axis=1).astype(np.int64)


def main():
    ref_shim.import_reference()
    from REC.model.IDNet.mf import MF

    rng = np.random.default_rng(C["seed"])
    batches = [batch(rng) for _ in range(4)]
    store = {"meta": np.array([C[k] for k in ("user_num", "item_num", "D", "B", "seed")]), "lr_wd": np.array([C["lr"], C["wd"]]),
             "users": np.stack([b[0] for b in batches]), "items": np.stack([b[1] for b in batches]),
             "eval.users": np.array([1, 2, 3, 4, 5, 6, 0, 3], dtype=np.int64)}
    for p, hidden in CONFIGS.items():
        store[p + ".hidden"] = np.array(hidden, dtype=np.int64)
        cfg = {"embedding_size": C["D"], "mlp_hidden_size": list(hidden), "dropout_prob": 0.0, "device": "cpu"}
        torch.manual_seed(C["seed"])
        model = MF(cfg, FakeData())
        g = torch.Generator().manual_seed(C["seed"] + 1)
        with torch.no_grad():
            for mod in model.modules():                  # BatchNorm affine parameters and running statistics: away from 1 / 0
                if isinstance(mod, torch.nn.BatchNorm1d):
                    mod.weight.copy_(1.0 + 0.3 * torch.randn(mod.weight.shape, generator=g))
                    mod.bias.copy_(0.2 * torch.randn(mod.bias.shape, generator=g))
                    mod.running_mean.copy_(0.2 * torch.randn(mod.running_mean.shape, generator=g))
                    mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
        sd0 = {k: v.clone() for k, v in model.state_dict().items()}
        for k, v in sd0.items():
            store[p + ".sd." + k] = v.numpy().copy()
        model.train()
        user, item = (torch.from_numpy(x) for x in batches[0])
        model.zero_grad()
        loss = model((user, item))
        loss.backward()
        store[p + ".loss"] = np.array(loss.item(), dtype=np.float32)
        for k, v in model.named_parameters():
            store[p + ".grad." + k] = v.grad.numpy().copy()
        model.eval()
        with torch.no_grad():
            feat = model.compute_item_all()
            store[p + ".eval.scores"] = model.predict(torch.from_numpy(store["eval.users"]), feat).numpy()
        model.train()
        model.load_state_dict(sd0, strict=True)
        opt = torch.optim.AdamW(model.parameters(), lr=C["lr"], weight_decay=C["wd"])
        for s, (u, it) in enumerate(batches):
            opt.zero_grad()
            l = model((torch.from_numpy(u), torch.from_numpy(it)))
            l.backward()
            opt.step()
            store[p + f".adamw.loss{s}"] = np.array(l.item(), dtype=np.float32)
        for k, v in model.state_dict().items():
            store[p + ".adamw.final." + k] = v.numpy().copy()
    path = os.path.join(ROOT, "tests", "golden", "mf_tiny.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB), loss c0={float(store['c0.loss']):.6f} "
          f"c1={float(store['c1.loss']):.6f}")


if __name__ == "__main__":
    main()
