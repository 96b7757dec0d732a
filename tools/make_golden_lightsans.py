"""Generates tests/golden/lightsans_tiny.npz by running the REFERENCE's LightSANs (REC/model/IDNet/lightsans.py with
REC/model/layers.py's LightTransformerEncoder) unmodified, imported through oracle/ref_shim.py.  Run where the reference is present:
    python tools/make_golden_lightsans.py

TwoTowerTrainDataset's rows are built here by its rule (the training sequence followed by one negative drawn outside it,
left-padded with 0 to L+2).  Tiny case: item_num = 30, D = 16, H = 2, K = 3, L = 6, B = 5, inner_size 1, dropout 0, rows covering a
history of one item (heavy left padding) and a full row.  One state_dict (sd.*, two layers); the one-layer model is the same
parameters without layer 1.  Stored for n_layers = 1 and 2 (prefix n1. / n2.): the state_dict key order, loss, every parameter
gradient (the table's dense, row 0 zero) and predict scores on an eval batch; for n_layers = 2 also a 4-step torch.optim.AdamW
trajectory (lr 1e-2, weight decay 0.1): losses and final parameters.  Each group of parameter-shaped arrays is stored as ONE
flat float32 vector in state_dict key order (keys / shapes alongside; tests/lightsans_restate.unpack splits it): a few
hundred small members would cost more in zip headers than in data, and the file stays well under 100 KB.
"""
import logging
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

C = dict(item_num=30, D=16, H=2, K=3, L=6, B=5, inner=1, seed=31, lr=1e-2, wd=0.1)

SEQS = [
    [7],                          # a history of nothing but padding: the positive is the only item
    [3, 9, 4, 12, 5, 21, 8],      # full row: L history items + the positive
    [11, 2, 11, 6],               # a revisit
    [14, 15],
    [27, 1, 29, 13, 22],
]


def row(seq, neg, L):
    s = list(seq) + [neg]
    return np.array(([0] * (L + 2 - len(s)) + s)[-(L + 2):], dtype=np.int64)


def make_batch(rng, seqs):
    """TwoTowerTrainDataset.__getitem__'s rule: sequence + a negative uniform on [1, item_num - 1] outside it, left-padded."""
    out = []
    for s in seqs:
        neg = int(rng.integers(1, C["item_num"]))
        while neg in s:
            neg = int(rng.integers(1, C["item_num"]))
        out.append(row(s, neg, C["L"]))
    return np.stack(out)


def config(n_layers):
    return {"n_layers": n_layers, "n_heads": C["H"], "embedding_size": C["D"], "inner_size": C["inner"], "k_interests": C["K"],
            "hidden_dropout_prob": 0.0, "attn_dropout_prob": 0.0, "hidden_act": "gelu", "layer_norm_eps": 1e-12, "device": "cpu",
            "initializer_range": 0.02, "MAX_ITEM_LIST_LENGTH": C["L"]}


def pack(store, name, tensors):
    store[name] = np.concatenate([np.asarray(t, dtype=np.float32).ravel() for t in tensors.values()])


def main():
    ref_shim.import_reference()
    from REC.model.IDNet.lightsans import LightSANs

    logging.disable(logging.CRITICAL)
    rng = np.random.default_rng(C["seed"])
    L = C["L"]
    store = {"meta": np.array([C[k] for k in ("item_num", "D", "H", "K", "L", "B", "inner", "seed")]),
             "lr_wd": np.array([C["lr"], C["wd"]])}
    batches = [make_batch(rng, SEQS)]
    for _ in range(3):
        perm = rng.permutation(len(SEQS))
        batches.append(make_batch(rng, [SEQS[i][:max(1, len(SEQS[i]) - int(rng.integers(0, 3)))] for i in perm]))
    for j, bt in enumerate(batches):
        store[f"b{j}.items"] = bt
    hists = [[3, 9, 4, 12, 5, 21, 8, 2], [7], [], [11, 2, 11, 6], [29, 1]]
    store["eval.item_seq"] = np.stack([np.array(([0] * L + h)[-L:] if h else [0] * L, dtype=np.int64) for h in hists])
    dl = type("D", (), {"item_num": C["item_num"]})()
    torch.manual_seed(C["seed"])
    sd2 = LightSANs(config(2), dl).state_dict()
    store["keys"] = np.array(list(sd2.keys()))
    store["shapes"] = np.array([[v.dim()] + list(v.shape) + [1] * (2 - v.dim()) for v in sd2.values()], dtype=np.int64)
    pack(store, "sd", sd2)
    for n_layers in (1, 2):
        model = LightSANs(config(n_layers), dl)
        res = model.load_state_dict({k: v for k, v in sd2.items() if n_layers == 2 or ".layer.1." not in k}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        model.eval()              # dropout 0 either way; eval() keeps nn.Dropout out of the picture
        p = f"n{n_layers}."
        store[p + "sd_keys"] = np.array(list(model.state_dict().keys()))
        model.zero_grad()
        loss = model(torch.from_numpy(batches[0]))
        loss.backward()
        store[p + "loss"] = np.array(loss.item(), dtype=np.float32)
        pack(store, p + "grad", {k: v.grad for k, v in model.named_parameters()})
        with torch.no_grad():
            store[p + "eval.scores"] = model.predict(torch.from_numpy(store["eval.item_seq"]), model.compute_item_all()).numpy()
        if n_layers == 1:
            continue
        opt = torch.optim.AdamW(model.parameters(), lr=C["lr"], weight_decay=C["wd"])
        for s, bt in enumerate(batches):
            opt.zero_grad()
            l = model(torch.from_numpy(bt))
            l.backward()
            opt.step()
            store[p + f"adamw.loss{s}"] = np.array(l.item(), dtype=np.float32)
        pack(store, p + "adamw.final", model.state_dict())
    path = os.path.join(ROOT, "tests", "golden", "lightsans_tiny.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB), loss n1={float(store['n1.loss']):.6f} "
          f"n2={float(store['n2.loss']):.6f}")


if __name__ == "__main__":
    main()
