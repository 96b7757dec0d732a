"""Generates tests/golden/srgnn_tiny.npz by running the REFERENCE's SRGNN (REC/model/IDNet/srgnn.py), its graph_train_collate /
graph_eval_collate (REC/data/dataset/collate_fn.py) and Data._build_aug_seq (REC/data/dataload.py) unmodified, imported through
oracle/ref_shim.py.  Run where the reference is present:   python tools/make_golden_srgnn.py

GraphTrainDataset / GraphEvalDataset pad with np.array(..., dtype=np.int), which NumPy 2 removed: the padded inputs are built
here by the datasets' rule (item_seq = history right-padded with 0 to L, mask = 1 on the real positions, target = (positive,
negative)) and handed to the collates.

Tiny case: item_num = 20, D = 12, L = 5, B = 6 sessions covering a revisit, a self-loop (5, 5), a repeated transition, a
length-1 session (no edges) and a full-length session without padding.  Stored for step = 1 and 2 (prefix s1. / s2.): the
collate's alias / A / items of the first batch, state_dict, loss, every parameter gradient (gnn.linear_edge_f has none),
predict scores on an eval batch (one history empty), and a 4-step torch.optim.AdamW trajectory (lr 1e-2, weight decay 0.1):
losses and final parameters.  Plus the AUGSEQ samples of tests/golden/TinyInter.csv at L = 5 (aug.*).
"""
import logging
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

C = dict(item_num=20, D=12, L=5, B=6, seed=23, lr=1e-2, wd=0.1)

SESSIONS = [
    [3, 5, 3, 7],            # revisit
    [5, 5, 6],               # self-loop
    [2, 9, 2, 9, 11],        # repeated transition 2 -> 9, full length (no padding)
    [8],                     # one item: no edges
    [12, 13, 14, 15],
    [5, 3, 5, 3],            # repeated transitions both ways
]


def pad(seq, L):
    s = list(seq)
    return np.array((s + [0] * (L - len(s)))[-L:], dtype=np.int64)


def make_batch(rng, sessions):
    """(item_seq, mask, target) per sample, by GraphTrainDataset.__getitem__'s rule."""
    L = C["L"]
    out = []
    for s in sessions:
        pos = int(rng.integers(1, C["item_num"]))
        while pos in s:
            pos = int(rng.integers(1, C["item_num"]))
        neg = int(rng.integers(1, C["item_num"]))
        while neg in s or neg == pos:
            neg = int(rng.integers(1, C["item_num"]))
        out.append((pad(s, L), pad([1] * min(len(s), L), L), np.array([pos, neg], dtype=np.int64)))
    return out


def main():
    ref_shim.import_reference()
    from REC.data.dataload import Data
    from REC.data.dataset.collate_fn import graph_eval_collate, graph_train_collate
    from REC.model.IDNet.srgnn import SRGNN
    from REC.utils.enum_type import InputType

    logging.disable(logging.CRITICAL)
    rng = np.random.default_rng(C["seed"])
    L = C["L"]
    store = {"meta": np.array([C[k] for k in ("item_num", "D", "L", "B", "seed")]), "lr_wd": np.array([C["lr"], C["wd"]])}
    # four training batches: the sessions above, then shuffled / cut variants of them
    batches = [make_batch(rng, SESSIONS)]
    for _ in range(3):
        perm = rng.permutation(len(SESSIONS))
        batches.append(make_batch(rng, [SESSIONS[i][:max(1, len(SESSIONS[i]) - int(rng.integers(0, 2)))] for i in perm]))
    for j, bt in enumerate(batches):
        store[f"b{j}.item_seq"] = np.stack([x[0] for x in bt])
        store[f"b{j}.mask"] = np.stack([x[1] for x in bt])
        store[f"b{j}.target"] = np.stack([x[2] for x in bt])
    alias, A, items, _, _ = graph_train_collate(batches[0])
    store["collate.alias"], store["collate.A"], store["collate.items"] = alias.numpy(), A.numpy(), items.numpy()
    # eval batch (GraphEvalDataset's rule: the last L history items, right-padded; the mask over them), one history empty
    hists = [[3, 5, 3, 7, 9, 4, 4], [5, 5, 6], [8], [], [2, 9, 2, 9, 11], [19, 1]]
    ev = [(torch.tensor(h, dtype=torch.long), pad(h[-L:], L), pad([1] * min(len(h), L), L), 1) for h in hists]
    (e_alias, e_A, e_items, e_mask), _, _, _ = graph_eval_collate(ev)
    store["eval.item_seq"] = np.stack([x[1] for x in ev])
    store["eval.mask"] = e_mask.numpy()
    torch.manual_seed(C["seed"])
    base = SRGNN({"embedding_size": C["D"], "step": 1, "device": "cpu"}, type("D", (), {"item_num": C["item_num"]})())
    sd0 = {k: v.detach().clone() for k, v in base.state_dict().items()}
    for k, v in sd0.items():
        store["sd." + k] = v.numpy().copy()
    for step in (1, 2):
        model = SRGNN({"embedding_size": C["D"], "step": step, "device": "cpu"}, type("D", (), {"item_num": C["item_num"]})())
        res = model.load_state_dict(sd0, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        p = f"s{step}."
        model.zero_grad()
        loss = model(graph_train_collate(batches[0]))
        loss.backward()
        store[p + "loss"] = np.array(loss.item(), dtype=np.float32)
        for k, v in model.named_parameters():
            if v.grad is not None:
                store[p + "grad." + k] = v.grad.numpy().copy()
        with torch.no_grad():
            store[p + "eval.scores"] = model.predict((e_alias, e_A, e_items, e_mask), model.compute_item_all()).numpy()
        opt = torch.optim.AdamW(model.parameters(), lr=C["lr"], weight_decay=C["wd"])
        for s, bt in enumerate(batches):
            opt.zero_grad()
            l = model(graph_train_collate(bt))
            l.backward()
            opt.step()
            store[p + f"adamw.loss{s}"] = np.array(l.item(), dtype=np.float32)
        for k, v in model.state_dict().items():
            store[p + "adamw.final." + k] = v.numpy().copy()
    # AUGSEQ samples of TinyInter.csv (the reference's Data with MODEL_INPUT_TYPE = AUGSEQ)
    gdir = os.path.join(ROOT, "tests", "golden")
    d = Data({"data_path": gdir, "dataset": "TinyInter", "MAX_ITEM_LIST_LENGTH": L, "MODEL_INPUT_TYPE": InputType.AUGSEQ})
    d.build()
    seqs = d.train_feat["item_seq"]
    store["aug.L"] = np.array(L)
    store["aug.user_id"] = np.asarray(d.train_feat["user_id"], dtype=np.int64)
    store["aug.flat"] = np.concatenate(seqs).astype(np.int64)
    store["aug.lens"] = np.array([len(x) for x in seqs], dtype=np.int64)
    path = os.path.join(gdir, "srgnn_tiny.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB), loss s1={float(store['s1.loss']):.6f} "
          f"s2={float(store['s2.loss']):.6f}, {len(seqs)} AUGSEQ samples")


if __name__ == "__main__":
    main()
