"""MOSRGNN training-step time at the shipped shape (configs/PixelNet/srgnn.yaml with overall/ViT.yaml: clip-vit-base-patch32,
tune_scale 165, embedding_size 512, step 2, L = 10, train_batch_size 16, synthetic 224 x 224 images) over a synthetic catalogue of
`--items` items and `--users` sessions of 3 .. L + 1 uniformly drawn items, cut into AUGSEQ prefixes and batched by
MoGraphTrainBatcher.

Two instances of the SAME class with the same seed, optimizer objects and batches:
  native:    the batcher's (index, image_ids) through modal_inputs: each distinct image of the batch encoded once;
  per_slot:  the same batches in the reference's form (alias_inputs, A [B, n, 2n], mask, items_all [B (n + 2), 3, H, W]), by
             mograph_train_collate's rule -- one image per node slot and target, n the batch's largest node count, pad images
             included.  The session graphs of this side are built on the host before the clock starts (the collate's loop runs in
             the reference's loader workers).  The baseline is this input form, never other native code.
Both run in the same process and alternate: `--rounds` rounds of `--steps` steps each; a side's figure is the median over the
rounds.  The tower weights are random (no checkpoint is read): the time does not depend on them.  Also counted over the epoch's
batches: images encoded per step both ways.
usage (on an MI355X): python tools/mosrgnn_bench.py [--steps 10] [--rounds 3] [--out profiles/mosrgnn/mosrgnn_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

L, D, BATCH, IMAGE, STEP = 10, 512, 16, 224, 2
ARGS = {"modal_lr": 1e-4, "rec_lr": 1e-4, "modal_decay": 0.0, "rec_decay": 0.1}


def make_data(I, n_users, seed=1):
    """A dataload of AUGSEQ prefixes, as GraphTrainBatcher reads it (tools/srgnn_bench.py host_rates)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(3, L + 2, size=n_users)
    flat = rng.integers(1, I, size=int(lens.sum())).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return type("DL", (), {"item_num": I, "_sorted_items": flat,
                           "train_feat": {"seq_start": np.repeat(starts, lens - 1),
                                          "seq_len": np.concatenate([np.arange(2, n + 1) for n in lens])}})()


def config():
    return {"model": "MOSRGNN", "embedding_size": D, "step": STEP, "MAX_ITEM_LIST_LENGTH": L, "seed": 2020, "train_batch_size": BATCH,
            "encoder_name": "clip-vit-base-patch32", "encoder_source": "transformers", "pretrain_path": None, "encoder_path": None,
            "fine_tune_arg": {"tune_scale": 165, "pre_trained": True, "activation": "relu", "dnn_layers": [], "method": "mean",
                              "allow_random_backbone": True}}


def session_graph(seq, n):
    """The collate's graph of item ids seq [B, L] at n nodes -> (nodes [B, n], alias [B, L], A [B, n, 2n])."""
    B = seq.shape[0]
    nodes, alias, A = np.zeros((B, n), np.int64), np.zeros((B, L), np.int64), np.zeros((B, n, 2 * n), np.float32)
    for b in range(B):
        u = np.unique(seq[b])
        nodes[b, :len(u)] = u
        alias[b] = np.searchsorted(u, seq[b])
        adj = np.zeros((n, n))
        for i in range(L - 1):
            if seq[b, i + 1] == 0:
                break
            adj[alias[b, i], alias[b, i + 1]] = 1.0
        si, so = adj.sum(0), adj.sum(1)
        si[si == 0] = 1.0
        so[so == 0] = 1.0
        A[b] = np.concatenate([adj / si, adj.T / so]).T
    return nodes, alias, A


def per_slot_parts(batch):
    """(index, image_ids) -> (alias_inputs, A, mask, the item id behind every row of items_all [B (n + 2)]) on the device."""
    index, image_ids = batch
    items = image_ids[index].numpy()
    seq, tgt = items[:, :L], items[:, L:]
    n = max(len(np.unique(r)) for r in seq)
    nodes, alias, A = session_graph(seq, n)
    slots = np.concatenate((nodes, tgt), axis=1).reshape(-1)
    return tuple(torch.from_numpy(x).cuda() for x in (alias, A, (seq != 0).astype(np.int64), slots))


def side(data, batches, store, per_slot):
    from pixelrec_amd import model
    from pixelrec_amd.optim import OptimizerGroup, PxrAdamW, VisualAdamW

    torch.manual_seed(0)
    m = model.MOSRGNN(config(), data).cuda().train()
    opt = OptimizerGroup(VisualAdamW(m.visual_encoder, lr=ARGS["modal_lr"], weight_decay=ARGS["modal_decay"]),
                         PxrAdamW(m, lr=ARGS["rec_lr"], weight_decay=ARGS["rec_decay"]))
    it = iter(range(1 << 30))
    one = torch.ones((), device="cuda")

    def step():
        batch = batches[next(it) % len(batches)]
        if per_slot:
            alias, A, mask, slots = batch
            inp = (alias, A, mask, store.batch(slots))
        else:
            inp = m.modal_inputs(store, batch)
        loss = m(inp)
        loss.backward(one)
        opt.step()

    return step, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--users", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from lightgcn_bench import timed
    from pixelrec_amd import ops
    from pixelrec_amd.data.dataset import MoGraphTrainBatcher
    from pixelrec_amd.data.images import ImageStore

    data = make_data(a.items, a.users)
    host = [b for b in MoGraphTrainBatcher(config(), data) if b[0].shape[0] == BATCH]
    slot = [per_slot_parts(b) for b in host]
    res = {"shape": {"encoder": "clip-vit-base-patch32", "tune_scale": 165, "D": D, "L": L, "step": STEP, "batch": BATCH, "image": IMAGE,
                     "items": a.items, "batches": len(host), "steps": a.steps, "rounds": a.rounds},
           "images_per_step": {"batch_dedup": round(float(np.mean([len(i) for _, i in host])), 1),
                               "per_slot": round(float(np.mean([len(s[3]) for s in slot])), 1)}}
    print(json.dumps(res["images_per_step"]))
    batches = [tuple(t.cuda() for t in b) for b in host]
    store = ImageStore.synthetic(a.items, IMAGE, 0, "cuda")
    built = {"native": side(data, batches, store, False), "per_slot": side(data, slot, store, True)}
    ms = {k: [] for k in built}
    for r in range(a.rounds):
        for k, (fn, _) in built.items():
            ms[k].append(timed(fn, a.steps, warm=2 if r == 0 else 0))
    ops.raise_on_bad_indices()
    res["MOSRGNN"] = {k + "_ms": round(statistics.median(v), 3) for k, v in ms.items()}
    res["MOSRGNN"]["rounds_ms"] = {k: [round(x, 3) for x in v] for k, v in ms.items()}
    res["MOSRGNN"]["per_slot_over_native"] = round(res["MOSRGNN"]["per_slot_ms"] / res["MOSRGNN"]["native_ms"], 4)
    print("MOSRGNN", json.dumps(res["MOSRGNN"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
