"""MOBERT4Rec training-step time at the shipped shape (configs/PixelNet/bert4rec.yaml with overall/ViT.yaml: clip-vit-base-patch32,
tune_scale 165, embedding_size 512, 2 layers, 4 heads, inner 1, dropout 0.1, L = 10, train_batch_size 16, synthetic 224 x 224
images) over a synthetic catalogue of `--items` items and `--chunks` chunks of 2 .. L + 1 uniformly drawn items, batched by
MoBert4RecTrainBatcher, and the time of the dense segment sum on its own.

Part 1, the step.  Two instances of the SAME class with the same seed, optimizer objects and batches:
  native:        the batcher's (index, masked_index, image_ids) through modal_inputs: each distinct image encoded once;
  per_position:  the same batches in the reference's form (input_ids, items_modal [B, 3 P, 3, H, W], masked_index), images by
                 MOBERT4RecTrainDataset's rule -- one image per (position, input | positive | negative), 3 B P of them (behind the
                 zero image the mapping puts in front).  The baseline is this input form, never other native code.
Both run in the same process and alternate: `--rounds` rounds of `--steps` steps each; a side's figure is the median over the
rounds.  The tower weights are random (no checkpoint is read): the time does not depend on them.  Also counted over the epoch's
batches: images encoded per step both ways.

Part 2, pxr_seq_occ_dense_f32 at B 64, P 51, D 512 on one of the batcher's index tensors at that shape, against the route the
library offered before it for the same result: materialise the [3 B P, D] occurrence rows with torch ops (dx0 | coef * out |
-coef * out), then pxr_embed_grad_dense_f32.  The largest difference between the two blocks is recorded with the times.
usage (on an MI355X): python tools/mobert4rec_bench.py [--steps 10] [--rounds 3] [--out profiles/mobert4rec/mobert4rec_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

L, D, BATCH, IMAGE = 10, 512, 16, 224
ARGS = {"modal_lr": 1e-4, "rec_lr": 1e-4, "modal_decay": 0.0, "rec_decay": 0.1}


class _Data:
    def __init__(self, I, n_chunks, max_len, seed=1):
        rng = np.random.default_rng(seed)
        self.item_num = I
        self.train_feat = {"item_seq": [rng.choice(np.arange(1, I), size=int(rng.integers(2, max_len + 2)), replace=False).tolist()
                                        for _ in range(n_chunks)], "user_id": list(range(1, n_chunks + 1))}


def config(length=L, batch=BATCH):
    return {"model": "MOBERT4Rec", "n_layers": 2, "n_heads": 4, "embedding_size": D, "inner_size": 1, "hidden_dropout_prob": 0.1,
            "attn_dropout_prob": 0.1, "hidden_act": "gelu", "layer_norm_eps": 1e-12, "initializer_range": 0.02, "mask_ratio": 0.6,
            "MAX_ITEM_LIST_LENGTH": length, "seed": 2020, "train_batch_size": batch, "encoder_name": "clip-vit-base-patch32",
            "encoder_source": "transformers", "pretrain_path": None, "encoder_path": None,
            "fine_tune_arg": {"tune_scale": 165, "pre_trained": True, "activation": "relu", "dnn_layers": [], "method": "mean",
                              "allow_random_backbone": True}}


def per_position_input(store, batch, item_num):
    """(index, masked_index, image_ids) -> the reference's (input_ids [B, P], items_modal [B, 3 P, 3, H, W], masked_index)."""
    index, masked, image_ids = batch
    items = image_ids[index]                                         # BERT4Rec's [B, 3, P] ids
    ids = items.permute(0, 2, 1).reshape(items.shape[0], -1)          # (input, positive, negative) per position
    ones = torch.zeros_like(ids, dtype=torch.bool)
    ones[:, 0::3] = (ids[:, 0::3] == 0) | (ids[:, 0::3] == item_num)  # the ones image at mask and padded input positions
    modal = store.batch(torch.where(ones | (ids == item_num), torch.zeros_like(ids), ids))
    modal[ones] = 1.0
    return items[:, 0].contiguous(), modal, masked


def side(data, batches, store, per_position):
    from pixelrec_amd import model
    from pixelrec_amd.optim import OptimizerGroup, PxrAdamW, VisualAdamW

    torch.manual_seed(0)
    m = model.MOBERT4Rec(config(), data).cuda().train()
    opt = OptimizerGroup(VisualAdamW(m.visual_encoder, lr=ARGS["modal_lr"], weight_decay=ARGS["modal_decay"]),
                         PxrAdamW(m, lr=ARGS["rec_lr"], weight_decay=ARGS["rec_decay"]))
    it = iter(range(1 << 30))
    one = torch.ones((), device="cuda")

    def step():
        batch = batches[next(it) % len(batches)]
        inp = per_position_input(store, batch, data.item_num) if per_position else m.modal_inputs(store, batch)
        loss = m(inp)
        loss.backward(one)
        opt.step()

    return step, m


def dense_sink_times(items, reps):
    from lightgcn_bench import timed
    from pixelrec_amd import ops
    from pixelrec_amd.data.dataset import MoBert4RecTrainBatcher

    B, Lk = 64, 50
    P = Lk + 1
    data = _Data(items, 4 * B, Lk, seed=2)
    index, _, image_ids = next(iter(MoBert4RecTrainBatcher(config(Lk, B), data)))
    index, M = index.cuda(), len(image_ids)
    g = torch.Generator().manual_seed(4)
    dx0, out = (torch.randn(B, P, D, generator=g).cuda() for _ in range(2))
    coef = torch.randn(B, P, generator=g).cuda()
    layout = (3 * P, 0, P, 2 * P)
    flat_ids = index.permute(1, 0, 2).reshape(-1)                     # inputs | targets | negatives, each (b, t)
    blk_a = torch.empty(M, D, device="cuda")
    blk_b = torch.empty(M, D, device="cuda")

    def fused():
        return ops.seq_occ_dense_grad(index, layout, dx0, out, coef, M, d_rows=blk_a)

    def materialised():
        co = coef.view(-1, 1) * out.view(-1, D)
        return ops.embed_grad_dense(flat_ids, torch.cat((dx0.view(-1, D), co, -co)), M, out=blk_b)

    a_ms, b_ms = [], []
    for r in range(3):
        a_ms.append(timed(fused, reps, warm=3 if r == 0 else 0))
        b_ms.append(timed(materialised, reps, warm=3 if r == 0 else 0))
    ops.raise_on_bad_indices()
    res = {"B": B, "P": P, "D": D, "n_rows": M, "occurrences": 3 * B * P, "seq_occ_dense_ms": round(statistics.median(a_ms), 4),
           "materialise_then_embed_grad_dense_ms": round(statistics.median(b_ms), 4), "rounds_ms": {"seq_occ_dense": [round(x, 4) for x in a_ms],
                                                                                                   "materialised": [round(x, 4) for x in b_ms]},
           "largest_difference": float((blk_a - blk_b).abs().max()), "largest_entry": float(blk_a.abs().max())}
    res["materialised_over_seq_occ_dense"] = round(res["materialise_then_embed_grad_dense_ms"] / res["seq_occ_dense_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--chunks", type=int, default=256)
    ap.add_argument("--sink-reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from lightgcn_bench import timed
    from pixelrec_amd.data.dataset import MoBert4RecTrainBatcher
    from pixelrec_amd.data.images import ImageStore

    data = _Data(a.items, a.chunks, L)
    host = list(MoBert4RecTrainBatcher(config(), data))
    P = L + 1
    res = {"shape": {"encoder": "clip-vit-base-patch32", "tune_scale": 165, "D": D, "L": L, "batch": BATCH, "image": IMAGE,
                     "items": a.items, "steps": a.steps, "rounds": a.rounds},
           "images_per_step": {"batch_dedup": round(float(np.mean([len(i) for _, _, i in host])), 1),
                               "per_position": round(float(np.mean([3 * x.shape[0] * P for x, _, _ in host])), 1),
                               "bound_2_plus_chunk_lengths_plus_masked": round(float(np.mean(
                                   [2 + int((x[:, 1] != 0).sum()) + int((mk != 0).sum()) for x, mk, _ in host])), 1)}}
    print(json.dumps(res["images_per_step"]))
    batches = [tuple(t.cuda() for t in b) for b in host]
    store = ImageStore.synthetic(a.items, IMAGE, 0, "cuda")
    built = {"native": side(data, batches, store, False), "per_position": side(data, batches, store, True)}
    ms = {k: [] for k in built}
    for r in range(a.rounds):
        for k, (fn, _) in built.items():
            ms[k].append(timed(fn, a.steps, warm=2 if r == 0 else 0))
    res["MOBERT4Rec"] = {k + "_ms": round(statistics.median(v), 3) for k, v in ms.items()}
    res["MOBERT4Rec"]["rounds_ms"] = {k: [round(x, 3) for x in v] for k, v in ms.items()}
    res["MOBERT4Rec"]["per_position_over_native"] = round(res["MOBERT4Rec"]["per_position_ms"] / res["MOBERT4Rec"]["native_ms"], 4)
    print("MOBERT4Rec", json.dumps(res["MOBERT4Rec"]))
    del built
    torch.cuda.empty_cache()
    res["dense_sink"] = dense_sink_times(a.items, a.sink_reps)
    print("dense_sink", json.dumps(res["dense_sink"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
