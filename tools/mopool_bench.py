"""MODSSM and MOFM training-step time at the shipped ViT-B shape (configs/PixelNet/dssm.yaml, fm.yaml with overall/ViT.yaml:
clip-vit-base-patch32, tune_scale 165, embedding_size 4096, L = 10, train_batch_size 16 chunks, synthetic 224 x 224 images) over a
synthetic catalogue of `--items` items and `--chunks` chunks of 2 .. L + 1 uniformly drawn items, batched by MoPoolTrainBatcher.

  native:      model/mopooled.py -- native tower, pxr_pool_pair_fwd_f32 / pxr_pool_pair_bwd_f32, the dense segment sum
               pxr_pool_dense_grad_f32 into dE, native tower backward, VisualOnlyAdamW;
  torch head:  the same native tower and optimizer with the head in torch ops (E[index], masked pooling, the pair loss, autograd:
               index_put-style scatter-add into dE).  The baseline is this restatement, never the native code.
Both run in the same process on the same batches and alternate: `--rounds` rounds of `--steps` steps each; a side's figure is the
median over the rounds.  The tower weights are random (no checkpoint is read): the time does not depend on them.
Also counted over the epoch's batches: images encoded per step with the batch-wide dedup (len(image_ids)), with the reference's
per-chunk listing (1 + 2 n per chunk of n items) and without any (one image per occurrence, S (L + 2)).
usage (on an MI355X): python tools/mopool_bench.py [--steps 10] [--rounds 3] [--out profiles/mopool/mopool_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

L, D, CHUNKS_PER_BATCH, IMAGE = 10, 4096, 16, 224
ARGS = {"modal_lr": 1e-4, "rec_lr": 1e-4, "modal_decay": 0.0, "rec_decay": 0.1}


class _Data:
    def __init__(self, I, n_chunks, seed=1):
        rng = np.random.default_rng(seed)
        self.item_num = I
        self.train_feat = {"item_seq": [rng.choice(np.arange(1, I), size=int(rng.integers(2, L + 2)), replace=False).tolist()
                                        for _ in range(n_chunks)], "user_id": list(range(1, n_chunks + 1))}


def config(name):
    return {"model": name, "embedding_size": D, "mlp_hidden_size": [], "dropout_prob": 0, "MAX_ITEM_LIST_LENGTH": L, "seed": 2020,
            "train_batch_size": CHUNKS_PER_BATCH, "encoder_name": "clip-vit-base-patch32", "encoder_source": "transformers",
            "pretrain_path": None, "encoder_path": None,
            "fine_tune_arg": {"tune_scale": 165, "pre_trained": True, "activation": "relu", "dnn_layers": [], "method": "mean",
                              "allow_random_backbone": True}}


def torch_head(E, profile, target, mean):
    m = (profile != 0).to(E.dtype)
    u = (E[profile] * m[:, :, None]).sum(-2)
    if mean:
        u = u / (m.sum(1, keepdim=True) + 1e-8)
    x = (u * E[target[:, 0]]).sum(-1) - (u * E[target[:, 1]]).sum(-1)
    return -torch.log(1e-8 + torch.sigmoid(x)).mean()


def side(name, data, batches, store, torch_ops):
    from pixelrec_amd import model
    from pixelrec_amd.optim import VisualOnlyAdamW

    base = cls = getattr(model, name)
    if torch_ops:
        class cls(base):
            def loss_from_embeddings(self, E, profile_idx, target_idx):
                return torch_head(E, profile_idx, target_idx, self.pool_mean)
    torch.manual_seed(0)
    m = cls(config(name), data).cuda().train()
    opt = VisualOnlyAdamW(m.visual_encoder, lr=ARGS["modal_lr"], weight_decay=ARGS["modal_decay"],
                          empty_trailing_group={"lr": ARGS["rec_lr"], "weight_decay": ARGS["rec_decay"]})
    it = iter(range(1 << 30))
    one = torch.ones((), device="cuda")

    def step():
        index, image_ids = batches[next(it) % len(batches)]
        loss = m(m.modal_inputs(store, (index, image_ids)))
        loss.backward(one)
        opt.step()

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--chunks", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from lightgcn_bench import timed
    from pixelrec_amd.data.dataset import MoPoolTrainBatcher
    from pixelrec_amd.data.images import ImageStore

    data = _Data(a.items, a.chunks)
    batcher = MoPoolTrainBatcher(config("MODSSM"), data)
    host = list(batcher)
    lens = np.array([len(s) for s in data.train_feat["item_seq"]])
    order = batcher._indices()
    per_chunk = [int((1 + 2 * lens[order[k * CHUNKS_PER_BATCH:(k + 1) * CHUNKS_PER_BATCH]]).sum()) for k in range(len(host))]
    res = {"shape": {"encoder": "clip-vit-base-patch32", "tune_scale": 165, "D": D, "L": L, "chunks_per_batch": CHUNKS_PER_BATCH,
                     "image": IMAGE, "items": a.items, "steps": a.steps, "rounds": a.rounds},
           "images_per_step": {"batch_dedup": round(float(np.mean([len(i) for _, i in host])), 1),
                               "per_chunk_listing": round(float(np.mean(per_chunk)), 1),
                               "per_occurrence": round(float(np.mean([x.shape[0] * (L + 2) for x, _ in host])), 1),
                               "samples": round(float(np.mean([x.shape[0] for x, _ in host])), 1)}}
    print(json.dumps(res["images_per_step"]))
    batches = [(x.cuda(), i.cuda()) for x, i in host]
    store = ImageStore.synthetic(a.items, IMAGE, 0, "cuda")
    for name in ("MODSSM", "MOFM"):
        sides = {"native": side(name, data, batches, store, False), "torch_head": side(name, data, batches, store, True)}
        ms = {k: [] for k in sides}
        for r in range(a.rounds):
            for k, fn in sides.items():
                ms[k].append(timed(fn, a.steps, warm=2 if r == 0 else 0))
        res[name] = {k + "_ms": round(statistics.median(v), 3) for k, v in ms.items()}
        res[name]["rounds_ms"] = {k: [round(x, 3) for x in v] for k, v in ms.items()}
        res[name]["torch_head_over_native"] = round(res[name]["torch_head_ms"] / res[name]["native_ms"], 4)
        print(name, json.dumps(res[name]))
        del sides
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
