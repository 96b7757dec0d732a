"""MODIN training-step and evaluation time at the shipped shape (configs/PixelNet/din.yaml with overall/ViT.yaml:
clip-vit-base-patch32, tune_scale 165, embedding_size 64, mlp_hidden_size [80, 40], L = 10, train_batch_size 16, synthetic
224 x 224 images) over a synthetic catalogue of `--items` items and `--chunks` chunks of 2 .. L + 1 uniformly drawn items, batched
by MoTowerTrainBatcher.

  native:      model/modin.py -- native tower, csrc/din.hip's attention input / head (reg = 0) / fold, the dense segment sum
               pxr_embed_grad_dense_f32 into dE, native tower backward, OptimizerGroup(VisualAdamW, PxrAdamW);
  torch head:  the same native tower and optimizer objects with the head in torch ops on the same parameters (E[index], cat, the
               sigmoid MLP, the masked weights, the pair loss, autograd into dE and the attention tensors' .grad, which are the
               flat gradient buffer's views).  The baseline is this restatement, never the native code.
Both run in the same process on the same batches and alternate: `--rounds` rounds of `--steps` steps each; a side's figure is the
median over the rounds.  The tower weights are random (no checkpoint is read): the time does not depend on them.
Also counted over the epoch's batches: images encoded per step with the batch-wide dedup (len(image_ids)) against one per position
(B (L + 2), the reference's forward).
Evaluation, over a random [items, D] item_feature: one fused batch (MODIN.fused_topk_batch: A q + b1 cached, pxr_din_topk_f32)
against chunked predict + masks + torch.topk, at eval_batch_size 64, 256 and 1024 (the chunked path at `--predict-users` users,
scaled: it is linear in the users).
usage (on an MI355X): python tools/modin_bench.py [--steps 10] [--rounds 3] [--out profiles/modin/modin_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

L, D, HIDDEN, BATCH, IMAGE, K = 10, 64, [80, 40], 16, 224, 10
ARGS = {"modal_lr": 1e-4, "rec_lr": 1e-4, "modal_decay": 0.0, "rec_decay": 0.1}


class _Data:
    def __init__(self, I, n_chunks, seed=1):
        rng = np.random.default_rng(seed)
        self.item_num = I
        self.train_feat = {"item_seq": [rng.choice(np.arange(1, I), size=int(rng.integers(2, L + 2)), replace=False).tolist()
                                        for _ in range(n_chunks)], "user_id": list(range(1, n_chunks + 1))}


def config():
    return {"model": "MODIN", "embedding_size": D, "mlp_hidden_size": list(HIDDEN), "dropout_prob": 0, "MAX_ITEM_LIST_LENGTH": L,
            "seed": 2020, "train_batch_size": BATCH, "encoder_name": "clip-vit-base-patch32", "encoder_source": "transformers",
            "pretrain_path": None, "encoder_path": None,
            "fine_tune_arg": {"tune_scale": 165, "pre_trained": True, "activation": "relu", "dnn_layers": [], "method": "mean",
                              "allow_random_backbone": True}}


def torch_head(m, E, profile, target):
    """modin.py:49-61 in torch ops on the model's own (flat-buffer) parameters."""
    k = E[profile]                                                   # [S, L, D]
    scores = []
    for c in range(2):
        q = E[target[:, c]][:, None, :].expand_as(k)
        x = torch.cat([q, k, q - k, q * k], dim=-1)
        for i in range(len(m.mlp_hidden_size)):
            lin = m.attention.att_mlp_layers.mlp_layers[3 * i + 1]
            x = torch.sigmoid(x @ lin.weight.T + lin.bias)
        s = (x @ m.attention.dense.weight.T + m.attention.dense.bias).squeeze(-1)
        s = s.masked_fill(profile == 0, 0.0) / (m.embedding_size ** 0.5)
        scores.append((s * (k * q).sum(-1)).sum(-1))
    return -torch.log((scores[0] - scores[1]).sigmoid() + 1e-8).mean()


def side(data, batches, store, torch_ops):
    from pixelrec_amd import model
    from pixelrec_amd.optim import OptimizerGroup, PxrAdamW, VisualAdamW

    cls = model.MODIN
    if torch_ops:
        class cls(model.MODIN):
            def loss_from_embeddings(self, E, profile_idx, target_idx):
                self._ensure_packed()
                return torch_head(self, E, profile_idx, target_idx)
    torch.manual_seed(0)
    m = cls(config(), data).cuda().train()
    opt = OptimizerGroup(VisualAdamW(m.visual_encoder, lr=ARGS["modal_lr"], weight_decay=ARGS["modal_decay"]),
                         PxrAdamW(m, lr=ARGS["rec_lr"], weight_decay=ARGS["rec_decay"]))
    it = iter(range(1 << 30))
    one = torch.ones((), device="cuda")

    def step():
        index, image_ids = batches[next(it) % len(batches)]
        if torch_ops:
            m.flat_parameters()[1].zero_()                           # autograd accumulates into the flat gradient views
        loss = m(m.modal_inputs(store, (index, image_ids)))
        loss.backward(one)
        opt.step()

    return step, m


def eval_times(m, items, sizes, predict_users, reps):
    from lightgcn_bench import timed
    from pixelrec_amd import ops

    g = torch.Generator().manual_seed(3)
    feat = (torch.randn(items, D, generator=g) * 0.3).cuda()
    feat[0] = 0.1
    m.eval()
    m.set_item_feature(feat)
    out = {}
    for B in sizes:
        win = torch.randint(1, items, (B, L), generator=g)
        win[torch.arange(L)[None, :] < torch.randint(0, L, (B, 1), generator=g)] = 0
        hu = torch.arange(B).repeat_interleave(L)[win.view(-1) != 0]
        hi = win.view(-1)[win.view(-1) != 0]
        ptr, hist = ops.history_csr(hu, hi, B, "cuda")
        wd = win.cuda()
        fused = timed(lambda: m.fused_topk_batch(wd, ptr, hist, K), reps, warm=2)
        nb = min(B, predict_users)
        wsmall = wd[:nb].contiguous()
        husm = hu[hu < nb].cuda()
        hism = hi[hu < nb].cuda()

        def chunked():
            s = m.predict(wsmall, feat)
            s[:, 0] = float("-inf")
            s[(husm, hism)] = float("-inf")
            return torch.topk(s, K, dim=-1).indices

        pred = timed(chunked, max(1, reps // 2), warm=1) * (B / nb)
        out[str(B)] = {"fused_ms": round(fused, 3), "chunked_predict_ms": round(pred, 3), "chunked_predict_users_timed": nb,
                       "chunked_over_fused": round(pred / fused, 2)}
        print("eval", B, json.dumps(out[str(B)]))
    m.train()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--chunks", type=int, default=256)
    ap.add_argument("--predict-users", type=int, default=64)
    ap.add_argument("--eval-reps", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from lightgcn_bench import timed
    from pixelrec_amd.data.dataset import MoTowerTrainBatcher
    from pixelrec_amd.data.images import ImageStore

    data = _Data(a.items, a.chunks)
    host = list(MoTowerTrainBatcher(config(), data))
    res = {"shape": {"encoder": "clip-vit-base-patch32", "tune_scale": 165, "D": D, "hidden": HIDDEN, "L": L, "batch": BATCH,
                     "image": IMAGE, "items": a.items, "steps": a.steps, "rounds": a.rounds},
           "images_per_step": {"batch_dedup": round(float(np.mean([len(i) for _, i in host])), 1),
                               "per_position": round(float(np.mean([x.shape[0] * (L + 2) for x, _ in host])), 1),
                               "samples": round(float(np.mean([x.shape[0] for x, _ in host])), 1)}}
    print(json.dumps(res["images_per_step"]))
    batches = [(x.cuda(), i.cuda()) for x, i in host]
    store = ImageStore.synthetic(a.items, IMAGE, 0, "cuda")
    built = {"native": side(data, batches, store, False), "torch_head": side(data, batches, store, True)}
    ms = {k: [] for k in built}
    for r in range(a.rounds):
        for k, (fn, _) in built.items():
            ms[k].append(timed(fn, a.steps, warm=2 if r == 0 else 0))
    res["MODIN"] = {k + "_ms": round(statistics.median(v), 3) for k, v in ms.items()}
    res["MODIN"]["rounds_ms"] = {k: [round(x, 3) for x in v] for k, v in ms.items()}
    res["MODIN"]["torch_head_over_native"] = round(res["MODIN"]["torch_head_ms"] / res["MODIN"]["native_ms"], 4)
    print("MODIN", json.dumps(res["MODIN"]))
    res["eval"] = eval_times(built["native"][1], a.items, (64, 256, 1024), a.predict_users, a.eval_reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
