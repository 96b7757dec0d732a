"""MOMF training-step time at the shipped shape (configs/PixelNet/mf.yaml with overall/ViT.yaml: clip-vit-base-patch32, tune_scale
165, embedding_size 4096, identity towers, train_batch_size 16, synthetic 224 x 224 images, a `--users`-row user table -- 200 001
as shipped) over a synthetic catalogue of `--items` items with a long-tailed popularity and `--pairs` interactions, batched by
MoPairTrainBatcher.

  dedup:         model/momf.py on the batcher's batches -- each distinct image of a batch encoded once;
  per_position:  the SAME model and optimizer objects fed the reference's own input form, one image per position (2B per batch).
Both are the native step (native tower, pxr_mf_pair_fwd_eps_f32, pxr_momf_pair_grad_f32, native tower backward,
OptimizerGroup(VisualAdamW, PxrAdamW) with the lazy user table) in one process on the same batches, alternating: `--rounds` rounds
of `--steps` steps each; a side's figure is the median over the rounds.  The weights are random (no checkpoint is read): the time
does not depend on them.  Also counted over the epoch's batches: images encoded per step both ways.

The gradient kernel alone, at one batch of the shape: pxr_momf_pair_grad_f32 in the head's mode against the route through kernels
that already exist -- materialise occ [3B, D] with torch ops (two gathers of E, one of the user table, the scaled difference and
the two signed copies), then the same entry in occ mode.
usage (on an MI355X): python tools/momf_bench.py [--steps 10] [--rounds 3] [--out profiles/momf/momf_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

D, BATCH, IMAGE = 4096, 16, 224
ARGS = {"modal_lr": 1e-4, "rec_lr": 1e-4, "modal_decay": 0.0, "rec_decay": 0.1}


class _Data:
    def __init__(self, U, I, n_pairs, seed=1):
        rng = np.random.default_rng(seed)
        self.user_num, self.item_num = U, I
        p = 1.0 / np.arange(1, I) ** 1.0                               # a long tail: popular items repeat inside a batch
        self.train_feat = {"user_id": rng.integers(0, U, size=n_pairs), "item_id": rng.choice(np.arange(1, I), size=n_pairs, p=p / p.sum())}


def config():
    return {"model": "MOMF", "embedding_size": D, "mlp_hidden_size": [], "dropout_prob": 0, "seed": 2020, "train_batch_size": BATCH,
            "encoder_name": "clip-vit-base-patch32", "encoder_source": "transformers", "pretrain_path": None, "encoder_path": None,
            "fine_tune_arg": {"tune_scale": 165, "pre_trained": True, "activation": "relu", "dnn_layers": [], "method": "mean",
                              "allow_random_backbone": True}}


def kernel_times(B, M, U, reps):
    from lightgcn_bench import timed
    from pixelrec_amd import ops

    g = torch.Generator().manual_seed(5)
    utable = (torch.randn(1 + U, D, generator=g) * 0.02).cuda()
    E = (torch.randn(M, D, generator=g) * 0.1).cuda()
    user = torch.randint(0, U, (B,), generator=g).cuda()
    index = torch.randint(0, M, (B, 2), generator=g)
    index[:, 1] = torch.where(index[:, 1] == index[:, 0], (index[:, 0] + 1) % M, index[:, 1])
    index = index.cuda()
    rows = ops.momf_pair_rows(user, index, U, M)
    _, coef = ops.mf_pair_fwd(utable, E, B, rows=rows, eps=0.0)
    sp = ops.SparseRows(B, D, "cuda")
    dE = torch.empty(M, D, device="cuda")
    occ = torch.empty(3 * B, D, device="cuda")

    def fused():
        ops.momf_pair_grad(rows, B, sp, M, utable=utable, E=E, coef=coef, out=dE)

    def materialised():
        u = utable[rows[:B]]
        cu = coef[:, None] * u
        occ[:B] = coef[:, None] * (E[index[:, 0]] - E[index[:, 1]])
        occ[B:].view(B, 2, D)[:, 0] = cu
        occ[B:].view(B, 2, D)[:, 1] = -cu
        ops.momf_pair_grad(rows, B, sp, M, occ=occ, out=dE)

    f, t = timed(fused, reps, warm=5), timed(materialised, reps, warm=5)
    return {"B": B, "M": M, "D": D, "pxr_momf_pair_grad_us": round(1e3 * f, 2), "materialised_occ_route_us": round(1e3 * t, 2),
            "materialised_over_kernel": round(t / f, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--users", type=int, default=200001)
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from lightgcn_bench import timed
    from pixelrec_amd import model
    from pixelrec_amd.data.dataset import MoPairTrainBatcher
    from pixelrec_amd.data.images import ImageStore
    from pixelrec_amd.optim import OptimizerGroup, PxrAdamW, VisualAdamW

    data = _Data(a.users, a.items, a.pairs)
    host = list(MoPairTrainBatcher(config(), data))
    res = {"shape": {"encoder": "clip-vit-base-patch32", "tune_scale": 165, "D": D, "hidden": [], "batch": BATCH, "image": IMAGE,
                     "users": a.users, "items": a.items, "steps": a.steps, "rounds": a.rounds},
           "images_per_step": {"batch_dedup": round(float(np.mean([len(i) for _, _, i in host])), 2),
                               "per_position": round(float(np.mean([2 * u.shape[0] for u, _, _ in host])), 2),
                               "samples": round(float(np.mean([u.shape[0] for u, _, _ in host])), 2)}}
    print(json.dumps(res["images_per_step"]))
    batches = [tuple(t.cuda() for t in b) for b in host]
    store = ImageStore.synthetic(a.items, IMAGE, 0, "cuda")
    torch.manual_seed(0)
    m = model.MOMF(config(), data).cuda().train()
    opt = OptimizerGroup(VisualAdamW(m.visual_encoder, lr=ARGS["modal_lr"], weight_decay=ARGS["modal_decay"]),
                         PxrAdamW(m, lr=ARGS["rec_lr"], weight_decay=ARGS["rec_decay"]))
    one = torch.ones((), device="cuda")
    its = {k: iter(range(1 << 30)) for k in ("dedup", "per_position")}

    def step(kind):
        user, index, image_ids = batches[next(its[kind]) % len(batches)]
        if kind == "dedup":
            inp = m.modal_inputs(store, (user, index, image_ids))
        else:
            inp = (user, store.batch(image_ids[index].view(-1)).view(user.shape[0], 2, 3, IMAGE, IMAGE))    # momf.py:51's form
        loss = m(inp)
        loss.backward(one)
        opt.step()

    ms = {k: [] for k in its}
    for r in range(a.rounds):
        for k in its:
            ms[k].append(timed(lambda: step(k), a.steps, warm=2 if r == 0 else 0))
    res["MOMF"] = {k + "_ms": round(statistics.median(v), 3) for k, v in ms.items()}
    res["MOMF"]["rounds_ms"] = {k: [round(x, 3) for x in v] for k, v in ms.items()}
    res["MOMF"]["per_position_over_dedup"] = round(res["MOMF"]["per_position_ms"] / res["MOMF"]["dedup_ms"], 4)
    print("MOMF", json.dumps(res["MOMF"]))
    M = int(round(res["images_per_step"]["batch_dedup"]))
    res["grad_kernel"] = kernel_times(BATCH, M, min(a.users, 4096), a.kernel_reps)
    print("grad kernel", json.dumps(res["grad_kernel"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
