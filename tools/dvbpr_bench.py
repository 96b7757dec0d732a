"""DVBPR's training step on one MI355X: the native step (im2col + library GEMMs, lazy tables, each distinct image encoded once)
against a float32 torch restatement of the reference in the same process (F.conv2d, autograd, dense nn.Embedding tables,
torch.optim.AdamW over the reference's two groups, 2B images a step), at the shipped batch (B = 16) and at B = 128.
    python tools/dvbpr_bench.py [--out profiles/dvbpr/dvbpr_bench.json] [--only native --batch 128 --steps 20]

Both sides see the same batches (a 1 / rank item popularity over `--items` items, `--users` users, synthetic 224 x 224 images in HBM).
Every shape is warmed first; the two alternate; the figure is the median of 3 rounds of `--steps` steps.  Also: compute_item per 1000
images, and the images encoded per step with and without the batch-wide dedup.  `--only native` runs the native step alone -- the
program to put behind `rocprofv3 --kernel-trace --stats --` for the per-kernel shares (a run of its own).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pixelrec_amd.model import DVBPR  # noqa: E402
from pixelrec_amd.model.cnnf import CNNF_CONVS, cnnf_flat_features  # noqa: E402
from pixelrec_amd.optim import OptimizerGroup, PxrAdamW, VisualAdamW  # noqa: E402

DEV = "cuda"


class _Data:
    def __init__(self, U, I):
        self.user_num, self.item_num = U, I


class TorchDVBPR(torch.nn.Module):
    """The reference restated: dvbpr.py's forward on torch ops, float32."""

    def __init__(self, U, I, Dh, p):
        super().__init__()
        self.convs = torch.nn.ModuleList([torch.nn.Conv2d(ci, co, (kh, kw), stride=(sh, sw)) for ci, co, kh, kw, sh, sw, _ in CNNF_CONVS])
        self.fcs = torch.nn.ModuleList([torch.nn.Linear(i, o) for i, o in ((cnnf_flat_features(), 512), (512, 512), (512, Dh))])
        self.theta_users, self.gamma_users = torch.nn.Embedding(U, Dh), torch.nn.Embedding(U, Dh)
        self.gamma_items = torch.nn.Embedding(I, Dh)
        self.p = p

    def encode(self, x):
        for conv, c in zip(self.convs, CNNF_CONVS):
            x = F.relu(conv(x))
            if c[6]:
                x = F.max_pool2d(x, 2)
        x = x.reshape(x.shape[0], -1)
        for fc in self.fcs:
            x = F.dropout(F.relu(fc(x)), self.p, self.training)
        return x

    def forward(self, user, item_id, images):
        B = user.shape[0]
        e = self.encode(images.flatten(0, 1)).view(B, 2, -1)
        s = (self.gamma_users(user)[:, None] * self.gamma_items(item_id)).sum(-1) + (self.theta_users(user)[:, None] * e).sum(-1)
        return -torch.mean(F.logsigmoid(s[:, 0] - s[:, 1]))


def batches(n, B, U, I, seed):
    rng = np.random.default_rng(seed)
    pop = 1.0 / np.arange(1, I)
    pop /= pop.sum()
    out = []
    for _ in range(n):
        user = rng.integers(0, U, size=B)
        item = 1 + rng.choice(I - 1, size=(B, 2), p=pop)
        ids, inv = np.unique(item.reshape(-1), return_inverse=True)
        out.append(tuple(torch.from_numpy(a).to(DEV) for a in (user, item, inv.reshape(B, 2), ids)))
    return out


def timed(fn, data):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for d in data:
        fn(d)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(data) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, choices=[None, "native"])
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--embedding_size", type=int, default=4096)
    ap.add_argument("--dropout", type=float, default=0.5)
    a = ap.parse_args()
    U, I, Dh = a.users, a.items, a.embedding_size // 2
    store = torch.randn(I, 3, 224, 224, device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    native = DVBPR({"embedding_size": 2 * Dh, "dropout_prob": a.dropout, "seed": 2020}, _Data(U, I)).to(DEV).train()
    nopt = OptimizerGroup(VisualAdamW(native.visual_encoder, lr=1e-4, weight_decay=0.0), PxrAdamW(native, lr=1e-4, weight_decay=0.1))

    def native_step(d):
        user, item, index, ids = d
        nopt.zero_grad()
        native((user, index, store[ids], ids)).backward()
        nopt.step()

    res = {"shape": dict(users=U, items=I, Dh=Dh, dropout=a.dropout, steps=a.steps, images="synthetic 224 x 224"), "batches": {}}
    if a.only != "native":
        ref = TorchDVBPR(U, I, Dh, a.dropout).to(DEV).train()
        enc = [p for n, p in ref.named_parameters() if n.startswith(("convs", "fcs"))]
        rec = [p for n, p in ref.named_parameters() if not n.startswith(("convs", "fcs"))]
        topt = torch.optim.AdamW([{"params": enc, "lr": 1e-4, "weight_decay": 0.0}, {"params": rec, "lr": 1e-4, "weight_decay": 0.1}])

        def torch_step(d):
            user, item, index, ids = d
            topt.zero_grad()
            ref(user, item, store[item]).backward()
            topt.step()

    for B in ([a.batch] if a.batch else [16, 128]):
        data = batches(a.steps, B, U, I, 7 + B)
        native_step(data[0]); native_step(data[1])                      # warm every shape first
        if a.only == "native":
            res["batches"][B] = {"native_ms": timed(native_step, data)}
            continue
        torch_step(data[0]); torch_step(data[1])
        nat, tor = [], []
        for _ in range(3):                                              # the two alternate
            nat.append(timed(native_step, data))
            tor.append(timed(torch_step, data))
        res["batches"][B] = {"native_ms": statistics.median(nat), "native_rounds": nat, "torch_ms": statistics.median(tor), "torch_rounds": tor,
                             "images_per_step_dedup": float(np.mean([len(d[3]) for d in data])), "images_per_step_reference": 2 * B}
    if a.only != "native":
        native.eval()
        native.compute_item(store[:100])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(0, 1000, 100):
            native.compute_item(store[s:s + 100])
        torch.cuda.synchronize()
        res["compute_item_ms_per_1000_images"] = (time.perf_counter() - t0) * 1e3
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
