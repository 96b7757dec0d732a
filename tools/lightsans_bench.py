"""LightSANs training-step time at the shipped shape (configs/IDNet/lightsans.yaml + overall/ID.yaml: D = 512, H = 4, K = 3,
n_layers = 1, inner 2, L = 10, dropout 0.1 / 0.1, B = 64) on a 400 001-item table, and at B = 512 and 2048.

  native: model/lightsans.py + PxrAdamW (lazy table), the whole step replayed from a hipGraph;
  torch:  the float64 restatement's arithmetic (tests/lightsans_restate.py) in fp32 on the same GPU -- autograd backward,
          torch.optim.AdamW over every parameter (the reference's dense table update), issued eagerly, no dropout masks.

Rows: 1..11 Zipf-drawn items per sequence (left-padded to L + 2 with the last one the positive), negatives uniform.
usage (on an MI355X): python tools/lightsans_bench.py [--steps 100] [--out lightsans_bench.json] [--quick] [--native-only]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pixelrec_amd import ops
from pixelrec_amd.graph import GraphedTrainStep
from pixelrec_amd.model import LightSANs
from pixelrec_amd.optim import PxrAdamW
from tests import lightsans_restate as R

N_ITEMS, D, H, K, L, N_LAYERS = 400_001, 512, 4, 3, 10, 1
CFG = {"n_layers": N_LAYERS, "n_heads": H, "embedding_size": D, "inner_size": 2, "k_interests": K, "hidden_dropout_prob": 0.1,
       "attn_dropout_prob": 0.1, "hidden_act": "gelu", "layer_norm_eps": 1e-12, "initializer_range": 0.02,
       "MAX_ITEM_LIST_LENGTH": L, "seed": 2020}


def rows(rng, B):
    ranks = np.arange(1, N_ITEMS, dtype=np.float64)
    cdf = np.cumsum(1.0 / ranks ** 1.1); cdf /= cdf[-1]
    seq = 1 + np.minimum(np.searchsorted(cdf, rng.random((B, L + 1))), N_ITEMS - 2)
    lens = rng.integers(1, L + 2, size=B)
    seq[np.arange(L + 1)[None, :] < (L + 1 - lens)[:, None]] = 0
    neg = rng.integers(1, N_ITEMS, size=(B, 1))
    return np.concatenate([seq, neg], 1).astype(np.int64)


def timed(fn, steps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def native_step_ms(B, steps, rng):
    m = LightSANs(CFG, type("D", (), {"item_num": N_ITEMS})()).cuda().train()
    opt = PxrAdamW(m, lr=1e-4, weight_decay=0.1)
    batches = []
    for _ in range(8):
        it = torch.from_numpy(rows(rng, B)).cuda()
        batches.append((it[:, :L].contiguous(), it[:, L:].contiguous()))
    gs = GraphedTrainStep(m, opt, *batches[0], warmup=0)
    k = [0]

    def one():
        gs(*batches[k[0] % 8])
        k[0] += 1
    ms = timed(one, steps)
    ops.raise_on_bad_indices()
    return ms


def torch_step_ms(B, steps, rng):
    torch.manual_seed(0)
    sd = LightSANs(dict(CFG, hidden_dropout_prob=0.0, attn_dropout_prob=0.0), type("D", (), {"item_num": N_ITEMS})()).state_dict()
    P = {k: v.cuda().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.AdamW(list(P.values()), lr=1e-4, weight_decay=0.1)
    batches = [torch.from_numpy(rows(rng, B)).cuda() for _ in range(8)]
    k = [0]

    def one():
        opt.zero_grad()
        R.loss_fn(P, batches[k[0] % 8], N_LAYERS, H, K).backward()
        opt.step()
        k[0] += 1
    return timed(one, steps, warm=3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="B = 64 only")
    ap.add_argument("--native-only", action="store_true", help="no torch restatement (a profiler run)")
    a = ap.parse_args()
    rng = np.random.default_rng(2020)
    res = {"shape": {"n_items": N_ITEMS, "D": D, "H": H, "K": K, "L": L, "n_layers": N_LAYERS, "inner": 2 * D, "dropout": [0.1, 0.1]},
           "device": torch.cuda.get_device_name(0), "native": {}, "torch": {}}
    for B in ((64,) if a.quick else (64, 512, 2048)):
        ms = native_step_ms(B, a.steps, rng)
        res["native"][B] = {"ms_per_step": round(ms, 4), "seq_per_s": round(B / ms * 1e3, 1)}
        if not a.native_only:
            tms = torch_step_ms(B, max(10, a.steps // 5), rng)
            res["torch"][B] = {"ms_per_step": round(tms, 4), "seq_per_s": round(B / tms * 1e3, 1)}
        print(json.dumps({"B": B, "native": res["native"][B], "torch": res["torch"].get(B)}), flush=True)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
