"""Captured training-step time of BERT4Rec next to SASRec at the same shape: 400 001-item catalogue, D = 512, 4 heads, FFN 2x, 2 layers,
dropout 0.1, B = 64, MAX_ITEM_LIST_LENGTH = 50 (BERT4Rec encodes 51 positions; mask_ratio 0.6).  Both steps are replayed from a
hipGraph (graph.GraphedTrainStep), like bench.py; ids follow the Zipf synthetic catalogue (pixelrec_amd/synth.py), BERT4Rec's batches
are masked by data/dataset.py BERT4RecTrainBatcher.
usage (on an MI355X): python tools/bert4rec_bench.py [--only bert4rec|sasrec] [--steps 200] [--out bert4rec_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pixelrec_amd import synth
from pixelrec_amd.data.dataset import BERT4RecTrainBatcher
from pixelrec_amd.graph import GraphedTrainStep
from pixelrec_amd.model import BERT4Rec, SASRec
from pixelrec_amd.optim import PxrAdamW
from pixelrec_amd.parallel import DataParallel

N, B, L, D = 400001, 64, 50, 512
CFG = {"n_layers": 2, "n_heads": 4, "embedding_size": D, "inner_size": 2, "hidden_dropout_prob": 0.1, "attn_dropout_prob": 0.1,
       "hidden_act": "gelu", "layer_norm_eps": 1e-12, "initializer_range": 0.02, "MAX_ITEM_LIST_LENGTH": L, "seed": 2020,
       "mask_ratio": 0.6, "train_batch_size": B, "device_sampler": None}


class _DL:
    item_num = N


def _batches(name, n):
    rng = np.random.default_rng(1)
    zipf = synth.ZipfItems(N, seed=2020)
    sas = [synth.train_batch(N, B, L, rng, zipf) for _ in range(n)]
    if name == "SASRec":
        return [tuple(torch.from_numpy(a).cuda() for a in b) for b in sas]
    # the same windows, masked like the host batcher does
    dl = _DL()
    dl.train_feat = {"item_seq": [w[w != 0] for b in sas for w in b[0][:, 0]]}
    tb = BERT4RecTrainBatcher(CFG, dl)
    return [tuple(torch.from_numpy(a).cuda() for a in tb.make_batch(np.arange(i * B, (i + 1) * B), rng)) for i in range(n)]


def run(name, steps, warm=20):
    torch.manual_seed(0)
    m = (SASRec if name == "SASRec" else BERT4Rec)(CFG, _DL()).cuda().train()
    opt = PxrAdamW(m, lr=1e-4, weight_decay=0.1)
    batches = _batches(name, 32)
    g = GraphedTrainStep(DataParallel(m), opt, *batches[0])
    for i in range(warm):
        g(*batches[i % len(batches)])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        g(*batches[i % len(batches)])
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    r = {"model": name, "items": N, "embedding_size": D, "batch": B, "MAX_ITEM_LIST_LENGTH": L,
         "positions": L + (name == "BERT4Rec"), "steps": steps, "ms_per_step": round(ms, 4),
         "sequences_per_s": round(B / ms * 1e3, 1), "final_loss": float(g.loss)}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("bert4rec", "sasrec"), default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    names = [n for n in ("SASRec", "BERT4Rec") if a.only in (None, n.lower())]
    out = []
    for n in names:
        out.append(run(n, a.steps))
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
