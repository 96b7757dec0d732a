"""SRGNN training-step time at the shipped shape (configs/IDNet/srgnn.yaml + overall/ID.yaml: D = 512, step = 2, L = 10, B = 64)
on a 400 001-item table, and at B = 512 and 2048.

  native: model/srgnn.py + PxrAdamW (lazy table), the whole step -- graph build included -- replayed from a hipGraph;
  torch:  a restatement of the reference's forward (GNN cell, readout, pair loss), autograd backward and torch.optim.AdamW on
          the same GPU, issued eagerly, with the session graphs prebuilt (alias, A, items of the same batches);
  host:   GraphTrainBatcher.make_batch (samples/s) against a per-sample restatement of the reference collate's loop (np.unique,
          the edge walk, the degree normalisation per session), both on the host.

Sessions: 0..10 Zipf-drawn history items per sample (right-padded), targets and negatives uniform.
usage (on an MI355X): python tools/srgnn_bench.py [--steps 100] [--out srgnn_bench.json] [--quick] [--native-only]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pixelrec_amd import ops
from pixelrec_amd.graph import GraphedTrainStep
from pixelrec_amd.model import SRGNN
from pixelrec_amd.optim import PxrAdamW

N_ITEMS, D, L, STEP = 400_001, 512, 10, 2


def sessions(rng, B, n_items=N_ITEMS):
    ranks = np.arange(1, n_items, dtype=np.float64)
    cdf = np.cumsum(1.0 / ranks ** 1.1); cdf /= cdf[-1]
    seq = 1 + np.minimum(np.searchsorted(cdf, rng.random((B, L))), n_items - 2)
    lens = rng.integers(1, L + 1, size=B)
    seq[np.arange(L)[None, :] >= lens[:, None]] = 0
    mask = (seq != 0).astype(np.int64)
    tgt = rng.integers(1, n_items, size=(B, 2))
    return seq.astype(np.int64), mask, tgt.astype(np.int64)


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
    m = SRGNN({"embedding_size": D, "step": STEP, "MAX_ITEM_LIST_LENGTH": L}, type("D", (), {"item_num": N_ITEMS})()).cuda().train()
    opt = PxrAdamW(m, lr=1e-4, weight_decay=0.1)
    batches = []
    for _ in range(8):
        seq, mask, tgt = sessions(rng, B)
        batches.append((torch.from_numpy(seq).cuda(), torch.from_numpy(np.concatenate([mask, tgt], 1)).cuda()))
    gs = GraphedTrainStep(m, opt, *batches[0], warmup=0)
    k = [0]

    def one():
        gs(*batches[k[0] % 8])
        k[0] += 1
    ms = timed(one, steps)
    ops.raise_on_bad_indices()
    return ms


class TorchSRGNN(torch.nn.Module):
    """The reference arithmetic (srgnn.py) in plain torch, graphs given."""

    def __init__(self):
        super().__init__()
        lin = torch.nn.Linear
        self.embedding = torch.nn.Embedding(N_ITEMS, D)
        self.w_ih = torch.nn.Parameter(torch.empty(3 * D, 2 * D)); self.w_hh = torch.nn.Parameter(torch.empty(3 * D, D))
        self.b_ih = torch.nn.Parameter(torch.empty(3 * D)); self.b_hh = torch.nn.Parameter(torch.empty(3 * D))
        self.b_iah = torch.nn.Parameter(torch.empty(D)); self.b_oah = torch.nn.Parameter(torch.empty(D))
        self.e_in, self.e_out, self.e_f = lin(D, D), lin(D, D), lin(D, D)
        self.l1, self.l2, self.l3, self.lt = lin(D, D), lin(D, D), lin(D, 1, bias=False), lin(2 * D, D)
        for w in self.parameters():
            w.data.uniform_(-D ** -0.5, D ** -0.5)

    def forward(self, alias, A, items, mask, targets):
        h = self.embedding(items)
        n = A.shape[1]
        for _ in range(STEP):
            x = torch.cat([A[:, :, :n] @ self.e_in(h) + self.b_iah, A[:, :, n:] @ self.e_out(h) + self.b_oah], 2)
            gi = torch.nn.functional.linear(x, self.w_ih, self.b_ih)
            gh = torch.nn.functional.linear(h, self.w_hh, self.b_hh)
            ir, ii, in_ = gi.chunk(3, 2)
            hr, hi, hn = gh.chunk(3, 2)
            r, z = torch.sigmoid(ir + hr), torch.sigmoid(ii + hi)
            ng = torch.tanh(in_ + r * hn)
            h = ng + z * (h - ng)
        sh = torch.gather(h, 1, alias.unsqueeze(-1).expand(-1, -1, D))
        ht = sh[torch.arange(mask.shape[0], device=mask.device), mask.sum(1) - 1]
        alpha = self.l3(torch.sigmoid(self.l1(ht)[:, None] + self.l2(sh)))
        a = self.lt(torch.cat([(alpha * sh * mask[..., None].float()).sum(1), ht], 1))
        s = (a[:, None] * self.embedding(targets)).sum(-1)
        return -torch.mean(1e-8 + torch.log(torch.sigmoid(s[:, 0] - s[:, 1])))


def torch_step_ms(B, steps, rng):
    m = TorchSRGNN().cuda()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=0.1)
    batches = []
    for _ in range(8):
        seq, mask, tgt = sessions(rng, B)
        g = ops.srgnn_graph(torch.from_numpy(seq).cuda(), N_ITEMS)
        batches.append((g["alias"].long(), g["A"], g["nodes"], torch.from_numpy(mask).cuda(), torch.from_numpy(tgt).cuda()))
    k = [0]

    def one():
        opt.zero_grad()
        m(*batches[k[0] % 8]).backward()
        opt.step()
        k[0] += 1
    return timed(one, steps, warm=3)


def collate_loop(seqs):
    """Per-sample restatement of the reference collate's session-graph loop (host)."""
    n_max = max(len(np.unique(s)) for s in seqs)
    out = []
    for s in seqs:
        node = np.unique(s)
        adj = np.zeros((n_max, n_max))
        for i in range(len(s) - 1):
            if s[i + 1] == 0:
                break
            adj[np.where(node == s[i])[0][0], np.where(node == s[i + 1])[0][0]] = 1
        si = adj.sum(0); si[si == 0] = 1
        so = adj.sum(1); so[so == 0] = 1
        A = np.concatenate([adj / si, adj.T / so]).T
        out.append((node, A, [np.where(node == i)[0][0] for i in s]))
    return out


def host_rates(B=64, reps=50):
    from pixelrec_amd.data.dataset import GraphTrainBatcher

    rng = np.random.default_rng(1)
    n_users = 20000
    lens = rng.integers(3, L + 2, size=n_users)
    flat = rng.integers(1, N_ITEMS, size=int(lens.sum())).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    k = lens - 1
    dl = type("DL", (), {"item_num": N_ITEMS, "_sorted_items": flat,
                         "train_feat": {"seq_start": np.repeat(starts, k), "seq_len": np.concatenate([np.arange(2, n + 1) for n in lens])}})()
    bt = GraphTrainBatcher({"MAX_ITEM_LIST_LENGTH": L, "train_batch_size": B, "seed": 0}, dl)
    idx = bt._indices()
    t0 = time.perf_counter()
    for r in range(reps):
        seq, _, _ = bt.make_batch(idx[r * B:(r + 1) * B], rng)
    t_batcher = (time.perf_counter() - t0) / (reps * B)
    t0 = time.perf_counter()
    for r in range(reps):
        seq, _, _ = bt.make_batch(idx[r * B:(r + 1) * B], rng)
        collate_loop(list(seq))
    t_ref = (time.perf_counter() - t0) / (reps * B) - t_batcher
    return 1.0 / t_batcher, 1.0 / t_ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="B = 64 only")
    ap.add_argument("--native-only", action="store_true", help="no torch restatement, no host rates (a profiler run)")
    a = ap.parse_args()
    rng = np.random.default_rng(2020)
    res = {"shape": {"n_items": N_ITEMS, "D": D, "L": L, "step": STEP}, "device": torch.cuda.get_device_name(0), "native": {},
           "torch": {}}
    for B in ((64,) if a.quick else (64, 512, 2048)):
        ms = native_step_ms(B, a.steps, rng)
        res["native"][B] = {"ms_per_step": round(ms, 4), "seq_per_s": round(B / ms * 1e3, 1)}
        if not a.native_only:
            tms = torch_step_ms(B, max(10, a.steps // 5), rng)
            res["torch"][B] = {"ms_per_step": round(tms, 4), "seq_per_s": round(B / tms * 1e3, 1)}
        print(json.dumps({"B": B, "native": res["native"][B], "torch": res["torch"].get(B)}), flush=True)
    if not a.native_only:
        hb, hr = host_rates()
        res["host_samples_per_s"] = {"GraphTrainBatcher": round(hb, 1), "collate_loop_restatement": round(hr, 1)}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
