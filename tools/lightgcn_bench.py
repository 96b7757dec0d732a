"""LightGCN training-step time on the Pixel200K-shaped synthetic graph (tools/synth_dataset.py's distribution: 200 K users, 96 K
items with a Zipf popularity tail, 5..40 interactions per user, all but the last two of each user train: ~4.1 M pairs, ~8.2 M
directed edges), D = 256, K = 1 (configs/IDNet/lightgcn.yaml), at B = 64 (overall/ID.yaml) and B = 2048.

  native: model/lightgcn.py + PxrAdamW, the whole step replayed from a hipGraph (graph.GraphedTrainStep);
  torch:  a restatement on the same GPU -- E_{k+1} = zeros.index_add_(0, dst, w * E_k[src]) (what the reference's PyG
          propagate does), the same loss under autograd, torch.optim.AdamW -- issued eagerly.

Per SpMM launch (one forward, one backward at K = 1, timed alone with events): gathered bytes/s counts every neighbour row read
(nnz * D * 4 + CSR), compulsory bytes/s what a perfect cache would move (x, acc_in and the output once, plus the CSR).
usage (on an MI355X): python tools/lightgcn_bench.py [--steps 100] [--out lightgcn_bench.json] [--quick]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pixelrec_amd import ops
from pixelrec_amd.data.dataload import norm_adj_csr
from pixelrec_amd.graph import GraphedTrainStep
from pixelrec_amd.model import LightGCN
from pixelrec_amd.optim import PxrAdamW

D, K = 256, 1


def synth_train(n_users=200_000, n_items=96_000, seed=2020):
    """(train users, train items, user_num, item_num) with ids as the data layer makes them: 1-based, 0 = [PAD]."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(5, 41, size=n_users)
    ranks = np.arange(1, n_items + 1, dtype=np.float64)
    cdf = np.cumsum(1.0 / ranks); cdf /= cdf[-1]
    keep = lens - 2
    users = np.repeat(np.arange(1, n_users + 1), keep)
    items = 1 + rng.permutation(n_items)[np.minimum(np.searchsorted(cdf, rng.random(int(keep.sum()))), n_items - 1)]
    return users.astype(np.int64), items.astype(np.int64), n_users + 1, n_items + 1


class _Data:
    def __init__(self, U, I, csr):
        self.user_num, self.item_num, self._csr = U, I, csr

    def get_norm_adj_csr(self):
        return self._csr


def batches(tu, ti, I, B, n, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        r = rng.integers(0, len(tu), size=B)
        out.append((torch.from_numpy(tu[r]).cuda(), torch.from_numpy(np.stack([ti[r], rng.integers(1, I, size=B)], 1)).cuda()))
    return out


def timed(fn, steps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def native_step_ms(data, bs, steps):
    torch.manual_seed(0)
    m = LightGCN({"embedding_size": D, "n_layers": K}, data).cuda().train()
    opt = PxrAdamW(m, lr=1e-4, weight_decay=0.1)
    g = GraphedTrainStep(m, opt, *bs[0], warmup=0)
    it = iter(range(1 << 30))
    ms = timed(lambda: g(*bs[next(it) % len(bs)]), steps)
    return ms, float(g.loss), m


def spmm_rates(m, steps):
    """(forward ms, backward ms, gathered B/s, compulsory B/s) of the K = 1 SpMM launches."""
    gr = m._graph
    N = gr.n_rows
    e0 = m._table(m.flat_parameters()[0])
    out, gin = torch.empty_like(e0), torch.randn_like(e0)
    fwd = timed(lambda: m.propagate(e0, out), steps)
    bwd = timed(lambda: m.propagate_grad(gin, out), steps)
    csr = gr.nnz * 8 + (N + 1) * 8
    gathered = gr.nnz * D * 4 + csr
    compulsory = 3 * N * D * 4 + csr                      # x (= acc_in here) read, acc_in read, output written
    rate = lambda ms, b: round(b / (ms * 1e-3) / 1e12, 3)
    return {"spmm_fwd_ms": round(fwd, 4), "spmm_bwd_ms": round(bwd, 4),
            "spmm_fwd_gathered_TBps": rate(fwd, gathered), "spmm_fwd_compulsory_TBps": rate(fwd, compulsory),
            "spmm_bwd_gathered_TBps": rate(bwd, gathered), "spmm_bwd_compulsory_TBps": rate(bwd, compulsory),
            "gathered_GB": round(gathered / 1e9, 3), "compulsory_GB": round(compulsory / 1e9, 3)}


def torch_step_ms(tu, ti, U, I, bs, steps):
    """The reference's arithmetic in plain torch on the same GPU (index_add_ propagation, autograd, torch.optim.AdamW)."""
    dev = "cuda"
    src = torch.from_numpy(np.concatenate([tu, ti + U])).to(dev)
    dst = torch.from_numpy(np.concatenate([ti + U, tu])).to(dev)
    deg = torch.bincount(src, minlength=U + I).float()
    nd = 1.0 / torch.sqrt(torch.where(deg == 0, torch.ones_like(deg), deg))
    w = (nd[src] * nd[dst]).view(-1, 1)
    torch.manual_seed(0)
    ue = torch.nn.Parameter(torch.nn.init.xavier_normal_(torch.empty(U, D, device=dev)))
    ie = torch.nn.Parameter(torch.nn.init.xavier_normal_(torch.empty(I, D, device=dev)))
    opt = torch.optim.AdamW([ue, ie], lr=1e-4, weight_decay=0.1)
    wt = torch.tensor([[1.0], [-1.0]], device=dev)
    it = iter(range(1 << 30))

    def step():
        user, item = bs[next(it) % len(bs)]
        e = torch.cat([ue, ie])
        embs = [e]
        for _ in range(K):
            e = torch.zeros_like(e).index_add_(0, dst, w * e[src])
            embs.append(e)
        ef = torch.stack(embs, 1).mean(1)
        uf, itf = ef[:U], ef[U:]
        score = (uf[user].unsqueeze(1) * itf[item]).sum(-1).view(-1, 2)
        loss = -torch.mean(1e-8 + torch.log(torch.sigmoid(score @ wt)))
        opt.zero_grad()
        loss.backward()
        opt.step()

    return timed(step, steps, warm=3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="B = 64 native only, few steps (for a profiler run)")
    a = ap.parse_args()
    tu, ti, U, I = synth_train()
    csr = norm_adj_csr(tu, ti, U, I)
    data = _Data(U, I, csr)
    res = {"users": U, "items": I, "train_pairs": len(tu), "edges": len(csr[1]), "max_degree": int(np.diff(csr[0]).max()),
           "embedding_size": D, "n_layers": K, "part_len": ops.LgcnGraph.PART_LEN, "runs": []}
    for B in ((64,) if a.quick else (64, 2048)):
        bs = batches(tu, ti, I, B, 32)
        steps = 10 if a.quick else a.steps
        ms, loss, m = native_step_ms(data, bs, steps)
        r = {"batch": B, "native_ms_per_step": round(ms, 4), "native_final_loss": loss}
        if not a.quick:
            r.update(spmm_rates(m, steps) if B == 64 else {})
            del m
            torch.cuda.empty_cache()
            r["torch_ms_per_step"] = round(torch_step_ms(tu, ti, U, I, bs, max(10, steps // 5)), 4)
        res["runs"].append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    ops.raise_on_bad_indices()
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
