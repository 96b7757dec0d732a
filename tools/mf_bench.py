"""MF training-step time at the Pixel200K shape of tools/synth_dataset.py (200 K users, 96 K items, Zipf item popularity; the
training pairs of tools/lightgcn_bench.synth_train), D = 4096 (configs/IDNet/mf.yaml), at B = 64 (overall/ID.yaml) and B = 2048,
with mlp_hidden_size [] (the shipped config) and [1024, 256].

  native: model/mf.py + PxrAdamW (lazy table rows), the whole step replayed from a hipGraph (graph.GraphedTrainStep);
  torch:  a restatement of the reference's MF on the same GPU -- two dense nn.Embedding tables, MLPLayers towers, the same loss
          under autograd, torch.optim.AdamW over every parameter (every row of both tables, every step) -- issued eagerly.
The two run in the same process and alternate: `--rounds` rounds of `--steps` native steps then `--steps` torch steps; each
side's figure is the median over the rounds.  Also timed: one fused top-k evaluation batch of 1024 users (encode_last +
pxr_score_topk_f32, K = 10, no history mask) after compute_item_all, and compute_item_all itself.
usage (on an MI355X): python tools/mf_bench.py [--steps 20] [--rounds 3] [--out profiles/mf/mf_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from lightgcn_bench import synth_train, timed
from pixelrec_amd import ops
from pixelrec_amd.graph import GraphedTrainStep
from pixelrec_amd.model import MF
from pixelrec_amd.optim import PxrAdamW

D = 4096


class _Data:
    def __init__(self, U, I):
        self.user_num, self.item_num = U, I


def batches(tu, ti, I, B, n, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        r = rng.integers(0, len(tu), size=B)
        out.append((torch.from_numpy(tu[r]).cuda(), torch.from_numpy(np.stack([ti[r], rng.integers(1, I, size=B)], 1)).cuda()))
    return out


def native(U, I, hidden, bs):
    torch.manual_seed(0)
    m = MF({"embedding_size": D, "mlp_hidden_size": hidden, "dropout_prob": 0.0}, _Data(U, I)).cuda().train()
    opt = PxrAdamW(m, lr=1e-4, weight_decay=0.1)
    g = GraphedTrainStep(m, opt, *bs[0], warmup=0)
    it = iter(range(1 << 30))
    return m, opt, g, (lambda: g(*bs[next(it) % len(bs)]))


def torch_ref(U, I, hidden, bs):
    """The reference's MF arithmetic in plain torch: dense tables, MLPLayers towers, autograd, torch.optim.AdamW."""
    dev = "cuda"
    torch.manual_seed(0)

    def tower():
        mods, sizes = [], [D] + hidden
        for i, o in zip(sizes[:-1], sizes[1:]):
            mods += [torch.nn.Dropout(0.0), torch.nn.Linear(i, o), torch.nn.BatchNorm1d(o), torch.nn.Tanh()]
        return torch.nn.Sequential(*mods)

    mod = torch.nn.ModuleDict({"ut": tower(), "it": tower(), "ue": torch.nn.Embedding(U, D), "ie": torch.nn.Embedding(I, D)}).to(dev)
    torch.nn.init.xavier_normal_(mod["ue"].weight)
    torch.nn.init.xavier_normal_(mod["ie"].weight)
    opt = torch.optim.AdamW(mod.parameters(), lr=1e-4, weight_decay=0.1)
    wt = torch.tensor([[1.0], [-1.0]], device=dev)
    out = hidden[-1] if hidden else D
    it = iter(range(1 << 30))

    def step():
        user, item = bs[next(it) % len(bs)]
        u = mod["ut"](mod["ue"](user)).unsqueeze(1)
        i = mod["it"](mod["ie"](item).view(-1, D)).view(user.shape[0], -1, out)
        score = (u * i).sum(-1).view(-1, 2)
        loss = -torch.mean(1e-8 + torch.log(torch.sigmoid(score @ wt)))
        opt.zero_grad()
        loss.backward()
        opt.step()

    return mod, opt, step


def eval_ms(m, U, n_users=1024, reps=10):
    m.eval()
    item_ms = timed(lambda: m.compute_item_all(), 3, warm=1)
    feat = m.compute_item_all()
    users = torch.arange(1, n_users + 1, dtype=torch.int64, device="cuda") % U

    def batch():
        _, last = m.encode_last(users, feat)
        ops.score_topk(last, last.stride(0), n_users, feat, 10)

    return item_ms, timed(batch, reps, warm=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tu, ti, U, I = synth_train()
    res = {"device": torch.cuda.get_device_name(0), "users": U, "items": I, "train_pairs": len(tu), "embedding_size": D,
           "steps_per_round": a.steps, "rounds": a.rounds, "runs": [],
           "note": "every figure below was measured in this run on the device named above; ms per step are medians over rounds"}
    for hidden in ([], [1024, 256]):
        for B in (64, 2048):
            bs = batches(tu, ti, I, B, 32)
            m, opt, g, nstep = native(U, I, hidden, bs)
            tmod, topt, tstep = torch_ref(U, I, hidden, bs)
            nat, tor = [], []
            for _ in range(a.rounds):
                nat.append(timed(nstep, a.steps, warm=2))
                tor.append(timed(tstep, a.steps, warm=2))
            r = {"mlp_hidden_size": hidden, "batch": B, "native_ms_per_step": round(statistics.median(nat), 4),
                 "torch_ms_per_step": round(statistics.median(tor), 4), "native_rounds_ms": [round(x, 4) for x in nat],
                 "torch_rounds_ms": [round(x, 4) for x in tor], "native_final_loss": float(g.loss)}
            r["speedup"] = round(r["torch_ms_per_step"] / r["native_ms_per_step"], 2)
            if B == 64:
                opt.flush()
                r["compute_item_all_ms"], r["topk_eval_batch_1024_ms"] = (round(x, 4) for x in eval_ms(m, U))
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
            del m, opt, g, tmod, topt
            torch.cuda.empty_cache()
    ops.raise_on_bad_indices()
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
