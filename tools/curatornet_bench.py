"""CuratorNet training-step and evaluation time at the shipped config (configs/ViNet/curatornet.yaml: embedding_size 512,
hidden_size 2, L = 10) over the 96 001-item catalogue of tools/lightgcn_bench.synth_train (Zipf item popularity) with F = 2048
synthetic features (ResNet-50's pooled width: an assumption about RN50.npy), at B = 512 (the shipped batch) and B = 64.

  native: model/curatornet.py + PxrAdamW (one flat launch), the whole step replayed from a hipGraph;
  torch:  a float32 restatement of the reference's CuratorNet on the same GPU -- a frozen nn.Embedding of the features, five
          nn.Linear, F.selu, the two adaptive pools, the same loss under autograd, torch.optim.AdamW -- issued eagerly.  The
          baseline is this restatement, never the native code.
The two run in the same process and alternate: `--rounds` rounds of `--steps` native steps then `--steps` torch steps; each
side's figure is the median over the rounds.  Also timed: compute_item_all, one fused top-k batch of 512 users (encode_last +
pxr_score_topk_f32 with pre-split planes, K = 10, 20 history items per user) and the literal predict + masks + torch.topk for the
same batch; and recorded: the share of distinct ids among a batch's B (L + 2) gathered rows (every occurrence goes through the
common tower: de-duplicating them is not built).
`--trace-steps N`: nothing is timed; N replayed native steps at B = 512 run for `rocprofv3 --kernel-trace --stats -- python
tools/curatornet_bench.py --trace-steps N` (a run of its own), and `--kernel-stats CSV --out JSON` folds that run's
kernel_stats.csv into the JSON as the step's split between GEMMs, the model's kernels and the optimizer.
usage (on an MI355X): python tools/curatornet_bench.py [--steps 20] [--rounds 3] [--out profiles/curatornet/curatornet_bench.json]"""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

E, HIDDEN, L, F = 512, 2, 10, 2048
ARGS = {"learning_rate": 1e-4, "weight_decay": 0.01}


class _Data:
    def __init__(self, I):
        self.item_num = I


def batches(ti, I, B, n, seed=1):
    """(profile [B, L], target [B, 2]) rows as CuratorTrainBatcher lays them out: chunks of 1..L+1 popularity-drawn items."""
    rng = np.random.default_rng(seed)
    out, distinct = [], []
    for _ in range(n):
        win = ti[rng.integers(0, len(ti), size=(B, L + 1))]
        lens = rng.integers(1, L + 2, size=B)
        win = np.where(np.arange(L + 1)[None, :] >= (L + 1 - lens)[:, None], win, 0)
        neg = rng.integers(1, I, size=B)
        neg[(neg[:, None] == win).any(1)] = 0              # never inside the chunk (0 is the padding row: a valid id)
        ids = np.concatenate((win.reshape(-1), neg))
        distinct.append(len(np.unique(ids)) / ids.size)
        out.append((torch.from_numpy(win[:, :L].copy()).cuda(), torch.from_numpy(np.stack([win[:, L], neg], 1)).cuda()))
    return out, float(np.mean(distinct))


def native(I, path, bs):
    from pixelrec_amd.graph import GraphedTrainStep
    from pixelrec_amd.model import CuratorNet
    from pixelrec_amd.optim import PxrAdamW

    torch.manual_seed(0)
    m = CuratorNet({"embedding_size": E, "hidden_size": HIDDEN, "MAX_ITEM_LIST_LENGTH": L, "v_feat_path": path}, _Data(I)).cuda().train()
    opt = PxrAdamW(m, lr=ARGS["learning_rate"], weight_decay=ARGS["weight_decay"])
    g = GraphedTrainStep(m, opt, *bs[0], warmup=0)
    it = iter(range(1 << 30))
    return m, opt, g, (lambda: g(*bs[next(it) % len(bs)]))


def torch_ref(v_feat, bs):
    """The reference's CuratorNet arithmetic in plain float32 torch: autograd, torch.optim.AdamW over the ten Linear tensors."""
    import torch.nn.functional as Fn

    torch.manual_seed(0)
    Hd = HIDDEN * E
    mod = torch.nn.ModuleDict({"c1": torch.nn.Linear(F, E), "c2": torch.nn.Linear(E, E), "p1": torch.nn.Linear(2 * E, Hd),
                               "p2": torch.nn.Linear(Hd, Hd), "p3": torch.nn.Linear(Hd, E)}).cuda()
    for lin in mod.values():
        torch.nn.init.xavier_uniform_(lin.weight)
    emb = torch.nn.Embedding.from_pretrained(v_feat, freeze=True)
    mx, av = torch.nn.AdaptiveMaxPool2d((1, E)), torch.nn.AdaptiveAvgPool2d((1, E))
    opt = torch.optim.AdamW(mod.parameters(), lr=ARGS["learning_rate"], weight_decay=ARGS["weight_decay"])
    common = lambda x: Fn.selu(mod["c2"](Fn.selu(mod["c1"](x))))
    it = iter(range(1 << 30))

    def step():
        profile, target = bs[next(it) % len(bs)]
        pi, ni = common(emb(target[:, 0])), common(emb(target[:, 1]))
        h = common(emb(profile))
        u = torch.cat((mx(h), av(h)), dim=-1)
        for k in ("p1", "p2", "p3"):
            u = Fn.selu(mod[k](u))
        u = u.squeeze(1)
        loss = -torch.mean(torch.log(1e-8 + torch.sigmoid((u * pi).sum(-1) - (u * ni).sum(-1))))
        opt.zero_grad()
        loss.backward()
        opt.step()

    return mod, opt, step


def eval_ms(m, I, n_users=512, n_hist=20, reps=10):
    from lightgcn_bench import timed
    from pixelrec_amd import ops

    m.eval()

    def item_all():
        m.invalidate_item_cache()
        m.compute_item_all()

    item_ms = timed(item_all, 3, warm=1)
    feat = m.compute_item_all()
    planes = ops.split_planes(feat) if ops.score_planes_supported(feat) else None
    nmax = ops.row_norm_max(feat) if planes is not None else None
    rng = np.random.default_rng(3)
    win = torch.from_numpy(rng.integers(1, I, size=(n_users, L))).cuda()
    hu = torch.from_numpy(np.repeat(np.arange(n_users), n_hist))
    hi = torch.from_numpy(rng.integers(1, I, size=n_users * n_hist))
    ptr, hitems = ops.history_csr(hu, hi, n_users, "cuda")
    hu_d, hi_d = hu.cuda(), hi.cuda()

    def fused():
        _, last = m.encode_last(win, feat)
        ops.score_topk(last, last.stride(0), n_users, feat, 10, ptr, hitems, table_planes=planes, table_norm_max=nmax)

    def literal():
        s = m.predict(win, feat)
        s[:, 0] = -np.inf
        s[(hu_d, hi_d)] = -np.inf
        torch.topk(s, 10, dim=-1)

    return item_ms, timed(fused, reps, warm=2), timed(literal, reps, warm=2)


def fold_kernel_stats(path, out):
    """rocprofv3's kernel_stats.csv -> {group: share of the traced kernel time} into the JSON at `out`."""
    groups = {}
    # the runtime's buffer copies and torch's fills are the set-up (features, moments) and the batch copy in front of a replay
    rows = [r for r in csv.DictReader(open(path)) if not (r["Name"].startswith("__amd_rocclr") or "at::native" in r["Name"])]
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    for r in rows:
        n = r["Name"]
        key = ("GEMMs (five Linears forward, input and weight gradients)" if ("gemm" in n.lower() or "grouped_dw" in n or "split" in n)
               else "curator kernels" if "curator_" in n else "feature gather" if "embed_gather" in n else "pair head" if "mf_pair" in n
               else "flat update and step scalars" if ("adamw" in n or "hyper" in n) else "other")
        g = groups.setdefault(key, {"share": 0.0, "kernels": {}})
        g["share"] += float(r["TotalDurationNs"]) / total
        g["kernels"][n.split("(")[0][-60:]] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                             "share": round(float(r["TotalDurationNs"]) / total, 4)}
    for g in groups.values():
        g["share"] = round(g["share"], 4)
    res = json.load(open(out)) if os.path.exists(out) else {}
    res["kernel_split_b512"] = groups
    res["kernel_split_note"] = ("shares of the traced time of the step's own kernels over the traced steps at B = 512 (rocprofv3 "
                                "--kernel-trace --stats in a run of its own); runtime copies and torch fills are left out")
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({k: v["share"] for k, v in groups.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        return fold_kernel_stats(a.kernel_stats, a.out)
    from lightgcn_bench import synth_train, timed
    from pixelrec_amd import ops

    _, ti, _, I = synth_train()
    v_np = np.random.default_rng(7).standard_normal((I, F), dtype=np.float32)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "features.npy")
    np.save(path, v_np)
    try:
        if a.trace_steps:
            bs, _ = batches(ti, I, 512, 32)
            m, opt, g, nstep = native(I, path, bs)
            for _ in range(a.trace_steps):
                nstep()
            torch.cuda.synchronize()
            ops.raise_on_bad_indices()
            return
        v_np[0] = 0
        v_feat = torch.from_numpy(v_np).cuda()
        res = {"device": torch.cuda.get_device_name(0), "items": I, "embedding_size": E, "hidden_size": HIDDEN, "L": L,
               "feature_width": F, "optim_args": ARGS, "steps_per_round": a.steps, "rounds": a.rounds, "runs": [],
               "note": "every figure below was measured in this run on the device named above; ms per step are medians over rounds"}
        for B in (512, 64):
            bs, distinct = batches(ti, I, B, 32)
            m, opt, g, nstep = native(I, path, bs)
            tmod, topt, tstep = torch_ref(v_feat, bs)
            nat, tor = [], []
            for _ in range(a.rounds):
                nat.append(timed(nstep, a.steps, warm=2))
                tor.append(timed(tstep, a.steps, warm=2))
            rows = B * (L + 2)
            Hd = HIDDEN * E
            r = {"batch": B, "native_ms_per_step": round(statistics.median(nat), 4),
                 "torch_ms_per_step": round(statistics.median(tor), 4), "native_rounds_ms": [round(x, 4) for x in nat],
                 "torch_rounds_ms": [round(x, 4) for x in tor], "native_final_loss": float(g.loss),
                 "distinct_id_share_per_batch": round(distinct, 4),
                 "gemm_flop_per_step": 2.0 * (rows * (2 * F * E + 3 * E * E) + 3 * B * (2 * E * Hd + Hd * Hd + Hd * E))}
            r["speedup"] = round(r["torch_ms_per_step"] / r["native_ms_per_step"], 2)
            if B == 512:
                (r["compute_item_all_ms"], r["fused_topk_batch_512_ms"],
                 r["literal_predict_topk_batch_512_ms"]) = (round(x, 4) for x in eval_ms(m, I))
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
            del m, opt, g, tmod, topt
            torch.cuda.empty_cache()
        ops.raise_on_bad_indices()
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)
    finally:
        os.remove(path)
        os.rmdir(tmp)


if __name__ == "__main__":
    main()
