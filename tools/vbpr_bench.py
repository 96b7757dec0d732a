"""VBPR training-step and evaluation time at the Pixel200K shape of tools/synth_dataset.py (200 K users, 96 K items, Zipf item
popularity; the training pairs of tools/lightgcn_bench.synth_train), embedding_size 4096 (Dh = 2048, configs/ViNet/vbpr.yaml),
F = 2048 synthetic features (ResNet-50's pooled width: an assumption about RN50.npy), at B = 512 (the shipped batch) and B = 64
(the batch of tools/mf_bench.py's table), under the shipped two parameter groups.

  native: model/vbpr.py + optim.flat_table_adamw (lazy table rows, one flat launch), the whole step replayed from a hipGraph;
  torch:  a restatement of the reference's VBPR on the same GPU -- three dense nn.Embedding tables, two bias-free nn.Linear over
          the gathered feature rows, the same loss under autograd, torch.optim.AdamW with the two groups over every parameter
          (every row of the three tables, every step) -- issued eagerly.  The baseline is this restatement, never the native code.
The two run in the same process and alternate: `--rounds` rounds of `--steps` native steps then `--steps` torch steps; each
side's figure is the median over the rounds.  Also timed: compute_item_all + scoring_item_matrix, one fused top-k batch of 512
users (encode_last + pxr_score_topk_f32 on the packed matrices with pre-split planes, K = 10, 20 history items per user) and the
literal predict + masks + torch.topk for the same batch.
`--trace-steps N`: nothing is timed; N replayed native steps at B = 512 run for `rocprofv3 --kernel-trace --stats -- python
tools/vbpr_bench.py --trace-steps N` (a run of its own), and `--kernel-stats CSV --out JSON` folds that run's kernel_stats.csv
into the JSON as the step's split between projection GEMMs, the model's kernels and the row updates.
usage (on an MI355X): python tools/vbpr_bench.py [--steps 20] [--rounds 3] [--out profiles/vbpr/vbpr_bench.json]"""
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

D, F = 4096, 2048
ARGS4 = {"modal_lr": 1e-4, "rec_lr": 1e-3, "modal_decay": 0.1, "rec_decay": 0}


class _Data:
    def __init__(self, U, I):
        self.user_num, self.item_num = U, I


def batches(tu, ti, I, B, n, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        r = rng.integers(0, len(tu), size=B)
        neg = rng.integers(1, I, size=B)
        neg[neg == ti[r]] = 0                              # never the positive (ids are 1-based in the data; 0 is a valid row)
        out.append((torch.from_numpy(tu[r]).cuda(), torch.from_numpy(np.stack([ti[r], neg], 1)).cuda()))
    return out


def native(U, I, path, bs):
    from pixelrec_amd.graph import GraphedTrainStep
    from pixelrec_amd.model import VBPR
    from pixelrec_amd.optim import flat_table_adamw

    torch.manual_seed(0)
    m = VBPR({"embedding_size": D, "v_feat_path": path}, _Data(U, I)).cuda().train()
    opt = flat_table_adamw(m, ARGS4, "projection")
    g = GraphedTrainStep(m, opt, *bs[0], warmup=0)
    it = iter(range(1 << 30))
    return m, opt, g, (lambda: g(*bs[next(it) % len(bs)]))


def torch_ref(U, I, v_feat, bs):
    """The reference's VBPR arithmetic in plain torch: dense tables, autograd, torch.optim.AdamW with the two groups."""
    dev, Dh = "cuda", D // 2
    torch.manual_seed(0)
    mod = torch.nn.ModuleDict({"feature_projection": torch.nn.Linear(F, Dh, bias=False),
                               "bias_projection": torch.nn.Linear(F, 1, bias=False), "uid": torch.nn.Embedding(U, Dh),
                               "iid": torch.nn.Embedding(I, Dh), "um": torch.nn.Embedding(U, Dh)}).to(dev)
    for p in mod.parameters():
        torch.nn.init.xavier_normal_(p)
    inside = [p for n, p in mod.named_parameters() if "projection" in n]
    outside = [p for n, p in mod.named_parameters() if "projection" not in n]
    opt = torch.optim.AdamW([{"params": inside, "lr": ARGS4["modal_lr"], "weight_decay": ARGS4["modal_decay"]},
                             {"params": outside, "lr": ARGS4["rec_lr"], "weight_decay": ARGS4["rec_decay"]}])
    wt = torch.tensor([[1.0], [-1.0]], device=dev)
    it = iter(range(1 << 30))

    def step():
        user, item = bs[next(it) % len(bs)]
        v = v_feat[item]
        score = ((mod["uid"](user).unsqueeze(1) * mod["iid"](item)).sum(-1)
                 + (mod["um"](user).unsqueeze(1) * mod["feature_projection"](v)).sum(-1) + mod["bias_projection"](v).squeeze(-1))
        loss = -torch.mean(torch.log(1e-8 + torch.sigmoid(score.view(-1, 2) @ wt)))
        opt.zero_grad()
        loss.backward()
        opt.step()

    return mod, opt, step


def eval_ms(m, U, I, n_users=512, n_hist=20, reps=10):
    from lightgcn_bench import timed
    from pixelrec_amd import ops

    m.eval()
    item_ms = timed(lambda: (m.compute_item_all(), m.scoring_item_matrix()), 3, warm=1)
    feat = m.compute_item_all()
    packed = m.scoring_item_matrix()
    planes = ops.split_planes(packed) if ops.score_planes_supported(packed) else None
    nmax = ops.row_norm_max(packed) if planes is not None else None
    rng = np.random.default_rng(3)
    users = torch.arange(1, n_users + 1, dtype=torch.int64, device="cuda") % U
    hu = torch.from_numpy(np.repeat(np.arange(n_users), n_hist))
    hi = torch.from_numpy(rng.integers(1, I, size=n_users * n_hist))
    ptr, hitems = ops.history_csr(hu, hi, n_users, "cuda")
    hu_d, hi_d = hu.cuda(), hi.cuda()

    def fused():
        _, last = m.encode_last(users, feat)
        ops.score_topk(last, last.stride(0), n_users, packed, 10, ptr, hitems, table_planes=planes, table_norm_max=nmax)

    def literal():
        s = m.predict(users, feat)
        s[:, 0] = -np.inf
        s[(hu_d, hi_d)] = -np.inf
        torch.topk(s, 10, dim=-1)

    return item_ms, timed(fused, reps, warm=2), timed(literal, reps, warm=2)


def fold_kernel_stats(path, out):
    """rocprofv3's kernel_stats.csv -> {group: share of the traced kernel time} into the JSON at `out`."""
    groups = {}
    # the runtime's buffer copies and torch's fills are the set-up (tables, moments) and the batch copy in front of a replay
    rows = [r for r in csv.DictReader(open(path)) if not (r["Name"].startswith("__amd_rocclr") or "at::native" in r["Name"])]
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    for r in rows:
        n = r["Name"]
        key = ("projection GEMMs" if ("gemm" in n.lower() or "grouped_dw" in n) else "vbpr kernels" if "vbpr_" in n else
               "row updates (adamw_rows)" if "adamw_rows" in n else "flat update and step scalars" if ("adamw" in n or "hyper" in n)
               else "other")
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

    tu, ti, U, I = synth_train()
    v_np = np.random.default_rng(7).standard_normal((I, F)).astype(np.float32)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "features.npy")
    np.save(path, v_np)
    try:
        if a.trace_steps:
            bs = batches(tu, ti, I, 512, 32)
            m, opt, g, nstep = native(U, I, path, bs)
            for _ in range(a.trace_steps):
                nstep()
            torch.cuda.synchronize()
            ops.raise_on_bad_indices()
            return
        v_feat = torch.from_numpy(v_np).cuda()
        res = {"device": torch.cuda.get_device_name(0), "users": U, "items": I, "train_pairs": len(tu), "embedding_size": D,
               "feature_width": F, "optim_args": ARGS4, "steps_per_round": a.steps, "rounds": a.rounds, "runs": [],
               "note": "every figure below was measured in this run on the device named above; ms per step are medians over rounds"}
        for B in (512, 64):
            bs = batches(tu, ti, I, B, 32)
            m, opt, g, nstep = native(U, I, path, bs)
            tmod, topt, tstep = torch_ref(U, I, v_feat, bs)
            nat, tor = [], []
            for _ in range(a.rounds):
                nat.append(timed(nstep, a.steps, warm=2))
                tor.append(timed(tstep, a.steps, warm=2))
            r = {"batch": B, "native_ms_per_step": round(statistics.median(nat), 4),
                 "torch_ms_per_step": round(statistics.median(tor), 4), "native_rounds_ms": [round(x, 4) for x in nat],
                 "torch_rounds_ms": [round(x, 4) for x in tor], "native_final_loss": float(g.loss),
                 "projection_gemm_flop_per_step": 2 * 2.0 * (2 * B) * F * (D // 2)}
            r["speedup"] = round(r["torch_ms_per_step"] / r["native_ms_per_step"], 2)
            if B == 512:
                opt.flush()
                (r["compute_item_all_and_pack_ms"], r["fused_topk_batch_512_ms"],
                 r["literal_predict_topk_batch_512_ms"]) = (round(x, 4) for x in eval_ms(m, U, I))
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
