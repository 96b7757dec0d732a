"""ACF training-step time at the Pixel200K shape (200 001 users, `--items` items -- 96 001 in the dataset -- Zipf item
popularity), embedding_size 512, L = 10, region features [items, 7, 7, 2048] (synthetic: the file holds zeros, the device copy is
filled with unit normals), at B = 512 (the shipped batch) and B = 64, learning_rate 1e-4, weight_decay 0.01.

  native: model/acf.py + PxrAdamW (lazy table rows, one flat launch), the whole step replayed from a hipGraph;
  torch:  a float32 restatement of the reference's ACF on the same GPU (tests/acf_restate.py's formulas: dense tables, autograd,
          torch.optim.AdamW over every parameter, every row of both tables, every step), issued eagerly.  The baseline is this
          restatement, never the native code.
The two run in the same process and alternate: `--rounds` rounds of `--steps` native steps then `--steps` torch steps; each side's
figure is the median over the rounds, the rounds are kept.  Also recorded: the distinct / occurrence ratio of the profile ids of
the batches (what computing x once per distinct item of a batch would save).
`--trace-steps N`: nothing is timed; N replayed native steps at B = 512 run for `rocprofv3 --kernel-trace --stats -- python
tools/acf_bench.py --trace-steps N` (a run of its own), and `--kernel-stats CSV --out JSON` folds that run's kernel_stats.csv into
the JSON as the step's split between GEMMs, the feature gather, the attention kernels and the table update.
usage (on an MI355X): python tools/acf_bench.py [--items 96001] [--steps 10] [--rounds 3] [--out profiles/acf/acf_bench.json]"""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

E, F, HW, L, U = 512, 2048, 7, 10, 200_001
LR, WD = 1e-4, 0.01


class _Data:
    def __init__(self, U, I):
        self.user_num, self.item_num = U, I


def batches(I, B, n, seed=1):
    """[B, L + 3] rows: Zipf-popular profile items (0 .. L of them, left-padded), a positive, a uniform negative, a user id."""
    rng = np.random.default_rng(seed)
    ranks = np.arange(1, I, dtype=np.float64)
    cdf = np.cumsum(1.0 / ranks)
    cdf /= cdf[-1]
    draw = lambda size: 1 + np.minimum(np.searchsorted(cdf, rng.random(size)), I - 2)
    out = []
    for _ in range(n):
        prof = draw((B, L))
        prof[np.arange(L)[None, :] < (L - rng.integers(0, L + 1, size=B))[:, None]] = 0
        tail = np.stack((draw(B), rng.integers(1, I, size=B), rng.integers(1, U, size=B)), axis=1)
        out.append(torch.from_numpy(np.concatenate((prof, tail), axis=1)).cuda())
    return out


def native(I, path, bs):
    from pixelrec_amd.graph import GraphedTrainStep
    from pixelrec_amd.model import ACF
    from pixelrec_amd.optim import PxrAdamW

    torch.manual_seed(0)
    m = ACF({"embedding_size": E, "v_feat_path": path, "MAX_ITEM_LIST_LENGTH": L}, _Data(U, I)).cuda().train()
    m.lazy_table()
    m.v_feat.normal_()
    opt = PxrAdamW(m, lr=LR, weight_decay=WD)
    split = lambda r: (r[:, :L].contiguous(), r[:, L:].contiguous())
    g = GraphedTrainStep(m, opt, *split(bs[0]), warmup=0)
    it = iter(range(1 << 30))
    return m, opt, g, (lambda: g(*split(bs[next(it) % len(bs)])))


def torch_ref(m, bs):
    """The reference's ACF arithmetic in plain float32 torch on the native model's features: dense tables, autograd, AdamW."""
    from tests import acf_restate as R

    P = {k: torch.nn.Parameter(v.detach().clone()) for k, v in m.named_parameters()}
    opt = torch.optim.AdamW(list(P.values()), lr=LR, weight_decay=WD)
    it = iter(range(1 << 30))

    def step():
        loss = R.loss(P, m.v_feat, bs[next(it) % len(bs)])
        opt.zero_grad()
        loss.backward()
        opt.step()

    return P, opt, step


def fold_kernel_stats(path, out):
    """rocprofv3's kernel_stats.csv -> {group: share of the traced kernel time} into the JSON at `out`."""
    groups = {}
    rows = [r for r in csv.DictReader(open(path)) if not (r["Name"].startswith("__amd_rocclr") or "at::native" in r["Name"])]
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    for r in rows:
        n = r["Name"]
        key = ("GEMMs" if ("gemm" in n.lower() or "grouped_dw" in n) else "attention kernels (acf_*)" if "acf_" in n else
               "gathers (embed_gather)" if "embed_gather" in n else
               "table gradient and update (sort, segsum, adamw_rows)" if any(t in n for t in ("adamw_rows", "segsum", "sort", "occ_", "embed_grad", "scan", "uniq")) else
               "flat update and step scalars" if ("adamw" in n or "hyper" in n) else "other")
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
    ap.add_argument("--items", type=int, default=96_001)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        return fold_kernel_stats(a.kernel_stats, a.out)
    from lightgcn_bench import timed
    from pixelrec_amd import ops

    I = a.items
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "regions.npy")
    np.lib.format.open_memmap(path, mode="w+", dtype=np.float32, shape=(I, HW, HW, F)).flush()      # zeros; filled on the device
    try:
        if a.trace_steps:
            bs = batches(I, 512, 8)
            m, opt, g, nstep = native(I, path, bs)
            for _ in range(a.trace_steps):
                nstep()
            torch.cuda.synchronize()
            ops.raise_on_bad_indices()
            return
        res = {"device": torch.cuda.get_device_name(0), "users": U, "items": I, "embedding_size": E, "feature_width": F,
               "regions": HW * HW, "max_item_list_length": L, "optim_args": {"learning_rate": LR, "weight_decay": WD},
               "steps_per_round": a.steps, "rounds": a.rounds, "runs": [],
               "note": "every figure below was measured in this run on the device named above; ms per step are medians over rounds"}
        for B in (512, 64):
            bs = batches(I, B, 8)
            m, opt, g, nstep = native(I, path, bs)
            P, topt, tstep = torch_ref(m, bs)
            nat, tor = [], []
            for _ in range(a.rounds):
                nat.append(timed(nstep, a.steps, warm=2))
                tor.append(timed(tstep, a.steps, warm=1))
            occ = [int((b[:, :L] != 0).sum()) for b in bs]
            dis = [int(torch.unique(b[:, :L][b[:, :L] != 0]).numel()) for b in bs]
            r = {"batch": B, "native_ms_per_step": round(statistics.median(nat), 4),
                 "torch_ms_per_step": round(statistics.median(tor), 4), "native_rounds_ms": [round(x, 4) for x in nat],
                 "torch_rounds_ms": [round(x, 4) for x in tor], "native_final_loss": float(g.loss),
                 "dim_reductor_rows_per_step": B * L * HW * HW,
                 "dim_reductor_gemm_flop_per_step": 2 * 2.0 * B * L * HW * HW * F * E,
                 "feature_gather_bytes_per_step": 4 * B * L * HW * HW * F,
                 "profile_distinct_over_occurrences": round(sum(dis) / max(1, sum(occ)), 4)}
            r["speedup"] = round(r["torch_ms_per_step"] / r["native_ms_per_step"], 2)
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
            del m, opt, g, P, topt
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
