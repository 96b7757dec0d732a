"""DSSM and FM training-step and evaluation time at the shipped configs (configs/IDNet/dssm.yaml: embedding_size 4096, no MLP;
fm.yaml: embedding_size 2048; L = 10) over the 96 001-item catalogue of tools/lightgcn_bench.synth_train (Zipf item popularity).

  native:        model/pooled.py + PxrAdamW (lazy table rows), the whole step replayed from a hipGraph; the table gradient through
                 pxr_pool_table_grad_f32 (MODE_POOL: the compact block G [3B, D], no row per occurrence);
  materialised:  the same step with the table gradient the way DIN and ACF make theirs: occ [B (L + 2), D] written out (here by
                 three torch launches: weight, expand, copy) and reduced by pxr_embed_grad_rows_f32 -- what MODE_POOL replaces;
  torch:         a float32 restatement of the reference's arithmetic on the same GPU (tests/pool_restate.py: a dense table,
                 autograd, torch.optim.AdamW over every row), issued eagerly, on EVERY row of the batch like the native step (the
                 reference's own forward keeps one row).  The baseline is this restatement, never the native code.
The three run in the same process and alternate: `--rounds` rounds of `--steps` steps each at B = 64 and B = 512; a side's figure is
the median over the rounds.  Evaluation, same process: one fused top-k batch of 1024 users (encode_last + pxr_score_topk_f32,
K = 10, 20 history items per user) against predict + masks + torch.topk.
`--trace MODEL`: nothing is timed; ten replayed B = 512 steps run for `rocprofv3 --kernel-trace --stats -- python
tools/pool_bench.py --trace MODEL` (a run of its own), and `--kernel-stats CSV --out JSON --tag NAME` folds that run's
kernel_stats.csv into the JSON.
usage (on an MI355X): python tools/pool_bench.py [--steps 20] [--rounds 3] [--out profiles/pool/pool_bench.json]"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

L, K = 10, 10
SHAPES = {"DSSM": 4096, "FM": 2048}
ARGS = {"learning_rate": 1e-4, "weight_decay": 0.1}


class _Data:
    def __init__(self, I):
        self.item_num = I


def batches(ti, I, B, n, seed=1):
    """(profile [B, L], target [B, 2]) rows as DinTrainBatcher lays them out: chunks of 1..L+1 popularity-drawn items."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        win = ti[rng.integers(0, len(ti), size=(B, L + 1))]
        lens = rng.integers(1, L + 2, size=B)
        win = np.where(np.arange(L + 1)[None, :] >= (L + 1 - lens)[:, None], win, 0)
        neg = rng.integers(1, I, size=B)
        clash = (neg[:, None] == win).any(1)
        neg[clash] = (win[clash].max(1) % (I - 1)) + 1
        out.append((torch.from_numpy(win[:, :L].copy()).cuda(), torch.from_numpy(np.stack([win[:, L], neg], 1)).cuda()))
    return out


def native(kind, I, bs, materialise=False):
    from pixelrec_amd import model, ops
    from pixelrec_amd.graph import GraphedTrainStep
    from pixelrec_amd.optim import PxrAdamW

    base = cls = getattr(model, kind)
    if materialise:
        class cls(base):                                  # the table gradient from one row per occurrence
            def _table_grad(self, gidx, B, L, G, w):
                D = G.shape[1]
                occ, tmp = self._buf("occ", (B * (L + 2), D)), self._buf("wG", (B, D))
                torch.mul(G[:B], w[:, None], out=tmp)
                occ[:B * L].view(B, L, D).copy_(tmp[:, None, :].expand(B, L, D))
                occ[B * L:].copy_(G[B:])
                return ops.embed_grad_rows(gidx, occ, self._table.shape[0], out=self._sparse_rows(B * (L + 2)))
    torch.manual_seed(0)
    m = cls({"embedding_size": SHAPES[kind], "mlp_hidden_size": [], "dropout_prob": 0, "MAX_ITEM_LIST_LENGTH": L}, _Data(I)).cuda().train()
    opt = PxrAdamW(m, lr=ARGS["learning_rate"], weight_decay=ARGS["weight_decay"])
    g = GraphedTrainStep(m, opt, *bs[0], warmup=0)
    it = iter(range(1 << 30))
    return m, opt, g, (lambda: g(*bs[next(it) % len(bs)]))


def torch_ref(kind, sd, bs):
    """The reference's arithmetic in plain float32 torch (FM: the literal factorisation machine): autograd over a dense table,
    torch.optim.AdamW."""
    from tests import pool_restate as R

    params = {k: torch.nn.Parameter(v.detach().clone().cuda()) for k, v in sd.items() if k != R.ALIAS}
    opt = torch.optim.AdamW(list(params.values()), lr=ARGS["learning_rate"], weight_decay=ARGS["weight_decay"])
    it = iter(range(1 << 30))

    def step():
        profile, target = bs[next(it) % len(bs)]
        loss = R.loss_of(kind, params, torch.cat((profile, target), dim=1), literal=True)
        opt.zero_grad()
        loss.backward()
        opt.step()

    return params, opt, step


def evaluation(m, I, B=1024, reps=10):
    from lightgcn_bench import timed
    from pixelrec_amd import ops

    m.eval()
    feat = m.compute_item_all()
    rng = np.random.default_rng(3)
    win = torch.from_numpy(rng.integers(1, I, size=(B, L))).cuda()
    hu = torch.from_numpy(np.repeat(np.arange(B), 20))
    hi = torch.from_numpy(rng.integers(1, I, size=B * 20))
    ptr, hitems = ops.history_csr(hu, hi, B, "cuda")
    hu_d, hi_d = hu.cuda(), hi.cuda()

    def fused():
        _, q = m.encode_last(win, feat)
        ops.score_topk(q, q.stride(0), B, feat.data, K, ptr, hitems)

    def literal():
        s = m.predict(win, feat)
        s[:, 0] = -np.inf
        s[(hu_d, hi_d)] = -np.inf
        torch.topk(s, K, dim=-1)

    f_ms, l_ms = timed(fused, reps, warm=2), timed(literal, reps, warm=2)
    return {"eval_batch_size": B, "fused_ms": round(f_ms, 4), "predict_topk_ms": round(l_ms, 4),
            "fused_users_per_s": round(B / f_ms * 1e3, 1), "predict_users_per_s": round(B / l_ms * 1e3, 1)}


def fold_kernel_stats(path, out, tag):
    """rocprofv3's kernel_stats.csv -> per-kernel calls / average / share into the JSON at `out` under `tag`."""
    rows = [r for r in csv.DictReader(open(path)) if not r["Name"].startswith("__amd_rocclr")]
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    table = {r["Name"].split("(")[0][-60:]: {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                             "share": round(float(r["TotalDurationNs"]) / total, 4)} for r in rows}
    res = json.load(open(out)) if os.path.exists(out) else {}
    res[tag] = table
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(table))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--items", type=int, default=96_000)
    ap.add_argument("--trace", default=None, choices=list(SHAPES))
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--tag", default="step_b512_kernel_trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        return fold_kernel_stats(a.kernel_stats, a.out, a.tag)
    from lightgcn_bench import synth_train, timed
    from pixelrec_amd import ops

    _, ti, _, I = synth_train(n_items=a.items)
    if a.trace:
        bs = batches(ti, I, 512, 8)
        m, opt, g, nstep = native(a.trace, I, bs)
        for _ in range(10):
            nstep()
        torch.cuda.synchronize()
        ops.raise_on_bad_indices()
        return
    res = {"device": torch.cuda.get_device_name(0), "items": I, "L": L, "embedding_size": SHAPES, "optim_args": ARGS,
           "steps_per_round": a.steps, "rounds": a.rounds, "runs": [],
           "note": "every figure below was measured in this run on the device named above; ms per step are medians over rounds"}
    for kind in SHAPES:
        for B in (64, 512):
            bs = batches(ti, I, B, 32)
            m, opt, g, nstep = native(kind, I, bs)
            m2, opt2, g2, mstep = native(kind, I, bs, materialise=True)
            tpar, topt, tstep = torch_ref(kind, {k: v.clone() for k, v in m.state_dict().items()}, bs)
            nat, mat, tor = [], [], []
            for _ in range(a.rounds):
                nat.append(timed(nstep, a.steps, warm=2))
                mat.append(timed(mstep, a.steps, warm=2))
                tor.append(timed(tstep, a.steps, warm=2))
            med = lambda v: round(statistics.median(v), 4)
            r = {"model": kind, "batch": B, "embedding_size": SHAPES[kind], "native_ms_per_step": med(nat),
                 "materialised_rows_ms_per_step": med(mat), "torch_ms_per_step": med(tor),
                 "native_rounds_ms": [round(x, 4) for x in nat], "materialised_rounds_ms": [round(x, 4) for x in mat],
                 "torch_rounds_ms": [round(x, 4) for x in tor], "native_final_loss": float(g.loss),
                 "materialised_final_loss": float(g2.loss), "occurrence_buffer_mb": round(B * (L + 2) * SHAPES[kind] * 4 / 1e6, 1)}
            r["speedup_over_torch"] = round(r["torch_ms_per_step"] / r["native_ms_per_step"], 2)
            r["materialised_over_native"] = round(r["materialised_rows_ms_per_step"] / r["native_ms_per_step"], 3)
            if B == 512:
                r["evaluation"] = evaluation(m, I)
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
            del m, opt, g, m2, opt2, g2, tpar, topt
            torch.cuda.empty_cache()
    ops.raise_on_bad_indices()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
