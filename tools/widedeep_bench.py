"""WideDeep training-step and evaluation time at the shipped config (configs/IDNet/widedeep.yaml: embedding_size 64,
mlp_hidden_size [128, 64], L = 10) over the 96 001-item catalogue of tools/lightgcn_bench.synth_train (Zipf item popularity).

  native: model/widedeep.py + PxrAdamW (lazy deep-table rows, one flat launch that also sweeps the dense wide vector), the whole
          step replayed from a hipGraph;
  torch:  a float32 restatement of the reference's WideDeep on the same GPU (tests/widedeep_restate.py, literal form: dense
          nn.Embedding-style tables, autograd, torch.optim.AdamW), issued eagerly.  The baseline is this restatement, never the
          native code.
The two run in the same process and alternate: `--rounds` rounds of `--steps` native steps then `--steps` torch steps at B = 64
and B = 512; each side's figure is the median over the rounds.  Evaluation, same process: one fused batch (pxr_wd_topk_f32, K = 10,
20 history items per user) against the chunked predict + masks + torch.topk at eval_batch_size 64 / 256 / 1024.  The fused
kernel's share of the fp32 MFMA peak (157.3 TFLOP/s at 2.4 GHz) is stated from its own FLOP count: per (user, item) the second
layer's 2 h1 h2 on the MFMA plus h1 adds and 2 h2 for the predict column, i.e. 2 h1 h2 + h1 + 2 h2; T's traffic is stated beside
it (every workgroup reads its users' item tiles of T: B x N x h1 x 4 bytes per batch through the caches).
usage (on an MI355X): python tools/widedeep_bench.py [--steps 20] [--rounds 3] [--out profiles/widedeep/widedeep_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

D, HIDDEN, L, K = 64, [128, 64], 10, 10
ARGS = {"learning_rate": 1e-4, "weight_decay": 0.1}
PEAK_TFLOPS = 157.3


class _Data:
    def __init__(self, I):
        self.item_num = I


def batches(ti, I, B, n, seed=1):
    """(profile [B, L], target [B, 2]) as CuratorTrainBatcher lays them out: chunks of 1..L+1 popularity-drawn items, the last
    one the positive, a negative outside the chunk."""
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


def native(I, bs):
    from pixelrec_amd.graph import GraphedTrainStep
    from pixelrec_amd.model import WideDeep
    from pixelrec_amd.optim import PxrAdamW

    torch.manual_seed(0)
    m = WideDeep({"embedding_size": D, "mlp_hidden_size": HIDDEN, "dropout_prob": 0, "MAX_ITEM_LIST_LENGTH": L}, _Data(I)).cuda().train()
    opt = PxrAdamW(m, lr=ARGS["learning_rate"], weight_decay=ARGS["weight_decay"])
    g = GraphedTrainStep(m, opt, *bs[0], warmup=0)
    it = iter(range(1 << 30))
    return m, opt, g, (lambda: g(*bs[next(it) % len(bs)]))


def torch_ref(sd, bs):
    """The reference's WideDeep arithmetic in plain float32 torch: autograd over dense tables, torch.optim.AdamW."""
    from tests import widedeep_restate as R

    params = {k: torch.nn.Parameter(v.detach().clone().cuda()) for k, v in sd.items()}
    opt = torch.optim.AdamW(list(params.values()), lr=ARGS["learning_rate"], weight_decay=ARGS["weight_decay"])
    it = iter(range(1 << 30))

    def step():
        profile, target = bs[next(it) % len(bs)]
        loss = R.loss_literal(params, torch.cat((profile, target), dim=1))
        opt.zero_grad()
        loss.backward()
        opt.step()

    return params, opt, step


def evaluation(m, I, reps=5):
    from lightgcn_bench import timed
    from pixelrec_amd import ops

    m.eval()
    feat = m.compute_item_all()
    rng = np.random.default_rng(3)
    out = []
    h1, h2 = HIDDEN
    flop_pair = 2.0 * h1 * h2 + h1 + 2.0 * h2
    for B in (64, 256, 1024):
        win = torch.from_numpy(rng.integers(1, I, size=(B, L))).cuda()
        hu = torch.from_numpy(np.repeat(np.arange(B), 20))
        hi = torch.from_numpy(rng.integers(1, I, size=B * 20))
        ptr, hitems = ops.history_csr(hu, hi, B, "cuda")
        hu_d, hi_d = hu.cuda(), hi.cuda()

        def fused():
            m.fused_topk_batch(win, ptr, hitems, K)

        def chunked():
            s = m.predict(win, feat)
            s[:, 0] = -np.inf
            s[(hu_d, hi_d)] = -np.inf
            torch.topk(s, K, dim=-1)

        f_ms = timed(fused, reps, warm=2)
        c_ms = timed(chunked, 2, warm=1)
        out.append({"eval_batch_size": B, "fused_ms": round(f_ms, 4), "chunked_predict_topk_ms": round(c_ms, 4),
                    "fused_users_per_s": round(B / f_ms * 1e3, 1), "chunked_users_per_s": round(B / c_ms * 1e3, 1),
                    "fused_tflops": round(B * I * flop_pair / f_ms / 1e9, 2),
                    "fused_share_of_fp32_mfma_peak": round(B * I * flop_pair / f_ms / 1e9 / PEAK_TFLOPS, 4),
                    "T_read_GB_per_s": round(B * I * h1 * 4 / f_ms / 1e6, 1)})
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from lightgcn_bench import synth_train, timed
    from pixelrec_amd import ops

    _, ti, _, I = synth_train()
    res = {"device": torch.cuda.get_device_name(0), "items": I, "embedding_size": D, "mlp_hidden_size": HIDDEN, "L": L,
           "optim_args": ARGS, "steps_per_round": a.steps, "rounds": a.rounds, "runs": [],
           "note": "every figure below was measured in this run on the device named above; ms per step are medians over rounds"}
    for B in (64, 512):
        bs = batches(ti, I, B, 32)
        m, opt, g, nstep = native(I, bs)
        tpar, topt, tstep = torch_ref({k: v.clone() for k, v in m.state_dict().items()}, bs)
        nat, tor = [], []
        for _ in range(a.rounds):
            nat.append(timed(nstep, a.steps, warm=2))
            tor.append(timed(tstep, a.steps, warm=2))
        r = {"batch": B, "native_ms_per_step": round(statistics.median(nat), 4), "torch_ms_per_step": round(statistics.median(tor), 4),
             "native_rounds_ms": [round(x, 4) for x in nat], "torch_rounds_ms": [round(x, 4) for x in tor],
             "native_final_loss": float(g.loss)}
        r["speedup"] = round(r["torch_ms_per_step"] / r["native_ms_per_step"], 2)
        res["runs"].append(r)
        print(json.dumps(r), flush=True)
        if B == 512:
            res["evaluation"] = evaluation(m, I)
            best = max(res["evaluation"], key=lambda e: e["fused_users_per_s"])
            res["best_eval_batch_size"] = best["eval_batch_size"]
        del m, opt, g, tpar, topt
        torch.cuda.empty_cache()
    ops.raise_on_bad_indices()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
