"""VISRANK evaluation throughput at the Pixel200K shape (96 001 items, F = 2048 synthetic features, synthetic histories of 3..38
items as tools/synth_dataset.py draws them): users/s of
  * the fused path (ops.visrank_topk) at several eval_batch_size values,
  * a torch restatement of the reference as shipped, one user per call (torch.cosine_similarity over [h, 1, F] x [1, N, F], topk
    over the history axis, mean, masks, torch.topk),
  * a batched torch restatement (gather, matmul of unit rows, topk over the history axis, masks, torch.topk) -- for information.
All in one process, torch.cuda events, one warm-up and --repeats timed repeats each.  Writes one JSON file.
usage: python tools/visrank_bench.py [--out FILE] [--users N] [--repeats R] [--one-batch B]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelrec_amd import ops  # noqa: E402

N_ITEMS, F, H, K, TOP_K = 96001, 2048, 50, 10, 1
PEAK_FP32_MFMA_2400 = 256 * 4 * 64 * 2.4e9        # 256 CUs x 4 SIMDs x 64 flop/cycle (v_mfma_f32_32x32x2_f32: 4096 flop in 64 cycles) at 2.4 GHz


def histories(n, rng):
    return [rng.integers(1, N_ITEMS, size=int(rng.integers(3, 39))) for _ in range(n)]


def pack(hists):
    B = len(hists)
    win = np.zeros((B, H), dtype=np.int64)
    for b, h in enumerate(hists):
        w = h[-H:]
        win[b, H - len(w):] = w
    ptr = np.zeros(B + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(h) for h in hists])
    return (torch.from_numpy(win).cuda(), torch.from_numpy(ptr).cuda(), torch.from_numpy(np.concatenate(hists)).cuda())


def timed(fn, repeats):
    fn()                                            # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3)
    return out


def reference_one_user(v, hist):
    user = hist[-50:]
    sim = torch.cosine_similarity(v[user].unsqueeze(1), v.unsqueeze(0), dim=-1)
    values, _ = torch.topk(sim, k=min(TOP_K, len(user)), dim=0)
    scores = values.mean(0)
    scores[0] = -np.inf
    scores[hist] = -np.inf
    return torch.topk(scores, K).indices


def batched_torch(unit, win, ptr, items):
    B = win.shape[0]
    S = (unit[win.reshape(-1)] @ unit.T).view(B, H, -1)
    S = S.masked_fill((win == 0)[:, :, None], -np.inf)
    scores = torch.topk(S, TOP_K, dim=1).values.mean(1)
    scores[:, 0] = -np.inf
    hu = torch.repeat_interleave(torch.arange(B, device=win.device), (ptr[1:] - ptr[:-1]).long())
    scores[(hu, items)] = -np.inf
    return torch.topk(scores, K, dim=1).indices


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="visrank_bench.json")
    ap.add_argument("--users", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--one-batch", type=int, default=0, help="run ONE fused batch of this size and exit (for a kernel trace)")
    a = ap.parse_args()
    rng = np.random.default_rng(2020)
    v = torch.from_numpy(rng.standard_normal((N_ITEMS, F)).astype(np.float32)).cuda()
    unit = ops.visrank_unit_rows(v)
    if a.one_batch:
        win, ptr, items = pack(histories(a.one_batch, rng))
        ops.visrank_topk(unit, win, TOP_K, K, ptr, items)
        torch.cuda.synchronize()
        ops.raise_on_bad_indices()
        return
    hists = histories(a.users, rng)
    rows = sum(len(h[-H:]) for h in hists)
    res = {"shape": {"items": N_ITEMS, "F": F, "window": H, "K": K, "top_k": TOP_K, "users": a.users, "window_rows": rows},
           "device": torch.cuda.get_device_name(0), "fused": {}, "repeats": a.repeats}
    for B in (64, 128, 256, 512, 1024):
        batches = [pack(hists[i:i + B]) for i in range(0, a.users, B)]

        def run():
            for win, ptr, items in batches:
                ops.visrank_topk(unit, win, TOP_K, K, ptr, items)

        t = timed(run, a.repeats)
        ops.raise_on_bad_indices()
        try:
            clock = float(torch.cuda.clock_rate())          # MHz, sampled right behind the timed repeats
        except Exception:
            clock = None
        slow = max(t)
        res["fused"][str(B)] = {"seconds": t, "users_per_s_slowest": a.users / slow, "users_per_s_fastest": a.users / min(t),
                                "useful_tflops_slowest": 2.0 * rows * N_ITEMS * F / slow / 1e12,
                                "tile_tflops_slowest": 2.0 * a.users * 64 * N_ITEMS * F / slow / 1e12,
                                "shader_clock_mhz_after": clock}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:                         # (the fused figures survive a restatement that runs out of memory)
        json.dump(res, f, indent=1)
    n1 = 8
    t = timed(lambda: [reference_one_user(v, torch.from_numpy(h).cuda()) for h in hists[:n1]], a.repeats)
    res["reference_batch1_torch"] = {"users": n1, "seconds": t, "users_per_s_fastest": n1 / min(t), "users_per_s_slowest": n1 / max(t)}
    nb, Bb = 256, 32
    bb = [pack(hists[i:i + Bb]) for i in range(0, nb, Bb)]
    t = timed(lambda: [batched_torch(unit, *b) for b in bb], a.repeats)
    res["batched_torch_info"] = {"users": nb, "batch": Bb, "seconds": t, "users_per_s_fastest": nb / min(t)}
    best = max(res["fused"], key=lambda k: res["fused"][k]["users_per_s_slowest"])
    res["best_eval_batch_size"] = int(best)
    fb = res["fused"][best]
    res["fused_slowest_over_reference_fastest"] = fb["users_per_s_slowest"] / res["reference_batch1_torch"]["users_per_s_fastest"]
    res["fraction_of_fp32_mfma_peak_at_2400mhz"] = {"useful": fb["useful_tflops_slowest"] * 1e12 / PEAK_FP32_MFMA_2400,
                                                    "tiles": fb["tile_tflops_slowest"] * 1e12 / PEAK_FP32_MFMA_2400}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("best_eval_batch_size", "fused_slowest_over_reference_fastest",
                                          "fraction_of_fp32_mfma_peak_at_2400mhz")}))
    assert fb["users_per_s_slowest"] > res["reference_batch1_torch"]["users_per_s_fastest"]


if __name__ == "__main__":
    main()
