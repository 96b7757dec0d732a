"""Full-sort eval: fused scoring+mask+top-k vs the literal predict -> mask -> torch.topk sequence (scratch tool)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from pixelrec_amd import ops, synth
dev = torch.device("cuda:0")
def timeit(fn, iters=10, warm=2):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / iters
N, D, B = 400001, 512, 1024
table = torch.randn(N, D, device=dev) * 0.02
users = torch.randn(B, D, device=dev)
rng = np.random.default_rng(0)
_, hu, hi, _ = synth.eval_batch(N, B, 50, rng, synth.ZipfItems(N))
hu, hi = torch.from_numpy(hu), torch.from_numpy(hi)
ptr, items = ops.history_csr(hu, hi, B, dev)
hud, hid = hu.to(dev), hi.to(dev)
scores = torch.empty(B, N, device=dev)
def literal():
    ops.gemm(True, True, B, N, D, users, D, table, D, scores, N, ops.EPI_NONE, use_ws=False)
    scores[:, 0] = -np.inf
    scores[(hud, hid)] = -np.inf
    return torch.topk(scores, 10, dim=-1)
def fused():
    return ops.score_topk(users, D, B, table, 10, ptr, items)
tp = ops.split_planes(table) if ops.score_planes_supported(table) else None
def fused_planes():
    return ops.score_topk(users, D, B, table, 10, ptr, items, table_planes=tp)
v1, i1 = literal(); i2, v2 = fused()
print("identical top-10:", torch.equal(i1, i2), "max |dval|", (v1 - v2).abs().max().item())
tl, tf = timeit(literal), timeit(fused)
fl = 2.0 * B * N * D
b3 = ops.gemm_mode() == "bf16x3"
pipe = (lambda t: 6 * fl / t / 1e9 / 2500.0) if b3 else (lambda t: fl / t / 1e9 / 157.3)
print(f"literal (gemm + masks + torch.topk): {tl:.2f} ms   fused: {tf:.2f} ms   speed-up {tl/tf:.2f}x   fused effective {fl/tf/1e9:.1f} "
      f"TFLOP/s algorithmic = {pipe(tf):.3f} of the {'bf16 MFMA pipe (6 products)' if b3 else 'f32-input MFMA peak'}")
if tp is not None:
    i3, v3 = fused_planes()
    print("planes: identical top-10:", torch.equal(i1, i3), "identical to fused:", torch.equal(i2, i3) and torch.equal(v2, v3))
    t_split = timeit(lambda: ops.split_planes(table, tp), iters=5)
    tp3 = timeit(fused_planes)
    print(f"fused on planes: {tp3:.2f} ms ({fl/tp3/1e9:.1f} TFLOP/s algorithmic = {pipe(tp3):.3f} of the bf16 pipe)   table split (once per "
          f"evaluation): {t_split:.2f} ms")
    import json
    json.dump({"literal_ms": tl, "fused_ms": tf, "fused_planes_ms": tp3, "table_split_ms": t_split, "alg_tflops_fused_planes": fl / tp3 / 1e9,
               "bf16_pipe_frac_fused_planes": pipe(tp3), "bf16_pipe_frac_fused": pipe(tf), "identical_top10": bool(torch.equal(i1, i3))},
              open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "eval_bench.json"), "w"), indent=1)
    # the threshold pass on 3 / 1 of the 6 bf16 products, survivors re-scored exactly (pxr_score_topk_f32)
    vmax = ops.row_norm_max(table)
    t_norm = timeit(lambda: ops.row_norm_max(table), iters=5)
    res = {}
    for prod in (6, 3, 1):
        os.environ["PXR_TOPK_PRODUCTS"] = str(prod)
        fn = lambda: ops.score_topk(users, D, B, table, 10, ptr, items, table_planes=tp, table_norm_max=vmax)
        ip, vp = fn()
        same = bool(torch.equal(ip, i3) and torch.equal(vp, v3))
        tq = timeit(fn)
        res[prod] = {"ms": tq, "identical_ids_and_values": same}
        print(f"threshold pass on {prod} product(s): {tq:.2f} ms   identical ids AND values: {same}")
    os.environ.pop("PXR_TOPK_PRODUCTS", None)
    print(f"row_norm_max (once per evaluation): {t_norm:.2f} ms")
    json.dump(res, open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "eval_bench_products.json"), "w"), indent=1)
