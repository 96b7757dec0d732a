#!/usr/bin/env python
"""bench.py -- user-sequences/sec of the SASRec (IDNet) training step at emb=512, seq_len=50 (BASELINE.json).

One "step" = zero_grad -> forward -> backward -> gradient exchange -> AdamW over ALL parameters incl. the whole
400 001 x 512 item table (the reference's trainer.py:116-125 loop body), on one synthetic batch of B sequences per
GPU that is already resident in HBM.  Workload = BASELINE.json configs[1]: SASRec IDNet, N=400 001 items, D=512,
L=50, 4 heads, inner 2x, 2 layers, fp32, dropout 0.1, AdamW lr 1e-4 wd 0.1, B=64 per GPU (the reference's
train_batch_size, overall/ID.yaml:19).  Synthetic ids: Zipf(1.0) positives through a fixed permutation, uniform
negatives, ~30 % left-padded sequences.

  python bench.py [--gpus N --steps K --warmup W]          # N>1 is launched by torch.distributed.run
  python bench.py --full [...]                             # ... and everything measured beside the headline

Prints ONE JSON line on rank 0: value = whole-job sequences/s.  A plain run sets up, ages the optimizer, warms up, times
the K steps, writes --dump-outputs and prints the line -- nothing else.  --full goes on after the timed steps: `roofline`
= the dominant kernel of the step -- the fp32-MFMA GEMM kernel behind every nn.Linear forward/backward (22 launches,
~60 % of the step's GPU time; MFMA-bound) -- `cpu_baseline` = the CPU oracle (plain PyTorch fp32 restatement of the
reference step) timed on this host, plus extra roofline objects for the north-star targets (embedding gather GB/s,
full-catalog scoring GEMM MFMA utilisation) and for the dense AdamW table sweep that the default lazy optimizer avoids.
"""
import argparse
import json
import os
import random
import subprocess
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

NS = dict(n_items=400_001, D=512, L=50, H=4, inner=2, n_layers=2)
HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.3 TB/s achievable)
MFMA_F32_PEAK_TF = 157.3    # MI355X_MICROARCH.md: fp32-input MFMA = fp32 vector peak
MFMA_BF16_PEAK_TF = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA peak (v_mfma_f32_32x32x16_bf16) -- the pipe bf16x3 runs on
B3_PRODUCTS = 6.0           # bf16 products issued per fp32 multiply in GEMM mode bf16x3 (gemm_b3.cuh)


def _pixelnet_traffic(encoder, B):
    """HBM/fabric bytes per GEMM-family launch of the shipped PixelNet shape (PMC passes of tools/r04_session.sh, stage pixelpmc), else None."""
    f = os.path.join(ROOT, "profiles", "r04", "pixelnet", "pixelnet_gemm_traffic_summary.json")
    if encoder != "clip-vit-base-patch16" or B != 16 or not os.path.exists(f):
        return None
    try:
        return json.load(open(f)).get("hbm_bytes_per_launch")
    except Exception:  # noqa: BLE001
        return None


def mfma_roof(alg_flops, seconds, b3, executed_flops=None):
    """`achieved`/`peak`/`frac` of an MFMA-bound kernel against the pipe it RUNS on ("if a bf16-split scheme is
    used quote that peak instead").  bf16x3: achieved = the 16-bit products actually executed (6 per algorithmic fp32 multiply
    on the 3 x bf16 split; `executed_flops` when some launches ran the 3-product fp16 two-plane kernels -- fp16 and bf16 MFMAs
    share the dense peak), peak = that peak; f32: algorithmic fp32 flops against the f32-input MFMA peak.  The algorithmic rate
    and its ratio to the f32-input peak travel as side fields (that ratio is NOT a roofline in bf16x3 mode: it can exceed 1)."""
    alg = alg_flops / seconds / 1e12
    if b3:
        ex = (executed_flops / seconds / 1e12) if executed_flops is not None else B3_PRODUCTS * alg
        r = {"achieved": ex, "peak": MFMA_BF16_PEAK_TF, "unit": "TFLOP/s", "frac": ex / MFMA_BF16_PEAK_TF,
             "pipe": "bf16 MFMA, 6 products per fp32 multiply", "algorithmic_tflops": alg,
             "algorithmic_over_f32_mfma_peak": alg / MFMA_F32_PEAK_TF}
        if executed_flops is not None:
            r["pipe"] = ("bf16 / fp16 MFMA (same dense peak): 6 products per fp32 multiply on the 3 x bf16 split, 3 on the fp16 "
                         "two-plane operands")
            r["products_per_multiply"] = ex / alg if alg else None
            # the same algorithmic rate expressed on the six-product scale of rounds 2-4 (what a six-product kernel would have to
            # sustain to finish in the same time): comparable with earlier rounds' `frac`, NOT a roofline of what was executed
            r["six_product_equivalent_frac"] = B3_PRODUCTS * alg / MFMA_BF16_PEAK_TF
        return r
    return {"achieved": alg, "peak": MFMA_F32_PEAK_TF, "unit": "TFLOP/s", "frac": alg / MFMA_F32_PEAK_TF,
            "pipe": "f32-input MFMA", "algorithmic_tflops": alg, "algorithmic_over_f32_mfma_peak": alg / MFMA_F32_PEAK_TF}


def executed_products(tag):
    """16-bit MFMA products per algorithmic fp32 multiply of a GEMM launch, from the kernel tag ops.py records."""
    return 3.0 if "HALF" in tag else B3_PRODUCTS


def model_config(p_drop=0.1):
    return {"n_layers": NS["n_layers"], "n_heads": NS["H"], "embedding_size": NS["D"], "inner_size": NS["inner"],
            "hidden_dropout_prob": p_drop, "attn_dropout_prob": p_drop, "hidden_act": "gelu",
            "layer_norm_eps": 1e-12, "initializer_range": 0.02, "MAX_ITEM_LIST_LENGTH": NS["L"], "seed": 2020}


def ev_pair():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def time_kernel(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = ev_pair()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def cpu_baseline(batch, budget_s=20.0):
    """The CPU oracle (checker, never the product) timed on this host's cores on a bounded sample."""
    from oracle import sasrec_oracle as O
    from pixelrec_amd import synth

    # all cores up to 32 threads: beyond that the 3.3 GB dense optimizer sweep and the intra-op thread pool stop
    # scaling (measured on the 256-core GPU host: 256 threads ran 60x SLOWER than 8 threads on the dev container); a thread count
    # the environment sets (OMP_NUM_THREADS: the CPUs this job was given) wins over the machine's core count
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS") or 0) or min(os.cpu_count() or 1, 32))
    cores = torch.get_num_threads()
    params = O.synth_params(NS["n_items"], NS["D"], NS["L"], NS["n_layers"], NS["inner"], seed=1, perturb=False)
    cfg = {"n_layers": NS["n_layers"], "n_heads": NS["H"], "layer_norm_eps": 1e-12}
    tr = O.OracleTrainer(params, cfg, lr=1e-4, weight_decay=0.1)
    rng = np.random.default_rng(7)
    zipf = synth.ZipfItems(NS["n_items"], seed=2020)
    items, mask = synth.train_batch(NS["n_items"], batch, NS["L"], rng, zipf)
    items, mask = torch.from_numpy(items), torch.from_numpy(mask)
    tr.step(items, mask)  # warm-up (page faults, thread pool)
    t0 = time.perf_counter()
    steps = 0
    while steps < 10 and (time.perf_counter() - t0) < budget_s:
        tr.step(items, mask)
        steps += 1
    dt = time.perf_counter() - t0
    # the reference launcher pins OMP_NUM_THREADS=1 (main.py:5): one step at one thread, for the record
    torch.set_num_threads(1)
    t1 = time.perf_counter()
    tr.step(items, mask)
    dt1 = time.perf_counter() - t1
    torch.set_num_threads(cores)
    return {"value": batch * steps / dt, "unit": "sequences/s", "cores": cores, "kind": "port",
            "sample": f"{steps} full training steps (fwd+bwd+dense AdamW, dropout off) of B={batch} at the same "
                      f"N=400001/D=512/L=50 config, torch {torch.__version__} CPU fp32, {dt / max(steps, 1):.2f} s/step",
            "one_thread": {"value": batch / dt1, "unit": "sequences/s", "cores": 1,
                           "sample": f"1 step, {dt1:.2f} s (the reference's own launcher setting, OMP_NUM_THREADS=1)"}}


def launch_ranks(args):
    """`python bench.py --gpus N` with N > 1 and no rendezvous in the environment: this process becomes the launcher and starts N
    ranks of itself, one per GPU, through torch.distributed.run (what the reference's launcher does with its `--device` list,
    main.py:21-28, and what `main.py` of this repo does); the ranks print the line.  Under torch.distributed.run (the driver's
    command) WORLD_SIZE is set and this returns at once.  Never a silent 1-rank run: fewer than N visible devices is an error
    (PXR_BENCH_SHARE_GPU=1, development only, puts all ranks on GPU 0 over gloo to exercise the control flow on a 1-GPU box)."""
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if "WORLD_SIZE" in os.environ:
        world = int(os.environ["WORLD_SIZE"])
        if world != args.gpus:
            raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks; pass --gpus {world}")
        return
    if args.gpus == 1:
        return
    n_dev = torch.cuda.device_count()
    if n_dev < args.gpus and os.environ.get("PXR_BENCH_SHARE_GPU") != "1":
        raise SystemExit(f"bench.py: --gpus {args.gpus} needs {args.gpus} visible devices, found {n_dev} "
                         "(one process per GPU; PXR_BENCH_SHARE_GPU=1 shares GPU 0 for a control-flow check only)")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(random.randint(20002, 29999)), os.path.abspath(__file__), *sys.argv[1:]]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.setdefault("OMP_NUM_THREADS", "1")
    sys.stdout.flush()
    raise SystemExit(subprocess.call(cmd, env=env))


def join_world(force=False):
    """-> (rank, local_rank, world, dev, share).  One process per GPU; world > 1 (or `force`) joins the RCCL group (backend "nccl"
    IS RCCL on ROCm); PXR_BENCH_SHARE_GPU=1: every rank on GPU 0 over gloo (development only, its numbers mean nothing)."""
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the product path)")
    share = os.environ.get("PXR_BENCH_SHARE_GPU") == "1"
    if share:
        local_rank = 0
    elif local_rank >= torch.cuda.device_count():
        raise SystemExit(f"bench.py: rank {rank} wants GPU {local_rank} but only {torch.cuda.device_count()} devices are visible")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if (world > 1 or force) and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if share:
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group(backend="nccl", device_id=dev, rank=rank, world_size=world)
    return rank, local_rank, world, dev, share


class _env:
    """Temporarily set environment knobs the library reads per call (PXR_SEQ_H2, PXR_TOWER_H2, ...)."""

    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


OPERANDS_B3 = "bf16x3_six_products"
OPERANDS_H2 = "fp16_two_plane_three_products"


def operand_fields(b3, h2):
    """`operands` / `arithmetic` of the IDNet line: b3 = GEMM mode bf16x3, h2 = the step's GEMMs ran on fp16 two-plane operands."""
    return {
        "operands": ((OPERANDS_H2 if h2 else OPERANDS_B3) if b3 else "f32_input_mfma"),
        "arithmetic": ("fp32 storage and accumulation everywhere; GEMM operands as TWO fp16 planes with a power-of-two scale (22 "
                       "significant bits; three MFMA products per multiply: hi*hi + lo*hi + hi*lo).  Per GEMM of this step no further "
                       "from fp64 than the f32-input MFMA (PXR_GEMM_MODE=f32, the reference's arithmetic class): 0.62-1.02 x its error; a "
                       "40-step AdamW trajectory as close to the f32 mode's as the six-product path's (tests/test_gpu_h2.py::"
                       "test_every_gemm_of_the_step_on_h2_is_no_further_from_fp64_than_the_f32_input_mfma, "
                       "::test_forty_adamw_steps_on_h2_stay_as_close_to_the_f32_mode_as_the_six_product_path; against an fp64 trajectory of "
                       "the same 40 steps the Linear weights end 1.8e-8 rms away on these operands, 2.8e-8 on the f32-input MFMA "
                       "(::test_forty_adamw_steps_against_an_fp64_trajectory_h2_is_no_further_than_the_f32_input_mfma, table in DESIGN.md 2; "
                       "profiles/r05/h2_evidence.log).  The six-product figure of the same run: `six_products` (--full).  Attention, "
                       "LayerNorm, loss, optimizer in fp32" if (b3 and h2) else
                       "fp32 storage and accumulation everywhere; GEMM products on the bf16 matrix pipe after an exact split of "
                       "each fp32 operand into 3 bf16 terms (6 of 9 cross products: error ~2^-25 |a||b| per product, fp32-class; "
                       "tests/test_gpu_gemm_b3.py); attention, LayerNorm, loss, optimizer in fp32" if b3 else
                       "fp32 end to end (f32-input MFMA)")}


def world_fields(world):
    """Top-level fields of the JSON line that say how many ranks really ran and over what."""
    return {"rccl_ranks": world, "dist_backend": (dist.get_backend() if dist.is_initialized() else None)}


LINE_LIMIT = 4096          # the driver parses the LAST stdout line; round 5's 22.6 KB line came back unparsed


def _num(x, digits=6):
    """Shorter float text for the one-line record (the side file keeps full precision)."""
    if isinstance(x, float) and x == x and abs(x) != float("inf"):
        return float(f"{x:.{digits}g}")
    return x


def _pick(d, keys, digits=6):
    return {k: _num(d[k], digits) for k in keys if isinstance(d, dict) and k in d}


def compact_line(out):
    """The ONE stdout line of the contract, cut from the full record: the contract's fields, `roofline` (dominant kernel family),
    `cpu_baseline`, the six-product twin of the headline and where the north-star kernel targets stand -- nothing else.  Everything
    bench.py measures beside that (throughput batches, PixelNet, scoring / gather / AdamW rooflines, spreads, notes) is written to
    the side file named in `extras`.  Always < LINE_LIMIT bytes: optional members are dropped, in a fixed order, until it fits."""
    keep = ("metric", "value", "unit", "n_gpus", "rccl_ranks", "dist_backend", "steps", "warmup", "ms_per_step", "higher_is_better",
            "scaling", "vs_baseline", "dtype", "operands", "data", "final_loss", "host_enqueue_ms_per_step", "h2_stale_overflows", "images_per_s")
    line = {k: _num(out[k], 8) for k in keep if k in out}
    cfg = dict(out.get("config", {}))
    if isinstance(cfg.get("workload"), str) and len(cfg["workload"]) > 200:
        cfg["workload"] = cfg["workload"][:197] + "..."
    cfg.pop("hip_graph_error", None)
    line["config"] = cfg
    r = out.get("roofline") or {}
    roof = _pick(r, ("bound", "achieved", "peak", "unit", "frac", "traffic", "launches_per_step", "avg_kernel_us",
                     "products_per_multiply", "algorithmic_tflops", "gemm_time_per_step_us", "gemm_mode"))
    if "kernel" in r:
        roof["kernel"] = r["kernel"].split(" (")[0][:120]
    if isinstance(r.get("rocprofv3"), dict) and "frac" in r["rocprofv3"]:
        roof["rocprofv3"] = _pick(r["rocprofv3"], ("avg_kernel_us", "achieved", "frac"))
        roof["rocprofv3"]["source"] = r["rocprofv3"].get("source", "").split(" (")[0]
    if r.get("traffic_source"):
        roof["traffic_source"] = r["traffic_source"].split(":")[0]
    line["roofline"] = roof
    cb = out.get("cpu_baseline")
    if isinstance(cb, dict):
        c = _pick(cb, ("value", "unit", "cores", "kind"))
        c["sample"] = str(cb.get("sample", ""))[:160]
        if isinstance(cb.get("one_thread"), dict):
            c["one_thread_value"] = _num(cb["one_thread"].get("value"))
        line["cpu_baseline"] = c
    else:
        line["cpu_baseline"] = cb
    optional = []          # (key, value) in the order they are dropped LAST -> FIRST
    if isinstance(out.get("six_products"), dict):
        optional.append(("six_products", _pick(out["six_products"], ("value", "unit", "ms_per_step", "operands"))))
    t = out.get("targets")
    if isinstance(t, dict):
        g, sc = t.get("gather_ge_0.70_of_hbm_peak", {}), t.get("scoring_ge_0.60_of_mfma_peak", {})
        optional.append(("targets", {
            "gather_frac_of_hbm_peak": {k: _num(v, 4) for k, v in g.items() if isinstance(v, float)}, "gather_met": g.get("met"),
            "scoring_frac_of_mfma_peak": {k: _num(v, 4) for k, v in sc.items() if isinstance(v, float)}, "scoring_met": sc.get("met")}))
    if isinstance(out.get("spread"), dict):
        optional.append(("spread_ms_per_step", [_num(x, 5) for x in out["spread"].get("ms_per_step", [])]))
    tb = [x for x in out.get("throughput_batches", []) if isinstance(x, dict)]
    if tb:
        optional.append(("throughput_batches", [{"batch_per_gpu": x.get("batch_per_gpu"), "value": _num(x.get("value"), 6),
                                                 "operands": x.get("operands")} for x in tb]))
    if isinstance(out.get("pixelnet"), dict) and "ms_per_step" in out["pixelnet"]:
        optional.append(("pixelnet", _pick(out["pixelnet"], ("value", "unit", "ms_per_step", "images_per_s"))))
    if out.get("extras"):
        line["extras"] = out["extras"]
    for k, v in optional:
        line[k] = v
    while len(json.dumps(line)) >= LINE_LIMIT and optional:
        line.pop(optional.pop()[0], None)
    while len(json.dumps(line)) >= LINE_LIMIT:       # pathological strings: cut the longest one
        k = max((k for k in line if isinstance(line[k], str)), key=lambda k: len(line[k]))
        line[k] = line[k][:len(line[k]) // 2]
    return line


def emit(out):
    """Full record -> the side file (PXR_BENCH_EXTRAS, default gpurun_out/bench_extras.json under the repo); compact record -> the
    last stdout line (print_line)."""
    path = os.environ.get("PXR_BENCH_EXTRAS") or os.path.join(ROOT, "gpurun_out", "bench_extras.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f)
            f.write("\n")
        out["extras"] = os.path.relpath(path, ROOT)
    except OSError as e:
        out["extras"] = f"not written ({type(e).__name__})"
    print_line(out)


def print_line(out):
    """Compact record -> the last stdout line (a plain run prints only this).  RCCL prints its version banner through C stdio
    (NCCL_DEBUG=VERSION may be exported) and that buffer is only flushed at exit: flush it first so the JSON line is the LAST
    line on stdout."""
    import ctypes
    ctypes.CDLL(None).fflush(None)
    text = json.dumps(compact_line(out))
    assert len(text) < LINE_LIMIT and "\n" not in text
    print(text, flush=True)


DUMP_LIMIT_BYTES = 64 << 20    # --dump-outputs: the whole dump stays under this
DUMP_SAMPLE_SEED = 2020


def dump_outputs(path, loss, model, write=True):
    """--dump-outputs: what the timed path hands its caller after its LAST timed step -- the step's loss and the parameters as
    `model.state_dict()` returns them (lazily updated table rows brought current) -- as `<path>/<name>.npy`, float32 (float64 stays
    float64).  A tensor too large for the budget is cut to a fixed, seeded sample of its elements (sorted flat indices drawn from
    DUMP_SAMPLE_SEED and the tensor's size alone), so two builds run with the same arguments compare output for output.  Every rank
    calls this (the flush must happen on all replicas alike); only the one with `write` writes.  -> summary for the full record."""
    sd = {k: v for k, v in model.state_dict().items() if v.is_floating_point()}
    arrays = {"loss": loss.detach().reshape(1)}
    width = 8 if any(v.dtype == torch.float64 for v in sd.values()) else 4
    cap = (DUMP_LIMIT_BYTES - 256 * (len(sd) + 1)) // width // max(len(sd), 1)   # elements per tensor (256 B: room for a header)
    for k, v in sd.items():
        flat = v.detach().reshape(-1)
        if flat.numel() > cap:
            idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(flat.numel(), cap, replace=False))
            arrays[k] = flat[torch.from_numpy(idx).to(flat.device)]
        else:
            arrays[k] = v.detach()
    if not write:
        return None
    os.makedirs(path, exist_ok=True)
    total, sampled = 0, []
    for k, t in arrays.items():
        a = t.cpu().numpy()
        a = a.astype(np.float64 if a.dtype == np.float64 else np.float32, copy=False)
        total += a.nbytes + 256
        if t.numel() != sd.get(k, t).numel():
            sampled.append(k)
        np.save(os.path.join(path, f"{k}.npy"), a)
    assert total <= DUMP_LIMIT_BYTES, total
    return {"dir": path, "arrays": len(arrays), "bytes": total, "sampled": sampled, "sample_seed": DUMP_SAMPLE_SEED}


def pixelnet_main(args):
    out = pixelnet_run(args, args.steps, max(args.warmup, 2), full=args.full)
    if out is not None:
        (emit if args.full else print_line)(out)
    if dist.is_initialized():
        dist.destroy_process_group()


def pixelnet_run(args, steps, warmup, init_dist=True, n_inst=3, full=True):
    """BASELINE configs[2] / [4]: one training step of MOSASRec (reference mosasrec.py:66-93) with the image encoder
    trained end to end (blocks >= tune_scale; reference load.py:90-120), both optimizer groups (trainer.py:74-96).
    Synthetic images already resident in HBM as fp32 pixel tensors; random-init weights of the named architecture.
    `full`: after the timed steps, instrumented eager steps for the GEMM roofline, the phases and `operands`."""
    from pixelrec_amd import ops
    from pixelrec_amd.model import MOSASRec
    from pixelrec_amd.model.visual import ENCODER_SHAPES
    from pixelrec_amd.optim import OptimizerGroup, PxrAdamW, VisualAdamW
    from pixelrec_amd.parallel import DataParallel

    if init_dist:
        rank, local_rank, world, dev, _ = join_world()
    else:
        rank, local_rank, world = 0, torch.cuda.current_device(), 1
        dev = torch.device("cuda", local_rank)
    hidden, n_layers, heads, inter, image, patch = ENCODER_SHAPES[args.encoder]
    B = 16 if args.batch == 64 else args.batch           # the reference's PixelNet batch (overall/ViT.yaml)
    L, D = 10, 512
    tune = 5 + 16 * (n_layers - 2) if args.encoder != "clip-vit-base-patch16" else 165      # ViT.yaml: tune_scale 165
    cfg = {"n_layers": 2, "n_heads": 4, "embedding_size": D, "inner_size": 2, "hidden_dropout_prob": 0.1,
           "attn_dropout_prob": 0.1, "hidden_act": "gelu", "layer_norm_eps": 1e-12, "initializer_range": 0.02,
           "MAX_ITEM_LIST_LENGTH": L, "seed": 2020, "encoder_name": args.encoder, "encoder_source": "transformers",
           "pretrain_path": None,
           "fine_tune_arg": {"tune_scale": tune, "pre_trained": False, "allow_random_backbone": True, "activation": "relu", "dnn_layers": [],
                             "method": "mean"}}

    class DL:
        item_num = 96_001

    torch.manual_seed(2020)
    m = MOSASRec(cfg, DL()).to(dev).train()
    dp = DataParallel(m)
    opt = OptimizerGroup(VisualAdamW(m.visual_encoder, lr=1e-4, weight_decay=0.0), PxrAdamW(m, lr=1e-4, weight_decay=0.1))
    g = torch.Generator(device=dev).manual_seed(1 + rank)
    pool = [(torch.randn(B, 2 * (L + 1), 3, image, image, device=dev, generator=g),
             torch.ones(B, L, dtype=torch.int64, device=dev)) for _ in range(2)]
    one = torch.ones((), dtype=torch.float32, device=dev)

    def opt_step():
        try:
            opt.step()
        except ops.H2StaleOverflow:        # (the optimizer's status poll, after the step has run: see step() below)
            pass

    def eager_step(i):
        opt.zero_grad()
        loss = dp(pool[i % 2])
        loss.backward(one)
        dp.sync_gradients(defer_flat=True)
        opt_step()
        return loss

    for i in range(warmup):
        eager_step(i)
    torch.cuda.synchronize()
    # the whole step -- image tower forward, backward of its trainable blocks, sequence block, both optimizer groups -- as ONE
    # captured hipGraph (round 5: VisualAdamW keeps its step number on the device like PxrAdamW); data parallel over RCCL: the
    # collectives are captured with it (round 6; --no-graph-collectives issues eagerly)
    gstep, graph_err = None, None
    rccl = world > 1 and dist.is_initialized() and dist.get_backend() == "nccl" and not getattr(args, "no_graph_collectives", False)
    if (world == 1 or rccl) and not getattr(args, "no_graph", False):
        try:
            from pixelrec_amd.graph import GraphedTrainStep
            gstep = GraphedTrainStep(dp, opt, *pool[0], warmup=1)
        except Exception as e:  # noqa: BLE001 -- the line then says hip_graph false and why
            gstep, graph_err = None, f"{type(e).__name__}: {e}"
            torch.cuda.synchronize()

    def step(i):
        try:
            if gstep is not None:
                return gstep(*pool[i % 2])
            return eager_step(i)
        except ops.H2StaleOverflow:        # (see main(): the step has run; a rank must not leave the others in a collective)
            return gstep.loss if gstep is not None else torch.zeros((), device=dev)

    for i in range(2 if gstep is not None else 0):
        step(i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        loss = step(i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    dump_dir = getattr(args, "dump_outputs", None) if init_dist else None
    dumped = dump_outputs(dump_dir, loss, m, write=rank == 0) if dump_dir else None
    # GEMM family of the step (ViT blocks + sequence block): HIP events around every launch of a few extra steps
    # (--full only, like the phases below: a plain run ends with its timed steps)
    ev = []
    ops.GEMM_TIMING = ev
    n_inst = min(steps, n_inst) if full else 0
    for i in range(n_inst):
        eager_step(i)
    ops.GEMM_TIMING = None
    torch.cuda.synchronize()
    # where a step's device time goes (events on the compute stream around the four host-level phases of `step`)
    ph_acc, n_ph = {}, min(steps, 3) if full else 0
    for i in range(n_ph):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        marks[0].record()
        opt.zero_grad()
        l_ = dp(pool[i % 2]); marks[1].record()
        l_.backward(one); marks[2].record()
        dp.sync_gradients(defer_flat=True); marks[3].record()
        opt_step(); marks[4].record()
        torch.cuda.synchronize()
        for k, nm in enumerate(("forward (tower + sequence block + loss)", "backward (sequence block, trainable tower blocks, weight gradients)",
                                "gradient exchange (enqueue; the flat all-reduces are joined in the optimizer)", "optimizer (both groups)")):
            ph_acc[nm] = ph_acc.get(nm, 0.0) + marks[k].elapsed_time(marks[k + 1]) / n_ph
    gsync = getattr(dp, "grad_sync", None)
    if rank != 0:
        return None
    gem = [(s_.elapsed_time(e_) * 1e-3, w, tag) for s_, e_, w, tag in ev if tag.startswith("gemm") or tag.startswith("grouped_dw")]
    g_s, g_fl = sum(x for x, _, _ in gem) or float("nan"), sum(w for _, w, _ in gem)
    g_ex = sum(w * executed_products(tag) for _, w, tag in gem)
    h2_s, h2_fl = sum(x for x, _, tag in gem if "HALF" in tag), sum(w for _, w, tag in gem if "HALF" in tag)
    n_img = B * 2 * (L + 1)
    T = (image // patch) ** 2 + 1
    out = {"metric": f"user-sequences/sec, SASRec PixelNet + {args.encoder} end to end (training step: image encoder fwd, "
                     "bwd of the trainable blocks, sequence block, both AdamW groups)",
           "value": world * B * steps / dt, "unit": "sequences/s", "n_gpus": world, **world_fields(world), "steps": steps,
           "warmup": warmup, "ms_per_step": dt / steps * 1e3, "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": f"BASELINE.json configs[2]-shaped: SASRec PixelNet + {args.encoder}, train_batch_size {B}, "
                                  f"MAX_ITEM_LIST_LENGTH {L} ({n_img} images of {image}x{image} = {n_img * T} tokens per step), "
                                  f"emb {D}, tune_scale {tune} ({(391 if n_layers == 24 else 199) - tune} trainable encoder tensors)",
                      "batch_per_gpu": B, "global_batch": world * B, "seq_len": L, "images_per_step": n_img,
                      "parallelism": f"dp{world}", "hip_graph": gstep is not None,
                      **({"hip_graph_error": graph_err} if graph_err else {})},
           "images_per_s": world * n_img * steps / dt, "final_loss": float(loss.detach()),
           **({"dumped_outputs": dumped} if dumped else {}),
           "operands": (OPERANDS_H2 + " (every ViT block and the sequence block; rec_fc: " + OPERANDS_B3 + ")") if h2_fl else
                       (OPERANDS_B3 if ops.gemm_mode() == "bf16x3" else "f32_input_mfma"),
           "data_parallel_phases": {"ms": ph_acc, "rccl_ranks": world if (gsync is not None and getattr(gsync, "active", False)) else 1,
                                    "note": "eager steps, events on the compute stream; with one rank no collective is issued"},
           "roofline": {"bound": "mfma", "gemm_mode": ops.gemm_mode(),
                        "kernel": "gemm_p3_kernel<P4Cfg 256x256 | 256x128> (ping-pong planes tiles, gemm_p4.cuh) + grouped_dw_p3_kernel: "
                                  "v_mfma_f32_32x32x16_f16 on two fp16 planes per operand (3 products per multiply: every ViT block -- "
                                  "forward, input and weight gradients; `fp16_two_plane`) and v_mfma_f32_32x32x16_bf16 on the exact "
                                  "3 x bf16 split (6 products: rec_fc, sequence block), operands pre-split as planes; f32 mode: "
                                  "gemm_kernel (v_mfma_f32_32x32x2_f32) -- see gemm_mode",
                        **mfma_roof(g_fl, g_s, ops.gemm_mode() == "bf16x3", g_ex if h2_fl else None),
                        "fp16_two_plane": ({"gemm_time_per_step_ms": h2_s / max(n_inst, 1) * 1e3,
                                            "algorithmic_gflop_per_step": h2_fl / max(n_inst, 1) / 1e9,
                                            "achieved": 3.0 * h2_fl / h2_s / 1e12, "frac": 3.0 * h2_fl / h2_s / 1e12 / MFMA_BF16_PEAK_TF,
                                            "algorithmic_tflops": h2_fl / h2_s / 1e12,
                                            "note": "the launches on fp16 two-plane operands alone (3 products per multiply executed); "
                                                    "PXR_TOWER_H2=0 puts them back on the six-product bf16x3 kernels"}
                                           if h2_fl else None),
                        "traffic": _pixelnet_traffic(args.encoder, B),
                        "gemm_time_per_step_ms": g_s / max(n_inst, 1) * 1e3, "algorithmic_gflop_per_step": g_fl / max(n_inst, 1) / 1e9,
                        "launches_per_step": len(gem) / max(n_inst, 1),
                        "traffic_source": "profiles/r04/pixelnet/pixelnet_gemm_traffic_summary.json (separate rocprofv3 --pmc passes of "
                                          "`bench.py --model pixelnet` on this round's ping-pong tiles; NOT measured in this run)",
                        "note": "HIP events around every GEMM launch of extra eager steps (sum of durations; one stream)"},
           "cpu_baseline": None}
    if not full:        # nothing was instrumented
        for k in ("operands", "data_parallel_phases", "roofline"):
            del out[k]
    del m, dp, opt, pool, gstep
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64, help="sequences per GPU per step (reference: 64)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, measure everything else: spread blocks, the six-product twin, the GEMM roofline "
                         "(instrumented eager steps), lazy-schedule figures, the extras of bench_extras.py and the CPU baseline; "
                         "writes the full record to a side file.  A plain run (the default) only sets up, warms up, times the "
                         "steps, writes --dump-outputs and prints the line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU oracle baseline")
    ap.add_argument("--no-extras", action="store_true", help="--full: skip the spread blocks and the extra measurement runs")
    ap.add_argument("--no-overlap", action="store_true", help="weight gradients on the main stream (A/B knob)")
    ap.add_argument("--no-group", action="store_true", help="per-layer weight-gradient GEMMs instead of one grouped launch")
    ap.add_argument("--no-graph", action="store_true", help="issue the step eagerly instead of replaying a hipGraph")
    ap.add_argument("--no-gemm-events", action="store_true", help="--full: do not bracket GEMM launches with HIP events")
    ap.add_argument("--clock-ramp-s", type=float, default=0.0, help="seconds of extra untimed steps before the warm-up")
    ap.add_argument("--age-steps", type=int, default=600,
                    help="untimed steps on DISTINCT batches before the warm-up: they bring the lazily updated table rows "
                         "to the steady-state distribution of gaps an epoch presents (and ramp the clocks)")
    ap.add_argument("--table-update", choices=("lazy", "dense"), default="lazy",
                    help="table AdamW schedule (dense = sweep all rows every step; eager only)")
    ap.add_argument("--dw-mode", default=None, help="weight-gradient placement: grouped | fork_tail | fork_layer | fork_half")
    ap.add_argument("--split-exchange", action="store_true",
                    help="data parallel: force the reduced-capacity two-collective row exchange (default from 4 ranks up)")
    ap.add_argument("--full-exchange", action="store_true",
                    help="data parallel: exchange the worst-case B*(2L+1) row slots (one collective) instead of the bound "
                         "computed from the batch stream (two collectives)")
    ap.add_argument("--lookahead", action="store_true",
                    help="hand the next batch's ids to the model (look-ahead catch-up of its table rows on a side stream; "
                         "measured slower on MI355X, off by default)")
    ap.add_argument("--emb", type=int, default=NS["D"], help="embedding size (default: the north-star 512)")
    ap.add_argument("--heads", type=int, default=NS["H"])
    ap.add_argument("--items", type=int, default=NS["n_items"], help="catalogue size incl. the padding id")
    ap.add_argument("--seq-len", type=int, default=NS["L"])
    ap.add_argument("--table-sharding", action="store_true",
                    help="row-shard the item table over the ranks (pixelrec_amd/model/sharded.py) instead of replicating it")
    ap.add_argument("--force-collectives", action="store_true",
                    help="1-GPU validation knob: create a 1-rank RCCL group and run every gradient collective anyway")
    ap.add_argument("--graph-collectives", action="store_true", help="(default since round 6; kept for old command lines)")
    ap.add_argument("--no-graph-collectives", action="store_true",
                    help="data parallel: issue the step eagerly instead of replaying a hipGraph that contains the RCCL collectives")
    ap.add_argument("--emulate-world", type=int, default=0,
                    help="--full: after the run, project the step of a W-rank data-parallel job on this ONE GPU: merge of W ranks' "
                         "sparse-gradient blocks + the merged row update are measured on a run fed W batches per step, the "
                         "collectives are modelled from bytes and a stated xGMI link rate (tools/world_projection.py)")
    ap.add_argument("--model", choices=("idnet", "pixelnet"), default="idnet",
                    help="idnet = the headline (BASELINE configs[1]); pixelnet = SASRec PixelNet + ViT end to end "
                         "(BASELINE configs[2]: train_batch_size 16, MAX_ITEM_LIST_LENGTH 10, 352 images per step)")
    ap.add_argument("--encoder", default="clip-vit-base-patch16", help="--model pixelnet: image encoder")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last of them computed (the loss and the parameters as "
                         "state_dict() returns them; a fixed seeded sample of the large ones, <= 64 MB in all) as DIR/<name>.npy. "
                         "The table is brought current there, so the untimed measurements after it start from a flushed table")
    args = ap.parse_args()
    if args.emulate_world > 1 and not args.full:
        ap.error("--emulate-world is a measurement beside the headline: add --full")
    launch_ranks(args)
    if args.model == "pixelnet":
        return pixelnet_main(args)
    custom = (args.emb, args.heads, args.items, args.seq_len) != (NS["D"], NS["H"], NS["n_items"], NS["L"]) or args.table_sharding
    NS.update(D=args.emb, H=args.heads, n_items=args.items, L=args.seq_len)   # other BASELINE configs on request

    rank, local_rank, world, dev, share = join_world(force=args.force_collectives)

    from pixelrec_amd import ops, synth
    from pixelrec_amd.model import SASRec
    from pixelrec_amd.optim import PxrAdamW
    from pixelrec_amd.parallel import DataParallel

    torch.manual_seed(2020)

    class DL:
        item_num = NS["n_items"]

    B, L, D, N = args.batch, NS["L"], NS["D"], NS["n_items"]
    if args.table_sharding:
        from pixelrec_amd.model import ShardedDataParallel, ShardedSASRec as SASRec   # noqa: F811
    with torch.device(dev):
        model = SASRec(model_config(0.1), DL())  # random-init weights of the reference architecture
    model.train()
    if args.no_group:
        model.group_weight_grads = False
        model.overlap_weight_grads = not args.no_overlap
    if args.dw_mode:
        model.weight_grad_mode = args.dw_mode
    model.defer_weight_grad_join = True      # every step below ends in opt.step(), which joins the side stream
    model.trust_optimizer_planes = True      # ... and nothing but the optimizer rewrites the weights between forwards
    model.h2_stale_scales = True             # ... in a loop of similar steps (what GraphedTrainStep / the Trainer set)
    opt = None

    # synthetic batches, rank-distinct, resident in HBM before the timed region.  The stream does NOT repeat inside
    # ageing + warm-up + timed steps (+ the instrumented steps after them): a lazily updated table row returns after the
    # gap its popularity dictates (Zipf positives, uniform negatives: mean ~120 steps at B=64), and the catch-up that
    # replays those steps is paid inside the timed region.
    rng = np.random.default_rng(2020 + 1000 * rank)
    zipf = synth.ZipfItems(N, seed=2020)
    n_inst_plan = 0 if args.no_gemm_events else min(args.steps, 20)
    n_spread = 0 if args.no_extras else 4          # extra blocks of --steps steps timed like the official one (box / clock spread)
    n_stream = min(args.age_steps + 2 * args.warmup + (2 + n_spread) * args.steps + n_inst_plan + 40, 4096)
    # two collectives with fewer rows pay off when the volume dominates the exchange (W x rows per rank received); at 1-2
    # ranks the extra collective costs more than the bytes it saves (1-rank RCCL group: 1.273 vs 1.249 ms/step)
    want_split = args.split_exchange or (world >= 4 and not args.full_exchange)
    split = (world > 1 or args.force_collectives) and want_split and not args.table_sharding
    # a plain run draws only the batches its own steps consume (+ the look-ahead's): the stream is drawn in order, so these are
    # the same batches, and it still wraps at n_stream.  The split exchange's row bound is taken over the whole stream
    n_draw = n_stream
    if not (args.full or split or args.clock_ramp_s > 0):
        n_draw = min(n_stream, args.age_steps + args.warmup + args.steps + 1)
    t_gen = time.perf_counter()
    its, mks = zip(*(synth.train_batch(N, B, L, rng, zipf) for _ in range(n_draw)))
    # a rigorous bound on the unique table rows any batch of THIS stream touches: the row capacity of the data-parallel
    # exchange (GradSync(exchange_rows=...)); all ranks agree on the maximum once, before the first step
    max_unique = max(int(np.count_nonzero(np.unique(it))) for it in its)
    # every batch is ONE packed int64 row (ids | mask), the two tensors are views of it: the graphed step copies a batch
    # into its static buffer with one copy (pixelrec_amd/graph.py)
    n_it = its[0].size
    packed_all = torch.from_numpy(np.concatenate([np.stack(its).reshape(n_draw, -1),
                                                  np.stack(mks).reshape(n_draw, -1).astype(np.int64)], axis=1)).to(dev)
    items_shape, mask_shape = its[0].shape, mks[0].shape
    t_gen = time.perf_counter() - t_gen
    del its, mks

    exchange_rows = None
    if split:
        t_mx = torch.tensor([max_unique], dtype=torch.int64, device=dev)
        dist.all_reduce(t_mx, op=dist.ReduceOp.MAX)
        exchange_rows = min(B * (2 * L + 1), (int(t_mx.item()) + 255) // 256 * 256)
    dp = (ShardedDataParallel(model, force_collectives=args.force_collectives) if args.table_sharding
          else DataParallel(model, force_collectives=args.force_collectives, exchange_rows=exchange_rows))
    opt = PxrAdamW(model, lr=1e-4, weight_decay=0.1, table_update=args.table_update)

    class _Pool:
        def __len__(self):
            return n_stream

        def __getitem__(self, i):
            row = packed_all[i]
            return row[:n_it].view(items_shape), row[n_it:].view(mask_shape)

    pool = _Pool()

    gemm_events = []
    # data parallel: the captured step contains its RCCL collectives (round 6 default: the eager multi-rank step is host-bound --
    # 1.47 ms against 0.85 ms replayed on a 1-rank RCCL group, profiles/r06).  Not over gloo (PXR_BENCH_SHARE_GPU: CPU staging).
    collectives = world > 1 or args.force_collectives
    use_graph = (not args.no_graph) and (not collectives or (not args.no_graph_collectives and dist.get_backend() == "nccl"))
    use_graph = use_graph and not args.table_sharding      # the sharded forward issues collectives: eager only
    use_graph = use_graph and args.table_update == "lazy"   # the dense sweep takes host-computed scalars
    gstep = None
    graph_err = None
    if use_graph:
        from pixelrec_amd.graph import GraphedTrainStep

        try:
            gstep = GraphedTrainStep(dp, opt, *pool[0], lookahead=not (not args.lookahead))
        except Exception as e:  # noqa: BLE001 -- a capture that fails is reported (stderr + `hip_graph_error`), the run goes on eagerly
            if not collectives:
                raise
            graph_err = f"{type(e).__name__}: {e}"
            print(f"bench.py: hipGraph capture of the data-parallel step failed ({graph_err}); issuing steps eagerly", file=sys.stderr)
            gstep, use_graph = None, False
            torch.cuda.synchronize()
        if collectives:        # every rank replays or none does: a mixed world would deadlock in the first collective
            ok = torch.tensor([1 if gstep is not None else 0], device=dev)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if int(ok.item()) == 0 and gstep is not None:
                gstep, use_graph, graph_err = None, False, "another rank failed to capture"

    one = torch.ones((), dtype=torch.float32, device=dev)
    cursor = [0]          # position in the batch stream: every step of every phase consumes the NEXT batch

    def next_batch():
        b = pool[cursor[0] % len(pool)]
        cursor[0] += 1
        return b

    def peek_items():
        """ids of the batch AFTER the one just handed out (the look-ahead a data loader's prefetch queue provides)."""
        return None if (not args.lookahead) else pool[cursor[0] % len(pool)][0]

    from types import SimpleNamespace
    state = SimpleNamespace(opt=opt)      # the optimizer eager_step steps (bench_extras swaps in the dense-sweep one for an A/B)

    stale_overflows = [0]

    def eager_step(batch, nxt=None):
        state.opt.zero_grad()
        if nxt is not None and hasattr(model, "set_next_batch"):
            model.set_next_batch(nxt)
        loss = dp(batch)
        loss.backward(one)       # preallocated d(loss)/d(loss): no ones_like fill per step
        dp.sync_gradients(defer_flat=True)
        try:
            state.opt.step()
        except ops.H2StaleOverflow:      # the optimizer's status poll, after the step has run (see step())
            stale_overflows[0] += 1
        return loss

    def replay(g, *b, **kw):
        """A captured step outside step() (the six-product twin, bench_extras): an overflow report is counted like step()'s."""
        try:
            return g(*b, **kw)
        except ops.H2StaleOverflow:
            stale_overflows[0] += 1
            return g.loss

    def step(i=None, record=False):
        b = next_batch()
        try:
            if gstep is not None:
                return gstep(*b, next_items=peek_items())
            return eager_step(b, peek_items())
        except ops.H2StaleOverflow:
            # raised by the status poll AFTER a step in which a gradient outgrew the headroom of its stale h2 scale (saturated there,
            # nothing non-finite written; model/seqcore.py): counted and reported in the line (`h2_stale_overflows`), the run goes on --
            # in a multi-rank job a rank that stopped here would leave the others hanging in the next collective
            stale_overflows[0] += 1
            return gstep.loss if gstep is not None else torch.zeros((), device=dev)

    def step_e():
        b = next_batch()
        return eager_step(b, peek_items())

    ref_ev = torch.cuda.Event(enable_timing=True)

    def instrumented_step(i=None):
        """Same step, eager, with HIP events around every GEMM launch (run AFTER the timed region)."""
        ops.GEMM_TIMING = gemm_events
        b = next_batch()
        loss = eager_step(b, peek_items())
        ops.GEMM_TIMING = None
        return loss

    # clock ramp: a cold process starts with the GPU at its idle clocks (sclk ~600 MHz); ~0.3 s of the same work before
    # the W counted warm-up steps keeps short runs from timing the governor instead of the step (untimed, like warm-up)
    t_ramp, i_ramp = time.perf_counter(), 0
    while args.clock_ramp_s > 0:
        for _ in range(8):
            step(i_ramp)
            i_ramp += 1
        torch.cuda.synchronize()
        if time.perf_counter() - t_ramp >= args.clock_ramp_s:
            break
    # ageing: real steps on distinct batches (untimed, like warm-up).  Afterwards the per-row "current through" stamps
    # have the gap distribution of a running epoch instead of a freshly initialised optimizer's
    t_age = time.perf_counter()
    for i in range(args.age_steps):
        step(i)
    torch.cuda.synchronize()
    t_age = time.perf_counter() - t_age
    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = step(i, record=True)
    t_enqueued = time.perf_counter() - t0   # host time to issue the K steps (== total when host-bound)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    final_loss = float(loss.detach())
    dumped = dump_outputs(args.dump_outputs, loss, model, write=rank == 0) if args.dump_outputs else None
    b3 = ops.gemm_mode() == "bf16x3"
    out = {
        "metric": (f"user-sequences/sec at emb={D} seq_len={L} (SASRec IDNet training step: fwd+bwd+AdamW)" if custom else
                   "user-sequences/sec at emb=512 seq_len=50 (SASRec IDNet training step: fwd+bwd+AdamW)"),
        "value": world * B * args.steps / dt, "unit": "sequences/s", "n_gpus": world, **world_fields(world), "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        # (the model's own switch; --full replaces it with what the instrumented launches ran)
        **operand_fields(b3, b3 and bool(getattr(model, "_h2_on", lambda b_: False)(B))),
        "config": {"workload": (f"custom shape (NOT the headline config): SASRec IDNet emb={D} seq_len={L}, {N} items, "
                                f"{NS['H']} heads, inner 2x, 2 layers" if custom else
                                "BASELINE.json configs[1]: SASRec IDNet emb=512 seq_len=50, 400001 items, 4 heads, "
                                "inner 2x, 2 layers, BPR loss vs 1 sampled negative, dropout 0.1, AdamW lr 1e-4 wd 0.1"),
                   "batch_per_gpu": B, "global_batch": world * B, "seq_len": L, "n_items": N, "embedding_size": D,
                   "parallelism": f"dp{world}" + ("+row-sharded-table" if args.table_sharding else ""),
                   "hip_graph": bool(use_graph), **({"hip_graph_error": graph_err} if graph_err else {})},
        "final_loss": final_loss, "host_enqueue_ms_per_step": t_enqueued / args.steps * 1e3, "h2_stale_overflows": stale_overflows[0],
        **({"dumped_outputs": dumped} if dumped else {}),
    }
    if not args.full:
        # a plain run ends with its timed steps: the line carries the headline and nothing measured beside it
        if rank == 0:
            print_line(out)
        if dist.is_initialized():
            dist.destroy_process_group()
        return
    # ---- --full: everything below is measured after (and beside) the headline ----------------------------------------------
    # the same K steps four more times (continuing the batch stream), each block bracketed like the official one: what one run can
    # say about the spread of its own number (boxes of the pool differ by a few percent, clocks move).
    # `value` / `ms_per_step` stay the FIRST block -- the contract's timed region.
    block_ms = [dt / args.steps * 1e3]
    for _ in range(n_spread):
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        tb0 = time.perf_counter()
        for i in range(args.steps):
            step(i)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        tb1 = time.perf_counter() - tb0
        if world > 1:
            tt = torch.tensor([tb1], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            tb1 = float(tt.item())
        block_ms.append(tb1 / args.steps * 1e3)
    # the same step on the OTHER arithmetic, same session (every figure on fp16 two-plane operands travels with
    # its six-product twin): a second captured step under PXR_SEQ_H2=0, warmed up and timed like the headline
    six = None
    if (not args.no_extras) and world == 1 and gstep is not None and ops.gemm_mode() == "bf16x3" and getattr(model, "_h2_on", lambda b: False)(B):
        from pixelrec_amd.graph import GraphedTrainStep
        with _env(PXR_SEQ_H2="0"):
            g6 = GraphedTrainStep(dp, opt, *pool[cursor[0] % len(pool)], lookahead=not (not args.lookahead))
            for i in range(args.warmup):
                replay(g6, *next_batch(), next_items=peek_items())
            torch.cuda.synchronize()
            t6 = time.perf_counter()
            for i in range(args.steps):
                replay(g6, *next_batch(), next_items=peek_items())
            torch.cuda.synchronize()
            t6 = time.perf_counter() - t6
        six = {"value": B * args.steps / t6, "unit": "sequences/s", "ms_per_step": t6 / args.steps * 1e3, "steps": args.steps,
               "operands": OPERANDS_B3, "PXR_SEQ_H2": "0",
               "note": "the same captured step with every GEMM on the exact 3 x bf16 split (six products per multiply), continuing the "
                       "batch stream right after the timed region"}
        del g6
    stream_repeats = cursor[0] > len(pool)
    # what the lazy schedule replayed in the steps just timed: gaps (in steps) of the NEXT batches' unique rows
    lazy_gaps = None
    if args.table_update == "lazy" and opt._last is not None:
        g_all = []
        for j in range(8):
            ids = torch.unique(pool[(cursor[0] + j) % len(pool)][0])
            ids = ids[ids > 0]
            g_all.append((opt.step_count - opt._last[ids].long()).clamp_(min=0).float())
        gaps = torch.cat(g_all)
        qs = torch.quantile(gaps, torch.tensor([0.5, 0.9, 0.99], device=dev)).tolist()
        lazy_gaps = {"unique_rows_per_step": gaps.numel() / 8.0, "mean": float(gaps.mean()), "p50": qs[0], "p90": qs[1],
                     "p99": qs[2], "max": float(gaps.max()), "frac_ge_256": float((gaps >= 256).float().mean()),
                     "mean_replayed_steps": float(gaps.clamp(max=256).mean()),
                     "note": "steps since each unique row of the next 8 batches was last brought current (= zero-gradient "
                             "AdamW steps replayed per row, exactly for <= 256, closed form beyond)"}
    n_inst = 0
    if not args.no_gemm_events:
        n_inst = n_inst_plan
        ref_ev.record()
        for i in range(n_inst):
            instrumented_step(i)
        torch.cuda.synchronize()
    # data parallel: where a step's device time goes (exchange wait, merge, optimizer), from events on the compute stream
    phases = None
    gsync = getattr(dp, "grad_sync", None)
    if gsync is not None and gsync.active and not args.table_sharding:
        acc, n_ph = {}, 10
        for _ in range(n_ph):
            marks = []
            gsync.phase_events = marks
            e0 = torch.cuda.Event(enable_timing=True); e0.record()
            b = next_batch()
            eager_step(b, peek_items())
            e1 = torch.cuda.Event(enable_timing=True); e1.record()
            gsync.phase_events = None
            torch.cuda.synchronize()
            names = ["step_start"] + [n for n, _ in marks] + ["step_end"]
            evs = [e0] + [e for _, e in marks] + [e1]
            for (na, ea), (nb, eb) in zip(zip(names, evs), zip(names[1:], evs[1:])):
                acc[f"{na}->{nb}"] = acc.get(f"{na}->{nb}", 0.0) + ea.elapsed_time(eb) * 1e3 / n_ph
        phases = {"us": acc, "rccl_ranks": world, "exchange_rows_per_rank": exchange_rows or B * (2 * L + 1),
                  "exchange_collectives": 2 if exchange_rows else 1,
                  "note": "eager steps; step_start->exchange_start = forward + input-gradient chain + segmented sum; "
                          "exchange_start->exchange_done = grouped weight-gradient GEMM + whatever of the all-gather it did not "
                          "hide; exchange_done->merge_done = rank merge; merge_done->step_end = row update, flat all-reduce "
                          "wait, flat update"}
    # the same eager step without the event brackets (the host keeps up at B=64): reference point for the dense A/B
    t_eager = None
    if world == 1 and not args.no_extras:
        for _ in range(3):
            step_e()
        torch.cuda.synchronize()
        t_eager = time.perf_counter()
        for _ in range(20):
            step_e()
        torch.cuda.synchronize()
        t_eager = (time.perf_counter() - t_eager) / 20
    # the amortised part of the lazy schedule: flush() brings EVERY row current (before an evaluation / checkpoint)
    lazy_flush = None
    if world == 1 and not args.no_extras and args.table_update == "lazy" and opt._last is not None:
        behind = (opt.step_count - opt._last.long()).clamp_(min=0).float()
        behind_stats = {"mean": float(behind.mean()), "max": float(behind.max()), "frac_current": float((behind == 0).float().mean())}
        torch.cuda.synchronize()
        tf = time.perf_counter()
        opt.flush()
        torch.cuda.synchronize()
        tf = time.perf_counter() - tf
        steps_per_epoch = 200_000 // B      # Pixel200K: one full-sort evaluation (hence one flush) per epoch
        lazy_flush = {"ms": tf * 1e3, "rows": N, "steps_behind": behind_stats,
                      "amortised_us_per_step": tf * 1e6 / steps_per_epoch,
                      "note": f"one flush per epoch of {steps_per_epoch} steps (Pixel200K users / {B}); every row is replayed "
                              "<= 256 steps exactly + closed form"}

    if rank != 0:
        if dist.is_initialized():
            dist.destroy_process_group()
        return

    # ---- roofline of the dominant kernel: the fp32-MFMA GEMM (all launches of the timed steps, HIP events) ------
    is_gemm = lambda tag: tag.startswith("gemm") or tag.startswith("grouped_dw")
    other_events = [ev for ev in gemm_events if not is_gemm(ev[3])]
    gemm_events = [ev for ev in gemm_events if is_gemm(ev[3])]
    # The weight-gradient launches run on a side stream BESIDE the input-gradient chain (seqcore weight_grad_mode), so
    # kernel durations overlap: the family's time is the UNION of the [start, end] intervals of its launches (absolute
    # times = elapsed since one reference event), not their sum.  Both are reported.
    iv = sorted((ref_ev.elapsed_time(s_) * 1e-3, ref_ev.elapsed_time(e_) * 1e-3) for s_, e_, _, _ in gemm_events)
    g_union, cur_s, cur_e = 0.0, None, None
    for a_, b_ in iv:
        if cur_e is None or a_ > cur_e:
            if cur_e is not None:
                g_union += cur_e - cur_s
            cur_s, cur_e = a_, b_
        else:
            cur_e = max(cur_e, b_)
    if cur_e is not None:
        g_union += cur_e - cur_s
    g_union = g_union or float("nan")
    g_sum = sum(s_.elapsed_time(e_) for s_, e_, _, _ in gemm_events) * 1e-3 or float("nan")
    g_fl = sum(f for _, _, f, _ in gemm_events)
    g_ex = sum(f * executed_products(t) for _, _, f, t in gemm_events)
    g_h2 = any("HALF" in t for _, _, _, t in gemm_events)
    n_launch = len(gemm_events)

    def per_tag(events, unit_scale, unit_name):
        acc = {}
        for s_, e_, f_, tag in events:     # one entry per kernel instantiation, comparable with rocprofv3's rows
            k = acc.setdefault(tag, [0, 0.0, 0.0])
            k[0] += 1; k[1] += s_.elapsed_time(e_) * 1e-3; k[2] += f_
        return {t: {"launches_per_step": c / max(n_inst, 1), "avg_kernel_us": sec / c * 1e6,
                    unit_name: fl / sec / unit_scale} for t, (c, sec, fl) in acc.items()}

    per_kernel = per_tag(gemm_events, 1e12, "tflops")
    traffic = None
    # (the r04 file describes the six-product kernels: only this round's PMC passes, taken on the kernels the line runs, count)
    tr_file = next((f for f in (os.path.join(ROOT, "profiles", r_, "pmc", "gemm_traffic_summary.json") for r_ in ("r06", "r05"))
                    if os.path.exists(f)), "")
    tr_rel = os.path.relpath(tr_file, ROOT) if tr_file else None
    if tr_file and not custom and B == 64:
        try:
            traffic = json.load(open(tr_file)).get("hbm_bytes_per_launch")
        except Exception:
            traffic = None
    planes_on = bool(b3 and getattr(model, "_planes_on", lambda: False)())
    # the same family in the committed rocprofv3 --kernel-trace --stats summary of this command (tools/r05_session.sh prof): kernel
    # durations without the event pair's launch gap -- what `avg_kernel_us` has to agree with (read from the file, not measured here)
    rp = None
    rp_file = next((f for f in (os.path.join(ROOT, "profiles", r_, "bench_b64_kernel_stats.csv") for r_ in ("r06", "r05")) if os.path.exists(f)), "")
    rp_rel = os.path.relpath(rp_file, ROOT) if rp_file else ""
    if rp_file and not custom and B == 64 and g_h2:
        try:
            import csv
            rows_ = list(csv.DictReader(open(rp_file)))
            steps_ = next(int(r_["Calls"]) for r_ in rows_ if "adamw_flat_tab" in r_["Name"])
            fam_ = [r_ for r_ in rows_ if "gemm_p3_kernel" in r_["Name"] or "grouped_dw_p3_kernel" in r_["Name"]]
            us_ = sum(int(r_["TotalDurationNs"]) for r_ in fam_) / steps_ * 1e-3
            n_ = sum(int(r_["Calls"]) for r_ in fam_) / steps_
            ex_ = g_ex / max(n_inst, 1) / (us_ * 1e-6) / 1e12
            rp = {"source": rp_rel + " (rocprofv3 --kernel-trace --stats of this command's captured steps; "
                              "read from the committed file, NOT measured in this run)",
                  "launches_per_step": n_, "gemm_time_per_step_us": us_, "avg_kernel_us": us_ / n_,
                  "achieved": ex_, "frac": ex_ / 2500.0,
                  "note": "kernel start-to-end durations inside the replayed graph; the HIP-event figures of this object add the gap "
                          "between an event and the launch behind it (~4-5 us per launch) and come from eagerly issued steps"}
        except Exception as e_:  # noqa: BLE001
            rp = {"error": f"{type(e_).__name__}: {e_}"}
    roof = {"bound": "mfma",
            "kernel": ("gemm_p3_kernel<P3Cfg<.., HALF>> / grouped_dw_p3_kernel<P4Cfg<.., HALF>> (v_mfma_f32_32x32x16_f16 on two fp16 planes per "
                       "operand that their producers / the optimizer wrote pre-split: 3 products per multiply, fp32 accumulate; every "
                       "nn.Linear fwd/bwd of the step)" if (planes_on and g_h2) else"gemm_p3_kernel / grouped_dw_p3_kernel (v_mfma_f32_32x32x16_bf16 on an exact 3 x bf16 split of the fp32 operands "
                       "that their producers wrote PRE-SPLIT as planes; 6 products per multiply, fp32 accumulate; every nn.Linear "
                       "fwd/bwd of the step)" if planes_on else
                       "gemm_b3_kernel / grouped_dw_b3_kernel (v_mfma_f32_32x32x16_bf16 on an exact 3 x bf16 split of the fp32 "
                       "operands inside the main loop, 6 products per multiply, fp32 accumulate; every nn.Linear fwd/bwd of the step)"
                       if b3 else
                       "gemm_kernel / grouped_dw_kernel (v_mfma_f32_32x32x2_f32; every nn.Linear fwd/bwd of the step)"),
            "gemm_mode": ("planes" if planes_on else ops.gemm_mode()),
            **mfma_roof(g_fl, g_union, b3, g_ex if g_h2 else None), "traffic": traffic,
            "traffic_source": (f"{tr_rel}: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of "
                               "this command on the same kernels (read from the committed file, NOT measured in this run)"
                               if traffic is not None else None),
            "launches_per_step": n_launch / max(n_inst, 1), "avg_kernel_us": g_union / max(n_launch, 1) * 1e6,
            "algorithmic_flops_per_step": g_fl / max(n_inst, 1),
            "gemm_time_per_step_us": g_union / max(n_inst, 1) * 1e6,
            "gemm_time_per_step_us_sum_of_durations": g_sum / max(n_inst, 1) * 1e6,
            "achieved_sum_of_durations": (B3_PRODUCTS if b3 else 1.0) * g_fl / g_sum / 1e12,
            "weight_grad_mode": getattr(model, "weight_grad_mode", None) if getattr(model, "group_weight_grads", False) else "per-layer",
            "kernels": per_kernel, "rocprofv3": rp,
            "note": f"HIP events (each on the stream its kernel runs on) around every GEMM launch of {n_inst} extra "
                    "eager steps issued right after the timed region (bracketing launches inside it would make the step "
                    "host-bound); achieved = ALGORITHMIC fp32 flops / union of the launches' [start,end] intervals (= the sum "
                    "of durations in the default one-stream schedule), x 6 in bf16x3 mode = the bf16 products executed; peak = the "
                    "dense peak of the pipe the kernels run on (bf16 MFMA 2.5 PFLOP/s in bf16x3 mode, f32-input MFMA 157.3 "
                    "TFLOP/s in f32 mode); `algorithmic_tflops` is the fp32-equivalent rate; `traffic`: see `traffic_source`"}
    hbm_kernels = per_tag(other_events, 1e9, "gbs")

    out.update({
        **operand_fields(b3, g_h2),
        "h2_stale_overflows": stale_overflows[0],
        "spread": {"blocks": len(block_ms), "steps_per_block": args.steps, "ms_per_step": block_ms,
                   "median_ms_per_step": sorted(block_ms)[len(block_ms) // 2], "min_ms_per_step": min(block_ms),
                   "max_ms_per_step": max(block_ms),
                   "note": "block 0 is the timed region `value` is computed from; the others repeat it on the following batches"},
        "roofline": roof,
        "stream": {"distinct_batches": n_stream, "age_steps": args.age_steps, "age_s": t_age, "host_gen_s": t_gen,
                   "repeats_inside_run": bool(stream_repeats), "optimizer_steps_before_timed_region": args.age_steps + args.warmup,
                   "table_update": args.table_update},
    })
    if six is not None:
        out["six_products"] = six
    if phases is not None:
        out["data_parallel_phases"] = phases
    if lazy_flush is not None:
        out["lazy_flush"] = lazy_flush
    if lazy_gaps is not None:
        # the lazy table AdamW as it runs in the timed steps: catch-up (before the forward reads the rows) + apply
        rows_us = sum(v["avg_kernel_us"] * v["launches_per_step"] for t, v in hbm_kernels.items() if t.startswith("adamw_rows"))
        # round 6: a gap is summed in closed form (csrc/adamw.hip "SERIES replay"), so the launches are bound by the rows they move --
        # every unique row of the batch is read and written once by a catch-up (p, m, v: 24 B per element) and once more by the apply
        # (+ its gradient row: 28 B) -- not by the replayed steps any more
        rows_bytes = float(lazy_gaps["unique_rows_per_step"]) * D * (24.0 + 28.0)
        rp_rows = None
        if rp_file and not custom and B == 64:
            try:
                import csv
                rows_ = list(csv.DictReader(open(rp_file)))
                steps_ = next(int(r_["Calls"]) for r_ in rows_ if "adamw_flat_tab" in r_["Name"])
                us_ = sum(int(r_["TotalDurationNs"]) for r_ in rows_ if "adamw_rows_kernel" in r_["Name"]) / steps_ * 1e-3
                rp_rows = {"source": rp_rel + " (read from the committed file, NOT measured in this run)", "us_per_step": us_,
                           "achieved": rows_bytes / (us_ * 1e-6) / 1e9, "frac": rows_bytes / (us_ * 1e-6) / 1e9 / HBM_PEAK_GBS}
            except Exception as e_:  # noqa: BLE001
                rp_rows = {"error": f"{type(e_).__name__}: {e_}"}
        out["roofline_adamw_rows"] = {
            "bound": "hbm", "kernel": "adamw_rows_kernel (catch-up of the input rows | of the target / negative rows | apply)",
            "us_per_step": rows_us, "algorithmic_bytes_per_step": rows_bytes, "achieved": rows_bytes / (rows_us * 1e-6) / 1e9 if rows_us else None,
            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": rows_bytes / (rows_us * 1e-6) / 1e9 / HBM_PEAK_GBS if rows_us else None,
            "rocprofv3": rp_rows,
            "kernels": {t: v for t, v in hbm_kernels.items() if t.startswith("adamw_rows")}, "gaps": lazy_gaps,
            "note": "HIP events around the three launches in the instrumented EAGER steps (an event pair adds 4-5 us per launch; the "
                    "captured step runs the second one beside the encoder); `rocprofv3`: the same launches inside the replayed graph.  "
                    "bytes = unique rows of the batch x D x (24 B catch-up + 28 B apply); random 2 KB rows, three dependent round trips "
                    "per row (id -> values | claim -> stores)"}
    gf = [v for t, v in hbm_kernels.items() if t.startswith("ln_fwd_kernel<GATHER>")]
    if gf:
        out["roofline_gather_fused"] = [{"bound": "hbm", "kernel": "ln_fwd_kernel<GATHER>", "batch_per_gpu": B,
                                         "operands": OPERANDS_B3 if b3 else "f32_input_mfma",
                                         "achieved": gf[0]["gbs"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                         "frac": gf[0]["gbs"] / HBM_PEAK_GBS, "avg_kernel_us": gf[0]["avg_kernel_us"],
                                         "note": "the gather as the step runs it: B*L table rows read + y + xhat written "
                                                 "(3 x B*L*D*4 bytes) + the three bf16 planes of y in planes mode (6 B per element)"}]

    if not args.no_extras and world == 1 and not custom:
        # everything measured beside the contract's timed region: bench_extras.py (its results go to the full record)
        import bench_extras
        from types import SimpleNamespace

        bench_extras.run(SimpleNamespace(args=args, world=world, custom=custom, dev=dev, B=B, L=L, D=D, N=N, model=model, dp=dp, state=state,
                                         rng=rng, zipf=zipf, use_graph=use_graph, b3=b3, dt=dt, t_eager=t_eager, eager_step=eager_step,
                                         next_batch=next_batch, replay=replay), out)
        out["h2_stale_overflows"] = stale_overflows[0]      # (the extras' steps count too)
        gstep = None

    if args.emulate_world > 1 and world == 1 and not custom:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import world_projection

        gstep = None
        torch.cuda.empty_cache()
        out["world_projection"] = world_projection.project(args.emulate_world, B=B, log=lambda *_: None)
    if not args.no_cpu_baseline and world == 1:
        out["cpu_baseline"] = cpu_baseline(B)
    elif world == 1:
        out["cpu_baseline"] = None

    emit(out)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
