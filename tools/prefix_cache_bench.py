"""What the prefix cache (pixelrec_amd/model/prefix_cache.py) buys at the shipped PixelNet shape -- measured, on one MI355X:

  * the MOSASRec training step (clip-vit-base-patch16, random weights, tune_scale 165, B 16, L 10: 352 images a step, both optimizer
    groups) over images and over item ids, ALTERNATING in one process on one model and one optimizer pair: 3 rounds of 10 eager
    steps each way, the median step of every round (host clock around a device synchronise);
  * the cache's fill and `compute_item` (evaluation) per 1000 images, both ways;
  * the gather + LayerNorm launch alone with plain and with streaming loads of the cache rows (PXR_PREFIX_NT), device events.

The catalogue is synthetic (2000 items of 224 x 224: a 301 MB store, a 1.2 GB cache).  Not measured here: the step captured as a
hipGraph (bench.py's figure), real Pixel200K images, several ranks.  Writes profiles/prefix_cache/prefix_cache_bench.json.

usage: python tools/prefix_cache_bench.py [--items 2000] [--rounds 3] [--steps 10] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encoder", default="clip-vit-base-patch16")
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefix_cache", "prefix_cache_bench.json"))
    args = ap.parse_args()

    from pixelrec_amd import ops
    from pixelrec_amd.data.images import ImageStore
    from pixelrec_amd.model import MOSASRec
    from pixelrec_amd.model.visual import ENCODER_SHAPES
    from pixelrec_amd.optim import OptimizerGroup, PxrAdamW, VisualAdamW

    if not torch.cuda.is_available():
        raise SystemExit("prefix_cache_bench: no GPU -- nothing here can be measured without one")
    dev = torch.device("cuda", 0)
    hidden, n_layers, heads, inter, image, patch = ENCODER_SHAPES[args.encoder]
    B, L, D = 16, 10, 512
    tune = 165 if n_layers == 12 else 5 + 16 * (n_layers - 2)          # the last two blocks train (overall/ViT.yaml: 165)
    cfg = {"n_layers": 2, "n_heads": 4, "embedding_size": D, "inner_size": 2, "hidden_dropout_prob": 0.1, "attn_dropout_prob": 0.1,
           "hidden_act": "gelu", "layer_norm_eps": 1e-12, "initializer_range": 0.02, "MAX_ITEM_LIST_LENGTH": L, "seed": 2020,
           "encoder_name": args.encoder, "encoder_source": "transformers", "pretrain_path": None,
           "fine_tune_arg": {"tune_scale": tune, "pre_trained": False, "allow_random_backbone": True, "activation": "relu",
                             "dnn_layers": [], "method": "mean"}}

    class DL:
        item_num = args.items

    torch.manual_seed(2020)
    m = MOSASRec(cfg, DL()).to(dev).train()
    opt = OptimizerGroup(VisualAdamW(m.visual_encoder, lr=1e-4, weight_decay=0.0), PxrAdamW(m, lr=1e-4, weight_decay=0.1))
    store = ImageStore.synthetic(args.items, image, 0, dev)
    enc = m.visual_encoder
    one = torch.ones((), dtype=torch.float32, device=dev)
    g = torch.Generator().manual_seed(1)
    pool = [(torch.randint(1, args.items, (B, 2 * (L + 1)), generator=g).to(dev), torch.ones(B, L, dtype=torch.int64, device=dev))
            for _ in range(2)]

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    # ---- the fill (the second one is timed: the first loads code objects and splits the frozen weights)
    assert enc.build_prefix_cache(store), "the cache was refused"
    fill_s = clock(lambda: enc.build_prefix_cache(store))
    cache = enc.prefix_cache
    T = cache.table.shape[1] // hidden

    def step(i, ids_form):
        ids, mask = pool[i % 2]
        opt.zero_grad()
        loss = m((ids if ids_form else store.batch(ids), mask))
        loss.backward(one)
        try:
            opt.step()
        except ops.H2StaleOverflow:
            pass
        return loss

    for i in range(3):
        step(i, False), step(i, True)
    rounds = {"images": [], "ids": []}
    for r in range(args.rounds):
        for form in ("images", "ids"):
            ts = [clock(lambda: step(i, form == "ids")) for i in range(args.steps)]
            rounds[form].append(statistics.median(ts) * 1e3)
    ops.raise_on_bad_indices(dev)

    # ---- evaluation: compute_item over the catalogue in the Trainer's chunks of 100
    m.eval()

    def encode(ids_form):
        for s in range(0, args.items, 100):
            ids = torch.arange(s, min(args.items, s + 100), device=dev)
            m.compute_item(ids if ids_form else store.batch(ids))

    encode(False), encode(True)
    eval_s = {"images": clock(lambda: encode(False)), "ids": clock(lambda: encode(True))}

    # ---- the gather + LayerNorm launch alone, plain against streaming loads of the cache rows (alternating, device events)
    gamma, beta = torch.ones(hidden, device=dev), torch.zeros(hidden, device=dev)
    ids = pool[0][0].flatten()
    kern = {"0": [], "1": []}
    keep = os.environ.get("PXR_PREFIX_NT")
    for rep in range(12):
        for nt in ("0", "1"):
            os.environ["PXR_PREFIX_NT"] = nt
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.ln_gather_fwd(cache.table, ids, T, gamma, beta, 1e-5, save=True, planes="h2", want_y=False)
            e1.record()
            e1.synchronize()
            if rep >= 2:
                kern[nt].append(e0.elapsed_time(e1) * 1e3)
    if keep is None:
        del os.environ["PXR_PREFIX_NT"]
    else:
        os.environ["PXR_PREFIX_NT"] = keep

    slow_ids, fast_img = max(rounds["ids"]), min(rounds["images"])
    out = {
        "device": torch.cuda.get_device_name(0), "encoder": args.encoder, "tune_scale": tune, "first_trainable_block": cache.k,
        "batch": B, "L": L, "images_per_step": B * 2 * (L + 1), "items": args.items, "cache_bytes": cache.table.numel() * 4,
        "mode": "eager steps, alternating rounds in one process; median step per round",
        "step_ms_images": [round(x, 3) for x in rounds["images"]], "step_ms_ids": [round(x, 3) for x in rounds["ids"]],
        "slowest_ids_round_over_fastest_images_round": round(slow_ids / fast_img, 4),
        "median_ids_over_median_images": round(statistics.median(rounds["ids"]) / statistics.median(rounds["images"]), 4),
        "flop_projection": 0.375, "cached_beats_uncached": slow_ids < fast_img,
        "fill_ms_per_1000_images": round(fill_s * 1e3 * 1000 / args.items, 2),
        "compute_item_ms_per_1000_images": {k: round(v * 1e3 * 1000 / args.items, 2) for k, v in eval_s.items()},
        "ln_gather_us": {"rows": int(ids.numel()) * T, "D": hidden, "outputs": "x_out + xhat + rstd + h2 planes",
                         "plain_loads_median": round(statistics.median(kern["0"]), 1),
                         "streaming_loads_median": round(statistics.median(kern["1"]), 1)},
        "not_measured": ["the step captured as a hipGraph (bench.py)", "real catalogue images", "more than one rank"],
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
