"""The bench.py output contract.  bench.py prints ONE short JSON line (< 4 KB: the driver's parser returned `parsed: null` for
round 5's 22.6 KB line) and writes everything else it measures to a side file.  Checked here on CPU: the short line bench.py's
own `compact_line` cuts from the last committed full record carries every key the driver parses with the right type, the
metric / config are BASELINE.json's, the derived fields agree with each other, and the full record still holds the extras.
(bench.py itself needs an MI355X: this guards the schema.)"""
import json
import math
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pxr_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _full():
    """The full record of the last committed default run: round 6's side file when a session has committed one, else round 5's line
    (which was the full record)."""
    for rel in (("profiles", "r06", "bench_extras.json"), ("profiles", "r05", "bench_default_line.json")):
        f = os.path.join(ROOT, *rel)
        if os.path.exists(f):
            text = open(f).read().strip().splitlines()
            assert len(text) == 1
            return json.loads(text[0])
    raise AssertionError("no committed bench record")


def _line():
    """What bench.py prints for that record."""
    b = _bench_module()
    full = dict(_full())
    full.setdefault("extras", "gpurun_out/bench_extras.json")
    text = json.dumps(b.compact_line(full))
    assert len(text) < 4096 == b.LINE_LIMIT, len(text)
    return json.loads(text)


def test_the_printed_line_is_short_and_the_committed_one_is_what_compact_line_gives():
    d = _line()
    for key in ("metric", "value", "unit", "n_gpus", "rccl_ranks", "steps", "warmup", "ms_per_step", "dtype", "operands", "config",
                "roofline", "cpu_baseline", "six_products", "extras"):
        assert key in d, key
    assert set(d["roofline"]) >= {"bound", "kernel", "achieved", "peak", "unit", "frac", "traffic"}
    assert set(d["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample"}
    f = os.path.join(ROOT, "profiles", "r06", "bench_default_line.json")
    if os.path.exists(f):       # the line a GPU session committed: one line, short, and the cut of its own side file
        text = open(f).read().strip().splitlines()
        assert len(text) == 1 and len(text[0]) < 4096
        got = json.loads(text[0])
        assert got["value"] == d["value"] and got["roofline"]["frac"] == d["roofline"]["frac"]


def test_compact_line_survives_oversized_members():
    b = _bench_module()
    full = dict(_full())
    full["metric"] = "m" * 9000
    full["throughput_batches"] = [{"batch_per_gpu": i, "value": 1.0, "operands": "x" * 50} for i in range(200)]
    text = json.dumps(b.compact_line(full))
    assert len(text) < 4096
    d = json.loads(text)
    assert "roofline" in d and "cpu_baseline" in d and "value" in d


def test_required_keys_and_types():
    d = _line()
    for key, typ in [("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                     ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str),
                     ("data", str), ("config", dict), ("roofline", dict), ("cpu_baseline", dict)]:
        assert isinstance(d[key], typ), key
    assert "vs_baseline" in d and d["vs_baseline"] is None          # BASELINE.md publishes no number for this metric
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["dtype"] == "f32"
    assert d["data"].startswith("synthetic")
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert "sequences" in d["unit"] and "sequences/sec" in base["metric"]
    cfg = d["config"]
    assert "workload" in cfg and "model" not in cfg
    assert (cfg["embedding_size"], cfg["seq_len"], cfg["n_items"], cfg["batch_per_gpu"]) == (512, 50, 400001, 64)


def test_value_is_consistent_with_the_step_time():
    d = _line()
    seqs_per_step = d["config"]["global_batch"]
    assert math.isclose(d["value"], seqs_per_step / (d["ms_per_step"] * 1e-3), rel_tol=1e-6)


def test_roofline_and_cpu_baseline_objects():
    d = _full()
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert r["peak"] > 0 and 0 < r["frac"] <= 1 and math.isclose(r["frac"], r["achieved"] / r["peak"], rel_tol=1e-6)
    assert r["traffic"] is None or r["traffic"] > 0
    # round 3: priced against the pipe the kernels run on -- in bf16x3 mode the dense bf16 MFMA peak with the 6 bf16 products
    # per fp32 multiply counted as executed work; the fp32-equivalent view travels beside it
    assert r["gemm_mode"] in ("planes", "bf16x3", "f32")
    # round 4: the line names the kernels the trace shows, and says where `traffic` comes from (a committed PMC file, not this run)
    if r["gemm_mode"] == "planes":
        assert "gemm_p3_kernel" in r["kernel"] and "grouped_dw_p3_kernel" in r["kernel"]
    assert r["traffic"] is None or "profiles/" in r["traffic_source"]
    if r["gemm_mode"] in ("planes", "bf16x3"):
        assert r["peak"] == 2500.0 and "bf16" in r["pipe"]
        # round 5: `achieved` counts the products EXECUTED -- 6 per multiply on the bf16x3 split, 3 on the fp16 two-plane operands
        # the step runs on by default; the six-product scale of the earlier rounds travels beside it
        prods = r.get("products_per_multiply", 6.0)
        assert 3.0 - 1e-6 <= prods <= 6.0 + 1e-6
        assert math.isclose(r["achieved"], prods * r["algorithmic_tflops"], rel_tol=1e-6)
        if "six_product_equivalent_frac" in r:
            assert math.isclose(r["six_product_equivalent_frac"], 6.0 * r["algorithmic_tflops"] / 2500.0, rel_tol=1e-6)
        assert math.isclose(r["algorithmic_over_f32_mfma_peak"], r["algorithmic_tflops"] / 157.3, rel_tol=1e-3)
    # round 5: the committed rocprofv3 summary of the same command, as the line reads it: kernel durations without the event pair's
    # launch gap -- the two views of the family must agree to the gap (4-5 us on ~26 us launches)
    rp = r["rocprofv3"]
    assert rp is not None and "error" not in rp and rp["source"].startswith(("profiles/r06/", "profiles/r05/"))
    assert 0 < rp["frac"] <= 1 and rp["launches_per_step"] == r["launches_per_step"]
    assert 0.65 <= rp["avg_kernel_us"] / r["avg_kernel_us"] <= 1.05      # (event pairs add 4-8 us to launches of ~25 us, box dependent)
    # round 2: the stream does not repeat inside the run and the line says what the lazy table update costs
    assert d["stream"]["repeats_inside_run"] is False and d["stream"]["age_steps"] >= 256
    assert d["roofline_adamw_rows"]["us_per_step"] > 0 and d["lazy_flush"]["amortised_us_per_step"] > 0
    for c in (d["cpu_baseline"], _line()["cpu_baseline"]):
        assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and isinstance(c["sample"], str)
    lr = _line()["roofline"]
    assert lr["bound"] == r["bound"] and math.isclose(lr["frac"], lr["achieved"] / lr["peak"], rel_tol=1e-4)
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and isinstance(c["sample"], str)
    assert c["unit"] == d["unit"]
    # the north-star targets travel with the line: gather >= 70 % of HBM peak; the scoring GEMM reported against the gfx950
    # peak of the pipe it runs on (bf16 MFMA, 6 products per multiply) AND as fp32-equivalent work (>= 60 % of the f32 peak)
    assert d["roofline_gather"]["frac"] >= 0.70
    sc = d["roofline_scoring"]
    assert sc["peak"] == 2500.0 and 0 < sc["frac"] <= 1 and sc["algorithmic_over_f32_mfma_peak"] >= 0.60
    # round 4: measured on the path the product evaluates with (fused top-k on the pre-split table), with the result checked in the run
    assert "score_thresh_p3_kernel" in sc["kernel"] and sc["identical_top10"] is True
    ft = d["roofline_scoring_fused_topk"]
    assert ft["identical_top10"] is True and ft["identical_ids_and_values_to_six_product_schedule"] is True
    assert ft["products_in_threshold_pass"] in (1, 3, 6) and 0 < ft["ms_per_1024_users"] <= ft["six_product_schedule_ms"] * 1.05


def test_round6_targets_are_priced_as_run_and_at_the_clock_the_kernel_records():
    d = _full()
    if "roofline_gather_fused_alone" not in d:          # a round-5 record
        return
    ft = d["roofline_scoring_fused_topk"]
    # the default scoring kernel records its own clock: well below the 2.4 GHz the nominal peak assumes (power limit), and the
    # executed-product fraction at THAT clock is what the kernel can be held to
    assert 1.2 <= ft["sustained_clock_ghz"] <= 2.3
    assert math.isclose(ft["peak_at_sustained_clock"], 256 * 4 * 1024 * ft["sustained_clock_ghz"] / 1e3, rel_tol=1e-6)
    assert math.isclose(ft["frac_of_sustained_peak"], ft["executed_tflops_whole_call"] / ft["peak_at_sustained_clock"], rel_tol=1e-6)
    assert ft["frac"] < ft["frac_of_sustained_peak"] <= 1.0
    g = d["targets"]["gather_ge_0.70_of_hbm_peak"]
    alone = {e["batch_per_gpu"]: e["frac"] for e in d["roofline_gather_fused_alone"]["batches"]}
    assert set(alone) == {64, 512, 2048} and g["alone_b2048"] == alone[2048]
    assert g["met"] is (min(alone[512], alone[2048]) >= 0.70)          # as the step runs it, at every batch >= 512 -- not the standalone kernel
    line = _line()
    assert line["targets"]["gather_met"] is g["met"] and "alone_b2048" in line["targets"]["gather_frac_of_hbm_peak"]
    assert d["roofline"]["rocprofv3"]["source"].startswith("profiles/r06/") and d["roofline"]["traffic_source"].startswith("profiles/r06/")


def test_round5_both_arithmetics_and_the_review_targets_travel_with_the_full():
    d = _full()
    H2, B3 = "fp16_two_plane_three_products", "bf16x3_six_products"
    assert d["operands"] == H2 and d["rccl_ranks"] == d["n_gpus"] == 1
    six = d["six_products"]
    assert six["operands"] == B3 and six["PXR_SEQ_H2"] == "0" and six["ms_per_step"] > d["ms_per_step"]
    sp = d["spread"]
    assert sp["blocks"] == len(sp["ms_per_step"]) == 5 and sp["ms_per_step"][0] == d["ms_per_step"]
    assert sp["max_ms_per_step"] <= 1.03 * sp["min_ms_per_step"]                  # one run, one box: blocks agree
    assert {(t["batch_per_gpu"], t["operands"]) for t in d["throughput_batches"]} == {(512, H2), (512, B3), (2048, H2), (2048, B3)}
    by = {(t["batch_per_gpu"], t["operands"]): t["value"] for t in d["throughput_batches"]}
    assert by[512, H2] > by[512, B3] and by[2048, H2] > by[2048, B3]
    assert d["pixelnet"]["config"]["hip_graph"] is True and H2 in d["pixelnet"]["operands"]
    assert d["pixelnet_six_products"]["ms_per_step"] > d["pixelnet"]["ms_per_step"]
    t = d["targets"]
    assert {"gather_ge_0.70_of_hbm_peak", "scoring_ge_0.60_of_mfma_peak", "b64_step_le_0.88_ms", "b2048_ge_150k_sequences_per_s",
            "pixelnet_step_le_60_ms"} <= set(t)
    assert t["b64_step_le_0.88_ms"]["met"] is (d["ms_per_step"] <= 0.88)
    assert t["b2048_ge_150k_sequences_per_s"]["met"] is (by[2048, H2] >= 150e3)
    assert t["pixelnet_step_le_60_ms"]["met"] is (d["pixelnet"]["ms_per_step"] <= 60.0)
    assert 1.5 <= t["scoring_ge_0.60_of_mfma_peak"]["sustained_clock_ghz"] <= 2.6
    lv = d["lazy_vs_dense"]
    assert 0.9 <= lv["lazy_graphed_over_dense_minus_sweep"] <= 1.2


def test_round4_extras_travel_with_the_default_full():
    d = _full()
    # the PixelNet (BASELINE configs[2]-shaped) step, a few steps of it
    px = d["pixelnet"]
    assert "error" not in px, px
    assert px["unit"] == "sequences/s" and px["ms_per_step"] > 0 and px["config"]["images_per_step"] == 352
    assert 0 < px["gemm_family"]["frac"] <= 1 and set(px["phases_ms"]) and all(v >= 0 for v in px["phases_ms"].values())
    # per-family device time of the step at the throughput-oriented batch sizes
    assert {t["batch_per_gpu"] for t in d["throughput_batches"]} == {512, 2048}
    for t in d["throughput_batches"]:
        fam = t["kernel_families_us_per_step"]
        assert any(k.startswith("gemm") for k in fam) and any(k.startswith("grouped") for k in fam)
        assert abs(sum(fam.values()) - t["ms_per_step"] * 1e3) <= 1e-3 * t["ms_per_step"] * 1e3      # the rows add up to the step
        assert 0 < t["gemm_family"]["frac"] <= 1
    # the fused gather is priced with the plane bytes it writes
    assert "planes" in d["roofline_gather_fused"][0]["note"]


# ---- round 5: `--gpus N` is real (reference launcher: code/main.py:21-28) ---------------------------------
def test_gpus_flag_never_degrades_to_a_silent_single_rank(monkeypatch):
    import argparse

    import pytest
    b = _bench_module()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("PXR_BENCH_SHARE_GPU", raising=False)
    monkeypatch.setattr(b.torch.cuda, "device_count", lambda: 1)
    with pytest.raises(SystemExit, match="needs 4 visible devices, found 1"):
        b.launch_ranks(argparse.Namespace(gpus=4))
    b.launch_ranks(argparse.Namespace(gpus=1))                      # one GPU: this process is the rank
    monkeypatch.setenv("WORLD_SIZE", "2")                           # under torch.distributed.run the flag must agree with the world
    b.launch_ranks(argparse.Namespace(gpus=2))
    with pytest.raises(SystemExit, match="WORLD_SIZE=2"):
        b.launch_ranks(argparse.Namespace(gpus=8))
    with pytest.raises(SystemExit, match="WORLD_SIZE=2"):
        b.launch_ranks(argparse.Namespace(gpus=1))


def test_gpus_flag_spawns_one_rank_per_gpu(monkeypatch):
    import argparse

    import pytest
    b = _bench_module()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(b.torch.cuda, "device_count", lambda: 8)
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 0

    monkeypatch.setattr(b.subprocess, "call", fake_call)
    monkeypatch.setattr(b.sys, "argv", ["bench.py", "--gpus", "8", "--steps", "7"])
    with pytest.raises(SystemExit) as e:
        b.launch_ranks(argparse.Namespace(gpus=8))
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "8", "--steps", "7"] and cmd[-5].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_dump_outputs_writes_the_loss_and_a_seeded_sample_of_the_parameters(tmp_path, monkeypatch):
    """`--dump-outputs DIR`: the loss and every floating parameter as DIR/<name>.npy in float32, the whole dump under the budget;
    a tensor over its share is a fixed, seeded sample of its elements, so two runs (two builds) write identical files."""
    import numpy as np
    import torch

    b = _bench_module()
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 64 << 10)

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.table = torch.nn.Parameter(torch.randn(1000, 32))          # 128 KB: over its share, sampled
            self.small = torch.nn.Parameter(torch.randn(4, 8, dtype=torch.float64))
            self.register_buffer("ids", torch.arange(5))                     # integer: not a parameter output

    torch.manual_seed(0)
    m, loss = M(), torch.tensor(1.25)
    info = b.dump_outputs(str(tmp_path / "a"), loss, m)
    b.dump_outputs(str(tmp_path / "b"), loss, m)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["loss.npy", "small.npy", "table.npy"] and info["sampled"] == ["table"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= b.DUMP_LIMIT_BYTES
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [1.25]
    small = np.load(tmp_path / "a" / "small.npy")
    assert small.dtype == np.float64 and np.array_equal(small, m.small.detach().numpy())
    table = np.load(tmp_path / "a" / "table.npy")
    assert table.dtype == np.float32 and 0 < table.size < m.table.numel()
    flat = m.table.detach().reshape(-1).numpy()
    idx = np.sort(np.random.default_rng(b.DUMP_SAMPLE_SEED).choice(flat.size, table.size, replace=False))
    assert np.array_equal(table, flat[idx])
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))


def test_dump_outputs_flag_is_parsed(monkeypatch):
    b = _bench_module()

    class Parsed(Exception):
        pass

    def stop(args):
        raise Parsed(args)

    monkeypatch.setattr(b, "launch_ranks", stop)
    monkeypatch.setattr(b.sys, "argv", ["bench.py", "--steps", "3", "--dump-outputs", "out_dir"])
    try:
        b.main()
    except Parsed as e:
        args = e.args[0]
    assert args.dump_outputs == "out_dir" and args.steps == 3


def _parsed(monkeypatch, argv):
    b = _bench_module()

    class Parsed(Exception):
        pass

    def stop(args):
        raise Parsed(args)

    monkeypatch.setattr(b, "launch_ranks", stop)
    monkeypatch.setattr(b.sys, "argv", ["bench.py", *argv])
    try:
        b.main()
    except Parsed as e:
        return e.args[0]
    raise AssertionError("bench.main() did not reach launch_ranks")


def test_a_plain_run_is_the_default_and_full_is_opt_in(monkeypatch):
    """`bench.py --gpus 1 --steps K --warmup W` is the plain run (headline only); whatever else it measures is behind --full."""
    import pytest
    assert _parsed(monkeypatch, ["--gpus", "1", "--steps", "5", "--warmup", "2"]).full is False
    args = _parsed(monkeypatch, ["--full", "--emulate-world", "8"])
    assert args.full is True and args.emulate_world == 8
    with pytest.raises(SystemExit) as e:                 # a projection beside the headline is a --full measurement
        _parsed(monkeypatch, ["--emulate-world", "8"])
    assert e.value.code == 2

