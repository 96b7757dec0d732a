"""The multi-launch occurrence sort (csrc/occ_sort.cuh: the path above FP_MAX_N occurrences) of this build against another build of
libpxr.so: ops.embed_grad_rows at n = FP_MAX_N + 1 and n = 16 FP_MAX_N, D = 64, Zipf ids over 400 001 rows.  Each library runs two
series, interleaved (other, this, other, this), every series in a fresh process; the margin a difference has to exceed is the
difference between the OTHER library's own two series.  Both libraries must also give the same unique ids and the same row bits.
usage: python tools/occ_sort_bench.py OTHER_LIBPXR_SO [OUT_FILE]"""
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_TABLE, D, WARMUP, ITERS = 400001, 64, 5, 50


def fp_max_n():
    src = open(os.path.join(ROOT, "pixelrec_amd", "csrc", "occ_sort.cuh")).read()
    val = lambda k: int(re.search(r"constexpr int %s = (\d+)" % k, src).group(1))
    return val("FP_MAX_N") * val("RS_THREADS") * val("RS_ITEMS")


def series(lib_path):
    """{n: [us per call, sha256 of the unique ids and rows]} of one library, in this process."""
    import numpy as np
    import torch

    from pixelrec_amd import lib, ops, synth

    lib.LIB_PATH = os.path.abspath(lib_path)
    out = {}
    for n in (fp_max_n() + 1, 16 * fp_max_n()):
        idx = torch.from_numpy(synth.ZipfItems(N_TABLE, seed=1).sample(np.random.default_rng(n), n).astype(np.int64)).cuda()
        rows = torch.randn(n, D, device="cuda", generator=torch.Generator("cuda").manual_seed(n))
        sp = ops.SparseRows(n, D, "cuda")
        for _ in range(WARMUP):
            ops.embed_grad_rows(idx, rows, N_TABLE, 1.0, out=sp)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(ITERS):
            ops.embed_grad_rows(idx, rows, N_TABLE, 1.0, out=sp)
        e.record()
        torch.cuda.synchronize()
        k = sp.count()
        h = hashlib.sha256(sp.idx[:k].cpu().numpy().tobytes() + sp.rows[:k].cpu().numpy().tobytes()).hexdigest()[:16]
        out[n] = [s.elapsed_time(e) / ITERS * 1e3, "%d rows %s" % (k, h)]
    return out


if __name__ == "__main__":
    if sys.argv[1] == "--series":
        print("SERIES " + json.dumps(series(sys.argv[2])))
        sys.exit(0)
    other, this = sys.argv[1], os.path.join(ROOT, "pixelrec_amd", "libpxr.so")
    runs = []
    for name, path in (("other", other), ("this", this)) * 2:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--series", path], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit("series %s failed (%d):\n%s" % (name, r.returncode, (r.stdout + r.stderr)[-2000:]))
        runs.append((name, json.loads(re.search(r"^SERIES (.*)$", r.stdout, re.M).group(1))))
    lines = ["ops.embed_grad_rows, D = %d, n_table = %d, %d calls per series after %d warm-up calls; us per call" % (D, N_TABLE, ITERS, WARMUP)]
    for n in runs[0][1]:
        t = {name: [r[n][0] for nm, r in runs if nm == name] for name in ("other", "this")}
        same = len({r[n][1] for _, r in runs}) == 1
        lines.append("n = %8s: other %8.1f %8.1f (margin %.1f)   this %8.1f %8.1f   mean this - mean other %+.1f   outputs %s (%s)"
                     % (n, *t["other"], abs(t["other"][0] - t["other"][1]), *t["this"], sum(t["this"]) / 2 - sum(t["other"]) / 2,
                        "equal" if same else "DIFFER", runs[0][1][n][1]))
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write(text + "\n")
    sys.exit(0 if all("equal" in ln for ln in lines[1:]) else 1)
