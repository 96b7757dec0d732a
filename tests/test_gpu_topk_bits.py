"""The bits of every fused top-k that runs on the shared selection core (csrc/topk_select.cuh: the sorted register list, the
collapse of a wave's lists, the owner search and bitmap of the history mask, the one merge kernel) against
tests/golden/topk_core_bits.json, which was recorded with `python tests/test_gpu_topk_bits.py --record FILE` on the build of
the commit BEFORE the core was shared (three copies of the list, three merge kernels, six owner searches).  Sharing the code
changes no product, no order of a sum and no tie rule, so per case the ids must be equal in full and so must a u32 checksum of
the values' bit patterns.

Cases (inputs from torch.Generator().manual_seed on the CPU; none holds NaN or +-inf, none overflows the candidate buffer --
ops.raise_on_bad_indices at the end of every run shows that no status bit was set, on the recording build as well):
  * score_topk, register lists: B 130 x N 777 x D 32, K 10 (two row blocks, the second ragged; seven item tiles, the last
    ragged; about five history items per user spread over the tiles), and B 3 x N 20 x D 4, K 32 (fewer than K unmasked items:
    (-inf, -1) tails pass through the merge).  The first also under PXR_TOPK_VARIANT 1 and 3 -- the library reads that knob once
    per process, so each value runs in one fresh child process (this file's --emit mode), as it did for the recording;
  * score_topk, threshold schedule: B 130 x N 65 601 x D 64, K 10 (513 item tiles: one above the threshold between the
    schedules, the last ragged; the sample pass scores 9 of them).  fp32 operands in both GEMM modes, switched in-process the
    way the pxr_mode fixture does (score_thresh_kernel<1> under bf16x3, <0> under f32); planes on six products
    (score_thresh_p3_kernel), with PXR_SCORE_P4=1, and on three and one products with the table's largest row norm -- the plane
    variants must also agree with each other, ids and bits, as tests/test_gpu_configs.py asserts at the full shape;
  * VISRANK: B 5 x N 300 x F 8, H 4, ragged window lengths, top_k 0 / 1 / 3, K 10, and a catalogue with fewer than K unmasked
    items (inputs by tests/test_gpu_visrank.py's helpers);
  * DIN: item_num 257 and 13 (fewer than K real items), B 3, L 4, hidden (16,) and (12, 4), K 10 (inputs by
    tests/din_restate.topk_case; the last user keeps fewer than K items unmasked).

The walk groups (din_walk, wd_walk, vr_walk) pin the tile-to-tile carry of din_topk_kernel, wd_topk_kernel and visrank_topk_kernel --
the cases above give a workgroup one tile at most, and none of them is WideDeep.  Their entries were recorded by the same --record
path on the build of commit 06ea9af, where each of the three kernels still carried its own walk frame (tile range, bitmap fill,
MLP tail, workspace carve); the frame shared since computes the same bits.  Per case a SHA-256 of the int64 id bytes and one of the
fp32 value bytes, both equal.  Cases, inputs and histories are those of tests/test_gpu_topk_walk.py (its case objects are shared:
one build per session), run the way that module runs them:
  * din_walk: every din_restate.WALK_CASES entry at K 10 (the odd hidden widths through ops.din_topk, "chunks" as users 0-1, 2-3,
    4 under a lowered ops.DIN_WS_CAP), "short splits" also at K 16 and 32;
  * wd_walk: every widedeep_restate.WALK_CASES entry at K 10, "short splits" also at K 16 and 32;
  * vr_walk: every visrank_restate.WALK_CASES entry with top_k 0, 1 and 3 at K 10."""
import contextlib
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                               # --record / --emit: run as a script, from anywhere
    sys.path.insert(0, ROOT)

from tests import din_restate as RD  # noqa: E402
from tests import visrank_restate as RV  # noqa: E402
from tests import widedeep_restate as RW  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "topk_core_bits.json")
REG = {"reg/b130_n777_d32_k10": (130, 777, 32, 10, 21), "reg/b3_n20_d4_k32": (3, 20, 4, 32, 22)}
VARIANT_CASE = "reg/b130_n777_d32_k10"
THRESH = (130, 65_601, 64, 10, 23)


def _record(idx, val):
    """ids in full + the u32 checksum of the values' bit patterns"""
    torch.cuda.synchronize()
    bits = val.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return {"ids": idx.cpu().reshape(-1).tolist(), "val_u32_sum": int(bits.sum().item()) & 0xFFFFFFFF}


def _score_inputs(B, N, D, K, seed):
    from pixelrec_amd import ops

    g = torch.Generator().manual_seed(seed)
    table = (torch.randn(N, D, generator=g) * 0.02).cuda()
    users = torch.randn(B, D, generator=g).cuda()
    hu = torch.arange(B).repeat_interleave(5)
    hi = torch.randint(1, N, (B * 5,), generator=g)
    ptr, items = ops.history_csr(hu, hi, B, "cuda")
    return users, table, ptr, items


def _register_list_case(name):
    from pixelrec_amd import ops

    B, N, D, K, seed = REG[name]
    users, table, ptr, items = _score_inputs(B, N, D, K, seed)
    out = _record(*ops.score_topk(users, D, B, table, K, ptr, items))
    ops.raise_on_bad_indices("cuda")
    return out


@contextlib.contextmanager
def _env(**kv):
    prev = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in prev.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _threshold_cases():
    from pixelrec_amd import ops

    B, N, D, K, seed = THRESH
    users, table, ptr, items = _score_inputs(B, N, D, K, seed)
    out = {}
    for mode in ("bf16x3", "f32"):
        prev = ops.set_gemm_mode(mode)
        try:
            out[f"thresh/fp32_operands/{mode}"] = _record(*ops.score_topk(users, D, B, table, K, ptr, items))
        finally:
            ops.set_gemm_mode(prev)
    assert ops.gemm_mode() == "bf16x3" and ops.score_planes_supported(table)
    tp, vmax = ops.split_planes(table), ops.row_norm_max(table)
    out["thresh/planes/products6"] = _record(*ops.score_topk(users, D, B, table, K, ptr, items, table_planes=tp))
    with _env(PXR_SCORE_P4="1"):
        out["thresh/planes/p4"] = _record(*ops.score_topk(users, D, B, table, K, ptr, items, table_planes=tp))
    for products in ("3", "1"):
        with _env(PXR_TOPK_PRODUCTS=products):
            out[f"thresh/planes/products{products}"] = _record(*ops.score_topk(users, D, B, table, K, ptr, items, table_planes=tp,
                                                                               table_norm_max=vmax))
    ops.raise_on_bad_indices("cuda")                     # no candidate-buffer overflow, no user short of K candidates
    return out


def _visrank_cases():
    from tests import test_gpu_visrank as V

    out = {}
    B, N, F, H, K = 5, 300, 8, 4, 10
    v, hists = V._case(B, N, F, [1, 4, 9, 2, 3], seed=31)
    for top_k in (0, 1, 3):
        out[f"visrank/b5_n300_f8_h4/top_k{top_k}"] = _record(*V._run(v, hists, H, top_k, K))     # (_run checks the status word)
    N = 14
    v, _ = V._case(1, N, F, [1], seed=32)
    hists = [np.array([i for i in range(1, N) if i not in (3, 8, 11)]), np.array([5, 6]), np.array([7, 2, 7])]
    out["visrank/fewer_than_k_n14/top_k3"] = _record(*V._run(v, hists, H, 3, K))
    return out


def _din_cases():
    from pixelrec_amd import ops
    from tests import din_restate as R
    from tests import test_gpu_din as T

    out = {}
    B, L, K = 3, 4, R.TOPK_K
    for item_num in (257, 13):
        for hidden in ((16,), (12, 4)):
            P, win, hist = R.topk_case(item_num, B, L, hidden)
            m = T._model(item_num, R.TOPK_HIDDEN[hidden], hidden, L=L, sd=P).eval()
            ptr, items = T._csr(hist, B)
            out[f"din/n{item_num}_h{'x'.join(map(str, hidden))}"] = _record(*m.fused_topk(win.cuda(), ptr, items, K))
            ops.raise_on_bad_indices("cuda")
    return out


def _variant_child(variant):
    """VARIANT_CASE under PXR_TOPK_VARIANT=variant, in a fresh process"""
    env = dict(os.environ, PXR_TOPK_VARIANT=str(variant))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--emit", VARIANT_CASE], env=env, capture_output=True, text=True,
                       timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


GROUPS = {"reg": lambda: {name: _register_list_case(name) for name in REG}, "thresh": _threshold_cases, "visrank": _visrank_cases,
          "din": _din_cases, "variant": lambda: {f"variant/{v}/{VARIANT_CASE}": _variant_child(v) for v in (1, 3)}}


def _digests(idx, val):
    """SHA-256 of the id bytes and of the value bytes (the callers have synchronised and read the status word)"""
    idx, val = idx.cpu().contiguous(), val.cpu().contiguous()
    assert idx.dtype == torch.int64 and val.dtype == torch.float32
    return {"ids_sha256": hashlib.sha256(idx.numpy().tobytes()).hexdigest(),
            "val_sha256": hashlib.sha256(val.numpy().tobytes()).hexdigest()}


def _mlp_walk(model_name, name, k):
    from pixelrec_amd import ops
    from tests import test_gpu_topk_walk as W

    c = (W.DIN_CASES if model_name == "din" else W.WD_CASES).get(name)
    prev = ops.DIN_WS_CAP
    if name == "chunks":                                 # as test_din_user_chunks_equal_the_unchunked_call: chunks of 2, 2 and 1 users
        ops.DIN_WS_CAP = 2 * c.L * (c.hidden[0] * c.D + 128) * 4
    try:
        return _digests(*W._fused(model_name, c, k))     # (_fused checks the status word)
    finally:
        ops.DIN_WS_CAP = prev


def _vr_walk(name, top_k):
    from tests import test_gpu_topk_walk as W

    return _digests(*W._vr_fused(W.VR_CASES.get(name, top_k), RV.WALK_K))


# case -> how to run it; the part of the name before the first "/" is the group
WALK = {}
for _model, _R in (("din", RD), ("wd", RW)):
    for _name in _R.WALK_CASES:
        for _k in (10, 16, 32) if _name == "short splits" else (10,):
            WALK[f"{_model}_walk/{_name}/k{_k}"] = (_mlp_walk, "din" if _model == "din" else "widedeep", _name, _k)
for _name in RV.WALK_CASES:
    for _top_k in (0, 1, 3):
        WALK[f"vr_walk/{_name}/top_k{_top_k}"] = (_vr_walk, _name, _top_k)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("group", list(GROUPS))
def test_bits_of_the_separate_copies_are_kept(group, golden):
    got = GROUPS[group]()
    want = {k: v for k, v in golden.items() if k.split("/")[0] == group}
    assert sorted(got) == sorted(want) and want
    for name in sorted(want):
        assert got[name]["ids"] == want[name]["ids"], name
        assert got[name]["val_u32_sum"] == want[name]["val_u32_sum"], name
    if group == "thresh":                                # the plane variants: the same ids and the same bits as each other
        planes = [got[n] for n in sorted(got) if n.startswith("thresh/planes/")]
        assert len(planes) == 4 and all(p == planes[0] for p in planes[1:])
    if group == "reg":                                   # fewer than K unmasked items: the tail is (-inf, -1)
        B, N, _, K, _ = REG["reg/b3_n20_d4_k32"]
        ids = np.asarray(got["reg/b3_n20_d4_k32"]["ids"]).reshape(B, K)
        assert (ids[:, N - 1:] == -1).all() and (ids[:, :N - 6] >= 1).all()


@pytest.mark.parametrize("name", list(WALK))
def test_bits_of_the_walks_are_kept(name, golden):
    run, *args = WALK[name]
    assert run(*args) == golden[name], name


def test_the_golden_file_holds_exactly_these_walks(golden):
    assert sorted(k for k in golden if k.split("/")[0] in ("din_walk", "wd_walk", "vr_walk")) == sorted(WALK)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--emit":
        print(json.dumps(_register_list_case(sys.argv[2])))
    else:
        assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: test_gpu_topk_bits.py --record FILE | --emit CASE"
        cases = {}
        for make in GROUPS.values():
            cases.update(make())
        for name, (run, *args) in WALK.items():
            cases[name] = run(*args)
        with open(sys.argv[2], "w") as f:                # one case per line
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(cases[k], sort_keys=True)}" for k in sorted(cases)) + "\n}\n")
