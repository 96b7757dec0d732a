"""ops.score_topk's threshold schedule (catalogues of 65 409 items or more; csrc/score_topk.hip) against a float64 top-K of the
masked float64 scores, on the cases of tests/score_topk_restate.py -- whose histories mask items that WOULD be top-K items, so a
mask that one of the kernels dropped changes an output (tests/test_score_topk_cases.py shows that without a GPU).

Every case runs through every schedule it supports:
  f32    GEMM mode f32, fp32 operands           sample pass, topk_tau_kernel, score_thresh_kernel<0>, topk_cand_merge_kernel
  b3     GEMM mode bf16x3, fp32 operands        score_thresh_kernel<1>
  p3     table planes                           score_thresh_p3_kernel
  p4     table planes, PXR_SCORE_P4=1           score_thresh_p4_kernel; the history is masked in the candidate merge
  fast3  planes + largest row norm, 3 products  topk_tau_fast_kernel, score_thresh_fast_kernel<2, 4>, topk_rescore_kernel
  fast1  the same on 1 product                  score_thresh_fast_kernel<1, 8>
and "ragged" also through the other ring depths of the fast kernel (PXR_TOPK_NS).  Planes need D % 32 == 0.

Comparison: tests/test_gpu_din._compare_topk -- ids equal wherever the float64 gaps around that rank exceed tol_abs, values within
tol_abs = 2e-6 sqrt(D) max|s64| + 1e-6 (the bound of tests/test_gpu_gemm.py::_check) -- with at most 4 % of the (user, rank) cells
excused (float64 alone: at most 1.8 %).  "crowd" has 3000 identical catalogue rows: there the values are compared within tol_abs
and the ids as a set -- duplicates only, none masked, all distinct.  The bf16x3 schedules (all but f32) must agree with each other
in every id and every value bit."""
import pytest
import torch

from tests import score_topk_restate as R
from tests.test_gpu_din import _compare_topk

pytestmark = pytest.mark.gpu

EXCUSED_CAP = 0.04
KNOBS = ("PXR_SCORE_P4", "PXR_TOPK_PRODUCTS", "PXR_TOPK_NS")
# (schedule, ring depth); a ring depth only on "ragged"
NS_RUNS = [("fast3", 3), ("fast3", 5), ("fast1", 3), ("fast1", 4), ("fast1", 6)]


def _schedules(name):
    D = R.CROWD[2] if name == "crowd" else R.SHAPES["ragged" if name in ("strided", "one_user") else name][2]
    runs = [("f32", 0), ("b3", 0)]
    if D % 32 == 0:
        runs += [("p3", 0), ("p4", 0), ("fast3", 0), ("fast1", 0)]
        if name == "ragged":
            runs += NS_RUNS
    return runs


RUNS = [(name, sched, ns) for name in R.CASES for sched, ns in _schedules(name)]


class _Cache:
    """one case on the device at a time (inputs, history CSR, planes, largest row norm); every result on the host"""

    def __init__(self):
        self.name, self.dev, self.results, self.excused = None, None, {}, {}

    def device_case(self, name):
        from pixelrec_amd import ops

        if self.name != name:
            self.dev = None
            torch.cuda.empty_cache()
            c = R.case(name)
            if c.ld_users == c.D:
                users = c.users.cuda()
            else:                                        # the evaluator's `last`: a view into a wider buffer
                users = torch.full((c.B, c.ld_users), float("nan"), device="cuda")[:, :c.D]
                users.copy_(c.users)
            c.users_dev, c.table_dev = users, c.table.cuda()
            hu = torch.tensor([u for u, h in enumerate(c.hist) for _ in h], dtype=torch.int64)
            hi = torch.tensor([i for h in c.hist for i in h], dtype=torch.int64)
            c.ptr, c.items = ops.history_csr(hu, hi, c.B, "cuda")
            c.planes = c.vmax = None
            if c.D % 32 == 0:
                assert ops.gemm_mode() == "bf16x3" and ops.score_planes_supported(c.table_dev)
                c.planes, c.vmax = ops.split_planes(c.table_dev), ops.row_norm_max(c.table_dev)
            c.tol = R.tol_abs(c.s64, c.D)
            c.top64 = torch.topk(c.s64, c.K, -1)
            self.name, self.dev = name, c
        return self.dev

    def run(self, name, sched, ns, monkeypatch):
        from pixelrec_amd import ops

        key = (name, sched, ns)
        if key not in self.results:
            c = self.device_case(name)
            for k in KNOBS:
                monkeypatch.delenv(k, raising=False)
            if sched == "p4":
                monkeypatch.setenv("PXR_SCORE_P4", "1")
            if sched in ("fast3", "fast1"):
                monkeypatch.setenv("PXR_TOPK_PRODUCTS", sched[-1])
            if ns:
                monkeypatch.setenv("PXR_TOPK_NS", str(ns))
            kw = {}
            if sched in ("p3", "p4", "fast3", "fast1"):
                kw["table_planes"] = c.planes
            if sched in ("fast3", "fast1"):
                kw["table_norm_max"] = c.vmax
            prev = ops.set_gemm_mode("f32" if sched == "f32" else "bf16x3")
            try:
                idx, val = ops.score_topk(c.users_dev, c.ld_users, c.B, c.table_dev, c.K, c.ptr, c.items, **kw)
                ops.raise_on_bad_indices("cuda")         # no overflow of the candidate buffer, no user short of K candidates
            finally:
                ops.set_gemm_mode(prev)
            self.results[key] = (idx.cpu(), val.cpu())
        return self.results[key]


@pytest.fixture(scope="module")
def cache():
    c = _Cache()
    yield c
    for name in R.CASES:
        if name in c.excused:
            print(f"\nscore_topk {name}: largest excused share {max(c.excused[name]):.4f}")
    c.dev = None
    torch.cuda.empty_cache()


def _check_ids(c, idx):
    """no item 0, nothing outside the catalogue, nothing of the user's history, no id twice"""
    assert idx.shape == (c.B, c.K) and idx.dtype == torch.int64
    assert bool((idx >= 1).all()) and bool((idx < c.N).all())
    for u in range(c.B):
        row = idx[u].tolist()
        assert len(set(row)) == c.K, (u, row)
        assert not set(row) & set(c.hist[u]), (u, sorted(set(row) & set(c.hist[u])))


@pytest.mark.parametrize("name,sched,ns", RUNS, ids=[f"{n}-{s}" + (f"-ns{k}" if k else "") for n, s, k in RUNS])
def test_threshold_schedule_matches_float64(name, sched, ns, cache, monkeypatch):
    idx, val = cache.run(name, sched, ns, monkeypatch)
    c = cache.device_case(name)
    _check_ids(c, idx)
    if c.crowd is None:
        cells, excused = _compare_topk(idx, val, c.s64, c.K, c.tol)
        share = excused / cells
        print(f"{name} {sched} ns={ns}: {excused} of {cells} cells excused ({share:.4f}); tol_abs {c.tol:.3e}")
        cache.excused.setdefault(name, []).append(share)
        assert cells == c.B * c.K and share <= EXCUSED_CAP, (excused, cells)
    else:
        # ties are exact duplicates: values against the float64 top-K, ids from the unmasked duplicates (the CPU tests show that
        # every other item scores lower by far more than tol_abs)
        err = float((val.double() - c.top64.values).abs().max())
        print(f"{name} {sched}: largest value error {err:.3e}; tol_abs {c.tol:.3e}")
        assert err <= c.tol, (err, c.tol)
        allowed = set(c.crowd) - set(c.hist[0])
        for u in range(c.B):
            assert set(idx[u].tolist()) <= (allowed if u == 0 else set(c.crowd)), u


@pytest.mark.parametrize("name", [n for n in R.CASES if len(_schedules(n)) > 2])
def test_bf16x3_schedules_agree_bit_for_bit(name, cache, monkeypatch):
    """fp32 operands split in the main loop, planes on six products, the ping-pong stream, three and one products with the exact
    re-scoring, every ring depth: the same products in the same order (score_topk.hip), so the same ids and the same value bits"""
    runs = [(s, k) for s, k in _schedules(name) if s != "f32"]
    base_idx, base_val = cache.run(name, *runs[0], monkeypatch)
    for sched, ns in runs[1:]:
        idx, val = cache.run(name, sched, ns, monkeypatch)
        assert torch.equal(idx, base_idx), (sched, ns, int((idx != base_idx).sum()))
        assert torch.equal(val.view(torch.int32), base_val.view(torch.int32)), (sched, ns)


@pytest.mark.parametrize("name", list(R.SHAPES) + ["crowd"])
def test_row_norm_max_matches_float64(name, cache):
    from pixelrec_amd import ops

    c = cache.device_case(name)
    want = float(c.table.double().norm(dim=1).max())
    got = float(ops.row_norm_max(c.table_dev))
    assert abs(got - want) <= 1e-5 * want, (got, want)


@pytest.mark.parametrize("sched", ["b3", "p3", "fast3"])
def test_too_few_unmasked_sampled_items_raise_the_overflow_error(sched, monkeypatch):
    """User 1's history leaves K - 1 unmasked items in the tiles that the sample pass scores: its K-th sample value is -inf, the
    threshold admits the whole catalogue (topk_tau_kernel) and the call must end in the candidate-buffer error -- never in a short
    or wrong list.  The status word is clean again afterwards."""
    from pixelrec_amd import ops

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    B, N, D, K = 3, R.MIN_N, 32, 10
    g = torch.Generator().manual_seed(109)
    table = (torch.randn(N, D, generator=g) * 0.02).cuda()
    users = torch.randn(B, D, generator=g).cuda()
    cols = R.sample_columns(N, K)
    cols = cols[cols != 0]
    keep = torch.randperm(cols.numel(), generator=g)[:K - 1]
    gone = torch.ones(cols.numel(), dtype=torch.bool)
    gone[keep] = False
    hist = [[5, 70], cols[gone].tolist(), []]
    hu = torch.tensor([u for u, h in enumerate(hist) for _ in h], dtype=torch.int64)
    hi = torch.tensor([i for h in hist for i in h], dtype=torch.int64)
    ptr, items = ops.history_csr(hu, hi, B, "cuda")
    assert ops.gemm_mode() == "bf16x3"
    kw = {}
    if sched != "b3":
        kw["table_planes"] = ops.split_planes(table)
    if sched == "fast3":
        kw["table_norm_max"] = ops.row_norm_max(table)
    with pytest.raises(RuntimeError, match="candidate buffer"):
        ops.score_topk(users, D, B, table, K, ptr, items, **kw)
        ops.raise_on_bad_indices("cuda")
    ops.raise_on_bad_indices("cuda")


@pytest.mark.parametrize("variant", [1, 3])
def test_register_list_variants_match_float64(variant):
    """PXR_TOPK_VARIANT = 1 (score tile through LDS) and 3 (16 waves, selection in the accumulators) are read once per process:
    each runs tests/test_gpu_topk_bits.py's register-list case in a fresh child.  The child returns ids only; the float64 scores
    of the returned ids stand in for the values, so an id passes only where its float64 score is the rank's within tol_abs."""
    from tests import test_gpu_topk_bits as T

    B, N, D, K, seed = T.REG[T.VARIANT_CASE]
    users, table, ptr, items = T._score_inputs(B, N, D, K, seed)
    ptr, items = ptr.cpu().tolist(), items.cpu().tolist()
    hist = [items[ptr[u]:ptr[u + 1]] for u in range(B)]
    s64 = R.masked_scores(users.cpu(), table.cpu(), hist)
    got = T._variant_child(variant)
    idx = torch.tensor(got["ids"], dtype=torch.int64).view(B, K)
    assert bool((idx >= 1).all()) and bool((idx < N).all()) and all(len(set(r.tolist())) == K for r in idx)
    cells, excused = _compare_topk(idx, s64.gather(1, idx), s64, K, R.tol_abs(s64, D))
    print(f"variant {variant}: {excused} of {cells} cells excused")
    assert cells == B * K and excused <= EXCUSED_CAP * cells, (excused, cells)


@pytest.mark.parametrize("N", [300, R.MIN_N])
def test_k_above_32_is_refused(N):
    from pixelrec_amd import ops
    from pixelrec_amd.lib import PxrError

    table, users = torch.zeros(N, 32, device="cuda"), torch.zeros(2, 32, device="cuda")
    with pytest.raises(PxrError, match=r"K must be in \[1, 32\]"):
        ops.score_topk(users, 32, 2, table, 33)
    ops.raise_on_bad_indices("cuda")                         # refused on the host: nothing was launched
