"""Every AdamW kernel of csrc/adamw.hip against torch.optim.AdamW in float64 (tests/adamw_restate.py): p, m and v elementwise
against a forward error bound derived from the roundings the kernels commit -- no scalar of the truth comes from the library.
tests/test_adamw_ref_cpu.py shows without a GPU that the bound is fair (a float32 emulation stays inside it on these very cases) and
sharp (every mutant of the update leaves it).

MEASURED on the MI355X: worst error / bound over every element of every case of the group (the margin against 1 is the evidence,
not a tolerance to tune):
    group                                         p       m       v
    b. adamw_flat == adamw_flat_tab (40 cases)    0.371   0.490   0.451
    c. flat_tab, plain launch of the segment set  0.348   0.444   0.436     (segment launches: bit-identical to it)
    e. adamw_table (10 cases)                     0.194   0.324   0.414
    f. lazy rows, PXR_LAZY_REPLAY=exact (16)      0.197   0.303   0.335
    f. lazy rows, default fast replay (16)        0.197   0.337   0.335
a. / d. are exact statements (1 ulp on the two pow-based scalars, bit equality elsewhere).  Wall time of the module: 27 s (101 tests).

MUTATION CHECK on the real kernels (by hand, not committed): a scratch build of the library with the weight decay dropped where
the scalar is made (decay = 1 in make_hyper and hyper_append_body, so that every kernel and the cumlog table stay consistent with
each other).  Of the 22 tests selected by `-k "run40 or D64 or hyper_append or close"` 18 fail (the 4 that pass run wd = 0);
tests/test_gpu_lazy_adamw.py and tests/test_gpu_lazy_series.py pass on the same library, 36 of 36.
"""
import time

import numpy as np
import pytest
import torch

from pixelrec_amd.lib import PxrError
from tests import adamw_restate as R

pytestmark = pytest.mark.gpu

EPS = R.EPS
FLAT, TABLE, LAZY = R.flat_cases(), R.table_cases(), R.lazy_cases()
_T0 = time.time()


def _ids(cases):
    return [c.name for c in cases]


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _report(group, name, ref, p, m, v):
    rp, rm, rv = ref.ratios(_np(p), _np(m), _np(v))
    print(f"[adamw-ref] {group} {name}: worst err/bound p {rp:.3f} m {rm:.3f} v {rv:.3f} (module wall time so far {time.time() - _T0:.0f} s)")
    assert rp <= 1.0 and rm <= 1.0 and rv <= 1.0, (group, name, rp, rm, rv)


def _assert_scalars(got4, lr, wd, b1, b2, t):
    """A float4 hyper entry against the float32-rounded float64 formulas: decay exact, the two pow-based scalars within 1 ulp."""
    want = np.array(R.step_scalars(lr, wd, b1, b2, t)).astype(np.float32)
    got = np.asarray(got4, dtype=np.float32)
    assert got[0] == want[0] and got[3] == 0.0, (t, got, want)
    assert R.ulp_distance(got[1:3], want[1:3]).max() <= 1, (t, got, want)


# ---------------------------------------------------------------------------------------------------------- a. hyper table
def _schedule(T, changing):
    if not changing:
        return [1e-3] * T, [0.1] * T
    lrs = [1e-3 * min(1.0, (k + 1) / 10.0) * (1.0 - 0.6 * k / T) for k in range(T)]
    wds = [0.1 if k % 7 else 0.05 for k in range(T)]
    return lrs, wds


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.8, 0.98)])
@pytest.mark.parametrize("changing", [False, True])
@pytest.mark.parametrize("form", ["host_step", "step_dev", "advance"])
def test_hyper_append(form, changing, betas):
    from pixelrec_amd import ops

    T, (b1, b2) = 60, betas
    lrs, wds = _schedule(T, changing)
    cap = T + 1                                                             # rows 0..T: step T is the last one that fits
    hyper_big = torch.full((cap + 4, 4), 7.0, device="cuda")
    cumlog_big = torch.full((cap + 4,), 7.0, dtype=torch.float64, device="cuda")
    hyper, cumlog = hyper_big[:cap], cumlog_big[:cap]
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    for t in range(1, T + 1):
        if form == "host_step":
            ops.adamw_hyper_append(hyper, cumlog, t, lrs[t - 1], b1, b2, EPS, wds[t - 1])
        elif form == "step_dev" or t == 1:
            ops.adamw_hyper_append(hyper, cumlog, 0, lrs[t - 1], b1, b2, EPS, wds[t - 1], step_dev=counter)
            assert int(counter) == (t - 1 if form == "step_dev" else 0)     # this form never counts
            if form == "step_dev":
                ops.counter_add(counter, 1)
        else:                                                               # closes step t-1, appends step t
            ops.adamw_hyper_append(hyper, cumlog, 0, lrs[t - 1], b1, b2, EPS, wds[t - 1], step_dev=counter, advance=True)
            assert int(counter) == t - 1                                    # advanced exactly once
    want_h, want_c = R.hyper_restate(lrs, wds, b1, b2)
    got_h, got_c = _np(hyper), _np(cumlog)
    assert tuple(got_h[0]) == (1.0, 0.0, 1.0, 0.0) and got_c[0] == 0.0      # the identity entry
    for t in range(1, T + 1):
        _assert_scalars(got_h[t], lrs[t - 1], wds[t - 1], b1, b2, t)
    assert (np.abs(got_c - want_c) <= R.cumlog_tolerance(want_c, want_h)).all(), np.abs(got_c - want_c).max()
    if changing:                                                            # the tolerance tells the mutant (h) apart
        assert (np.abs(got_c - R.hyper_restate(lrs, wds, b1, b2, mutant="h")[1]) > R.cumlog_tolerance(want_c, want_h)).any()
    # step >= capacity: nothing is written, neither inside the table nor behind it
    before_h, before_c = hyper_big.clone(), cumlog_big.clone()
    if form == "host_step":
        with pytest.raises(PxrError, match="pxr_adamw_hyper_append"):
            ops.adamw_hyper_append(hyper, cumlog, cap, 1e-3, b1, b2, EPS, 0.1)
    else:
        counter.fill_(cap - 1)
        ops.adamw_hyper_append(hyper, cumlog, 0, 1e-3, b1, b2, EPS, 0.1, step_dev=counter, advance=form == "advance")
        assert int(counter) == (cap if form == "advance" else cap - 1)
    assert torch.equal(hyper_big, before_h) and torch.equal(cumlog_big, before_c)
    assert bool((hyper_big[cap:] == 7.0).all()) and bool((cumlog_big[cap:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------- b. flat kernels
class _GpuFlat:
    """ops.adamw_flat on one copy, ops.adamw_flat_tab (scalars from a hyper table filled by adamw_hyper_append) on another: both
    must hold the same bits after every step.  Even steps take the table's host `step` form, odd ones the device counter."""

    def __init__(self, p0, m0, v0, c):
        from pixelrec_amd import ops

        self.ops, self.c = ops, c
        self.a = [_cu(x) for x in (p0, m0, v0)]
        self.b = [x.clone() for x in self.a]
        rows = c.t0 + c.T + 8
        self.hyper = torch.zeros(rows, 4, device="cuda")
        self.cumlog = torch.zeros(rows, dtype=torch.float64, device="cuda")
        self.counter = torch.zeros(1, dtype=torch.int64, device="cuda")
        ops.counter_add(self.counter, c.t0)
        assert int(self.counter) == c.t0

    def step(self, g, lr, wd, t):
        ops, (b1, b2) = self.ops, self.c.betas
        gd = _cu(g)
        ops.adamw_flat(*self.a[:1], gd, *self.a[1:], lr, b1, b2, EPS, wd, t)
        ops.adamw_hyper_append(self.hyper, self.cumlog, t, lr, b1, b2, EPS, wd)
        if t % 2 == 0:
            ops.adamw_flat_tab(self.b[0], gd, self.b[1], self.b[2], self.hyper, t, b1, b2, EPS)
        else:
            ops.adamw_flat_tab(self.b[0], gd, self.b[1], self.b[2], self.hyper, 0, b1, b2, EPS, step_dev=self.counter)
        ops.counter_add(self.counter, 1)
        for x, y in zip(self.a, self.b):
            assert torch.equal(x, y), ("adamw_flat and adamw_flat_tab differ", self.c.name, t)


@pytest.mark.parametrize("c", FLAT, ids=_ids(FLAT))
def test_flat_and_flat_tab(c):
    ref, be = R.run_flat(c, lambda p, m, v: _GpuFlat(p, m, v, c))
    assert int(be.counter) == c.t0 + c.T
    _report("flat", c.name, ref, *be.a)


def test_slot_fill_and_counter_add():
    from pixelrec_amd import ops

    for n in (1, 255, 2048 * 256 + 77):                                     # the last one is past the 2048-block launch cap
        big = torch.full((n + 8,), 5, dtype=torch.int32, device="cuda")
        ops.slot_fill(big[:n], -1)
        assert bool((big[:n] == -1).all()) and bool((big[n:] == 5).all())
        ops.slot_fill(big[:n], 3)
        assert bool((big[:n] == 3).all()) and bool((big[n:] == 5).all())
    c = torch.tensor([2 ** 40], dtype=torch.int64, device="cuda")
    ops.counter_add(c, 5); ops.counter_add(c, -7); ops.counter_add(c)
    assert int(c) == 2 ** 40 - 1


# ---------------------------------------------------------------------------------------------------------- c. plane segments
def _flat_problem(c):
    """One step of a flat case of adamw_restate (SEGMENT_CASE / CLOSE_CASE: also run by test_flat_and_flat_tab and by the CPU check)."""
    from pixelrec_amd import ops

    p0, m0, v0, gs = R.flat_inputs(c)
    t, lr, wd, (b1, b2) = c.t0 + 1, c.lrs()[0], c.wd, c.betas
    hyper = torch.zeros(t + 8, 4, device="cuda")
    cumlog = torch.zeros(t + 8, dtype=torch.float64, device="cuda")
    ops.adamw_hyper_append(hyper, cumlog, t, lr, b1, b2, EPS, wd)
    state = lambda: [_cu(x) for x in (p0, m0, v0)]
    return state, _cu(gs[0]), hyper, cumlog, (t, lr, wd, b1, b2), (p0, m0, v0, gs[0])


def _plain(state, g, hyper, hp):
    from pixelrec_amd import ops

    p, m, v = state()
    ops.adamw_flat_tab(p, g, m, v, hyper, hp[0], hp[3], hp[4], EPS)
    return p, m, v


def test_flat_tab_plain_launch_of_the_segment_problem_against_the_reference():
    state, g, hyper, _, hp, (p0, m0, v0, gn) = _flat_problem(R.SEGMENT_CASE)
    ref = R.Reference(p0, hp[3], hp[4], EPS, t0=hp[0] - 1, m0=m0, v0=v0)
    ref.step(gn, hp[1], hp[2])
    _report("planes", "plain launch", ref, *_plain(state, g, hyper, hp))


@pytest.mark.parametrize("n_seg", [3, 16, 17])
def test_flat_tab_bf16x3_segments(n_seg):
    """17 segments: the 17th is split by the launch behind the optimizer's (MULTI_MAX = 16 per fused launch)."""
    from pixelrec_amd import ops

    shapes = [(32, 64), (64, 32), (96, 32)] if n_seg == 3 else [(32, 32)] * n_seg
    state, g, hyper, _, hp, _ = _flat_problem(R.SEGMENT_CASE)
    want = _plain(state, g, hyper, hp)
    segs, off = [], 128                                                     # gaps before, between and behind the segments
    for r, c in shapes:
        segs.append((off, r, c, ops.Planes.alloc(r, c, "cuda")))
        off += r * c + 64
    assert off < 64 * 400
    p, m, v = state()
    ops.adamw_flat_tab(p, g, m, v, hyper, hp[0], hp[3], hp[4], EPS, plane_segments=segs)
    for x, y in zip((p, m, v), want):
        assert torch.equal(x, y)                                            # the fp32 result is the no-segments launch's, everywhere
    assert not torch.equal(p, state()[0])
    for o, r, c, pl in segs:
        assert torch.equal(pl.to_dense(), p[o:o + r * c].view(r, c)), (o, r, c)


def test_flat_tab_h2_segments_and_the_range_flag():
    from pixelrec_amd import ops

    shapes = [(32, 64), (64, 32), (96, 32)]
    state, g, hyper, _, hp, _ = _flat_problem(R.SEGMENT_CASE)
    want = _plain(state, g, hyper, hp)
    offs, off = [], 128
    for r, c in shapes:
        offs.append(off)
        off += r * c + 64
    mats = [want[0][o:o + r * c].view(r, c) for o, (r, c) in zip(offs, shapes)]
    status = ops.device_status("cuda")
    status.zero_()
    split = ops.split_planes_multi(mats, h2=True)                           # the existing split entry point, host-chosen exponents
    exps = torch.tensor([s.exp for s in split], dtype=torch.int32, device="cuda")
    segs = [(o, r, c, ops.Planes.alloc(r, c, "cuda", fmt=1)) for o, (r, c) in zip(offs, shapes)]
    p, m, v = state()
    ops.adamw_flat_tab(p, g, m, v, hyper, hp[0], hp[3], hp[4], EPS, plane_segments=segs, planes_exps=exps)
    for x, y in zip((p, m, v), want):
        assert torch.equal(x, y)
    for (o, r, c, pl), s in zip(segs, split):
        assert torch.equal(pl.buf, s.buf), (o, r, c)                        # same planes, bit for bit, under the same exponent
        pl.exp = s.exp
        assert torch.equal(pl.to_dense(), s.to_dense())
    assert int(status) == 0
    # a weight pushed past the exponent's range: |w| 2^exp beyond 65504 raises the flag in the status word, nothing else happens
    far = exps.clone()
    far[1] += 6
    p, m, v = state()
    ops.adamw_flat_tab(p, g, m, v, hyper, hp[0], hp[3], hp[4], EPS, plane_segments=segs, planes_exps=far)
    torch.cuda.synchronize()
    assert int(status) & 64                                                 # PXR_STATUS_H2_RANGE
    for x, y in zip((p, m, v), want):
        assert torch.equal(x, y)                                            # the fp32 update itself is untouched
    status.zero_()


# ---------------------------------------------------------------------------------------------------------- d. close=
def test_flat_tab_close_counts_the_step_and_appends_the_next_entry():
    from pixelrec_amd import ops

    state, g, hyper, cumlog, hp, _ = _flat_problem(R.CLOSE_CASE)
    t, lr, wd, b1, b2 = hp
    lr_next, wd_next = 0.7 * lr, 0.05
    want = _plain(state, g, hyper, hp)
    # twin table closed by a launch of its own
    h2_, c2_ = hyper.clone(), cumlog.clone()
    cnt2 = torch.tensor([t - 1], dtype=torch.int64, device="cuda")
    ops.adamw_hyper_append(h2_, c2_, 0, lr_next, b1, b2, EPS, wd_next, step_dev=cnt2, advance=True)
    cnt = torch.tensor([t - 1], dtype=torch.int64, device="cuda")
    cur = hyper[t].clone()
    p, m, v = state()
    ops.adamw_flat_tab(p, g, m, v, hyper, 0, b1, b2, EPS, step_dev=cnt, close=(cumlog, cur, lr_next, wd_next))
    for x, y in zip((p, m, v), want):
        assert torch.equal(x, y)
    assert int(cnt) == t == int(cnt2)
    assert torch.equal(hyper, h2_) and torch.equal(cumlog, c2_)
    _assert_scalars(_np(hyper[t + 1]), lr_next, wd_next, b1, b2, t + 1)
    step_log = float(np.log(np.float64(np.float32(1.0 - lr_next * wd_next))))
    assert abs(float(cumlog[t + 1]) - (float(cumlog[t]) + step_log)) <= 2.0 ** -51 * abs(step_log) + 2.0 ** -53 * abs(float(cumlog[t + 1]))


# ---------------------------------------------------------------------------------------------------------- e. dense table sweep
class _GpuTable:
    def __init__(self, p0, c):
        from pixelrec_amd import ops

        self.ops, self.c = ops, c
        self.p = _cu(p0)
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.slot = torch.full((c.N,), 9, dtype=torch.int32, device="cuda")
        ops.slot_fill(self.slot, -1)

    def step(self, ids, n, rows, g, lr, wd, t):
        ops, c = self.ops, self.c
        sp = None
        if ids is not None:
            sp = ops.SparseRows(c.cap, c.D, "cuda")
            sp.idx.copy_(_cu(ids)); sp.rows.copy_(_cu(rows)); sp.n.fill_(n)
        ops.adamw_table(self.p, self.m, self.v, self.slot, sp, lr, c.betas[0], c.betas[1], EPS, wd, t)
        assert int((self.slot != -1).sum()) == 0


@pytest.mark.parametrize("c", TABLE, ids=_ids(TABLE))
def test_table_sweep(c):
    ref, be = R.run_table(c, lambda p: _GpuTable(p, c))
    _report("table", c.name, ref, be.p, be.m, be.v)


# ---------------------------------------------------------------------------------------------------------- f. lazy rows
class _GpuLazy:
    """The lazy schedule on the library: hyper_append, catch-up from raw id lists (flat and 2-D in turn), apply, flush.  Odd-seeded
    cases read the step from the device counter."""

    def __init__(self, p0, c):
        from pixelrec_amd import ops

        self.ops, self.c = ops, c
        self.p = _cu(p0)
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.last = torch.zeros(c.N, dtype=torch.int32, device="cuda")
        self.hyper = torch.zeros(c.T + 8, 4, device="cuda")
        self.cumlog = torch.zeros(c.T + 8, dtype=torch.float64, device="cuda")
        self.dev = c.seed % 2 == 1
        self.counter = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.lrwd = {}

    def _st(self):
        return (self.p, self.m, self.v, self.last, self.hyper, self.cumlog)

    def append(self, lr, wd, t):
        self.lrwd[t] = (lr, wd)
        self.ops.adamw_hyper_append(self.hyper, self.cumlog, t, lr, self.c.betas[0], self.c.betas[1], EPS, wd)

    def catch_up_raw(self, raw, t_prev, k):
        ops, c, (b1, b2) = self.ops, self.c, self.c.betas
        before = self.last.clone()
        sd = self.counter if self.dev else None
        if (k // 5) % 2 == 0:
            ops.adamw_rows_ids(*self._st(), t_prev, b1, b2, EPS, _cu(raw), step_dev=sd)
        else:
            n_lists, row_len, stride = 4, raw.size // 4, raw.size // 4 + 3
            win = np.full((n_lists, stride), 2 ** 50, dtype=np.int64)        # outside the window: never read
            win[:, :row_len] = raw.reshape(n_lists, row_len)
            cur = torch.full((4,), 9.0, device="cuda")
            ops.adamw_rows_ids2d(*self._st(), t_prev, b1, b2, EPS, _cu(win), n_lists, row_len, stride, step_dev=sd, cur_hyper_out=cur)
            _assert_scalars(_np(cur), *self.lrwd[t_prev + 1], b1, b2, t_prev + 1)     # the step about to run
        want = before.clone()
        want[_cu(R.valid_rows(raw, c.N))] = t_prev
        assert torch.equal(self.last, torch.maximum(want, before))          # the rows named, once; nothing else

    def apply(self, ids, n, rows, t):
        ops, c, (b1, b2) = self.ops, self.c, self.c.betas
        n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
        ops.adamw_rows(*self._st(), t - 1, t, b1, b2, EPS, rows=_cu(ids), n_rows=n_dev, max_rows=c.cap, grows=_cu(rows),
                       step_dev=self.counter if self.dev else None)
        if self.dev:
            ops.counter_add(self.counter, 1)

    def flush(self, T):
        b1, b2 = self.c.betas
        self.ops.adamw_rows(*self._st(), T, 0, b1, b2, EPS)
        assert int((self.last != T).sum()) == 0


@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("c", LAZY, ids=_ids(LAZY))
def test_lazy_rows(c, mode, monkeypatch):
    if mode == "exact":
        monkeypatch.setenv("PXR_LAZY_REPLAY", "exact")
    else:
        monkeypatch.delenv("PXR_LAZY_REPLAY", raising=False)
    ref, be = R.run_lazy(c, mode, lambda p: _GpuLazy(p, c))
    _report("lazy-" + mode, c.name, ref, be.p, be.m, be.v)
