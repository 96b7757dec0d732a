"""The yardstick of tests/test_gpu_adamw_ref.py, pinned without a GPU (tests/adamw_restate.py):
  * the restated per-step scalars and recurrence agree with torch.optim.AdamW in float64;
  * on EVERY case the GPU tests run, a numpy-float32 emulation of adam_elem (1-ulp sqrt / reciprocal included) stays inside the
    derived bound on every element -- the bound is fair (for the lazy kernels' fast mode this covers the window truncation and the
    closed-form tail, not the fast arithmetic itself: adamw_restate.EmuLazy);
  * every mutant of the update leaves the bound on at least one of those cases -- the bound is sharp enough to mean something.
No element is masked out anywhere: the statements are max(err / bound) <= 1 over whole tensors."""
import math

import numpy as np
import pytest
import torch

from tests import adamw_restate as R

FLAT = R.flat_cases()
TABLE = R.table_cases()
LAZY = R.lazy_cases()


def _ids(cases):
    return [c.name for c in cases]


def test_step_scalars_match_what_torch_applies():
    """One zero-gradient torch step from known moments with eps = 0 is p decay - step_size m b1 / (sqrt(v b2) inv_sqrt_bc2): the three
    restated scalars are the ones torch applies, at small and very large step numbers."""
    for b1, b2 in ((0.9, 0.999), (0.8, 0.98)):
        for t in (1, 2, 10, 1000, 100000):
            lr, wd = 3e-3, 0.1
            p = torch.full((1,), 2.0, dtype=torch.float64, requires_grad=True)
            opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=0.0, weight_decay=wd, foreach=False, amsgrad=False)
            m0, v0 = 0.37, 0.81
            opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.full((1,), m0, dtype=torch.float64),
                            "exp_avg_sq": torch.full((1,), v0, dtype=torch.float64)}
            p.grad = torch.zeros(1, dtype=torch.float64)
            opt.step()
            dec, ss, isb = R.step_scalars(lr, wd, b1, b2, t)
            want = 2.0 * dec - ss * (m0 * b1) / (math.sqrt(v0 * b2) * isb)
            assert abs(float(p.detach()) - want) <= 4e-15 * abs(want), (b1, b2, t)


def test_hyper_restatement_and_its_mutant():
    lrs = [1e-3 * (1 + 0.1 * math.sin(k)) for k in range(50)]
    wds = [0.1] * 50
    hyper, cumlog = R.hyper_restate(lrs, wds, 0.9, 0.999)
    assert tuple(hyper[0]) == (1.0, 0.0, 1.0) and cumlog[0] == 0.0
    want = np.cumsum([math.log(float(np.float32(1.0 - a * b))) for a, b in zip(lrs, wds)])
    tol = R.cumlog_tolerance(cumlog, hyper)
    assert (np.abs(cumlog[1:] - want) <= tol[1:]).all()
    # mutant (h): the previous step's lr in the running sum leaves the tolerance as soon as lr moves ...
    _, bad = R.hyper_restate(lrs, wds, 0.9, 0.999, mutant="h")
    assert (np.abs(bad - cumlog) > tol).any()
    # ... and is invisible at constant lr, which is why the GPU test of the table runs a changing schedule
    _, same = R.hyper_restate([1e-3] * 50, wds, 0.9, 0.999, mutant="h")
    assert np.array_equal(same, R.hyper_restate([1e-3] * 50, wds, 0.9, 0.999)[1])


def _check(ref, be, what):
    rp, rm, rv = ref.ratios(*be.result())
    print(f"[adamw-ref-cpu] {what}: worst err/bound p {rp:.3f} m {rm:.3f} v {rv:.3f}; restated vs torch {ref.restate_gap:.1e}")
    assert ref.restate_gap <= 2e-15, ref.restate_gap          # the bound's intermediates are torch's, to float64 rounding
    assert max(rp, rm, rv) <= 1.0, (what, rp, rm, rv)
    return max(rp, rm, rv)


@pytest.mark.parametrize("c", FLAT, ids=_ids(FLAT))
def test_flat_emulation_inside_the_bound(c):
    rng = np.random.default_rng(7)
    _check(*R.run_flat(c, lambda p, m, v: R.EmuDense(p, m, v, c.betas, rng=rng)), c.name)


@pytest.mark.parametrize("c", TABLE, ids=_ids(TABLE))
def test_table_emulation_inside_the_bound(c):
    rng = np.random.default_rng(8)
    z = lambda p: np.zeros_like(p)
    _check(*R.run_table(c, lambda p: R.EmuTable(p, z(p), z(p), c.betas, rng=rng)), c.name)


@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("c", LAZY, ids=_ids(LAZY))
def test_lazy_emulation_inside_the_bound(c, mode):
    rng = np.random.default_rng(9)
    # (run_lazy itself asserts, from the schedule the launches really follow, that rows with moments meet gaps beyond the window)
    ref, be = R.run_lazy(c, mode, lambda p: R.EmuLazyBackend(p, c.betas, R.WINDOW[mode], rng=rng))
    _check(ref, be, f"{c.name}/{mode}")


@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("tail_mutant", ["rem", "cumlog"])
def test_a_wrong_closed_form_tail_leaves_the_bound(tail_mutant, mode):
    """The lazy cases reach the closed-form tail on rows that carry moments: a tail with one step too many in its powers of b1 / b2,
    or a decay product that starts one table entry late, is caught (weight decay on: D36 runs wd 0.1)."""
    c = next(x for x in LAZY if x.name == "D36")
    assert c.wd > 0
    ref, be = R.run_lazy(c, mode, lambda p: R.EmuLazyBackend(p, c.betas, R.WINDOW[mode], tail_mutant=tail_mutant))
    rp, rm, rv = ref.ratios(*be.result())
    print(f"[adamw-ref-cpu] tail mutant {tail_mutant}/{mode}: err/bound p {rp:.3g} m {rm:.3g} v {rv:.3g}")
    assert (max(rm, rv) > 1.0) if tail_mutant == "rem" else (rp > 1.0)


def _mutant_cases():
    small = [c for c in FLAT if c.n <= 16384]
    return small, TABLE


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_leaves_the_bound(mutant):
    flat, table = _mutant_cases()
    caught = []
    for c in flat:
        ref, be = R.run_flat(c, lambda p, m, v: R.EmuDense(p, m, v, c.betas, mutant=mutant))
        if max(ref.ratios(*be.result())) > 1.0:
            caught.append(c.name)
    for c in table:
        z = lambda p: np.zeros_like(p)
        ref, be = R.run_table(c, lambda p: R.EmuTable(p, z(p), z(p), c.betas, mutant=mutant))
        if max(ref.ratios(*be.result())) > 1.0:
            caught.append("table-" + c.name)
    print(f"[adamw-ref-cpu] mutant ({mutant}) caught by {len(caught)} of {len(flat) + len(table)} cases: {caught[:6]} ...")
    assert caught, mutant
