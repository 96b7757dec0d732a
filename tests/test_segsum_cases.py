"""The inputs of tests/test_gpu_segsum_passes.py, checked without a GPU and with nothing from the library: every case reaches the
path, pass count and epoch count it is meant to, holds the segment lengths it is meant to hold at the ranks (= passes) it is meant to
hold them, and its float64 segment sums are float32 numbers -- so the GPU tests may compare with torch.equal.  The sums are formed
here on a CPU draw of the values (the first 32 columns of the wide cases: the columns are independent draws of one distribution, and
the argument -- multiples of 1/8, below 2^18 -- is per element); the GPU tests assert the same of their own draw at full width."""
import numpy as np
import pytest
import torch

from tests import segsum_cases as SC


def _segments(name):
    """-> (spec, ids as built, flat occurrence ids, ascending valid unique ids, their occurrence counts)."""
    spec = SC.SPECS[name]
    items = SC.case_ids(name)
    flat = SC.occurrence_ids(items, spec)
    valid = flat[(flat > 0) & (flat < spec.n_table)]
    uniq, cnt = np.unique(valid, return_counts=True)
    return spec, items, flat, uniq, cnt


@pytest.mark.parametrize("name", list(SC.SPECS))
def test_case_reaches_its_path_passes_and_epochs(name):
    spec, items, flat, uniq, cnt = _segments(name)
    n = flat.size
    assert n == spec.n_occ and uniq.size == spec.n_uniq
    got = SC.predict(n, uniq.size, spec.D)
    sort = "fused" if n <= SC.FUSED_SORT_MAX else "multi-launch"
    print(f"{name}: n={n} n_uniq={uniq.size} -> path={got[0]} G={got[1]} passes={got[2]} epochs={got[3]}, {sort} sort")
    assert got == spec.expect
    assert sort == ("multi-launch" if spec.D == 1028 else "fused")
    # id 0; MODE_ROWS: one id beyond the table and one negative id
    assert int((flat == 0).sum()) >= 1
    if spec.mode == "rows":
        assert int((flat >= spec.n_table).sum()) == 1 and int((flat < 0).sum()) == 1
    else:
        assert flat.min() == 0 and flat.max() < spec.n_table
    if spec.mode == "sasrec" and spec.layout == "sasrec":           # the slot nobody reads holds the top id
        assert (items[:, 1, 0] == uniq[-1]).all() and cnt[-1] == spec.high[-1]
    # the lengths at both ends; every length of ENDS somewhere, where the case has room for it
    assert tuple(cnt[:len(spec.low)]) == spec.low and tuple(cnt[-len(spec.high):]) == spec.high
    want = set(SC.ENDS) if n > 2 * sum(SC.ENDS[-2:]) else {1, 2, 8, 9}
    assert want <= set(cnt.tolist())
    # where the long segments are: the first pass, the last, and every pass the case names
    passes = got[2]
    long_passes = set((np.nonzero(cnt > SC.SEG_SHORT)[0] // SC.geometry(n, spec.D)[2]).tolist())
    assert {0, passes - 1} | set(spec.mid) <= long_passes, long_passes
    if got[3] == 2:
        assert {SC.SEG_EPOCH - 1, SC.SEG_EPOCH} <= long_passes and passes - 1 > SC.SEG_EPOCH
    elif passes >= 3:
        assert any(0 < p < passes - 1 for p in long_passes)
    assert all(c == SC.planted(spec).get(r, c) for r, c in enumerate(cnt.tolist()))
    # short path: every pass sums short segments of 2 and of 3 or more occurrences (the first two ids of a segment travel in
    # registers from the pass before, the others are read in the pass itself)
    if got[0] == "short":
        ps = np.arange(uniq.size) // SC.geometry(n, spec.D)[2]
        for p in range(passes):
            here = cnt[ps == p]
            assert ((here >= 2) & (here <= SC.SEG_SHORT)).any() and ((here >= 3) & (here <= SC.SEG_SHORT)).any(), p
    # the same ids on every build
    SC.case_ids.cache_clear()
    assert np.array_equal(SC.case_ids(name), items)


@pytest.mark.parametrize("name", list(SC.SPECS))
def test_case_sums_are_float32_numbers(name):
    spec, items, flat, uniq, cnt = _segments(name)
    values = SC.case_values(name, "cpu", cols=min(spec.D, 32))
    for v in values:
        assert torch.equal(v, v.double().float())
    rows, coefs = (values[:-1], values[-1:]) if spec.mode != "rows" else (values, ())
    for v in rows:
        assert float(v.abs().max()) <= 8 and torch.equal(v * 4, (v * 4).round())
    for v in coefs:
        assert set(v.abs().unique().tolist()) <= {0.5, 1.0, 2.0}
    u, ref, c = SC.segment_reference(SC.contributions(name, torch.from_numpy(flat), values), spec.n_table)
    assert np.array_equal(u.numpy(), uniq) and np.array_equal(c.numpy(), cnt)
    for scale in (1.0, 0.5):
        r = ref * scale
        assert torch.equal(r.float().double(), r) and float(r.abs().max()) < 2 ** 20
    assert float(ref.abs().max()) <= 16 * int(cnt.max())
    assert int((ref != 0).any(1).sum()) > 0.99 * uniq.size


@pytest.mark.parametrize("length", [1, 9, 513, 1025, 12000])
def test_exact_recipe_sums_the_same_bits_in_any_order(length):
    """One segment of `length` occurrences: the products are exact (so a fused multiply-add changes nothing) and float32 running sums
    taken forwards, backwards and in a random order all end on the float64 sum."""
    gen = torch.Generator().manual_seed(length)
    prod = SC.exact_rows((length, 16), gen) * SC.exact_coef((length, 1), gen)
    assert torch.equal(prod * 8, (prod * 8).round()) and float(prod.abs().max()) <= 16          # multiples of 1/8 up to 16
    want = prod.double().sum(0)
    assert torch.equal(want.float().double(), want)
    for order in (torch.arange(length), torch.arange(length - 1, -1, -1), torch.randperm(length, generator=gen)):
        acc = torch.zeros(16, dtype=torch.float32)
        for row in prod[order]:
            acc = acc + row
        assert torch.equal(acc, want.float()) and torch.equal(0.5 * acc, (0.5 * want).float())


def test_the_cases_cover_every_row_group_geometry():
    two_epochs = {SC.SPECS[k].mode for k in SC.SPECS if SC.SPECS[k].expect[3] == 2}
    assert two_epochs == {"rows", "sasrec", "pool"}
    multi = {SC.SPECS[k].expect[1] for k in SC.SPECS if SC.SPECS[k].expect[0] == "short" and SC.SPECS[k].expect[2] >= 2}
    assert multi >= {1, 2, 4, 5, 7, 8}
    assert {SC.SPECS[k].expect[0] for k in SC.ROWS_CASES} == {"row", "short", "wide"}
    assert {SC.SPECS[k].layout for k in SC.SASREC_CASES} == {"sasrec", "bert4rec"}


def test_predict_at_the_thresholds():
    assert SC.predict(40000, 16384, 512) == ("short", 4, 1, 1) and SC.predict(40000, 16385, 512) == ("short", 4, 2, 1)
    assert SC.predict(72000, 65536, 1028) == ("short", 1, 16, 1) and SC.predict(72000, 65537, 1028) == ("short", 1, 17, 2)
    assert SC.predict(300, 300, 2048) == ("short", 1, 1, 1) and SC.predict(300, 203, 4096) == ("wide", 1, 1, 1)   # a grid of n < 4096
    assert SC.predict(5000, 5000, 248)[:2] == ("short", 8) and SC.predict(5000, 5000, 224)[:2] == ("row", 9)
    assert SC.predict(5000, 5000, 2048)[:2] == ("short", 1) and SC.predict(5000, 5000, 2052)[:2] == ("wide", 1)
