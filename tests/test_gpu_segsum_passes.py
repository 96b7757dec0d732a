"""The segment sums of the table gradient (csrc/embed_grad.hip: segsum_body behind segsum_kernel<MODE_ROWS | MODE_SASREC | MODE_POOL>,
segsum_apply_kernel and segsum_dense_kernel) on LATER passes and in the SECOND epoch of the short path, in every row-group geometry,
bit for bit: the inputs of tests/segsum_cases.py make every fp32 operation exact, so the float64 sums cast to float32 are the one
right answer and every comparison is torch.equal -- a dropped, doubled, misrouted or mis-signed occurrence moves an element by at
least 1/16.  tests/test_segsum_cases.py shows on the CPU which path, pass count and epoch count each case reaches and where its long
segments sit.  One Gaussian case per mode is held to the worst-case bound of a length-cnt fp32 sum in any order,
(cnt + 2) 2^-24 sum_j |cf_j v_j| |scale|."""
import pytest
import torch

from tests import segsum_cases as SC
from tests import test_gpu_rows_fused as RF

pytestmark = pytest.mark.gpu

T_PREV, B1, B2, EPS = RF.T_PREV, RF.B1, RF.B2, RF.EPS
STATUS_BAD_INDEX = 1                # PXR_STATUS_BAD_INDEX (csrc/pxr_common.h)


def _ids(name):
    return torch.from_numpy(SC.case_ids(name)).cuda()


def _reference(name, items, values, absolute=False):
    spec = SC.SPECS[name]
    uniq, ref, cnt = SC.segment_reference(SC.contributions(name, SC.occurrence_ids(items, spec), values), spec.n_table, absolute)
    assert uniq.numel() == spec.n_uniq
    return uniq, ref, cnt


def _exact(ref, scale):
    r = ref * scale
    assert torch.equal(r.float().double(), r) and float(r.abs().max()) < 2 ** 20      # this draw too: the sums are fp32 numbers
    return r.float()


def _assert_rows(got, want, name, what="rows"):
    if torch.equal(got, want):
        return
    spec = SC.SPECS[name]
    bad = torch.nonzero((got != want).any(1)).view(-1)
    passes = sorted(set((bad // SC.geometry(spec.n_occ, spec.D)[2]).tolist()))
    pytest.fail(f"{name}: {bad.numel()} of {want.shape[0]} {what} differ from the exact sums, in passes {passes} of "
                f"{SC.predict(spec.n_occ, spec.n_uniq, spec.D)}; first ranks {bad[:8].tolist()}")


def _status():
    from pixelrec_amd import ops

    return int(ops.device_status("cuda").item())


# ---- MODE_ROWS ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.ROWS_CASES)
def test_rows_sums_are_exact_on_every_pass(name):
    from pixelrec_amd import ops

    spec = SC.SPECS[name]
    idx = _ids(name)
    (rows,) = SC.case_values(name, "cuda")
    sp = ops.SparseRows(spec.n, spec.D, "cuda")
    sp.rows.fill_(float("nan"))
    ops.embed_grad_rows(idx, rows, spec.n_table, 0.5, out=sp)
    uniq, ref, _ = _reference(name, idx, (rows,))
    k = sp.count()
    assert k == spec.n_uniq and torch.equal(sp.idx[:k], uniq)
    _assert_rows(sp.rows[:k], _exact(ref, 0.5), name)
    assert torch.isnan(sp.rows[k:]).all()                         # nothing beyond the unique rows is written


# ---- MODE_SASREC ----------------------------------------------------------------------------------------------------------------
def _sasrec_inputs(name, draw=SC.exact_rows, draw_coef=SC.exact_coef):
    from pixelrec_amd import ops

    spec = SC.SPECS[name]
    items = _ids(name)
    values = SC.case_values(name, "cuda", draw, draw_coef)
    layout = None if spec.layout == "sasrec" else SC.bert4rec_layout(spec.L)
    ws = torch.empty(ops.occ_ws_bytes(spec.B, spec.L), dtype=torch.uint8, device="cuda")
    return spec, items, values, layout, ws


@pytest.mark.parametrize("name", SC.SASREC_CASES)
def test_sasrec_sums_are_exact_on_every_pass_in_both_layouts_and_routes(name):
    """scale 1 and 0.5; at D = 512 also the split route (ws2: the segment of 1 025 occurrences goes through segsum_parts_kernel /
    segsum_big_kernel), whose sums on exact inputs are the same bits."""
    from pixelrec_amd import ops

    spec, items, (dx0, out, coef), layout, ws = _sasrec_inputs(name)
    uniq, ref, cnt = _reference(name, items, (dx0, out, coef))
    routes = [None]
    if spec.D == 512:
        need2 = ops.occ_split_ws_bytes(spec.B, spec.L, spec.D)
        assert need2 > 0 and int((cnt > SC.SEG_SPLIT).sum()) == 1
        routes.append(torch.zeros(need2, dtype=torch.uint8, device="cuda"))
    ops.device_status("cuda").zero_()
    sp = ops.SparseRows(spec.n_occ, spec.D, "cuda")
    for scale in (1.0, 0.5):
        want = _exact(ref, scale)
        for ws2 in routes:
            sp.rows.fill_(float("nan"))
            sp.n.zero_()
            ops.occ_sort(items, spec.L, layout, spec.n_table, sp, ws)
            ops.sasrec_occ_segsum(ws, dx0, out, coef, spec.n_table, sp, scale, ws2=ws2)
            k = sp.count()
            assert k == spec.n_uniq and torch.equal(sp.idx[:k], uniq)
            _assert_rows(sp.rows[:k], want, name, "rows (split route)" if ws2 is not None else "rows")
            assert torch.isnan(sp.rows[k:]).all()
            if ws2 is not None:                                   # one row went the split way; the cursor is back at zero
                assert ws2[:8].view(torch.int32).tolist() == [0, 1]
    assert _status() == 0


def test_sasrec_id_outside_the_table_is_flagged_and_dropped():
    from pixelrec_amd import ops

    name = "sasrec D=512"
    spec, items, (dx0, out, coef), layout, ws = _sasrec_inputs(name)
    neg = items[:, 1, 1:]
    z0, z1 = torch.nonzero(neg == 0)[:2].tolist()                 # two negatives that held id 0 (dropped either way)
    neg[z0[0], z0[1]] = spec.n_table + 7
    neg[z1[0], z1[1]] = -1
    uniq, ref, _ = _reference(name, items, (dx0, out, coef))
    sp = ops.SparseRows(spec.n_occ, spec.D, "cuda")
    ops.device_status("cuda").zero_()
    try:
        ops.occ_sort(items, spec.L, layout, spec.n_table, sp, ws)
        ops.sasrec_occ_segsum(ws, dx0, out, coef, spec.n_table, sp, 1.0)
        k = sp.count()
        assert _status() & STATUS_BAD_INDEX
        assert k == spec.n_uniq and torch.equal(sp.idx[:k], uniq)
        _assert_rows(sp.rows[:k], _exact(ref, 1.0), name)
    finally:
        ops.device_status("cuda").zero_()


# ---- the apply sink -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hyper():
    return RF._hyper(T_PREV + 1)


def _apply_both(name, hyper, monkeypatch, stale_rank=None):
    """-> (state after segment sums + apply launch, state after the fused launch, the start state, the unique ids)."""
    from pixelrec_amd import ops

    hy, cumlog = hyper
    spec, items, (dx0, out, coef), layout, ws = _sasrec_inputs(name)
    uniq, ref, _ = _reference(name, items, (dx0, out, coef))
    want = _exact(ref, 1.0)
    del ref
    monkeypatch.setattr(RF, "N_TABLE", spec.n_table)              # the aged table, sized to cover the ids
    start = RF._aged_table(spec.D, spec.D)
    assert start[0].shape == (spec.n_table, spec.D)
    if stale_rank is not None:
        start[3][uniq[stale_rank]] = T_PREV - 2
    sp = ops.SparseRows(spec.n_occ, spec.D, "cuda")
    res = []
    for fused in (False, True):
        p, m, v, last = (t.clone() for t in start)
        sp.rows.fill_(float("nan"))
        sp.n.zero_()
        ops.occ_sort(items, spec.L, layout, spec.n_table, sp, ws)
        if fused:
            ops.sasrec_occ_segsum_apply(ws, dx0, out, coef, spec.n_table, sp, p, m, v, last, hy, T_PREV, B1, B2, EPS)
            assert torch.isnan(sp.rows).all()                     # the summed rows are never written
        else:
            ops.sasrec_occ_segsum(ws, dx0, out, coef, spec.n_table, sp, 1.0)
            ops.adamw_rows(p, m, v, last, hy, cumlog, T_PREV, T_PREV + 1, B1, B2, EPS, rows=sp.idx, n_rows=sp.n, max_rows=sp.cap,
                           grows=sp.rows)
            k = sp.count()
            assert k == spec.n_uniq and torch.equal(sp.idx[:k], uniq)
            _assert_rows(sp.rows[:k], want, name)
        torch.cuda.synchronize()
        res.append((p, m, v, last))
    return res[0], res[1], start, uniq


@pytest.mark.parametrize("name", SC.SASREC_CASES)
def test_apply_sink_equals_segment_sums_then_apply_on_every_pass(name, hyper, monkeypatch):
    from pixelrec_amd import ops

    ops.device_status("cuda").zero_()
    two, one, start, uniq = _apply_both(name, hyper, monkeypatch)
    for a, b, what in zip(two, one, "pmvl"):
        assert torch.equal(a, b), what
    named = torch.zeros(SC.SPECS[name].n_table, dtype=torch.bool, device="cuda")
    named[uniq] = True
    assert not bool(named[0]) and int(named.sum()) == SC.SPECS[name].n_uniq
    assert (one[3][named] == T_PREV + 1).all() and (one[3][~named] == T_PREV).all()
    assert (one[0][named] != start[0][named]).any(1).all()        # every named row moved
    for a, s in zip(one, start):                                  # rows not named (row 0 among them) are untouched
        assert torch.equal(a[~named], s[~named])
    assert _status() == 0


@pytest.mark.parametrize("kind", ["short", "long"])
def test_apply_sink_leaves_a_stale_row_of_the_second_epoch_untouched_and_flags_it(kind, hyper, monkeypatch):
    """One named row in pass 16 (the first of the second epoch) is not current through the previous step: a short segment (its mark
    waits in s_close for the epoch's barrier) or the long one the case plants there (seg_long_row closes it).  The fused launch
    leaves it exactly as it was and raises the status bit; every other row is updated as usual."""
    from pixelrec_amd import ops

    name = "sasrec D=1028"
    spec = SC.SPECS[name]
    long_rank = next(r for r, c in SC.planted(spec).items() if SC.pass_of(r, spec.n_occ, spec.D) == SC.SEG_EPOCH)
    rank = long_rank if kind == "long" else long_rank + 5
    assert SC.pass_of(rank, spec.n_occ, spec.D) == SC.SEG_EPOCH and (rank in SC.planted(spec)) == (kind == "long")
    ops.device_status("cuda").zero_()
    try:
        two, one, start, uniq = _apply_both(name, hyper, monkeypatch, stale_rank=rank)
        assert _status() & ops.STATUS_ROWS_STALE
        with pytest.raises(RuntimeError, match="not current"):
            ops.raise_on_bad_indices("cuda")
        assert _status() == 0
    finally:
        ops.device_status("cuda").zero_()
    row = int(uniq[rank])
    for a, s in zip(one, start):
        assert torch.equal(a[row], s[row])
    assert int(two[3][row]) == T_PREV + 1                         # (the reference path replayed and applied it)
    others = torch.ones(spec.n_table, dtype=torch.bool, device="cuda")
    others[row] = False
    for a, b in zip(two, one):
        assert torch.equal(a[others], b[others])
    named = torch.zeros(spec.n_table, dtype=torch.bool, device="cuda")
    named[uniq] = True
    assert (one[3][named & others] == T_PREV + 1).all()


# ---- MODE_POOL ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.POOL_CASES)
def test_pool_sums_are_exact_in_sparse_rows_and_in_the_dense_block(name):
    from pixelrec_amd import ops

    spec = SC.SPECS[name]
    gidx = _ids(name)
    G, w = SC.case_values(name, "cuda")
    uniq, ref, _ = _reference(name, gidx, (G, w))
    want = _exact(ref, 1.0)
    sp = ops.SparseRows(spec.n_occ, spec.D, "cuda")
    sp.rows.fill_(float("nan"))
    ops.pool_table_grad(gidx, spec.B, spec.L, G, w, spec.n_table, out=sp)
    k = sp.count()
    assert k == spec.n_uniq and torch.equal(sp.idx[:k], uniq)
    _assert_rows(sp.rows[:k], want, name)
    assert torch.isnan(sp.rows[k:]).all()
    d = torch.full((spec.n_table, spec.D), float("nan"), device="cuda")
    assert ops.pool_dense_grad(gidx, spec.B, spec.L, G, w, spec.n_table, out=d) is d
    _assert_rows(d[uniq], want, name, "rows of the dense block")
    named = torch.zeros(spec.n_table, dtype=torch.bool, device="cuda")
    named[uniq] = True
    assert (d[~named].view(torch.int32) == 0).all()               # +0.0, sign bit included, at row 0 and every unreferenced row


# ---- Gaussian inputs ------------------------------------------------------------------------------------------------------------
def _assert_within_sum_bound(got, ref, absref, cnt, scale, name):
    bound = (cnt + 2).double().unsqueeze(1) * 2.0 ** -24 * absref * abs(scale)
    err = (got.double() - ref * scale).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: max |error| / bound = {ratio:.4f} (max |error| {float(err.max()):.3e}, longest segment {int(cnt.max())})")
    assert torch.isfinite(got).all() and (err <= bound).all(), ratio


@pytest.mark.parametrize("name", SC.GAUSS_CASES)
def test_gaussian_inputs_stay_inside_the_worst_case_bound_of_an_fp32_sum(name):
    from pixelrec_amd import ops

    spec = SC.SPECS[name]
    items = _ids(name)
    values = SC.case_values(name, "cuda", SC.gauss, SC.gauss)
    uniq, ref, cnt = _reference(name, items, values)
    _, absref, _ = _reference(name, items, values, absolute=True)
    sp = ops.SparseRows(spec.n_occ, spec.D, "cuda")
    sp.rows.fill_(float("nan"))
    scale = 1.0
    if spec.mode == "rows":
        scale = 0.5
        ops.embed_grad_rows(items, values[0], spec.n_table, scale, out=sp)
    elif spec.mode == "sasrec":
        scale = 0.5
        ws = torch.empty(ops.occ_ws_bytes(spec.B, spec.L), dtype=torch.uint8, device="cuda")
        ops.occ_sort(items, spec.L, None, spec.n_table, sp, ws)
        ops.sasrec_occ_segsum(ws, *values, spec.n_table, sp, scale)
    else:
        ops.pool_table_grad(items, spec.B, spec.L, *values, spec.n_table, out=sp)
    k = sp.count()
    assert k == spec.n_uniq and torch.equal(sp.idx[:k], uniq)
    _assert_within_sum_bound(sp.rows[:k], ref, absref, cnt, scale, name)
    if spec.mode == "pool":
        d = ops.pool_dense_grad(items, spec.B, spec.L, *values, spec.n_table)
        assert torch.equal(d[uniq], sp.rows[:k])
