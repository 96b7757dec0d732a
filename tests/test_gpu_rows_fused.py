"""The lazy AdamW row update applied inside the segment sums of the table gradient (csrc/embed_grad.hip: segsum_apply_kernel behind
pxr_sasrec_occ_segsum_apply) == the two launches it replaces (pxr_sasrec_occ_segsum, then pxr_adamw_rows_f32 in apply mode), bit
for bit: the same adds in the same order, the same per-element AdamW body (csrc/adam_row.cuh).  No tolerance anywhere."""
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_TABLE, T_PREV = 2000, 7
B1, B2, EPS = 0.9, 0.999, 1e-8
B, L = 16, 40


def _hyper(steps, dev="cuda"):
    """The per-step scalar table with entries 1 .. steps (lr 1e-3, weight decay 0.1)."""
    from pixelrec_amd import ops

    hyper = torch.zeros(steps + 8, 4, dtype=torch.float32, device=dev)
    cumlog = torch.zeros(steps + 8, dtype=torch.float64, device=dev)
    for s in range(1, steps + 1):
        ops.adamw_hyper_append(hyper, cumlog, s, 1e-3, B1, B2, EPS, 0.1)
    return hyper, cumlog


def _aged_table(D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.randn(N_TABLE, D, device="cuda", generator=g)
    m = torch.randn(N_TABLE, D, device="cuda", generator=g) * 1e-2
    v = torch.rand(N_TABLE, D, device="cuda", generator=g) * 1e-3
    last = torch.full((N_TABLE,), T_PREV, dtype=torch.int32, device="cuda")
    return p, m, v, last


def _items():
    """[B, 2, L + 1] ids whose occurrence counts hold segments of 1, 2, 8 (the longest a group sums on its own), 9 (the first the whole
    workgroup sums) and 513 occurrences (one past a staged chunk), and id 0.  The input / target plane holds distinct ids (one
    occurrence at the ends of a sequence, two inside) and left padding; the negatives are counted once each."""
    items = (1000 + np.arange(B * (L + 1))).reshape(B, L + 1)
    items[:, :2][np.arange(B) % 3 == 0] = 0                       # left padding: id 0 as input and as target
    neg = np.zeros(B * L, dtype=np.int64)                         # the rest of the negatives: id 0
    k = 0
    for ident, cnt in ((11, 513), (12, 8), (13, 9), (14, 1), (15, 2)):
        neg[k:k + cnt] = ident
        k += cnt
    neg = np.random.default_rng(0).permutation(neg).reshape(B, L)
    out = np.zeros((B, 2, L + 1), dtype=np.int64)
    out[:, 0] = items
    out[:, 1, 1:] = neg
    return torch.from_numpy(out).cuda()


def _counts(items):
    occ = torch.cat([items[:, 0, :L].reshape(-1), items[:, 0, 1:].reshape(-1), items[:, 1, 1:].reshape(-1)])
    return torch.bincount(occ, minlength=N_TABLE)


@pytest.fixture(scope="module")
def hyper():
    return _hyper(T_PREV + 1)


def _both(D, items, hyper, seed=1, stale_row=None, n_zero=False):
    """-> (state after segsum + apply launch, state after the fused launch, the start state, the unique ids)."""
    from pixelrec_amd import ops

    hy, cumlog = hyper
    g = torch.Generator(device="cuda").manual_seed(seed)
    dx0 = torch.randn(B, L, D, device="cuda", generator=g)
    out = torch.randn(B, L, D, device="cuda", generator=g)
    coef = torch.randn(B, L, device="cuda", generator=g)
    start = _aged_table(D, seed)
    if stale_row is not None:
        start[3][stale_row] = T_PREV - 2
    cap = B * (2 * L + 1)
    ws = torch.empty(ops.occ_ws_bytes(B, L), dtype=torch.uint8, device="cuda")
    res = []
    for fused in (False, True):
        p, m, v, last = (t.clone() for t in start)
        sp = ops.SparseRows(cap, D, "cuda")
        sp.rows.fill_(float("nan"))
        ops.occ_sort(items, L, None, N_TABLE, sp, ws)
        if n_zero:
            sp.n.zero_()
        if fused:
            ops.sasrec_occ_segsum_apply(ws, dx0, out, coef, N_TABLE, sp, p, m, v, last, hy, T_PREV, B1, B2, EPS)
            assert torch.isnan(sp.rows).all()                     # the summed rows are never written
        else:
            ops.sasrec_occ_segsum(ws, dx0, out, coef, N_TABLE, sp, 1.0)
            ops.adamw_rows(p, m, v, last, hy, cumlog, T_PREV, T_PREV + 1, B1, B2, EPS, rows=sp.idx, n_rows=sp.n, max_rows=sp.cap,
                           grows=sp.rows)
        torch.cuda.synchronize()
        res.append((p, m, v, last))
        uniq = sp.idx[:sp.count()].clone()
    return res[0], res[1], start, uniq


@pytest.mark.parametrize("D", [512, 64])
def test_fused_launch_equals_segment_sums_then_apply(D, hyper):
    items = _items()
    cnt = _counts(items)
    assert {1, 2, 8, 9, 513} <= set(cnt[1:].unique().tolist()) and int(cnt[0]) > 0
    two, one, start, uniq = _both(D, items, hyper, seed=D)
    for a, b, name in zip(two, one, "pmvl"):
        assert torch.equal(a, b), name
    named = torch.zeros(N_TABLE, dtype=torch.bool, device="cuda")
    named[uniq] = True
    named[0] = False
    assert int(named.sum()) == int((cnt[1:] > 0).sum())
    assert (one[3][named] == T_PREV + 1).all() and not torch.equal(one[0][named], start[0][named])
    for a, s in zip(one, start):                                  # rows not named (row 0 among them) are untouched
        assert torch.equal(a[~named], s[~named])


def test_no_unique_rows_changes_nothing(hyper):
    two, one, start, _ = _both(64, _items(), hyper, n_zero=True)
    for a, b, s in zip(two, one, start):
        assert torch.equal(a, s) and torch.equal(b, s)


@pytest.mark.parametrize("row", [12, 11])                        # a short segment (row groups) and a long one (whole workgroup)
def test_stale_row_is_left_untouched_and_flagged(row, hyper):
    """A named row that is not current through the previous step must not be updated from stale state: the fused launch leaves it
    exactly as it was and raises the status bit (the two-launch path would replay it); every other row is updated as usual."""
    from pixelrec_amd import ops

    ops.device_status("cuda").zero_()
    two, one, start, uniq = _both(512, _items(), hyper, stale_row=row)
    assert int(ops.device_status("cuda").item()) & ops.STATUS_ROWS_STALE
    with pytest.raises(RuntimeError, match="not current"):
        ops.raise_on_bad_indices("cuda")
    assert int(ops.device_status("cuda").item()) == 0
    for a, s in zip(one, start):
        assert torch.equal(a[row], s[row])
    assert int(two[3][row]) == T_PREV + 1                         # (the reference path replayed and applied it)
    others = torch.ones(N_TABLE, dtype=torch.bool, device="cuda")
    others[row] = False
    for a, b in zip(two, one):
        assert torch.equal(a[others], b[others])


def test_current_rows_raise_no_flag(hyper):
    from pixelrec_amd import ops

    ops.device_status("cuda").zero_()
    _both(64, _items(), hyper)
    assert int(ops.device_status("cuda").item()) == 0


# ---- step level -----------------------------------------------------------------------------------------------------------------
CFG = {"n_layers": 2, "n_heads": 2, "embedding_size": 64, "inner_size": 2, "hidden_dropout_prob": 0.1, "attn_dropout_prob": 0.1,
       "hidden_act": "gelu", "layer_norm_eps": 1e-12, "initializer_range": 0.02, "MAX_ITEM_LIST_LENGTH": 8, "seed": 2020}
N_ITEMS, SB, STEPS = 1000, 4, 5


def _batches():
    from pixelrec_amd import synth

    rng = np.random.default_rng(5)
    z = synth.ZipfItems(N_ITEMS, seed=2)
    return [tuple(torch.from_numpy(a).cuda() for a in synth.train_batch(N_ITEMS, SB, 8, rng, z)) for _ in range(STEPS + 1)]


def _row_launches(step):
    """Tags of the launches one eager step records through ops.GEMM_TIMING (the hooks bench.py's roofline reads)."""
    from pixelrec_amd import ops

    ops.GEMM_TIMING = []
    try:
        step()
        torch.cuda.synchronize()
        return [tag for *_, tag in ops.GEMM_TIMING]
    finally:
        ops.GEMM_TIMING = None


def _captured(monkeypatch, knob, force=False, table_update="lazy"):
    from pixelrec_amd.graph import GraphedTrainStep
    from pixelrec_amd.model import SASRec
    from pixelrec_amd.optim import PxrAdamW
    from pixelrec_amd.parallel import DataParallel

    class DL:
        item_num = N_ITEMS

    monkeypatch.setenv("PXR_ROWS_FUSED", knob)
    torch.manual_seed(11)
    model = SASRec(CFG, DL()).cuda().train()
    dp = DataParallel(model, force_collectives=force)
    opt = PxrAdamW(model, lr=1e-3, weight_decay=0.1, table_update=table_update)
    batches = _batches()
    losses = []
    if table_update == "lazy":
        gstep = GraphedTrainStep(dp, opt, *batches[0], warmup=1)
        for b in batches[1:]:
            losses.append(float(gstep(*b)))
        step = gstep._eager
    else:                                                         # the dense sweep takes host scalars: eager steps of the same shape
        model.defer_weight_grad_join = True

        def step(b=batches[0]):
            loss = dp(b)
            loss.backward()
            opt.step()
            return loss

        for b in batches[1:]:
            losses.append(float(step(b).detach()))
    torch.cuda.synchronize()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    osd = {k: v.detach().clone() for k, v in opt.state_dict().items() if torch.is_tensor(v)}
    tags = _row_launches(step)
    return losses, sd, osd, tags


def _same(a, b):
    assert a[0] == b[0]
    for x, y in ((a[1], b[1]), (a[2], b[2])):
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k], y[k]), k


def _rows(tags):
    return [t for t in tags if t.startswith("adamw_rows_kernel")]


def test_captured_steps_are_bit_identical_with_one_row_launch_fewer(monkeypatch):
    off = _captured(monkeypatch, "0")
    on = _captured(monkeypatch, "1")
    _same(off, on)
    assert len(_rows(on[3])) == len(_rows(off[3])) - 1
    assert any("apply" in t for t in _rows(off[3])) and not any("apply" in t for t in _rows(on[3]))
    assert sum(t.startswith("segsum_apply_kernel") for t in on[3]) == 1 and not any(t.startswith("segsum_apply_kernel") for t in off[3])
    assert len(on[3]) == len(off[3])                              # (the fused launch is recorded in the row launch's place)


def test_dense_table_update_keeps_its_launches(monkeypatch):
    off = _captured(monkeypatch, "0", table_update="dense")
    on = _captured(monkeypatch, "1", table_update="dense")
    _same(off, on)
    assert on[3] == off[3] and not any(t.startswith("segsum_apply_kernel") for t in on[3])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture
def rccl_world1():
    import torch.distributed as dist

    assert not dist.is_initialized()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


def test_forced_collectives_keep_the_two_launches(rccl_world1, monkeypatch):
    """A two-rank-shaped step (the row exchange runs between the segment sums and the row update) with the knob on: two launches,
    and the bits of the one-rank step with the knob off."""
    off = _captured(monkeypatch, "0")
    on = _captured(monkeypatch, "1", force=True)
    _same(off, on)
    assert any("apply" in t for t in _rows(on[3])) and not any(t.startswith("segsum_apply_kernel") for t in on[3])


# ---- the catch-up's two ways to find its rows -----------------------------------------------------------------------------------
def test_claimed_catch_up_equals_the_listed_one_over_every_kind_of_gap():
    """Claim mode (raw ids: duplicates, id 0, an id outside the table) == list mode (sorted unique rows) on rows that lag by 0, 1, 5,
    6 (the first gap the series replay takes), 50 and 300 steps (beyond the replay window: closed-form tail), bit for bit."""
    from pixelrec_amd import ops

    t_prev, D = 320, 512
    hy, cumlog = _hyper(t_prev + 1)
    gaps = {3: 0, 40: 1, 41: 5, 700: 6, 701: 50, 1999: 300}
    p0, m0, v0, last0 = _aged_table(D, 9)
    last0.fill_(t_prev)
    for r, gp in gaps.items():
        last0[r] = t_prev - gp
    raw = torch.tensor([701, 3, 0, 40, 1999, 41, 700, 3, 701, N_TABLE + 5, 0, 1999], dtype=torch.int64, device="cuda")
    uniq = torch.tensor(sorted(gaps), dtype=torch.int64, device="cuda")
    n = torch.tensor([uniq.numel()], dtype=torch.int32, device="cuda")
    a = [t.clone() for t in (p0, m0, v0, last0)]
    b = [t.clone() for t in (p0, m0, v0, last0)]
    ops.adamw_rows_ids(*a, hy, cumlog, t_prev, B1, B2, EPS, raw)
    ops.adamw_rows(*b, hy, cumlog, t_prev, 0, B1, B2, EPS, rows=uniq, n_rows=n, max_rows=uniq.numel())
    torch.cuda.synchronize()
    for x, y, name in zip(a, b, "pmvl"):
        assert torch.equal(x, y), name
    lag = torch.tensor([r for r, gp in gaps.items() if gp], device="cuda")
    assert (a[3][lag] == t_prev).all() and not torch.equal(a[0][lag], p0[lag])
    keep = torch.ones(N_TABLE, dtype=torch.bool, device="cuda")
    keep[lag] = False
    assert torch.equal(a[0][keep], p0[keep]) and torch.equal(a[3][keep], last0[keep])
