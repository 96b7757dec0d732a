"""The occurrence sort in front of the segment sums (csrc/occ_sort.cuh: sort_occurrences) across pass counts, on both sorts: the two
(keys, vals) buffer pairs of the workspace swap once per radix pass, phase 2 and the dense sink find the sorted order -- and the
spare pair -- from the PREDICTED pass count (final_vals_buffer), and the pass count differs between the fused sort (digits of up to
10 bits, n <= FP_MAX_N) and the multi-launch sort (8-bit digits):

    n_table        200   1000   2^17 + 1   2^21
    radix passes     1      2          3      3
    fused passes     1      1          2      3

Every table runs on both sides of the cut-over, through the three entry families and both sinks.  n = FP_MAX_N and FP_MAX_N + 1
for the plain and the pooled occurrences; the sequence form has n = 3 B L, and neither 2^16 nor the prime 2^16 + 1 is a multiple of
3, so it takes the nearest n on either side, 65 535 and 65 538.  D = 4; the ids hold 0, negatives, ids >= n_table, the last row of
the table and one id repeated more than SEG_CHUNK times; rows and coefficients are small integers (as in tests/segsum_cases.py), so
every sum is an integer below 2^24 and every comparison is an equality: uniq_idx[:n_uniq] is the sorted set of valid ids, the rows
are an int64 index_add_, the dense block is those rows scattered over zeros, and the bad-index bit is set exactly by the sequence
form fed an id outside the table."""
import numpy as np
import pytest
import torch

from tests.mo_common import sort_constants

pytestmark = pytest.mark.gpu

D = 4
STATUS_BAD_INDEX = 1                # PXR_STATUS_BAD_INDEX (csrc/pxr_common.h)
FP_MAX_N, _, SEG_CHUNK = sort_constants()
N_TABLES = [200, 1000, 2 ** 17 + 1, 2 ** 21]
SIDES = ["fused", "multi"]          # n <= FP_MAX_N | n > FP_MAX_N


def _ids(n, n_table, seed, bad=True):
    """n ids: uniform over the table (bad: and an eighth of its width on either side of it), then the fixed entries."""
    rng = np.random.default_rng(seed)
    m = n_table // 8 if bad else 0
    ids = rng.integers(-m, n_table + m, size=n)
    if not bad:
        ids[ids == 0] = 1
    rep = n_table // 2 + 1
    ids[8:8 + SEG_CHUNK + 3] = rep                                  # one segment longer than a chunk
    ids[:5] = [0, 7, n_table - 1, 3, rep] if not bad else [0, -1, n_table - 1, n_table, n_table + 5]
    return torch.from_numpy(ids).cuda()


def _ints(shape, seed, lo=-4, hi=5):
    return torch.from_numpy(np.random.default_rng(seed).integers(lo, hi, size=shape)).cuda()


def _expect(occ_ids, contrib, n_table):
    """(sorted unique valid ids, their int64 row sums as float32) of occurrence ids [n] and integer contributions [n, D]."""
    valid = (occ_ids > 0) & (occ_ids < n_table)
    uniq, inv = torch.unique(occ_ids[valid], return_inverse=True)
    sums = torch.zeros(uniq.numel(), D, dtype=torch.int64, device="cuda").index_add_(0, inv, contrib[valid])
    assert int(sums.abs().max()) < 2 ** 24
    return uniq, sums.float()


def _check(sp, dense, uniq, rows, n_table, status):
    from pixelrec_amd import ops

    k = sp.count()
    assert k == uniq.numel() and torch.equal(sp.idx[:k], uniq)
    assert torch.equal(sp.rows[:k], rows)
    want = torch.zeros(n_table, D, device="cuda")
    want[uniq] = rows
    assert torch.equal(dense, want)
    assert int(ops.device_status("cuda").item()) == status


def _factor(n, least):
    """(n // d, d) for the smallest divisor d >= least of n."""
    d = next(d for d in range(least, n + 1) if n % d == 0)
    return n // d, d


@pytest.fixture(autouse=True)
def _clean_status():
    from pixelrec_amd import ops

    ops.device_status("cuda").zero_()
    yield
    ops.device_status("cuda").zero_()


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("n_table", N_TABLES)
def test_rows_sort_parity(n_table, side):
    from pixelrec_amd import ops

    n = FP_MAX_N + (side == "multi")
    idx = _ids(n, n_table, seed=n_table + n)
    rows = _ints((n, D), 1)
    uniq, want = _expect(idx, rows, n_table)
    sp = ops.embed_grad_rows(idx, rows.float(), n_table)
    dense = ops.embed_grad_dense(idx, rows.float(), n_table, out=torch.full((n_table, D), float("nan"), device="cuda"))
    _check(sp, dense, uniq, want, n_table, 0)                       # the plain keys drop a bad id without a flag


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("n_table", N_TABLES)
def test_pool_sort_parity(n_table, side):
    """n = B (L + 2): FP_MAX_N = 16 384 * 4; FP_MAX_N + 1 is prime, so B = 1 with a history of FP_MAX_N - 1 positions."""
    from pixelrec_amd import ops

    n = FP_MAX_N + (side == "multi")
    B, L2 = _factor(n, 3)
    L = L2 - 2
    gidx = _ids(n, n_table, seed=n_table + n + 1)
    G, w = _ints((3 * B, D), 2), _ints((B,), 3, 1, 3)
    o = torch.arange(n, device="cuda")
    hist = o < B * L
    b = torch.where(hist, o // L, torch.zeros_like(o))
    contrib = torch.where(hist[:, None], w[b][:, None] * G[b], G[torch.where(hist, torch.zeros_like(o), B + o - B * L)])
    uniq, want = _expect(gidx, contrib, n_table)
    sp = ops.pool_table_grad(gidx, B, L, G.float(), w.float(), n_table)
    dense = ops.pool_dense_grad(gidx, B, L, G.float(), w.float(), n_table, out=torch.full((n_table, D), float("nan"), device="cuda"))
    _check(sp, dense, uniq, want, n_table, 0)


@pytest.mark.parametrize("layout", ["sasrec", "bert4rec"])
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("n_table", N_TABLES)
def test_sequence_sort_parity(n_table, side, layout):
    """pxr_seq_occ_sort + pxr_sasrec_occ_segsum and pxr_seq_occ_dense_f32 in SASRec's shifted windows and BERT4Rec's planes, with
    and without ids outside the table: the bad-index bit is set with them and clear without."""
    from pixelrec_amd import ops

    n = FP_MAX_N // 3 * 3 if side == "fused" else (FP_MAX_N // 3 + 1) * 3
    assert (n <= FP_MAX_N) == (side == "fused") and abs(n - FP_MAX_N) <= 2
    B, L = _factor(n // 3, 2)
    dx0, out, coef = _ints((B, L, D), 4), _ints((B, L, D), 5), _ints((B, L), 6, -2, 3)
    ws = torch.empty(ops.occ_ws_bytes(B, L), dtype=torch.uint8, device="cuda")
    for bad in (False, True):
        ids = _ids(n, n_table, seed=n_table + n + 2, bad=bad).view(3, B, L)     # input | target | negative of (b, t)
        if layout == "sasrec":                                       # items[b, 0, t] | items[b, 0, t + 1] | items[b, 1, t + 1]
            ids[1, :, :-1] = ids[0, :, 1:]                           # the target of t is the input of t + 1
            items = torch.ones(B, 2, L + 1, dtype=torch.int64, device="cuda")
            items[:, 0, :L], items[:, 0, L], items[:, 1, 1:] = ids[0], ids[1, :, -1], ids[2]
            lay = None
        else:
            items = ids.permute(1, 0, 2).contiguous()                # [B, 3, L]
            lay = (3 * L, 0, L, 2 * L)
        co = (coef[:, :, None] * out).view(-1, D)
        uniq, want = _expect(ids.reshape(-1), torch.cat([dx0.view(-1, D), co, -co]), n_table)
        ops.device_status("cuda").zero_()
        sp = ops.SparseRows(n, D, "cuda")
        ops.occ_sort(items, L, lay, n_table, sp, ws)
        ops.sasrec_occ_segsum(ws, dx0.float(), out.float(), coef.float(), n_table, sp)
        dense = ops.seq_occ_dense_grad(items, lay, dx0.float(), out.float(), coef.float(), n_table,
                                       d_rows=torch.full((n_table, D), float("nan"), device="cuda"))
        _check(sp, dense, uniq, want, n_table, STATUS_BAD_INDEX if bad else 0)
