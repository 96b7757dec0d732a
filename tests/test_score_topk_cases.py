"""The inputs of tests/test_gpu_score_topk_ref.py, checked without a GPU: every case of tests/score_topk_restate.py is
deterministic, its histories decide outputs (hot block, masked float64 top items, more than ST4_HIST_CAP pairs in one workgroup's
range), the sample pass keeps K unmasked items per user, the restated candidate counts stay inside the buffer, and float64 alone --
the float64 top-K put through the comparison rule in place of a kernel's output -- excuses at most 2 % of the (user, rank) cells,
half of what the GPU tests allow."""
import pytest
import torch

from tests import score_topk_restate as R
from tests.test_gpu_din import _compare_topk


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()                                # one case at a time: "wide" alone holds 0.8 GB
            cache[name] = R.case(name)
        return cache[name]

    yield get
    cache.clear()


@pytest.mark.parametrize("name", R.CASES)
def test_case_is_deterministic(name, built):
    a, b = built(name), R.case(name)
    assert torch.equal(a.users, b.users) and torch.equal(a.table, b.table) and a.hist == b.hist and torch.equal(a.s64, b.s64)
    assert a.users.stride(0) == a.ld_users and a.users.shape == (a.B, a.D) and a.s64.shape == (a.B, a.N)
    assert a.N >= R.MIN_N and all(0 <= i < a.N for h in a.hist for i in h)
    if name == "strided":
        r = R.case("ragged")
        assert a.ld_users == 2 * a.D and torch.equal(a.users, r.users[:a.B]) and torch.equal(a.s64, r.s64[:a.B])
    if name == "one_user":
        assert a.B == 1


@pytest.mark.parametrize("name", [n for n in R.CASES if n != "crowd"])
def test_float64_alone_excuses_at_most_two_percent(name, built):
    c = built(name)
    tol = R.tol_abs(c.s64, c.D)
    top = torch.topk(c.s64, c.K, -1)
    assert bool((top.values > float("-inf")).all())
    cells, excused = _compare_topk(top.indices, top.values, c.s64, c.K, tol)
    print(f"{name}: float64 alone excuses {excused} of {cells} cells; tol_abs {tol:.3e}")
    assert cells == c.B * c.K and excused <= 0.02 * cells, (excused, cells)


@pytest.mark.parametrize("name", [n for n in R.CASES if n != "crowd"])
def test_histories_decide_outputs(name, built):
    c = built(name)
    top = torch.topk(c.s64, c.K, -1).indices
    hot = int(((top >= 1) & (top <= R.HOT)).sum())
    print(f"{name}: {hot} of {top.numel()} top-K cells lie in the hot block")
    assert hot >= 0.10 * top.numel()
    # every even user's masked top items would be in its top-K were they not masked
    raw = c.users.double() @ c.table.double().t()
    raw[:, 0] = float("-inf")
    unmasked = torch.topk(raw, c.K, -1).indices
    for u in range(c.B):
        want = min(c.K, 1 + u % 5) if u % 2 == 0 else 0
        assert len(c.own_top[u]) == want
        assert set(c.own_top[u]) <= set(unmasked[u].tolist()) and set(c.own_top[u]) <= set(c.hist[u])
        assert all(c.s64[u, i] == float("-inf") for i in c.hist[u]) and not set(top[u].tolist()) & set(c.hist[u])
    # users 0-63: more pairs in the first workgroup's item range than its LDS list holds ("wide" and "one_user" have 5 users and
    # 1 user: their workgroups keep the LDS list)
    if c.B >= R.HOT_USERS:
        pairs = sum(1 for h in c.hist[:R.HOT_USERS] for i in h if 1 <= i <= R.HOT)
        assert pairs > R.HIST_CAP, pairs
    if c.B > 3:
        assert 0 in c.hist[2] and max(c.hist[2].count(i) for i in c.hist[2]) == 3
        assert set(R.border_items(c.N)) <= set(c.hist[3])


@pytest.mark.parametrize("name", R.CASES)
def test_sample_pass_keeps_k_items_and_the_candidates_fit(name, built):
    c = built(name)
    tiles = R.sampled_tiles(c.N, c.K)
    n_tiles = (c.N + R.TILE - 1) // R.TILE
    assert tiles[0] == 0 and tiles[-1] < n_tiles and len(tiles) == -(-n_tiles // (32 if c.K > 16 else 64))
    live = (c.s64[:, R.sample_columns(c.N, c.K)] > float("-inf")).sum(1)
    assert int(live.min()) >= c.K, int(live.min())
    for products in (6, 3, 1):
        n = R.survivors(c, products)
        print(f"{name}: products {products}: {int(n.min())} .. {int(n.max())} candidates per user")
        assert int(n.min()) >= c.K
        if name != "crowd":
            assert int(n.max()) < R.CAND_CAP, (products, int(n.max()))
        else:
            # more than topk_rescore_kernel keeps in registers, fewer than the buffer holds -- on every user
            assert R.RESCORE_INREG < int(n.min()) and int(n.max()) < R.CAND_CAP, (products, int(n.min()), int(n.max()))


def test_crowd_ties_are_the_duplicates(built):
    c = built("crowd")
    dup, masked = set(c.crowd), set(c.hist[0])
    assert len(dup) == R.CROWD_DUP and len(masked) == R.CROWD_MASKED and masked == set(sorted(dup)[:R.CROWD_MASKED])
    top = torch.topk(c.s64, c.K, -1)
    assert all(set(row.tolist()) <= dup for row in top.indices) and not set(top.indices[0].tolist()) & masked
    # the duplicates outscore every other item by far more than the tolerance: ids can only differ among them
    others = c.s64.clone()
    others[:, torch.tensor(sorted(dup))] = float("-inf")
    assert float((top.values[:, -1] - others.max(1).values).min()) > 100 * R.tol_abs(c.s64, c.D)
