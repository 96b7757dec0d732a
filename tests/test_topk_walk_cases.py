"""The inputs of tests/test_gpu_topk_walk.py, checked without a GPU: every case builder is deterministic, holds the users the
walk tests are about, and float64 alone -- the float64 top-K put through the comparison rule in place of a kernel's output --
excuses far fewer (user, rank) cells than the 2 % the GPU tests allow (at most half of that, and none in the 3- and 5-user cases)."""
import numpy as np
import pytest
import torch

from tests import din_restate as RD
from tests import visrank_restate as RV
from tests import widedeep_restate as RW
from tests.test_gpu_din import FUSED_MEASURED as DIN_MEASURED
from tests.test_gpu_din import _compare_topk
from tests.test_gpu_widedeep import FUSED_MEASURED as WD_MEASURED

# the bounds of tests/test_gpu_topk_walk.py (its header has the measurement): both are the models' existing ones
TOL = {"din": 4 * DIN_MEASURED, "widedeep": 4 * WD_MEASURED}
CASES = [("din", n) for n in RD.WALK_CASES] + [("widedeep", n) for n in RW.WALK_CASES]


@pytest.mark.parametrize("model_name,name", CASES)
def test_mlp_walk_case_is_deterministic_and_float64_alone_excuses_almost_nothing(model_name, name):
    R = RD if model_name == "din" else RW
    item_num, B, L, hidden, D, seed = R.WALK_CASES[name]
    P, win, hist = R.walk_case(item_num, B, L, hidden, D, seed)
    P2, win2, hist2 = R.walk_case(item_num, B, L, hidden, D, seed)
    assert all(torch.equal(P[k], P2[k]) for k in P) and torch.equal(win, win2) and hist == hist2
    s64 = R.scores64(P, win)
    tol_abs = TOL[model_name] * float(s64.abs().max())
    full, stale = R.walk_histories(s64, hist, tol_abs)
    _, masked = R.masked_topk(s64, full, 1)
    # the users
    assert int((win[0] != 0).sum()) == L and len(full[0]) == len(hist[0]) + 3                     # user 0: its float64 top-3 masked
    assert all(set(w[w != 0].tolist()) <= set(h) for w, h in zip(win, full))
    live2 = torch.nonzero(masked[2] > float("-inf")).view(-1).tolist()
    assert 0 < len(live2) < RD.WALK_K and set(live2) <= set(RD.WALK_KEEP) and min(live2) < 128 <= max(live2)
    if B > 4:
        n_real = (win != 0).sum(1)
        assert int(n_real[4]) == 0 and int(n_real[1:4].min()) >= 1
        assert B == 5 or len(set(n_real[5:].tolist())) >= min(L, 4)                                   # random pad lengths
        assert len(full[1]) > 256 and set(RD.WALK_BORDERS) <= set(full[3])
    if B >= 128:
        assert len(stale) >= 8, stale
        for u, y in stale:
            assert y >= 129 and (y - 128) in full[u] and int(torch.argmax(masked[u])) == y
    # float64 alone under the comparison rule
    real = (win != 0).any(1) if model_name == "din" else None
    for K in ((1, 10, 16, 32) if name == "short splits" else (10,)):
        top = torch.topk(masked, K, -1)
        idx = torch.where(top.values > float("-inf"), top.indices, torch.full_like(top.indices, -1))
        cells, excused = _compare_topk(idx, top.values, masked, K, tol_abs, real)
        print(f"{model_name} {name} K={K}: float64 alone excuses {excused} of {cells}; stale users {len(stale)}")
        assert excused <= (0.01 * cells if B >= 128 else 0), (excused, cells)


@pytest.mark.parametrize("name", list(RV.WALK_CASES))
def test_visrank_walk_case_is_deterministic_and_holds_its_users(name):
    B, N, F, seed = RV.WALK_CASES[name]
    v, hists = RV.walk_case(B, N, F, seed)
    v2, hists2 = RV.walk_case(B, N, F, seed)
    assert np.array_equal(v, v2) and all(np.array_equal(a, b) for a, b in zip(hists, hists2)) and len(hists) == B
    assert all(len(h) >= 1 and h.min() >= 1 and h.max() < N for h in hists)
    assert len(hists[1]) > 256 and set(range(1, N)) - set(hists[2].tolist()) == set(RV.WALK_KEEP)
    assert tuple(hists[3][:5]) == RV.WALK_BORDERS and len(set(len(h) for h in hists)) > 20
    unit = RV.unit_rows(v)
    for top_k in (0, 1, 3):
        full, stale = RV.walk_histories(v, hists, top_k, unit)
        method, top_num = RV.method_of(top_k)
        assert len(full[0]) == len(hists[0]) + 3 and np.array_equal(full[0][-RV.WALK_H:], hists[0][-RV.WALK_H:])
        print(f"visrank {name} top_k={top_k}: stale users {len(stale)}")
        assert len(stale) >= 8, stale
        for u, y in stale:
            assert y >= 129 and full[u][0] == y - 128 and np.array_equal(full[u][1:], hists[u])
            assert int(RV.topk(v, full[u], 1, method, top_num, RV.WALK_H, unit)[0][0]) == y
