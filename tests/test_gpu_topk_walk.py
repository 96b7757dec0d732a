"""The fused top-k kernels of DIN, WideDeep and VISRANK (din_topk_kernel, wd_topk_kernel, visrank_topk_kernel) on multi-tile walks:
one workgroup that walks every 128-item tile of the catalogue (n_split = 1, the regime of the shipped eval_batch_size), splits that
own fewer tiles than the others or none, the same users bit for bit in both regimes, a history item that a bitmap left over from
the previous tile would turn into a wrong mask, histories at the loop edges, the three list lengths (KT 10, 16, 32), the stated
limits of the kernels, and the user chunking of ops.din_topk.

Reference and rule: the float64 restatements (tests/din_restate.py, tests/widedeep_restate.py: predict_factorised on .double()
parameters, then masked_topk; tests/visrank_restate.py: topk on unit_rows) under the rules the models' own tests use --
_compare_topk of tests/test_gpu_din.py and tests/test_gpu_widedeep.py, _check of tests/test_gpu_visrank.py.  At most 2 % of the
(user, rank) cells of a case may be excused by the gap rule; tests/test_topk_walk_cases.py asserts on the CPU that float64 alone
stays far inside that.

Which split a case runs with is recovered from the host-only workspace queries (the candidate buffers are 2 a256(B n_split 2 KT 4)
bytes: the query at K = 32 minus the query at K = 10, over 352 B) and asserted, so a case fails, not loses its point, when the
library chooses another split.

Value tolerance, DIN and WideDeep: four times the larger of the file's FUSED_MEASURED and the largest error of the reference-form
float32 predict (the literal [B, N, L + 1] form, CPU) against the float64 restatement over the inputs of this module, relative to
the largest |score| of the case (python tools/measure_topk_walk.py):
    DIN       2.325e-7 (case "limits": D 128, hidden (128, 128), L 64, B 3, item_num 257)   < FUSED_MEASURED 2.284e-6 -> 9.14e-6
    WideDeep  2.578e-7 (case "short splits": D 16, hidden (12, 4), L 10, B 128, item_num 600) < FUSED_MEASURED 4.417e-7 -> 1.767e-6
so both bounds are the existing ones.  VISRANK: R.tol(F), derived."""
import math
from types import SimpleNamespace

import pytest
import torch

from pixelrec_amd import lib as _l
from pixelrec_amd import ops
from tests import din_restate as RD
from tests import test_gpu_din as TD
from tests import test_gpu_visrank as TV
from tests import test_gpu_widedeep as TW
from tests import visrank_restate as RV
from tests import widedeep_restate as RW

pytestmark = pytest.mark.gpu
DIN_WALK_MEASURED, WD_WALK_MEASURED = 2.325e-7, 2.578e-7
DIN_TOL = 4 * max(DIN_WALK_MEASURED, TD.FUSED_MEASURED)
WD_TOL = 4 * max(WD_WALK_MEASURED, TW.FUSED_MEASURED)
K = RD.WALK_K
# case -> (n_split, per = ceil(tiles / n_split)) under n_split = min(ceil(512 / B), tiles)
DIN_SPLITS = {"one split, small": (1, 3), "one split, shipped": (1, 3), "short splits": (4, 2), "short splits, one layer": (4, 2),
              "limits": (3, 1), "hidden 5": (3, 1), "hidden 127 33": (3, 1), "hidden 1": (3, 1), "chunks": (3, 1)}
WD_SPLITS = {"one split, small": (1, 3), "one split, shipped": (1, 3), "one split, one layer": (1, 3), "short splits": (4, 2),
             "limits": (3, 1), "hidden 4": (3, 1)}
VR_SPLITS = {"one split": (1, 3), "short splits": (4, 2), "short splits, odd batch": (4, 2)}
DIN_WALKS = ["one split, small", "one split, shipped", "short splits", "short splits, one layer"]      # the multi-tile cases
WD_WALKS = ["one split, small", "one split, shipped", "one split, one layer", "short splits"]


def _split_of(query, B, N):
    """(n_split, per) recovered from a workspace query K -> bytes."""
    n_split = round((int(query(32)) - int(query(10))) / (352 * B))
    return n_split, math.ceil(math.ceil(N / 128) / n_split)


def _din_split(B, N, L, D, hidden):
    h1, h2 = hidden[0], (hidden[1] if len(hidden) == 2 else 0)
    return _split_of(lambda k: _l.load().pxr_din_topk_ws_bytes(B, L, N, D, h1, h2, k), B, N)


def _wd_split(B, N, L, hidden):
    h1, h2 = hidden[0], (hidden[1] if len(hidden) == 2 else 0)
    return _split_of(lambda k: _l.load().pxr_wd_topk_ws_bytes(B, L, N, h1, h2, k), B, N)


def _vr_split(B, N):
    return _split_of(lambda k: _l.load().pxr_visrank_topk_ws_bytes(B, RV.WALK_H, N, k), B, N)


def _ids_are_live(idx, masked):
    """No masked item, no item 0 and no id >= N: every returned id is -1 or an item whose masked float64 score is finite."""
    N = masked.shape[1]
    assert int(idx.max()) < N and int(idx.min()) >= -1
    got = masked.gather(1, idx.clamp(min=0))
    assert bool(((idx == -1) | (got > float("-inf"))).all())
    assert bool((idx != 0).all())


# ------------------------------------------------------------------------------------------------------------ DIN and WideDeep
class _MlpCases:
    """The cases of one model, each built once (float64 reference on the device) and shared by the tests of this module."""

    def __init__(self, R, T, tol):
        self.R, self.T, self.tol, self.built = R, T, tol, {}

    def get(self, name):
        if name not in self.built:
            R = self.R
            item_num, B, L, hidden, D, seed = R.WALK_CASES[name]
            P, win, hist = R.walk_case(item_num, B, L, hidden, D, seed)
            s64 = R.scores64(P, win, device="cuda")
            tol_abs = self.tol * float(s64.abs().max())
            hist, stale = R.walk_histories(s64, hist, tol_abs)
            _, masked = R.masked_topk(s64, hist, 1)
            c = SimpleNamespace(name=name, item_num=item_num, B=B, L=L, hidden=list(hidden), D=D, P=P, win=win, hist=hist, stale=stale,
                                masked=masked, tol_abs=tol_abs, real=(win != 0).any(1), runs={}, model=None)
            if all(h % 4 == 0 for h in hidden):                                     # (the models take multiples of 4 only)
                c.model = self.T._model(item_num, D, c.hidden, L=L, sd=P).eval()
                assert c.model.fused_topk_supported
            self.built[name] = c
        return self.built[name]


DIN_CASES, WD_CASES = _MlpCases(RD, TD, DIN_TOL), _MlpCases(RW, TW, WD_TOL)   # also read by tests/test_gpu_topk_bits.py: one build


@pytest.fixture(scope="module")
def din_cases():
    return DIN_CASES


@pytest.fixture(scope="module")
def wd_cases():
    return WD_CASES


def _din_operands(c):
    """The operands of ops.din_topk from the state itself, for hidden widths the model does not take: A, Bm, C by the library's
    fold, A q + b1 in float64 rounded once."""
    P = {k: v.cuda() for k, v in c.P.items()}
    keys = RD.names(len(c.hidden))
    A, Bm, C = ops.din_fold_w1(P[keys[0]].contiguous(), c.D)
    aq = (P[RD.TABLE].double() @ A.double().T + P[keys[1]].double()).float().contiguous()
    two = len(c.hidden) == 2
    return (P[RD.TABLE].contiguous(), aq, Bm, C, P[keys[2]].contiguous() if two else None, P[keys[3]].contiguous() if two else None,
            P["attention.dense.weight"].view(-1).contiguous(), P["attention.dense.bias"].contiguous())


def _fused(model_name, c, k, users=None):
    """One fused call on the case's users (or its first `users`), status word checked -> (ids, values) on the host."""
    n = c.B if users is None else users
    T = TD if model_name == "din" else TW
    ptr, items = T._csr(c.hist[:n], n)
    win = c.win[:n].contiguous().cuda()
    if c.model is not None:
        idx, val = c.model.fused_topk(win, ptr, items, k)
    else:
        table, aq, Bm, C, w2, b2, wd, bd = _din_operands(c)
        idx, val = ops.din_topk(table, win, aq, Bm, C, w2, b2, wd, bd, k, ptr, items)
    torch.cuda.synchronize()
    ops.raise_on_bad_indices()
    return idx.cpu(), val.cpu()


def _run(model_name, c, k):
    if k not in c.runs:
        c.runs[k] = _fused(model_name, c, k)
    return c.runs[k]


def _compare(model_name, c, k):
    idx, val = _run(model_name, c, k)
    assert tuple(idx.shape) == (c.B, k) and tuple(val.shape) == (c.B, k)
    _ids_are_live(idx, c.masked)
    live = val > float("-inf")
    ref = torch.topk(c.masked, min(k, c.item_num), -1).values[:, :k]
    err = float((val.double() - ref)[live].abs().max())
    print(f"{model_name} {c.name} K={k}: value error {err:.3e} (bound {c.tol_abs:.3e})")
    if model_name == "din":
        cells, excused = TD._compare_topk(idx, val.double(), c.masked, k, c.tol_abs, c.real)
    else:
        cells, excused = TW._compare_topk(idx, val.double(), c.masked, k, c.tol_abs)
    print(f"{model_name} {c.name} K={k}: excused {excused} of {cells}")
    assert excused <= 0.02 * cells, (excused, cells)
    return idx, val


def _walk_properties(c, idx, val, k):
    """What the case was built for besides the stale-bitmap users (test_a_stale_bitmap_would_show): the long history, the user with
    fewer than K items, the tile borders, the all-padding window (user 0's masked float64 top-3 is part of the comparison itself)."""
    assert len(c.hist[1]) > 256
    live2 = int((c.masked[2] > float("-inf")).sum())
    assert 0 < live2 < k and int((idx[2] >= 0).sum()) == live2 and bool(torch.isneginf(val[2, live2:]).all())
    kept = idx[2, :live2].tolist()
    assert min(kept) < 128 <= max(kept)                     # ... spread over two tiles
    assert set(RD.WALK_BORDERS) <= set(c.hist[3]) and not set(RD.WALK_BORDERS) & set(idx[3].tolist())
    assert not bool(c.real[4]) and bool(c.real[:4].all())


@pytest.mark.parametrize("name", DIN_WALKS)
def test_din_walk_matches_float64(din_cases, name):
    """Cases 1, 2, 4, 5 for din_topk_kernel: B 512 x N 300 runs n_split 1 / per 3 (the last tile holds 44 items), B 128 x N 600
    n_split 4 / per 2 (the splits own 2, 2, 1 and 0 tiles), with two hidden layers and with one."""
    c = din_cases.get(name)
    assert _din_split(c.B, c.item_num, c.L, c.D, c.hidden) == DIN_SPLITS[name]
    idx, val = _compare("din", c, K)
    _walk_properties(c, idx, val, K)
    assert bool((val[4] == 0).all())                        # the all-padding window scores exactly 0 everywhere


@pytest.mark.parametrize("name", WD_WALKS)
def test_widedeep_walk_matches_float64(wd_cases, name):
    """Cases 1, 2, 4, 5 for wd_topk_kernel, as for DIN.  The all-padding window (user 4) reads row 0 of both tables like the
    reference and is ranked like any other user."""
    c = wd_cases.get(name)
    assert _wd_split(c.B, c.item_num, c.L, c.hidden) == WD_SPLITS[name]
    idx, val = _compare("widedeep", c, K)
    _walk_properties(c, idx, val, K)
    assert int((idx[4] >= 0).sum()) == K


@pytest.mark.parametrize("model_name,name", [("din", n) for n in DIN_WALKS] + [("widedeep", n) for n in WD_WALKS])
def test_a_stale_bitmap_would_show(din_cases, wd_cases, model_name, name):
    """Case 4: for the users of c.stale the float64 best unmasked item y is >= 129, clear of ranks 2 and 3 by twice the tolerance,
    and y - 128 -- the same bit of the history bitmap, one tile earlier -- is in the history.  A bitmap that is not cleared
    between tiles masks y; it must come back at rank 1."""
    c = (din_cases if model_name == "din" else wd_cases).get(name)
    idx, _ = _run(model_name, c, K)
    assert len(c.stale) >= 8, c.stale
    for u, y in c.stale:
        assert y >= 129 and (y - 128) in c.hist[u] and y not in c.hist[u]
    lost = [(u, y, int(idx[u, 0])) for u, y in c.stale if int(idx[u, 0]) != y]
    assert not lost, lost


@pytest.mark.parametrize("k", [1, 16, 32])
@pytest.mark.parametrize("model_name", ["din", "widedeep"])
def test_list_lengths_on_short_splits(din_cases, wd_cases, model_name, k):
    """Case 6: K 1, 16, 32 (the KT 10, 16 and 32 instantiations) on B 128 x N 600; at K 32 user 2 keeps fewer
    than 32 items: the tail is (-inf, -1)."""
    c = (din_cases if model_name == "din" else wd_cases).get("short splits")
    idx, val = _compare(model_name, c, k)
    live2 = int((c.masked[2] > float("-inf")).sum())
    if k == 32:
        assert 0 < live2 < k and bool((idx[2, live2:] == -1).all()) and bool(torch.isneginf(val[2, live2:]).all())
    for u, y in c.stale:
        assert int(idx[u, 0]) == y, (u, y)


def _same_ids_where_distinct(top, idx_a, idx_f):
    """ids equal for the users whose float32 top-(K + 1) values `top` are pairwise distinct (at least two of the three)."""
    checked = 0
    for u in range(3):
        v = top[u][top[u] > float("-inf")]
        if len(set(v.tolist())) == len(v):
            assert torch.equal(idx_a[u], idx_f[u]), (u, idx_a[u], idx_f[u])
            checked += 1
    assert checked >= 2


def _same_bits(model_name, c, split_alone, split_full):
    """Case 3: users 0..2 alone (one tile per workgroup) and as the first three of the full batch (one workgroup walks every
    tile).  An item's score does not depend on which workgroup computes it: values bit-identical, ids equal for the users whose
    float32 top-(K + 1) values are pairwise distinct.  No tolerance."""
    assert split_full == (1, 3) and split_alone == (3, 1)
    idx_f, val_f = _run(model_name, c, K)
    idx_a, val_a = _fused(model_name, c, K, users=3)
    assert torch.equal(val_a.view(torch.int32), val_f[:3].view(torch.int32))
    top = _fused(model_name, c, K + 1, users=3)[1]
    _same_ids_where_distinct(top, idx_a, idx_f)


@pytest.mark.parametrize("name", ["one split, small", "one split, shipped"])
def test_din_same_users_bit_for_bit_in_both_regimes(din_cases, name):
    c = din_cases.get(name)
    _same_bits("din", c, _din_split(3, c.item_num, c.L, c.D, c.hidden), _din_split(c.B, c.item_num, c.L, c.D, c.hidden))


@pytest.mark.parametrize("name", ["one split, small", "one split, shipped", "one split, one layer"])
def test_widedeep_same_users_bit_for_bit_in_both_regimes(wd_cases, name):
    """The window term h_b is a library GEMM over the batch, whose schedule may follow the batch size: both calls take their rows
    from the one h_b of the full batch, so the comparison is of wd_topk_kernel alone."""
    c = wd_cases.get(name)
    assert _wd_split(3, c.item_num, c.L, c.hidden) == (3, 1) and _wd_split(c.B, c.item_num, c.L, c.hidden) == (1, 3)
    m = c.model
    win = c.win.cuda()
    hb = m._window_term(win)
    two = len(c.hidden) == 2
    out = {}
    for n, k in ((c.B, K), (3, K), (3, K + 1)):
        ptr, items = TW._csr(c.hist[:n], n)
        idx, val = ops.wd_topk(m._eval_T(), hb[:n].contiguous(), win[:n].contiguous(), m._p("wide.w").view(-1), m._p("wide.b"),
                               m._p("l1.w") if two else None, m._p("l1.b") if two else None, m._p("pred.w").view(-1), m._p("pred.b"),
                               k, ptr, items)
        torch.cuda.synchronize()
        ops.raise_on_bad_indices()
        out[(n, k)] = (idx.cpu(), val.cpu())
    (idx_f, val_f), (idx_a, val_a), top = out[(c.B, K)], out[(3, K)], out[(3, K + 1)][1]
    assert torch.equal(val_f.view(torch.int32), _run("widedeep", c, K)[1].view(torch.int32))    # the model's own call: the same bits
    assert torch.equal(val_a.view(torch.int32), val_f[:3].view(torch.int32))
    _same_ids_where_distinct(top, idx_a, idx_f)


@pytest.mark.parametrize("name", ["limits", "hidden 5", "hidden 127 33", "hidden 1"])
def test_din_limits_and_odd_hidden_widths(din_cases, name):
    """Case 7 for DIN: D 128, hidden (128, 128), L 64 through the model; hidden (5,), (127, 33) and (1,) -- no multiple of 4 or 8:
    the second layer's k loop reads past h1 and relies on zero padding -- through ops.din_topk on operands made from the state."""
    c = din_cases.get(name)
    assert _din_split(c.B, c.item_num, c.L, c.D, c.hidden) == DIN_SPLITS[name]
    assert ops.din_topk_supported(c.D, c.hidden, c.L, K)
    idx, val = _compare("din", c, K)
    live2 = int((c.masked[2] > float("-inf")).sum())
    assert 0 < live2 < K and int((idx[2] >= 0).sum()) == live2


@pytest.mark.parametrize("name", ["limits", "hidden 4"])
def test_widedeep_limits(wd_cases, name):
    """Case 7 for WideDeep: hidden (128, 128) and (4,) at L 64."""
    c = wd_cases.get(name)
    assert _wd_split(c.B, c.item_num, c.L, c.hidden) == WD_SPLITS[name]
    assert ops.wd_topk_supported(c.hidden, c.L, K)
    idx, val = _compare("widedeep", c, K)
    live2 = int((c.masked[2] > float("-inf")).sum())
    assert 0 < live2 < K and int((idx[2] >= 0).sum()) == live2


def test_one_step_past_each_limit_is_not_supported():
    assert ops.din_topk_supported(128, [128, 128], 64, 32)
    for D, hidden, L, k in ((132, [128, 128], 64, 32), (128, [129, 128], 64, 32), (128, [132], 64, 32), (128, [128, 129], 64, 32),
                            (128, [128, 128], 65, 32), (128, [128, 128], 64, 33), (128, [16, 8, 4], 64, 32)):
        assert ops.din_topk_supported(D, hidden, L, k) is False, (D, hidden, L, k)
    assert TD._model(300, 132, [128, 128], L=64).fused_topk_supported is False
    assert TD._model(300, 128, [128, 128], L=65).fused_topk_supported is False
    assert ops.wd_topk_supported([128, 128], 64, 32)
    for hidden, L, k in (([132, 128], 64, 32), ([128, 132], 64, 32), ([128, 129], 64, 32), ([128, 128], 65, 32), ([128, 128], 64, 33),
                         ([16, 8, 4], 64, 32)):
        assert ops.wd_topk_supported(hidden, L, k) is False, (hidden, L, k)
    assert TW._model(300, 8, [128, 128], L=65).fused_topk_supported is False
    assert TW._model(300, 8, [132], L=64).fused_topk_supported is False


def test_din_user_chunks_equal_the_unchunked_call(din_cases, monkeypatch):
    """Case 8: ops.DIN_WS_CAP set so that B 5 goes out as chunks of 2, 2 and 1 users; each chunk's hist_ptr slice keeps absolute
    offsets, so a wrong slice masks another user's items.  Values bit for bit, ids as well for the users with a real window."""
    c = din_cases.get("chunks")
    assert c.B == 5 and all(len(h) for h in c.hist)
    assert _din_split(c.B, c.item_num, c.L, c.D, c.hidden) == DIN_SPLITS["chunks"]
    idx, val = _compare("din", c, K)
    asked = []
    get = ops._ws.get
    monkeypatch.setattr(ops._ws, "get", lambda nbytes, device: (asked.append(nbytes), get(nbytes, device))[1])
    monkeypatch.setattr(ops, "DIN_WS_CAP", 2 * c.L * (c.hidden[0] * c.D + 128) * 4)
    idx2, val2 = _fused("din", c, K)
    monkeypatch.undo()
    assert len(asked) == 3, asked                           # three launches: users 0-1, 2-3, 4
    assert torch.equal(val2.view(torch.int32), val.view(torch.int32))
    assert torch.equal(idx2[c.real], idx[c.real])
    TD._compare_topk(idx2, val2.double(), c.masked, K, c.tol_abs, c.real)


# ------------------------------------------------------------------------------------------------------------ VISRANK
class _VrCases:
    def __init__(self):
        self.built = {}

    def get(self, name, top_k):
        if (name, top_k) not in self.built:
            if name not in self.built:
                B, N, F, seed = RV.WALK_CASES[name]
                v, hists = RV.walk_case(B, N, F, seed)
                self.built[name] = (v, hists, RV.unit_rows(v), ops.visrank_unit_rows(torch.from_numpy(v).cuda()))
            v, hists, unit64, unit = self.built[name]
            hists, stale = RV.walk_histories(v, hists, top_k, unit64)
            self.built[(name, top_k)] = SimpleNamespace(name=name, B=len(hists), N=v.shape[0], F=v.shape[1], v=v, hists=hists,
                                                        stale=stale, unit64=unit64, unit=unit, top_k=top_k)
        return self.built[(name, top_k)]


VR_CASES = _VrCases()


@pytest.fixture(scope="module")
def vr_cases():
    return VR_CASES


def _vr_fused(c, k, users=None):
    hists = c.hists if users is None else c.hists[:users]
    win, ptr, items = TV._batch(hists, RV.WALK_H)
    idx, val = ops.visrank_topk(c.unit, win, c.top_k, k, ptr, items)
    torch.cuda.synchronize()
    ops.raise_on_bad_indices()
    return idx, val


@pytest.mark.parametrize("name,top_k", [("one split", 1), ("one split", 3), ("short splits", 0), ("short splits", 1),
                                        ("short splits, odd batch", 1), ("short splits, odd batch", 0)])
def test_visrank_walk_matches_float64(vr_cases, name, top_k):
    """Cases 1, 2, 4, 5 for visrank_topk_kernel under the threshold rule (_check, tol(F)): B 1024 x N 300 runs n_split 1 / per 3,
    B 256 and B 255 x N 600 n_split 4 / per 2 (the splits own 2, 2, 1 and 0 tiles); at B 255 the last 2-user row block holds one
    user.  The reductions 0 (mean) and 1 (maximum) on the short splits."""
    c = vr_cases.get(name, top_k)
    assert _vr_split(c.B, c.N) == VR_SPLITS[name]
    idx, val = _vr_fused(c, K)
    TV._check(c.v, c.hists, RV.WALK_H, top_k, K, idx, val, c.unit64)
    idx = idx.cpu()
    assert len(c.stale) >= 8, c.stale
    for u, y in c.stale:
        assert (y - 128) in c.hists[u] and int(idx[u, 0]) == y, (u, y, idx[u].tolist())
    assert len(c.hists[1]) > 256
    assert sorted(idx[2, :len(RV.WALK_KEEP)].tolist()) == sorted(RV.WALK_KEEP) and bool((idx[2, len(RV.WALK_KEEP):] == -1).all())
    assert not set(RV.WALK_BORDERS) & set(idx[3].tolist())


def test_visrank_same_users_bit_for_bit_in_both_regimes(vr_cases):
    """Case 3 for VISRANK: users 0..2 alone (two row blocks, one tile per workgroup) and as the first three of B 1024."""
    c = vr_cases.get("one split", 1)
    assert _vr_split(3, c.N) == (3, 1) and _vr_split(c.B, c.N) == (1, 3)
    idx_f, val_f = (t.cpu() for t in _vr_fused(c, K))
    idx_a, val_a = (t.cpu() for t in _vr_fused(c, K, users=3))
    assert torch.equal(val_a.view(torch.int32), val_f[:3].view(torch.int32))
    top = _vr_fused(c, K + 1, users=3)[1].cpu()
    _same_ids_where_distinct(top, idx_a, idx_f)
