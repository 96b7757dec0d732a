"""VISRANK on the gfx950 kernels (csrc/visrank.hip): the fused cosine top-k against the float64 restatement -- exact ids where the
float64 gaps allow it, the threshold rule everywhere -- at the shipped width and at the edges of the kernel's shape, the literal
predict against the same rule and against the reference's golden fixture, bad ids, and main.py end to end.  Every test here needs
the model or its kernels, so each fails without the feature.

Threshold rule (every user of every case): the returned ids are distinct and none is masked; for each rank r,
s64[id_r] >= sorted_s64[r] - tol(F) and |val_r - s64[id_r]| <= tol(F), tol(F) = 2 (F + 8) 2^-24 (tests/visrank_restate.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pixelrec_amd import lib as _l
from pixelrec_amd import ops
from tests import visrank_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "visrank_tiny.npz")


def _method(top_k):
    return ("mean", None) if top_k == 0 else (("maximum", None) if top_k == 1 else ("average_top_k", top_k))


def _batch(hists, H):
    """window int64 [B, H] left-padded with 0 (the last H items) + the CSR of the full histories, on the device."""
    B = len(hists)
    win = np.zeros((B, H), dtype=np.int64)
    for b, h in enumerate(hists):
        w = np.asarray(h)[-H:]
        win[b, H - len(w):] = w
    ptr = np.zeros(B + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(h) for h in hists])
    items = np.concatenate([np.asarray(h, dtype=np.int64) for h in hists])
    return torch.from_numpy(win).cuda(), torch.from_numpy(ptr).cuda(), torch.from_numpy(items).cuda()


def _case(B, N, F, lens, seed, dup=()):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((N, F)).astype(np.float32)
    for a, b in dup:
        v[b] = v[a]
    hists = [rng.integers(1, N, size=int(n)) for n in lens]
    assert len(hists) == B
    return v, hists


def _check(v, hists, H, top_k, K, idx, val, unit64=None):
    """The threshold rule for every user; returns the float64 (ids, sorted scores) per user."""
    F = v.shape[1]
    tol = R.tol(F)
    unit64 = R.unit_rows(v) if unit64 is None else unit64
    method, top_num = _method(top_k)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    assert idx.shape == (len(hists), K) and val.shape == (len(hists), K)
    refs, worst = [], 0.0
    for b, h in enumerate(hists):
        ids64, vals64, s64 = R.topk(v, h, K, method, top_num, window=H, unit=unit64)
        refs.append((ids64, np.sort(s64)[::-1]))
        n_live = int(np.isfinite(s64).sum())
        live = min(K, n_live)
        got = idx[b, :live]
        assert len(set(got.tolist())) == live, (b, got)                             # distinct
        assert (got >= 1).all() and (got < len(s64)).all() and np.isfinite(s64[got]).all(), (b, got)     # none is masked
        assert (val[b, :-1] >= val[b, 1:]).all(), (b, val[b])                          # descending
        for r in range(live):
            assert s64[got[r]] >= vals64[r] - tol, (b, r, got[r], s64[got[r]], vals64[r])
            assert abs(val[b, r] - s64[got[r]]) <= tol, (b, r, val[b, r], s64[got[r]])
            worst = max(worst, abs(val[b, r] - s64[got[r]]))
        assert np.isneginf(val[b, live:]).all(), (b, val[b])                        # fewer than K unmasked items: -inf
    print(f"F={F} top_k={top_k} K={K}: largest |value - float64| = {worst:.3e} (tol {tol:.3e})")
    return refs


def _run(v, hists, H, top_k, K):
    unit = ops.visrank_unit_rows(torch.from_numpy(v).cuda())
    win, ptr, items = _batch(hists, H)
    idx, val = ops.visrank_topk(unit, win, top_k, K, ptr, items)
    torch.cuda.synchronize()
    ops.raise_on_bad_indices()
    return idx, val


def test_unit_rows_match_float64():
    rng = np.random.default_rng(0)
    v = rng.standard_normal((301, 2048)).astype(np.float32)
    v[5] = 0.0                                                                      # a zero row stays zero (eps floor)
    u = ops.visrank_unit_rows(torch.from_numpy(v).cuda()).cpu().numpy()
    assert np.abs(u - R.unit_rows(v)).max() <= 8 * 2.0 ** -24 and not u[5].any()
    with pytest.raises(_l.PxrError):
        ops.visrank_unit_rows(torch.zeros(4, 10).cuda())                            # F % 4


@pytest.mark.parametrize("top_k", [1, 3, 0])
def test_exact_ids_where_the_float64_gaps_allow_it(top_k):
    B, N, F, H, K = 64, 4001, 32, 50, 10
    rng = np.random.default_rng(11)
    v, hists = _case(B, N, F, rng.integers(1, 90, size=B), seed=12)
    idx, val = _run(v, hists, H, top_k, K)
    refs = _check(v, hists, H, top_k, K, idx, val)
    clear = [b for b, (_, s) in enumerate(refs) if (-(np.diff(s[:K + 1])) > 2 * R.tol(F)).all()]
    assert len(clear) >= 0.9 * B, len(clear)                                        # a statement about float64 alone
    got = idx.cpu().numpy()
    for b in clear:
        assert np.array_equal(got[b], refs[b][0]), (b, got[b], refs[b][0])


SHAPES = [
    # B, N, F, H, lens, K, top_k
    (5, 1333, 2048, 50, [1, 50, 89, 7, 23], 10, 1),            # the shipped width; h = 1 and h = 50; B odd; N % 128 != 0
    (3, 1333, 2048, 50, [60, 2, 50], 5, 3),
    (4, 700, 64, 64, [64, 100, 1, 63], 10, 16),                # H = 64 (the widest window), the longest list
    (7, 4001, 32, 50, [1, 2, 3, 16, 17, 50, 80], 10, 16),
    (7, 4001, 32, 50, [1, 2, 3, 16, 17, 50, 80], 5, 0),
    (2, 128, 12, 50, [4, 9], 10, 3),                           # one full tile
    (1, 129, 12, 7, [20], 32, 1),                              # K = 32, a short window
]


@pytest.mark.parametrize("B,N,F,H,lens,K,top_k", SHAPES)
def test_shapes_the_kernel_must_handle(B, N, F, H, lens, K, top_k):
    v, hists = _case(B, N, F, lens, seed=100 + B + N)
    idx, val = _run(v, hists, H, top_k, K)
    _check(v, hists, H, top_k, K, idx, val)
    idx2, val2 = _run(v, hists, H, top_k, K)                                        # run-to-run bit identity
    assert torch.equal(idx, idx2) and torch.equal(val.view(torch.int32), val2.view(torch.int32))


def test_fewer_unmasked_items_than_k_and_duplicate_rows():
    N, F, H, K = 40, 12, 50, 10
    v, _ = _case(1, N, F, [1], seed=3, dup=[(7, 9), (7, 21), (30, 31)])
    hists = [np.array([i for i in range(1, N) if i not in (7, 9, 30)]),             # all but three items masked
             np.array([5, 6]), np.array([7, 30, 7])]                                # duplicate rows in the catalogue and the window
    for top_k in (0, 1, 3):
        idx, val = _run(v, hists, H, top_k, K)
        _check(v, hists, H, top_k, K, idx, val)
        assert sorted(idx[0, :3].tolist()) == [7, 9, 30] and torch.isneginf(val[0, 3:]).all()


def test_fused_and_literal_predict_agree_with_float64_and_the_fixture(tmp_path):
    from pixelrec_amd.model import VISRANK

    g = np.load(GOLD)
    path = str(tmp_path / "v.npy")
    np.save(path, g["v_feat"])

    class D:
        item_num = 80

    gh = [g[f"hist{i}"] for i in range(4)]
    for mi, (m, t) in enumerate(zip(g["methods"], g["top_nums"])):
        model = VISRANK({"method": str(m), "top_num": int(t), "v_feat_path": path}, D()).cuda()
        for i, h in enumerate(gh):                                                  # the reference form: a 1-D unpadded history
            s = model.predict(torch.from_numpy(h).cuda(), None).cpu().numpy()
            ref = g[f"scores.{mi}.{i}"]
            assert s.shape == (80,) and s[0] == -np.inf and np.abs(s[1:] - ref[1:]).max() <= R.tol(12), (m, t, i)
    # the same batches through both paths, each under the threshold rule
    B, N, F, H, K = 9, 1500, 32, 50, 10
    v, hists = _case(B, N, F, [1, 3, 50, 70, 12, 2, 33, 49, 51], seed=77)
    np.save(path, v)

    class D2:
        item_num = N

    for method, top_num, top_k in (("maximum", 0, 1), ("average_top_k", 3, 3), ("average_top_k", 50, 0), ("mean", 0, 0)):
        model = VISRANK({"method": method, "top_num": top_num, "v_feat_path": path}, D2()).cuda()
        assert model.reduction() == top_k
        win, ptr, items = _batch(hists, H)
        idx = model.fused_topk_batch(win, ptr, items, K)
        fval = ops.visrank_topk(model.unit_rows(), win, top_k, K, ptr, items)[1]
        _check(v, hists, H, top_k, K, idx, fval)
        s = model.predict(win, None)                                                # literal: scores, masks, torch.topk
        assert tuple(s.shape) == (B, N) and torch.isneginf(s[:, 0]).all()
        hu = torch.repeat_interleave(torch.arange(B, device="cuda"), (ptr[1:] - ptr[:-1]).long())
        s[(hu, items)] = -np.inf
        lval, lidx = torch.topk(s, K, dim=1)
        _check(v, hists, H, top_k, K, lidx, lval)
    m17 = VISRANK({"method": "average_top_k", "top_num": 17, "v_feat_path": path}, D2()).cuda()
    assert not m17.fused_topk_supported                                             # evaluated through predict
    s = m17.predict(_batch(hists, H)[0], None).cpu().numpy()
    u64 = R.unit_rows(v)
    for b, h in enumerate(hists):
        ref = R.scores(v, h, "average_top_k", 17, unit=u64)
        assert np.abs(s[b, 1:] - ref[1:]).max() <= R.tol(F), b


def test_one_bad_id_raises_and_leaves_the_outputs_untouched():
    B, N, F, H, K = 3, 300, 16, 50, 5
    v, hists = _case(B, N, F, [4, 9, 60], seed=5)
    unit = ops.visrank_unit_rows(torch.from_numpy(v).cuda())
    Lb = _l.load()

    def call(win, ptr, items):
        idx = torch.full((B, K), -7, dtype=torch.int64, device="cuda")
        val = torch.full((B, K), -7.0, device="cuda")
        nb = int(Lb.pxr_visrank_topk_ws_bytes(B, H, N, K))
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        ops.device_status("cuda")
        _l.check(Lb.pxr_visrank_topk_f32(_l.ptr(unit), N, F, _l.ptr(win), B, H, 1, _l.ptr(ptr), _l.ptr(items), K, _l.ptr(idx),
                                         _l.ptr(val), _l.ptr(ws), nb, _l.stream_ptr()), "pxr_visrank_topk_f32")
        torch.cuda.synchronize()
        return idx, val

    win, ptr, items = _batch(hists, H)
    idx, val = call(win, ptr, items)
    ops.raise_on_bad_indices()                                                      # a clean call: no flag, outputs written
    assert (idx >= 1).all() and (val > -7).all()
    for what in ("window", "history", "empty"):
        w2, i2 = win.clone(), items.clone()
        if what == "window":
            w2[1, H - 1] = N                                                        # one id past the table
        elif what == "history":
            i2[2] = -1
        else:
            w2[0] = 0                                                               # h == 0: the mean of nothing
        idx, val = call(w2, ptr, i2)
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices()
        assert (idx == -7).all() and (val == -7.0).all(), what
    idx, val = call(win, ptr, items)                                                # and the next clean call is clean
    ops.raise_on_bad_indices()
    assert (idx >= 1).all()
    assert Lb.pxr_visrank_topk_ws_bytes(B, 65, N, K) == -1 and Lb.pxr_visrank_topk_ws_bytes(B, H, N, 33) == -1
    assert Lb.pxr_visrank_topk_ws_bytes(0, H, N, K) == -1 and Lb.pxr_visrank_topk_ws_bytes(B, 0, N, K) == -1
    with pytest.raises(_l.PxrError):
        ops.visrank_topk(unit, win, 17, K, ptr, items)                              # top_k outside 0..16


E2E = dict(users=150, items=200, F=32, feat_seed=0)


def e2e_dataset(tmp_path, feat_seed=E2E["feat_seed"]):
    """The synthetic dataset, its feature file and override YAML -> (config files, user sequences, features)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth_dataset

    from pixelrec_amd.config import Config
    from pixelrec_amd.data import load_data

    synth_dataset.main(str(tmp_path / "data"), E2E["users"], E2E["items"])
    shipped = os.path.join(ROOT, "configs", "ViNet", "visrank.yaml")
    (tmp_path / "o.yaml").write_text(f"state: INFO\nreproducibility: True\ncheckpoint_dir: '{tmp_path}/saved'\nlog_path: '{tmp_path}/log'\n"
                                     f"data_path: {tmp_path}/data/\nv_feat_path: {tmp_path}/feat.npy\nneed_training: False\n"
                                     "eval_batch_size: 64\n")
    files = [shipped, str(tmp_path / "o.yaml")]
    data = load_data(Config(files))
    data.build()
    v = np.random.default_rng(feat_seed).standard_normal((data.item_num, E2E["F"])).astype(np.float32)
    np.save(str(tmp_path / "feat.npy"), v)
    return files, [np.asarray(s, dtype=np.int64) for s in data.user_seq.values()], v


def e2e_float64(seqs, v, K=10):
    """-> ({phase: metrics}, the smallest float64 gap among any user's top K + 1 scores) for the shipped method (top_num 1)."""
    u64 = R.unit_rows(v)
    out, gap = {}, np.inf
    for phase, cut in (("valid", 2), ("test", 1)):
        ids, tg = [], []
        for s in seqs:
            hist, target = s[:len(s) - cut], s[len(s) - cut]
            i, _, s64 = R.topk(v, hist, K, "average_top_k", 1, unit=u64)
            top = np.sort(s64)[::-1][:K + 1]
            gap = min(gap, float(np.min(-np.diff(top))))
            ids.append(i); tg.append(target)
        out[phase] = R.metrics(np.stack(ids), np.array(tg))
    return out, gap


def test_main_py_evaluates_without_training_and_matches_float64_metrics(tmp_path):
    files, seqs, v = e2e_dataset(tmp_path)
    want, gap = e2e_float64(seqs, v)
    assert gap > 2 * R.tol(E2E["F"]), gap                     # no user of this dataset has a close gap: the ids are determined
    env = {k: v_ for k, v_ in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "OMP_NUM_THREADS")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--device", "0", "--config_file", *files],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert not re.findall(r"epoch \d+ training \[time", out), out[-3000:]           # nothing is trained
    assert "Loading model structure and parameters from" in out, out[-3000:]        # the placeholder checkpoint saves and loads
    for tag, phase in (("best valid", "valid"), ("test result", "test")):
        for metric in ("recall@5", "ndcg@5", "recall@10", "ndcg@10"):
            mm = re.search(r"%s ?: .*?'%s', ([0-9.]+)\)" % (tag, metric), out)
            assert mm is not None, out[-2000:]
            assert abs(float(mm.group(1)) - want[phase][metric]) <= 1e-6, (tag, metric, mm.group(1), want[phase][metric])
