"""MODSSM and MOFM on the gfx950 kernels: the dense sink of the pooled segment sum (pxr_pool_dense_grad_f32) against the sparse sink
bit for bit and against float64, the head without the tower against the float64 restatement, the models against the fixtures of the
reference's own MODSSM and MOFM (loss, every trainable encoder gradient, compute_item, predict, the fused top-k), run-to-run bit
identity, bad ids, and main.py end to end.  Every test here needs the new kernel entry or the new models, so each fails without the
feature."""
import os

import numpy as np
import pytest
import torch

from pixelrec_amd import ops
from tests import pool_restate as R
from tests.mo_common import GOLD, assert_two_fresh_models_agree, bits as _bits, my_name, run_main_py, sort_constants as _sort_constants
from tests.test_mopool_cpu import CASES, _config, build_from_fixture

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------ the kernel
def _edge_index(B, L, n_rows, seed):
    """test_gpu_pool.py's edge rows over a batch-local row space: positions in [1, n_rows - 1) -- row n_rows - 1 is listed and read
    by nobody --, an empty profile, padded positions, a repeat within and across profiles, a positive inside its own profile, one
    sample's positive as another's negative."""
    rng = np.random.default_rng(seed)
    hi = max(2, n_rows - 1)
    prof = torch.from_numpy(rng.integers(1, hi, size=(B, L)))
    tgt = torch.from_numpy(rng.integers(1, hi, size=(B, 2)))
    if B >= 3:
        prof[1, :] = 0
        prof[2, :max(1, L // 2)] = 0
        prof[0, -1] = prof[0, 0]
        prof[2, -1] = prof[0, 0]
        tgt[0, 0] = prof[0, 0]
        tgt[1, 0] = tgt[0, 1]
    elif B == 2:
        prof[1, 0] = 0
    return prof, tgt


def _weights(prof, mean):
    cnt = (prof != 0).sum(1).float()
    return torch.where(cnt > 0, 1.0 / (cnt + 1e-8), torch.zeros(())) if mean else (cnt > 0).float()


def _check_dense(prof, tgt, G, w, n_rows):
    """The assertions of the kernel tests for one input; returns the dense block."""
    B, L = prof.shape
    D = G.shape[1]
    gidx = torch.cat((prof.reshape(-1), tgt.reshape(-1))).cuda()
    G, w = G.cuda(), w.cuda()
    sp = ops.pool_table_grad(gidx, B, L, G, w, n_rows)
    n = sp.count()
    out = torch.full((n_rows, D), float("nan"), device="cuda")
    d = ops.pool_dense_grad(gidx, B, L, G, w, n_rows, out=out)
    assert d.data_ptr() == out.data_ptr()
    want = torch.zeros(n_rows, D, device="cuda")
    want[sp.idx[:n]] = sp.rows[:n]
    assert torch.equal(_bits(d), _bits(want))                      # the sparse sink's rows, bit for bit, and +0.0 elsewhere
    referenced = torch.zeros(n_rows, dtype=torch.bool, device="cuda")
    live = gidx[(gidx > 0) & (gidx < n_rows)]
    referenced[live] = True
    assert sorted(set(live.tolist())) == sp.idx[:n].tolist()
    assert not bool(referenced[0]) and int(_bits(d[~referenced]).abs().max()) == 0        # +0.0 where a NaN stood before the call
    assert not bool(referenced[n_rows - 1]) or n_rows == 2
    # float64: (k + 1) 2^-24 sum|terms| with k the occurrences of the row
    terms = torch.cat(((w.double()[:, None] * G[:B].double()).repeat_interleave(L, 0), G[B:].double()))
    keep = ((gidx > 0) & (gidx < n_rows)).double()[:, None]
    safe = gidx.clamp(0, n_rows - 1)
    z = lambda: torch.zeros(n_rows, D, dtype=torch.float64, device="cuda")
    d64, dabs = z().index_add_(0, safe, terms * keep), z().index_add_(0, safe, terms.abs() * keep)
    k = torch.zeros(n_rows, dtype=torch.float64, device="cuda").index_add_(0, safe, keep[:, 0])
    over = (d.double() - d64).abs() - (k[:, None] + 1) * U32 * dabs
    assert float(over.max()) <= 0, float((d.double() - d64).abs().max())
    out2 = torch.full((n_rows, D), float("nan"), device="cuda")
    assert torch.equal(_bits(ops.pool_dense_grad(gidx, B, L, G, w, n_rows, out=out2)), _bits(d))          # twice: the same bits
    return d


@pytest.mark.parametrize("mean", [False, True], ids=["sum", "mean"])
@pytest.mark.parametrize("B,L,D,n_rows", [(1, 1, 4, 3), (3, 4, 8, 9), (5, 10, 64, 40), (3, 4, 260, 9), (2, 3, 4096, 8), (3, 4, 2052, 9),
                                          (24, 4, 256, 6)])
def test_dense_sink_equals_the_sparse_sink_scattered(B, L, D, n_rows, mean):
    """pxr_pool_dense_grad_f32 against pxr_pool_table_grad_f32 on the same input: the same sort and the same segsum_body<MODE_POOL>
    in the same order, so the dense block IS zeros with the sparse rows scattered in -- derived, not measured -- and rows nobody
    reads (row 0 too) are +0.0 although the block held NaN before the call.  D = 260: a row ends inside a 64-lane chunk; 4096 and
    2052: the one-row-per-workgroup path and just past its threshold; (24, 4, 256, 6): 144 occurrences over four rows, every
    segment longer than SEG_SHORT, on the row-group path's long-row branch.  Against float64 each entry is within
    (k + 1) 2^-24 sum|terms|, k the occurrences of its row.  Ids outside [0, n_rows) are dropped."""
    prof, tgt = _edge_index(B, L, n_rows, 100 * B + L)
    g = torch.Generator().manual_seed(B + L + D)
    G = torch.randn(3 * B, D, generator=g)
    d = _check_dense(prof, tgt, G, _weights(prof, mean), n_rows)
    if B >= 3:                                                     # an id past the block and a negative one: dropped, nothing else moves
        prof2, tgt2 = prof.clone(), tgt.clone()
        keep_row = int(prof2[0, 1])
        prof2[0, 1], tgt2[2, 1] = n_rows, -3
        d2 = _check_dense(prof2, tgt2, G, _weights(prof2, mean), n_rows)
        assert d2.shape == d.shape and keep_row >= 1


def test_dense_sink_above_the_fused_sort_cut_over():
    """n = B (L + 2) just above FP_MAX_N: the multi-launch radix sort, whose ping-pong buffers the entry hands over in another
    order (the unique-row list lives in the free pair).  48 rows share the occurrences, so every segment is longer than SEG_CHUNK
    as well (several staged chunks per row)."""
    fp_max_n, seg_short, seg_chunk = _sort_constants()
    L, D, n_rows = 2, 64, 50
    B = fp_max_n // (L + 2) + 16
    assert B * (L + 2) > fp_max_n and B * (L + 2) // (n_rows - 2) > seg_chunk > seg_short
    rng = np.random.default_rng(3)
    prof = torch.from_numpy(rng.integers(1, n_rows - 1, size=(B, L)))
    prof[np.arange(B) % 5 == 1, 0] = 0
    prof[np.arange(B) % 7 == 2, :] = 0
    tgt = torch.from_numpy(rng.integers(1, n_rows - 1, size=(B, 2)))
    G = torch.randn(3 * B, D, generator=torch.Generator().manual_seed(4))
    _check_dense(prof, tgt, G, _weights(prof, True), n_rows)


def test_dense_sink_refuses_what_it_cannot_serve():
    from pixelrec_amd.lib import PxrError

    gidx = torch.tensor([1, 2, 1, 2], device="cuda")
    G, w = torch.zeros(3, 8, device="cuda"), torch.ones(1, device="cuda")
    ops.pool_dense_grad(gidx, 1, 2, G, w, 3)
    with pytest.raises(PxrError):
        ops.pool_dense_grad(gidx, 1, 2, G, w, 3, out=G)             # d_rows must not alias G
    with pytest.raises(PxrError):
        ops.pool_dense_grad(gidx[:3], 1, 2, G, w, 3)
    with pytest.raises(PxrError):
        ops.pool_dense_grad(gidx, 1, 2, torch.zeros(3, 6, device="cuda"), w, 3)     # D % 4


# ------------------------------------------------------------------------------------------------------------ the head
def _tiny_model(name, D, L=4):
    import pixelrec_amd.model as M

    class DL:
        item_num = 13

    torch.manual_seed(0)
    return getattr(M, name)(_config(D, L, 37), DL()).cuda().train()


@pytest.mark.parametrize("name", ["MODSSM", "MOFM"])
@pytest.mark.parametrize("B,L,D,n_rows", [(3, 4, 8, 9), (2, 3, 4096, 8)])
def test_head_without_the_tower_matches_float64(name, B, L, D, n_rows):
    """loss_from_embeddings on a random leaf E: the loss and E.grad against pool_restate.analytic (float64 with the float32 bounds
    carried), rows nobody reads exactly zero; the no-grad call gives the same loss bits."""
    kind = "DSSM" if name == "MODSSM" else "FM"
    m = _tiny_model(name, D, L)
    prof, tgt = _edge_index(B, L, n_rows, 7 * B + L)
    tgt[:, 1] = tgt[:, 0] % (n_rows - 2) + 1                        # the negative differs from the positive
    E = (torch.randn(n_rows, D, generator=torch.Generator().manual_seed(D + B)) * 0.5).cuda().requires_grad_(True)
    a = R.analytic(kind, {R.TABLE: E.detach()}, torch.cat((prof, tgt), 1).cuda())
    loss = m.loss_from_embeddings(E, prof.cuda(), tgt.cuda())
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    ops.raise_on_bad_indices()
    got = float(loss.detach())
    print(name, (B, L, D), "loss", got, float(a["loss"][0]), "bound", float(a["loss"][1]))
    assert abs(got - float(a["loss"][0])) <= float(a["loss"][1])
    gv, gb = a["grad"][R.TABLE]
    assert E.grad.shape == E.shape
    err = (E.grad.double() - gv).abs()
    print(name, (B, L, D), "dE", float(err.max()), "bound up to", float(gb.max()))
    assert float((err - gb).max()) <= 0
    quiet = a["count"] == 0
    assert bool(quiet[0]) and bool(quiet[n_rows - 1]) and int(_bits(E.grad[quiet]).abs().max()) == 0
    with torch.no_grad():
        assert float(m.loss_from_embeddings(E.detach(), prof.cuda(), tgt.cuda())) == got
    # a fully frozen input still drives the head's backward
    frozen = m.loss_from_embeddings(E.detach(), prof.cuda(), tgt.cuda())
    assert frozen.requires_grad
    frozen.backward()


@pytest.mark.parametrize("name", ["MODSSM", "MOFM"])
def test_bad_index_raises_index_error(name):
    m = _tiny_model(name, 8)
    E = torch.randn(9, 8).cuda().requires_grad_(True)
    prof, tgt = _edge_index(3, 4, 9, 1)
    ops.raise_on_bad_indices()
    for where, val in (("p", 9), ("t", 9), ("t", -2), ("p", -1)):
        p2, t2 = prof.clone(), tgt.clone()
        if where == "p":
            p2[0, 0] = val
        else:
            t2[0, 1] = val
        m.loss_from_embeddings(E, p2.cuda(), t2.cuda()).backward()
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices()
    m.loss_from_embeddings(E, prof.cuda(), tgt.cuda()).backward()
    ops.raise_on_bad_indices()                                      # a clean batch leaves the word clear


# ------------------------------------------------------------------------------------------------------------ the fixtures
@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    name, kind = CASES[request.param]
    return name, kind, np.load(os.path.join(GOLD, request.param + ".npz"))


def _ref_input(name, index):
    return R.fm_form(index).cuda() if name == "MOFM" else torch.as_tensor(index).cuda()


def _step(m, name, g, j, store):
    """One forward / backward on fixture batch j in the reference's input form -> (loss, {parameter name: gradient})."""
    modal = store[torch.from_numpy(g[f"b{j}.image_ids"]).cuda()]
    loss = m((_ref_input(name, g[f"b{j}.index"]), modal))
    loss.backward()
    loss = loss.detach().clone()
    return loss, {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad and p.grad is not None}


def test_models_match_the_reference_fixtures(case):
    """Loss, every trainable encoder gradient, compute_item and predict against the stored results of the reference's MODSSM / MOFM.
    Budgets: the project's measured ones for this tiny tower (test_hip_mosasrec_matches_reference_golden) -- loss 3e-5 max(1,
    |loss|), gradients 5e-6 + 5e-4 max|g|, item features 3e-5, scores 1e-4 -- each plus the quantity's stored ref_err."""
    name, kind, g = case
    m = build_from_fixture(name, g).cuda().train()
    store = torch.from_numpy(g["store"].astype(np.float32)).cuda()
    names = [str(k) for k in g["param.keys"]]
    for j in range(2):
        loss, grads = _step(m, name, g, j, store)
        ops.raise_on_bad_indices()
        ref = float(g[f"b{j}.loss"])
        print(name, "batch", j, "loss", float(loss), ref, "err", abs(float(loss) - ref), "ref_err", float(g[f"ref_err.b{j}.loss"]))
        assert abs(float(loss) - ref) <= 3e-5 * max(1.0, abs(ref)) + float(g[f"ref_err.b{j}.loss"])
        checked = 0
        for k in names:
            mine = my_name(k)
            want = torch.from_numpy(g[f"b{j}.grad." + k])
            err = float((grads[mine].cpu() - want).abs().max())
            print(name, "batch", j, "grad", k, err, "max|g|", float(want.abs().max()), "ref_err", float(g[f"ref_err.b{j}.grad." + k]))
            assert err <= 5e-6 + 5e-4 * float(want.abs().max()) + float(g[f"ref_err.b{j}.grad." + k]), (k, err)
            checked += 1
        assert checked == len(names) == len(grads) == 18
    m.eval()
    feat = m.compute_item(store)
    err = float((feat.cpu() - torch.from_numpy(g["eval.item_feature"])).abs().max())
    print(name, "item features", err, "ref_err", float(g["ref_err.item_feature"]))
    assert err <= 3e-5 + float(g["ref_err.item_feature"])
    win = torch.from_numpy(g["eval.windows"]).cuda()
    scores = m.predict(win, feat)
    err = float((scores.cpu() - torch.from_numpy(g["eval.scores"])).abs().max())
    print(name, "scores", err, "ref_err", float(g["ref_err.scores"]))
    assert err <= 1e-4 + float(g["ref_err.scores"])
    assert float(scores[5].abs().max()) == 0                        # the all-padding window: exactly 0 for every item
    # the fused top-k through encode_last against predict + masks + topk
    K, Bw = 5, len(win)
    hist = [sorted(set(w[w != 0].tolist())) for w in g["eval.windows"]]
    hu = torch.tensor([b for b in range(Bw) for _ in hist[b]], dtype=torch.int64)
    hi = torch.tensor([i for b in range(Bw) for i in hist[b]], dtype=torch.int64)
    ptr, items = ops.history_csr(hu, hi, Bw, "cuda")
    out, last = m.encode_last(win, feat)
    assert out.shape == (Bw, 1, feat.shape[1]) and last.shape == (Bw, feat.shape[1])
    idx, _ = ops.score_topk(last, last.stride(0), Bw, feat.data, K, ptr, items)
    ops.raise_on_bad_indices()
    masked = scores.cpu().clone()
    masked[:, 0] = float("-inf")
    for b, h in enumerate(hist):
        masked[b, h] = float("-inf")
    real = torch.from_numpy((g["eval.windows"] != 0).any(1))
    assert torch.equal(idx.cpu()[real], torch.topk(masked, K, -1).indices[real])


def test_two_fresh_models_give_the_same_bits(case):
    name, _, g = case
    store = torch.from_numpy(g["store"].astype(np.float32)).cuda()
    assert_two_fresh_models_agree(lambda: build_from_fixture(name, g).cuda().train(), lambda m, j: _step(m, name, g, j, store), 19)


def test_gradient_clipping_covers_a_model_without_a_flat_buffer(case):
    """clip_grad_norm_ on a model whose gradients are the encoder's alone: the norm it returns is the norm of those gradients, and
    they leave scaled to max_norm."""
    from pixelrec_amd.optim import clip_grad_norm_

    name, _, g = case
    m = build_from_fixture(name, g).cuda().train()
    store = torch.from_numpy(g["store"].astype(np.float32)).cuda()
    _, grads = _step(m, name, g, 0, store)
    norm = torch.sqrt(sum(v.double().pow(2).sum() for v in grads.values()))
    total = clip_grad_norm_(m, max_norm=0.01 * float(norm))
    assert abs(float(total) - float(norm)) <= 1e-5 * float(norm)
    after = torch.sqrt(sum(p.grad.double().pow(2).sum() for _, p in m.named_parameters() if p.requires_grad and p.grad is not None))
    assert abs(float(after) - 0.01 * float(norm)) <= 1e-4 * 0.01 * float(norm)


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("name", ["MODSSM", "MOFM"])
def test_main_py_trains_evaluates_and_the_checkpoint_reloads(name, tmp_path):
    """main.py on TinyInter with synthetic 64 x 64 images and the tiny tower, two epochs: finite losses that change, Recall@10 and
    NDCG@10 reported from the reloaded checkpoint, whose state_dict is the encoder's and loads with strict=True."""
    from pixelrec_amd.utils import get_model

    _, _, ck, config, data = run_main_py(tmp_path, f"model: {name}\nembedding_size: 32\ndropout_prob: 0\nmlp_hidden_size: []\n")
    assert all(k.startswith("visual_encoder.") for k in ck["state_dict"])
    assert [len(x["params"]) for x in ck["optimizer"]["param_groups"]] == [18, 0]       # the reference's two groups, the second empty
    fresh = get_model(name)(config, data)
    fresh.load_state_dict(ck["state_dict"], strict=True)
