"""MODIN on the gfx950 kernels: the dense sink of the plain occurrence-row segment sum (pxr_embed_grad_dense_f32) against the sparse
sink bit for bit and against float64, the head's regulariser argument (pxr_din_head_fwd_reg_f32), the head without the tower against
the float64 restatement, bit identity with DIN's launches, the batch-wide dedup against one row per position, the model against the
fixture of the reference's own MODIN in both input forms (loss, all 24 gradients, compute_item, predict, the fused top-k), the fused
top-k against DIN's, bad positions, the optimizer's two groups, and main.py end to end.  Every test here needs the new entries, the
new op or the new class, so each fails without the feature."""
import os

import numpy as np
import pytest
import torch

from pixelrec_amd import lib as _l
from pixelrec_amd import ops
from tests import din_restate as DR
from tests import modin_restate as R
from tests.mo_common import (GOLD, assert_optimizer_state_round_trips, assert_two_fresh_models_agree, bits as _bits, my_name, run_main_py,
                              sort_constants as _sort_constants)
from tests.test_modin_cpu import _config, build_from_fixture

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24
FUSED_MEASURED = 2.284e-6          # tests/test_gpu_din.py: the reference's own float32 predict against float64, relative
FUSED_TOL = 4 * FUSED_MEASURED     # ... and what the fused kernel is allowed there


# ------------------------------------------------------------------------------------------------------------ 1. the dense sink
def _occ_ids(n, n_rows, seed):
    """n ids in [1, n_rows - 1) -- row n_rows - 1 is read by nobody --, with a stretch of id 0 and a repeat (n permitting)."""
    rng = np.random.default_rng(seed)
    idx = torch.from_numpy(rng.integers(1, max(2, n_rows - 1), size=n))
    if n >= 4:
        idx[1:1 + max(1, n // 8)] = 0
        idx[-1] = idx[0]
    return idx


def _check_dense(idx, rows, n_rows):
    """The assertions of the kernel tests for one input (idx, rows on the CPU); returns the dense block."""
    n, D = rows.shape
    idx, rows = idx.cuda(), rows.cuda()
    sp = ops.embed_grad_rows(idx, rows, n_rows, scale=1.0)
    nu = sp.count()
    out = torch.full((n_rows, D), float("nan"), device="cuda")
    d = ops.embed_grad_dense(idx, rows, n_rows, out=out)
    assert d.data_ptr() == out.data_ptr()
    want = torch.zeros(n_rows, D, device="cuda")
    want[sp.idx[:nu]] = sp.rows[:nu]
    assert torch.equal(_bits(d), _bits(want))                      # the sparse sink's rows, bit for bit, and +0.0 elsewhere
    referenced = torch.zeros(n_rows, dtype=torch.bool, device="cuda")
    live = idx[(idx > 0) & (idx < n_rows)]
    referenced[live] = True
    assert sorted(set(live.tolist())) == sp.idx[:nu].tolist()
    assert not bool(referenced[0]) and int(_bits(d[~referenced]).abs().max()) == 0        # +0.0 where a NaN stood before the call
    assert not bool(referenced[n_rows - 1])
    # float64: (k + 1) 2^-24 sum|terms| with k the occurrences of the row
    keep = ((idx > 0) & (idx < n_rows)).double()[:, None]
    safe = idx.clamp(0, n_rows - 1)
    z = lambda: torch.zeros(n_rows, D, dtype=torch.float64, device="cuda")
    d64, dabs = z().index_add_(0, safe, rows.double() * keep), z().index_add_(0, safe, rows.double().abs() * keep)
    k = torch.zeros(n_rows, dtype=torch.float64, device="cuda").index_add_(0, safe, keep[:, 0])
    over = (d.double() - d64).abs() - (k[:, None] + 1) * U32 * dabs
    assert float(over.max()) <= 0, float((d.double() - d64).abs().max())
    out2 = torch.full((n_rows, D), float("nan"), device="cuda")
    assert torch.equal(_bits(ops.embed_grad_dense(idx, rows, n_rows, out=out2)), _bits(d))                 # twice: the same bits
    return d


@pytest.mark.parametrize("n,D,n_rows", [(1, 4, 3), (18, 8, 9), (70, 64, 40), (18, 260, 9), (10, 4096, 8), (18, 2052, 9), (144, 256, 6)])
def test_dense_sink_equals_the_sparse_sink_scattered(n, D, n_rows):
    """pxr_embed_grad_dense_f32 against pxr_embed_grad_rows_f32 (scale 1) on the same input: the same sort and the same
    segsum_body<MODE_ROWS> in the same order, so the dense block IS zeros with the sparse rows scattered in -- derived, not measured
    -- and rows nobody reads (row 0 too) are +0.0 although the block held NaN before the call.  D = 260: a row ends inside a
    64-lane chunk; 4096 and 2052: the one-row-per-workgroup path and just past its threshold; (144, 256, 6): every segment longer
    than SEG_SHORT, on the row-group path's long-row branch.  Against float64 each entry is within (k + 1) 2^-24 sum|terms|, k the
    occurrences of its row.  Ids n_rows and -3 are dropped and nothing else moves."""
    idx = _occ_ids(n, n_rows, 100 * n + D)
    rows = torch.randn(n, D, generator=torch.Generator().manual_seed(n + D))
    if (n, D, n_rows) == (144, 256, 6):
        cnt = torch.bincount(idx[idx > 0], minlength=n_rows)
        assert int(cnt[1:n_rows - 1].min()) > 8                     # SEG_SHORT
    d = _check_dense(idx, rows, n_rows)
    if n >= 18:
        idx2 = idx.clone()
        a, b = n // 2, n // 2 + 1
        touched = {int(idx2[a]), int(idx2[b])}
        idx2[a], idx2[b] = n_rows, -3
        d2 = _check_dense(idx2, rows, n_rows)
        same = torch.tensor([r not in touched for r in range(n_rows)], device="cuda")
        assert torch.equal(_bits(d2[same]), _bits(d[same]))


def test_dense_sink_above_the_fused_sort_cut_over():
    """n just above FP_MAX_N: the multi-launch radix sort, whose ping-pong buffers the entry hands over in another order (the
    unique-row list lives in the free pair).  48 rows share the occurrences, so every segment is longer than SEG_CHUNK as well
    (several staged chunks per row); about 17 MB of occurrence rows."""
    fp_max_n, seg_short, seg_chunk = _sort_constants()
    D, n_rows = 64, 50
    n = fp_max_n + 64
    assert n // (n_rows - 2) > seg_chunk > seg_short and n * D * 4 < 20e6
    rng = np.random.default_rng(3)
    idx = torch.from_numpy(rng.integers(1, n_rows - 1, size=n))
    idx[np.arange(n) % 5 == 1] = 0
    idx[100:400] = 0
    rows = torch.randn(n, D, generator=torch.Generator().manual_seed(4))
    _check_dense(idx, rows, n_rows)


def test_dense_sink_refuses_what_it_cannot_serve():
    from pixelrec_amd.lib import PxrError

    idx = torch.tensor([1, 2, 1, 2], device="cuda")
    rows = torch.zeros(4, 8, device="cuda")
    ops.embed_grad_dense(idx, rows, 3)
    with pytest.raises(PxrError):
        ops.embed_grad_dense(idx, rows, 4, out=rows)                # d_rows must not alias rows
    with pytest.raises(PxrError):
        ops.embed_grad_dense(idx[:3], rows, 3)                      # a length mismatch
    with pytest.raises(PxrError):
        ops.embed_grad_dense(idx, torch.zeros(4, 6, device="cuda"), 3)     # D % 4


# ------------------------------------------------------------------------------------------------------------ 2. the head's reg
def _edge_index(B, L, n_rows, seed):
    """test_gpu_mopool.py's edge rows over a batch-local row space: positions in [1, n_rows - 1) -- row n_rows - 1 is listed and read
    by nobody --, an empty profile, padded positions, a repeat within and across profiles, a positive inside its own profile, one
    sample's positive as another's negative; no sample's negative equals its positive."""
    rng = np.random.default_rng(seed)
    hi = max(2, n_rows - 1)
    prof = torch.from_numpy(rng.integers(1, hi, size=(B, L)))
    tgt = torch.from_numpy(rng.integers(1, hi, size=(B, 2)))
    tgt[:, 1] = tgt[:, 0] % (hi - 1) + 1
    if B >= 3:
        prof[1, :] = 0
        prof[2, :max(1, L // 2)] = 0
        prof[0, -1] = prof[0, 0]
        prof[2, -1] = prof[0, 0]
        tgt[0, 0] = prof[0, 0]
        tgt[0, 1] = tgt[0, 0] % (hi - 1) + 1
        tgt[1, 1] = tgt[0, 0]
        tgt[1, 0] = tgt[1, 1] % (hi - 1) + 1
    assert bool((tgt[:, 0] != tgt[:, 1]).all())
    return prof, tgt


@pytest.mark.parametrize("B,L,D,hl", [(3, 4, 8, 4), (5, 10, 64, 40)])
def test_head_regulariser_is_an_argument(B, L, D, hl):
    """reg = 0.01 is pxr_din_head_fwd_f32 (the entry DIN has called so far, reached here through ctypes) bit for bit; reg = 0 leaves
    head[1] == +0.0, the same s, kq, coef and x, and a loss within test_gpu_din.py's err_loss -- without the norm's share of its
    reduction term -- of -mean log(sigmoid(x64) + 1e-8) in float64."""
    g = torch.Generator().manual_seed(B + L + D)
    M = 23
    E = (torch.randn(M, D, generator=g) * 0.5).cuda()
    prof, tgt = (t.cuda() for t in _edge_index(B, L, M, 100 * B + L))
    rows, _ = ops.din_positions(prof, tgt, M)
    emb, _ = ops.din_att_input(E, rows, B, L)
    alast = torch.rand(2 * B * L, hl, generator=g).cuda()
    wd, bd = (torch.randn(hl, generator=g) * 0.5).cuda(), torch.randn(1, generator=g).cuda()
    s0, kq0, head0 = (torch.full((k,), float("nan"), device="cuda") for k in (2 * B * L, 2 * B * L, 2 + 3 * B))
    _l.check(_l.load().pxr_din_head_fwd_f32(_l.ptr(alast), _l.ptr(wd), _l.ptr(bd), _l.ptr(emb), _l.ptr(prof), B, L, D, hl, _l.ptr(s0),
                                            _l.ptr(kq0), _l.ptr(head0), _l.stream_ptr()), "pxr_din_head_fwd_f32")
    loss1, s1, kq1, head1 = ops.din_head_fwd(alast, wd, bd, emb, prof, reg=0.01)
    lossd, sd_, kqd, headd = ops.din_head_fwd(alast, wd, bd, emb, prof)
    for a, b in ((s1, s0), (kq1, kq0), (head1, head0), (sd_, s0), (kqd, kq0), (headd, head0)):
        assert torch.equal(_bits(a), _bits(b))
    assert float(head0[1]) > 0
    loss0, s, kq, head = ops.din_head_fwd(alast, wd, bd, emb, prof, reg=0.0)
    assert int(_bits(head[1:2])) == 0
    assert torch.equal(_bits(s), _bits(s0)) and torch.equal(_bits(kq), _bits(kq0))
    assert torch.equal(_bits(head[2:2 + 2 * B]), _bits(head0[2:2 + 2 * B]))               # coef | x
    d = lambda t: t.double()
    kk = emb[:B * L].view(B, L, D)[None].expand(2, B, L, D)
    qq = emb[B * L:].view(B, 2, D).transpose(0, 1)[:, :, None, :].expand(2, B, L, D)
    mask = (prof == 0)[None].expand(2, B, L)
    s64 = (d(alast) @ d(wd) + d(bd)).view(2, B, L).masked_fill(mask, 0.0) / D ** 0.5
    kq64 = (d(kk) * d(qq)).sum(-1)
    err_s = (hl + 4) * U32 * float(((d(alast).abs() @ d(wd).abs()) + d(bd).abs()).max()) / D ** 0.5
    err_kq = (D + 1) * U32 * float((d(kk) * d(qq)).abs().sum(-1).max())
    sc64 = (s64 * kq64).sum(-1)
    x64 = sc64[0] - sc64[1]
    loss64 = -(torch.log(torch.sigmoid(x64) + 1e-8)).mean()
    err_x = 2 * L * (err_s * float(kq64.abs().max()) + float(s64.abs().max()) * err_kq + (L + 2) * U32 * float((s64 * kq64).abs().max()))
    err_loss = err_x + (B + 8) * U32 * (float(loss64.abs()) + 1.0)
    print("loss", float(loss0), float(loss64), "err", abs(float(loss0) - float(loss64)), "bound", err_loss)
    assert abs(float(loss0) - float(loss64)) <= err_loss
    assert float(loss0) == float(head[0]) and float(loss1) > float(loss0)


# ------------------------------------------------------------------------------------------------------------ 3. the head alone
def _tiny_model(D, L=4, hidden=(12, 4), seed=0):
    import pixelrec_amd.model as M

    class DL:
        item_num = 13

    torch.manual_seed(seed)
    m = M.MODIN(_config(D, L, 37, hidden), DL())
    with torch.no_grad():                                           # biases off zero, so that their part in the function shows
        for p in m.attention.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return m.cuda().train()


def _att(m, dtype):
    return {k: m.get_parameter(k).detach().to(dtype).clone() for k in R.names(len(m.mlp_hidden_size))}


HEAD_SHAPES = [(3, 4, 8, (12, 4), 9), (64, 10, 64, (80, 40), 257)]


def _head_case(S, L, D, hidden, M):
    m = _tiny_model(D, L, hidden)
    prof, tgt = _edge_index(S, L, M, 7 * S + L)
    E = (torch.randn(M, D, generator=torch.Generator().manual_seed(D + S)) * 0.5).cuda()
    index = torch.cat((prof, tgt), 1).cuda()
    res = {dt: R.loss_and_grads(_att(m, dt), E.to(dt), index) for dt in (torch.float64, torch.float32)}
    return m, prof.cuda(), tgt.cuda(), E, index, res


def _assert_grads(tag, got, res, names):
    (_, g64), (_, g32) = res[torch.float64], res[torch.float32]
    for k in names:
        err, d32 = float((got[k].double() - g64[k]).abs().max()), float((g32[k].double() - g64[k]).abs().max())
        big = float(g64[k].abs().max())
        print(tag, "grad", k, "err", err, "float32 restatement", d32, "largest entry", big)
        assert err <= 2 * d32 + 1e-6 * big, k


@pytest.mark.parametrize("S,L,D,hidden,M", HEAD_SHAPES)
def test_head_without_the_tower_matches_float64(S, L, D, hidden, M):
    """loss_from_embeddings on a random leaf E against modin_restate in float64 on the same device, by
    test_a_step_at_the_shipped_widths_matches_float64's rule: the loss within 2 |L32 - L64| + 2e-6 max(1, |L64|), every gradient (the
    six attention tensors and dE) within 2 d32 + 1e-6 max|g64|, L32 / d32 from the float32 restatement on the same inputs.  Rows of
    E nobody reads (row 0, the last row) get exactly zero; the no_grad call gives the same loss bits; a detached E still drives the
    head's backward."""
    m, prof, tgt, E, index, res = _head_case(S, L, D, hidden, M)
    E = E.requires_grad_(True)
    (L64, _), (L32, _) = res[torch.float64], res[torch.float32]
    loss = m.loss_from_embeddings(E, prof, tgt)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    ops.raise_on_bad_indices()
    print("loss", float(loss.detach()), L64, "float32 restatement", L32)
    assert abs(float(loss.detach()) - L64) <= 2 * abs(L32 - L64) + 2e-6 * max(1.0, abs(L64))
    names = R.names(len(hidden))
    got = {k: m.get_parameter(k).grad.detach().clone() for k in names}
    got[R.E_KEY] = E.grad
    assert E.grad.shape == E.shape
    _assert_grads((S, L, D), got, res, names + [R.E_KEY])
    read = torch.zeros(M, dtype=torch.bool, device="cuda")
    read[index.view(-1)] = True
    read[0] = False
    assert not bool(read[M - 1]) and int(_bits(E.grad[~read]).abs().max()) == 0 and float(E.grad[read].abs().max()) > 0
    with torch.no_grad():
        again = m.loss_from_embeddings(E.detach(), prof, tgt)
    assert not again.requires_grad and torch.equal(_bits(again), _bits(loss.detach()))
    before = {k: got[k].clone() for k in names}
    frozen = m.loss_from_embeddings(E.detach(), prof, tgt)
    assert frozen.requires_grad
    frozen.backward()
    for k in names:                                                 # the same step again: the same attention gradients
        assert torch.equal(_bits(m.get_parameter(k).grad), _bits(before[k]))


def test_bad_position_raises_index_error():
    m = _tiny_model(8)
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


# ------------------------------------------------------------------------------------------------------------ 4. DIN's launches
def _din_like(m, table, L):
    """A DIN whose attention weights are MODIN m's and whose item rows are `table` (item id j reads table[j])."""
    from pixelrec_amd.model import DIN

    class DL:
        item_num = table.shape[0]

    d = DIN({"embedding_size": m.embedding_size, "mlp_hidden_size": list(m.mlp_hidden_size), "dropout_prob": 0,
             "MAX_ITEM_LIST_LENGTH": L}, DL())
    sd = {k: v.cpu() for k, v in _att(m, torch.float32).items()}
    sd[DR.TABLE] = table.detach().cpu()
    d.load_state_dict(sd, strict=True)
    return d.cuda().train()


def test_attention_gradients_are_dins_bit_for_bit():
    """A DIN with item_num = M whose table rows are E and whose attention weights are MODIN's, on the same [S, L + 2] rows: both go
    through the same launches, and DIN's regulariser touches only the loss and the occurrence rows, so the six attention gradients
    are bit-identical."""
    S, L, D, hidden, M = HEAD_SHAPES[0]
    m, prof, tgt, E, index, _ = _head_case(S, L, D, hidden, M)
    m.loss_from_embeddings(E.requires_grad_(True), prof, tgt).backward()
    din = _din_like(m, E, L)
    din(index).backward()
    ops.raise_on_bad_indices()
    for k in R.names(len(hidden)):
        a, b = m.get_parameter(k).grad, din.get_parameter(k).grad
        assert float(a.abs().max()) > 0 and torch.equal(_bits(a), _bits(b)), k


# ------------------------------------------------------------------------------------------------------------ 5. the dedup
@pytest.mark.parametrize("S,L,D,hidden,M", HEAD_SHAPES[:1])
def test_dedup_does_not_change_the_function(S, L, D, hidden, M):
    """One row per position (the reference's form: E_x[1 + o] = E[index_o], positions 1 + o, 0 at padding) against the batch-wide
    dedup: the same loss bits; dE[r] is the sum of its copies' gradients, in float64 within (k + 1) 2^-24 sum|terms|; the attention
    gradients within the bounds of the float64 comparison."""
    m, prof, tgt, E, index, res = _head_case(S, L, D, hidden, M)
    E = E.requires_grad_(True)
    loss = m.loss_from_embeddings(E, prof, tgt)
    loss.backward()
    names = R.names(len(hidden))
    flat = index.view(-1)
    Ex = torch.cat((E.detach()[:1], E.detach()[flat])).requires_grad_(True)
    pos = torch.where(index != 0, 1 + torch.arange(flat.numel(), device="cuda").view(index.shape), torch.zeros_like(index))
    loss_x = m.loss_from_embeddings(Ex, pos[:, :L], pos[:, L:])
    loss_x.backward()
    ops.raise_on_bad_indices()
    assert torch.equal(_bits(loss_x.detach()), _bits(loss.detach()))
    terms = Ex.grad[1:].double()
    keep = (flat != 0).double()[:, None]
    z = lambda: torch.zeros(M, D, dtype=torch.float64, device="cuda")
    d64, dabs = z().index_add_(0, flat, terms * keep), z().index_add_(0, flat, terms.abs() * keep)
    k = torch.zeros(M, dtype=torch.float64, device="cuda").index_add_(0, flat, keep[:, 0])
    over = (E.grad.double() - d64).abs() - (k[:, None] + 1) * U32 * dabs
    print("dE against the summed copies", float((E.grad.double() - d64).abs().max()))
    assert float(over.max()) <= 0 and float(Ex.grad[0].abs().max()) == 0
    _assert_grads("one row per position", {k_: m.get_parameter(k_).grad for k_ in names}, res, names)


# ------------------------------------------------------------------------------------------------------------ 6. the fixture
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "modin_tiny.npz"))


def _inputs(g, j, store, form):
    items = g[f"b{j}.items"]
    if form == "positions":                                         # what MoTowerTrainBatcher.make_batch builds
        uniq = np.unique(items)
        image_ids = np.concatenate((np.zeros(1, dtype=np.int64), uniq[uniq != 0]))
        return torch.from_numpy(np.searchsorted(image_ids, items)).cuda(), store[torch.from_numpy(image_ids).cuda()]
    it = torch.from_numpy(items).cuda()
    return store[it], it                                            # modin.py:46: (items_modal [B, L + 2, 3, H, W], items)


def _step(m, g, j, store, form):
    loss = m(_inputs(g, j, store, form))
    loss.backward()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad and p.grad is not None}


@pytest.mark.parametrize("form", ["positions", "reference"])
def test_model_matches_the_reference_fixture(gold, form):
    """Loss, all 24 gradients, compute_item and predict (both forms) against the stored results of the reference's MODIN, with the
    batch in the batcher's form and in the reference's 5-D form.  Budgets: the project's recorded ones for this tiny tower
    (tests/test_gpu_mopool.py::test_models_match_the_reference_fixtures) -- loss 3e-5 max(1, |loss|), gradients 5e-6 + 5e-4 max|g|,
    item features 3e-5, scores 1e-4 -- each plus the quantity's stored ref_err.  Then the fused top-k on the fixture's windows."""
    g = gold
    m = build_from_fixture(g).cuda().train()
    store = torch.from_numpy(g["store"].astype(np.float32)).cuda()
    names = [str(k) for k in g["param.keys"]]
    for j in range(2):
        loss, grads = _step(m, g, j, store, form)
        ops.raise_on_bad_indices()
        ref = float(g[f"b{j}.loss"])
        budget = 3e-5 * max(1.0, abs(ref)) + float(g[f"ref_err.b{j}.loss"])
        print(form, "batch", j, "loss", float(loss), ref, "err", abs(float(loss) - ref), "budget", budget)
        assert abs(float(loss) - ref) <= budget
        for k in names:
            want = torch.from_numpy(g[f"b{j}.grad." + k])
            err = float((grads[my_name(k)].cpu() - want).abs().max())
            budget = 5e-6 + 5e-4 * float(want.abs().max()) + float(g[f"ref_err.b{j}.grad." + k])
            print(form, "batch", j, "grad", k, err, "budget", budget)
            assert err <= budget, (k, err)
        assert len(names) == len(grads) == 24
    m.eval()
    feat = m.compute_item(store)
    err = float((feat.cpu() - torch.from_numpy(g["eval.item_feature"])).abs().max())
    print("item features", err, "budget", 3e-5 + float(g["ref_err.item_feature"]))
    assert err <= 3e-5 + float(g["ref_err.item_feature"])
    win = torch.from_numpy(g["eval.windows"]).cuda()
    N = feat.shape[0]
    for what, seq in (("windows", win), ("reference form", R.reference_form(win.cpu(), N).cuda())):
        scores = m.predict(seq, feat)
        err = float((scores.cpu() - torch.from_numpy(g["eval.scores"])).abs().max())
        print("scores,", what, err, "budget", 1e-4 + float(g["ref_err.scores"]))
        assert tuple(scores.shape) == (len(win), N) and err <= 1e-4 + float(g["ref_err.scores"])
        assert float(scores[5].abs().max()) == 0                    # the all-padding window: exactly 0 for every item
    # the fused top-k on item_feature against predict + masks + topk
    K, Bw = 5, len(win)
    hist = [sorted(set(w[w != 0].tolist())) for w in g["eval.windows"]]
    hu = torch.tensor([b for b in range(Bw) for _ in hist[b]], dtype=torch.int64)
    hi = torch.tensor([i for b in range(Bw) for i in hist[b]], dtype=torch.int64)
    ptr, items = ops.history_csr(hu, hi, Bw, "cuda")
    m.set_item_feature(feat)
    assert m.fused_topk_supported is True
    idx, val = m.fused_topk(win, ptr, items, K)
    assert torch.equal(m.fused_topk_batch(win, ptr, items, K), idx)
    ops.raise_on_bad_indices()
    top, _ = DR.masked_topk(scores.cpu(), hist, K)
    real = torch.from_numpy((g["eval.windows"] != 0).any(1))
    assert torch.equal(idx.cpu()[real], top.indices[real])
    s64 = R.predict(_att(m, torch.float64), feat.double(), win)
    top64, _ = DR.masked_topk(s64.cpu(), hist, K)
    tol = FUSED_TOL * float(s64.abs().max())
    errv = float((val.cpu().double()[real] - top64.values[real]).abs().max())
    print("fused values", errv, "budget", tol)
    assert errv <= tol and torch.equal(idx.cpu()[real], top64.indices[real])


def test_two_fresh_models_give_the_same_bits(gold):
    store = torch.from_numpy(gold["store"].astype(np.float32)).cuda()
    assert_two_fresh_models_agree(lambda: build_from_fixture(gold).cuda().train(), lambda m, j: _step(m, gold, j, store, "positions"), 25)


# ------------------------------------------------------------------------------------------------------------ 7. the fused top-k
def test_fused_topk_is_dins():
    """With the same [N, D] matrix as DIN's table and the same attention weights, MODIN.fused_topk returns DIN's ids and values bit
    for bit; A q + b1 is cached, dropped by train() and by a new set_item_feature, after which the result follows the new matrix;
    without an item_feature the model says so."""
    from pixelrec_amd.lib import PxrError

    N, B, L, hidden, K = 131, 3, 4, (12, 4), DR.TOPK_K
    P, window, hist = DR.topk_case(N, B, L, hidden)
    D = P[DR.TABLE].shape[1]
    assert D == 16
    m = _tiny_model(D, L, hidden)
    missing = m.load_state_dict({k: v for k, v in P.items() if k != DR.TABLE}, strict=False)
    assert not missing.unexpected_keys and all(k.startswith("visual_encoder.") for k in missing.missing_keys)
    m.eval()
    din = _din_like(m, P[DR.TABLE], L).eval()
    hu = torch.tensor([b for b in range(B) for _ in hist[b]], dtype=torch.int64)
    hi = torch.tensor([i for b in range(B) for i in hist[b]], dtype=torch.int64)
    ptr, items = ops.history_csr(hu, hi, B, "cuda")
    win = window.cuda()
    with pytest.raises(PxrError):
        m.fused_topk(win, ptr, items, K)                            # no item_feature yet
    m.set_item_feature(P[DR.TABLE].cuda())
    idx, val = m.fused_topk(win, ptr, items, K)
    didx, dval = din.fused_topk(win, ptr, items, K)
    ops.raise_on_bad_indices()
    assert torch.equal(idx, didx) and torch.equal(_bits(val), _bits(dval))
    cache = m._eval_cache
    assert cache is not None and m.fused_topk(win, ptr, items, K)[0] is not None and m._eval_cache is cache
    m.train()
    assert m._eval_cache is None
    m.eval()
    assert torch.equal(_bits(m.fused_topk(win, ptr, items, K)[1]), _bits(val)) and m._eval_cache is not None
    other = (P[DR.TABLE] * 1.5).cuda()
    m.set_item_feature(other)
    assert m._eval_cache is None
    idx2, val2 = m.fused_topk(win, ptr, items, K)
    didx2, dval2 = _din_like(m, other, L).eval().fused_topk(win, ptr, items, K)
    assert torch.equal(idx2, didx2) and torch.equal(_bits(val2), _bits(dval2)) and not torch.equal(val2, val)
    scores = m.predict(win)                                         # without an argument: the stored item_feature
    assert torch.equal(_bits(scores), _bits(m.predict(win, other)))


# ------------------------------------------------------------------------------------------------------------ optimizer, end to end
def test_optimizer_steps_both_groups_and_its_state_round_trips(gold):
    """Four optim_args: the encoder group and a rec group without a table, [18, 6] parameters; one step moves both; the torch-layout
    state loads into torch.optim.AdamW over the reference's two groups and back."""
    store = torch.from_numpy(gold["store"].astype(np.float32)).cuda()

    def moved(moved, trainable):
        # (a key projection's bias has a zero gradient by the softmax's shift invariance: it may stay where it is)
        assert moved <= trainable and len(moved) >= 21 and set(R.names(2)) <= moved and any("visual_encoder" in k for k in moved)

    assert_optimizer_state_round_trips(lambda: build_from_fixture(gold).cuda().train(), lambda m: _step(m, gold, 0, store, "positions"),
                                       [18, 6], list(range(24)), moved=moved)


def test_main_py_trains_evaluates_and_the_checkpoint_reloads(tmp_path):
    """main.py on TinyInter with synthetic 64 x 64 images and the tiny tower, two epochs, through the fused evaluation: finite losses
    that change, Recall@10 and NDCG@10 reported from the reloaded checkpoint, whose state_dict loads with strict=True."""
    from pixelrec_amd.utils import get_model

    _, _, ck, config, data = run_main_py(tmp_path, "model: MODIN\nembedding_size: 32\ndropout_prob: 0\nmlp_hidden_size: [16, 8]\n")
    assert list(ck["state_dict"])[:6] == R.names(2)
    assert [len(x["params"]) for x in ck["optimizer"]["param_groups"]] == [18, 6]         # the reference's two groups
    fresh = get_model("MODIN")(config, data)
    fresh.load_state_dict(ck["state_dict"], strict=True)
