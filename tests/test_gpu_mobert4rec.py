"""MOBERT4Rec on the gfx950 kernels: the dense sink of the sequence models' three-term segment sum (pxr_seq_occ_dense_f32) against
the sparse route bit for bit and against float64, under three id layouts, on long segments and above the fused-sort cut-over; the
head without the tower against the float64 restatement in every GEMM mode; inert padding; the batch-wide dedup against one row per
position; bit identity with BERT4Rec's launches; the model against the fixture of the reference's own MOBERT4Rec in both input
forms (loss, all 53 gradients, compute_item with the mask row, predict, the generic fused top-k); dropout; the optimizer's two
groups; main.py end to end.  Every test here needs the new entry, the new op or the new class, so each fails without the feature."""
import os

import numpy as np
import pytest
import torch

from pixelrec_amd import ops
from tests import mobert4rec_restate as R
from tests.test_gpu_bert4rec import MODES, mode  # noqa: F401  (the GEMM-mode fixture of the ID model's tests)
from tests.mo_common import (GOLD, assert_optimizer_state_round_trips, assert_two_fresh_models_agree, bits as _bits, my_name, run_main_py,
                              sort_constants as _sort_constants)
from tests.test_mobert4rec_cpu import N_BLOCK, _config, build_from_fixture

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------ 1. the dense sink
def _layouts(L):
    return {"bert4rec": (3 * L, 0, L, 2 * L), "sasrec": (2 * (L + 1), 0, 1, L + 2), "lightsans": (L + 2, 0, 1, 2)}


def _occ_case(B, L, D, n_rows, layout, seed, p_zero=0.15, p_mask=0.0):
    """(items [B, id_bstride] ids in [1, n_rows - 1) -- row n_rows - 1 is read by nobody --, dx0, out [B, L, D], coef [B, L]) on the
    CPU: a share of id 0 (padding), repeats, and with p_mask a row 1 that most inputs read; coef 0 at a share of positions."""
    rng = np.random.default_rng(seed)
    hi = max(2, n_rows - 1)
    items = rng.integers(1, hi, size=(B, layout[0]))
    items[rng.random(items.shape) < p_zero] = 0
    if p_mask and hi > 1:
        plane = items[:, layout[1]:layout[1] + L]
        plane[rng.random(plane.shape) < p_mask] = 1
    if items.size >= 4:
        items.reshape(-1)[-1] = items.reshape(-1)[0]                # a repeat
    g = torch.Generator().manual_seed(seed + 1)
    dx0, out = torch.randn(B, L, D, generator=g), torch.randn(B, L, D, generator=g)
    coef = torch.randn(B, L, generator=g)
    coef[torch.rand(B, L, generator=g) < 0.3] = 0.0
    return torch.from_numpy(items), dx0, out, coef


def _planes(items, L, layout):
    return [items[:, off:off + L].reshape(-1) for off in layout[1:]]


def _check_seq_dense(items, L, layout, dx0, out, coef, n_rows):
    """The assertions of the kernel tests for one input (on the CPU); returns the dense block."""
    B, _, D = out.shape
    items, dx0, out, coef = items.cuda(), dx0.cuda(), out.cuda(), coef.cuda()
    sp = ops.SparseRows(3 * B * L, D, "cuda")
    sp.rows.fill_(float("nan"))
    ws = torch.empty(ops.occ_ws_bytes(B, L), dtype=torch.uint8, device="cuda")
    ops.occ_sort(items, L, layout, n_rows, sp, ws)                  # existing code: the yardstick
    ops.sasrec_occ_segsum(ws, dx0, out, coef, n_rows, sp, 1.0)
    nu = sp.count()
    blk = torch.full((n_rows, D), float("nan"), device="cuda")
    d = ops.seq_occ_dense_grad(items, layout, dx0, out, coef, n_rows, d_rows=blk)
    assert d.data_ptr() == blk.data_ptr()
    want = torch.zeros(n_rows, D, device="cuda")
    want[sp.idx[:nu]] = sp.rows[:nu]
    assert torch.equal(_bits(d), _bits(want))                      # the sparse route's rows, bit for bit, and +0.0 elsewhere
    ids = torch.cat(_planes(items, L, layout))                      # [3 B L] in occurrence order: inputs | targets | negatives
    live = ids[(ids > 0) & (ids < n_rows)]
    referenced = torch.zeros(n_rows, dtype=torch.bool, device="cuda")
    referenced[live] = True
    assert sorted(set(live.tolist())) == sp.idx[:nu].tolist()
    assert not bool(referenced[0]) and int(_bits(d[~referenced]).abs().max()) == 0        # +0.0 where a NaN stood before the call
    assert not bool(referenced[n_rows - 1])
    # float64: (k + 2) 2^-24 sum|terms| with k the occurrences of the row (one rounding more for the product coef * out)
    co = (coef.double().view(-1, 1) * out.double().view(-1, D))
    terms = torch.cat((dx0.double().view(-1, D), co, -co))
    keep = ((ids > 0) & (ids < n_rows)).double()[:, None]
    safe = ids.clamp(0, n_rows - 1)
    z = lambda: torch.zeros(n_rows, D, dtype=torch.float64, device="cuda")
    d64, dabs = z().index_add_(0, safe, terms * keep), z().index_add_(0, safe, terms.abs() * keep)
    k = torch.zeros(n_rows, dtype=torch.float64, device="cuda").index_add_(0, safe, keep[:, 0])
    over = (d.double() - d64).abs() - (k[:, None] + 2) * U32 * dabs
    print("dense vs float64: worst", float((d.double() - d64).abs().max()), "largest segment", int(k.max()))
    assert float(over.max()) <= 0, float((d.double() - d64).abs().max())
    blk2 = torch.full((n_rows, D), float("nan"), device="cuda")
    assert torch.equal(_bits(ops.seq_occ_dense_grad(items, layout, dx0, out, coef, n_rows, d_rows=blk2)), _bits(d))   # twice: same bits
    return d, k


def _check_with_bad_ids(items, L, layout, dx0, out, coef, n_rows):
    """A clean call leaves the status word clear; two ids outside [0, n_rows) are dropped, move only the rows they had pointed at and
    raise IndexError through the status word."""
    ops.raise_on_bad_indices()
    d, k = _check_seq_dense(items, L, layout, dx0, out, coef, n_rows)
    ops.raise_on_bad_indices()                                      # clean: the word is clear
    if 3 * out.shape[0] * L < 18:
        return d, k
    bad = items.clone()
    p_in, p_neg = layout[1] + L // 2, layout[3] + L - 1             # one input position, one negative position of the first sequence
    reads = lambda buf, pos: [int(buf[0, pos])] if any(off <= pos < off + L for off in layout[1:]) else []
    touched = set(reads(bad, p_in) + reads(bad, p_neg))
    bad[0, p_in], bad[0, p_neg] = n_rows, -3
    d2, _ = _check_seq_dense(bad, L, layout, dx0, out, coef, n_rows)
    with pytest.raises(IndexError):
        ops.raise_on_bad_indices()
    same = torch.tensor([r not in touched for r in range(n_rows)], device="cuda")
    assert torch.equal(_bits(d2[same]), _bits(d[same]))
    return d, k


@pytest.mark.parametrize("B,L,D,n_rows", [(1, 1, 4, 3), (3, 5, 8, 12), (4, 6, 260, 20), (2, 3, 4096, 8), (2, 3, 2052, 8), (24, 40, 64, 6)])
def test_dense_sink_equals_the_sparse_route_scattered(B, L, D, n_rows):
    """pxr_seq_occ_dense_f32 against pxr_seq_occ_sort + pxr_sasrec_occ_segsum (scale 1) on the same input: the same keys, the same
    sort and the same segsum_body<MODE_SASREC> in the same order, so the dense block IS zeros with the sparse rows scattered in --
    derived, not measured -- and rows nobody reads (row 0 too) are +0.0 although the block held NaN before the call.  D = 260: a row
    ends inside a 64-lane chunk; 4096 and 2052: the one-row-per-workgroup path and just past its threshold; (24, 40, 64, 6): every
    live row has more than SEG_CHUNK occurrences.  Against float64 each entry is within (k + 2) 2^-24 sum|terms|."""
    layout = _layouts(L)["bert4rec"]
    long_rows = (B, L, D, n_rows) == (24, 40, 64, 6)
    case = _occ_case(B, L, D, n_rows, layout, 100 * B + D, p_zero=0.02 if long_rows else 0.15, p_mask=0.8 if n_rows == 12 else 0.0)
    d, k = _check_with_bad_ids(case[0], L, layout, *case[1:], n_rows)
    if long_rows:
        _, seg_short, seg_chunk = _sort_constants()
        assert seg_chunk > seg_short and int(k[1:n_rows - 1].min()) > seg_chunk
    if n_rows == 12:
        ins = case[0][:, :L]
        assert int((ins == 1).sum()) > ins.numel() // 2 and int((case[0] == 0).sum()) > 0      # the mask row most inputs read; padding


@pytest.mark.parametrize("name", ["bert4rec", "sasrec", "lightsans"])
def test_dense_sink_under_every_id_layout(name):
    """The (3, 5, 8, 12) case under BERT4Rec's aligned planes (3L, 0, L, 2L), SASRec's shifted windows (2(L+1), 0, 1, L+2) and
    LightSANs' rows (L+2, 0, 1, 2): the entry takes the layout as arguments, as pxr_seq_occ_sort does."""
    B, L, D, n_rows = 3, 5, 8, 12
    layout = _layouts(L)[name]
    case = _occ_case(B, L, D, n_rows, layout, 77, p_mask=0.8)
    _check_with_bad_ids(case[0], L, layout, *case[1:], n_rows)
    if name == "sasrec":                                            # layout=None means SASRec's windows, here as in occ_sort
        items, dx0, out, coef = (t.cuda() for t in case)
        a = ops.seq_occ_dense_grad(items, None, dx0, out, coef, n_rows)
        assert torch.equal(_bits(a), _bits(ops.seq_occ_dense_grad(items, layout, dx0, out, coef, n_rows)))


def test_dense_sink_above_the_fused_sort_cut_over():
    """3 B L just above FP_MAX_N: the multi-launch radix sort, whose ping-pong buffers the entry hands over in another order (the
    unique-row list lives in the free pair).  About 50 rows share the occurrences, so every segment is longer than SEG_CHUNK too."""
    fp_max_n, seg_short, seg_chunk = _sort_constants()
    L, D, n_rows = 16, 64, 52
    B = fp_max_n // (3 * L) + 1
    assert fp_max_n < 3 * B * L <= fp_max_n + 3 * L and 2 * B * L * D * 4 < 40e6
    layout = _layouts(L)["bert4rec"]
    case = _occ_case(B, L, D, n_rows, layout, 5)
    d, k = _check_with_bad_ids(case[0], L, layout, *case[1:], n_rows)
    assert int(k[1:n_rows - 1].min()) > seg_chunk > seg_short


def test_dense_sink_refuses_what_it_cannot_serve():
    from pixelrec_amd.lib import PxrError

    B, L, D = 2, 3, 8
    layout = _layouts(L)["bert4rec"]
    items, dx0, out, coef = (t.cuda() for t in _occ_case(B, L, D, B * L, layout, 1))
    ops.seq_occ_dense_grad(items, layout, dx0, out, coef, B * L)
    with pytest.raises(PxrError):
        ops.seq_occ_dense_grad(items, layout, dx0, out, coef, B * L, d_rows=dx0.view(B * L, D))     # d_rows must not alias dx0
    with pytest.raises(PxrError):
        ops.seq_occ_dense_grad(items, layout, dx0, out, coef, B * L, d_rows=out.view(B * L, D))     # ... nor out
    z6 = torch.zeros(B, L, 6, device="cuda")
    with pytest.raises(PxrError):
        ops.seq_occ_dense_grad(items, layout, z6, z6.clone(), coef, 5)                              # D % 4
    with pytest.raises(PxrError):
        ops.seq_occ_dense_grad(items, (3 * L, 0, L, 2 * L + 1), dx0, out, coef, 5)                  # the negatives leave id_bstride
    with pytest.raises(PxrError):
        ops.seq_occ_dense_grad(items, layout, dx0, out, coef, 5, ws=torch.empty(16, dtype=torch.uint8, device="cuda"))
    ops.raise_on_bad_indices()


# ------------------------------------------------------------------------------------------------------------ 4. the head alone
HEAD = dict(B=5, L=8, D=32, M=23)


def _tiny_model(D=32, L=8, seed=0, p_drop=0.0):
    import pixelrec_amd.model as M

    class DL:
        item_num = 13

    torch.manual_seed(seed)
    m = M.MOBERT4Rec(_config(D, L, 37, p_drop=p_drop), DL())
    with torch.no_grad():                                           # biases and LayerNorm affine off their initial (0, 1)
        for n, p in m.named_parameters():
            if "visual_encoder" not in n and p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return m.cuda().train()


def _block(m, dtype):
    return {k: m.get_parameter(k).detach().to(dtype).clone() for k in R.names(m.n_layers)}


def _edge_batch(B, P, M, seed):
    """The fixture's edge rows over a batch-local row space: item rows in [2, M - 1) -- row M - 1 is listed and read by nobody --,
    row 1 the mask row, 0 padding: a full window, windows with one, two and three padded positions, a window with every real position
    masked and one with none; negatives outside their own sequence; items shared between samples."""
    rng = np.random.default_rng(seed)
    rows = np.arange(2, M - 1)
    index = np.zeros((B, 3, P), dtype=np.int64)
    masked = np.zeros((B, P), dtype=np.int64)
    for b in range(B):
        n = P - (b % 4)
        s = rng.choice(rows, size=n, replace=False)
        mk = rng.random(n) < 0.6
        if b == 3:
            mk[:] = True
        elif b == 4:
            mk[:] = False
        elif not mk.any() or mk.all():
            mk[0], mk[-1] = True, False
        neg = np.where(mk, rng.choice(rows[~np.isin(rows, s)], size=n), 0)
        index[b, 0, P - n:] = np.where(mk, 1, s)
        index[b, 1, P - n:] = s
        index[b, 2, P - n:] = neg
        masked[b, P - n:] = mk
    return torch.from_numpy(index), torch.from_numpy(masked)


def _head_case(seed=0):
    B, L, D, M = (HEAD[k] for k in ("B", "L", "D", "M"))
    m = _tiny_model(D, L, seed)
    index, masked = _edge_batch(B, L + 1, M, 7)
    E = (torch.randn(M, D, generator=torch.Generator().manual_seed(3)) * 0.5).cuda()
    return m, index.cuda(), masked.cuda(), E


def _cfg(m):
    return {"n_layers": m.n_layers, "n_heads": m.n_heads, "layer_norm_eps": 1e-12, "hidden_act": "gelu"}


def _block_grads(m):
    return {k: m.get_parameter(k).grad.detach().clone() for k in R.names(m.n_layers)}


@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_head_without_the_tower_matches_float64(mode):
    """loss_from_embeddings on a random leaf E [23, 32] (B = 5, L = 8, 2 heads, 2 layers, dropout 0, the fixture's edge rows) against
    mobert4rec_restate in float64 on the same device, within tests/test_gpu_bert4rec.py's budgets for the same block: loss
    2e-5 max(1, |L64|), dE 3e-6 + 1e-4 max|g64|, block parameters 5e-6 + 2e-4 max|g64|; in every GEMM mode of that file.  Rows of E
    nobody reads get exactly zero; the no_grad call gives the same loss bits; a detached E still drives the block's backward."""
    m, index, masked, E = _head_case()
    M = E.shape[0]
    L64, g64 = R.loss_and_grads(_block(m, torch.float64), E.double(), index, masked, _cfg(m))
    E = E.requires_grad_(True)
    loss = m.loss_from_embeddings(E, index, masked)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    ops.raise_on_bad_indices()
    print(mode, "loss", float(loss.detach()), L64, "err", abs(float(loss.detach()) - L64))
    assert abs(float(loss.detach()) - L64) <= 2e-5 * max(1.0, abs(L64))
    got = _block_grads(m)
    for k in R.names(m.n_layers):
        err, big = float((got[k].double() - g64[k]).abs().max()), float(g64[k].abs().max())
        print(mode, "grad", k, "err", err, "budget", 5e-6 + 2e-4 * big)
        assert err <= 5e-6 + 2e-4 * big, k
    err, big = float((E.grad.double() - g64[R.E_KEY]).abs().max()), float(g64[R.E_KEY].abs().max())
    print(mode, "dE err", err, "budget", 3e-6 + 1e-4 * big)
    assert E.grad.shape == E.shape and err <= 3e-6 + 1e-4 * big
    read = torch.zeros(M, dtype=torch.bool, device="cuda")
    read[index.view(-1)] = True
    read[0] = False
    assert not bool(read[M - 1]) and int(_bits(E.grad[~read]).abs().max()) == 0 and float(E.grad[read].abs().max()) > 0
    with torch.no_grad():
        again = m.loss_from_embeddings(E.detach(), index, masked)
    assert not again.requires_grad and torch.equal(_bits(again), _bits(loss.detach()))
    frozen = m.loss_from_embeddings(E.detach(), index, masked)
    assert frozen.requires_grad
    frozen.backward()
    for k, v in _block_grads(m).items():                            # the same step again: the same block gradients
        assert torch.equal(_bits(v), _bits(got[k])), k


def test_bad_position_raises_index_error():
    m, index, masked, E = _head_case()
    ops.raise_on_bad_indices()
    for plane, val in ((0, E.shape[0]), (1, E.shape[0]), (2, -2)):
        bad = index.clone()
        bad[3, plane, -1] = val                                     # sample 3: every real position is masked, so all planes are read
        m.loss_from_embeddings(E.clone().requires_grad_(True), bad, masked).backward()
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices()
    m.loss_from_embeddings(E.clone().requires_grad_(True), index, masked).backward()
    ops.raise_on_bad_indices()                                      # a clean batch leaves the word clear


# ------------------------------------------------------------------------------------------------------------ 5. padding is inert
def test_padding_is_inert():
    """The reference feeds the ones image at padded input positions; here they hold position 0.  Let row 0 hold what row 1 (the mask
    image's encoding) holds, so that padded positions read the reference's values under the same key mask: the same loss bits, the
    same bits in every block gradient and in every gradient row that was referenced before, and still exactly nothing for row 0.
    (Replacing the INDEX 0 by 1 would also turn the padded positions into real keys -- the key mask is index != 0 -- which is
    another function, not the reference's.)"""
    m, index, masked, E = _head_case()
    assert int((index[:, 0] == 0).sum()) > 0
    runs = []
    for Ei in (E, torch.cat((E[1:2], E[1:]))):
        Ei = Ei.clone().requires_grad_(True)
        loss = m.loss_from_embeddings(Ei, index, masked)
        loss.backward()
        runs.append((loss.detach().clone(), Ei.grad.clone(), _block_grads(m)))
    ops.raise_on_bad_indices()
    (l0, e0, b0), (l1, e1, b1) = runs
    assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(_bits(e0), _bits(e1)) and int(_bits(e1[0]).abs().max()) == 0
    for k in b0:
        assert torch.equal(_bits(b0[k]), _bits(b1[k])), k


# ------------------------------------------------------------------------------------------------------------ 6. the dedup
def test_dedup_does_not_change_the_function():
    """One row per position (the reference-form mapping on E's rows: E_x[1 + 3 (b P + t) + k] = E[index[b, k, t]]) against the
    batch-wide dedup: the same loss bits; dE[r] is the sum of its copies' gradients, in float64 within (k + 1) 2^-24 sum|terms|."""
    m, index, masked, E = _head_case()
    M, D = E.shape
    E = E.requires_grad_(True)
    loss = m.loss_from_embeddings(E, index, masked)
    loss.backward()
    flat = index.permute(0, 2, 1).reshape(-1)                       # (b, t, k) order
    Ex = torch.cat((E.detach()[:1], E.detach()[flat])).requires_grad_(True)
    pos = m.reference_positions(index[:, 0], masked)
    assert torch.equal(pos.cpu(), R.reference_positions(index[:, 0].cpu(), masked.cpu()))
    loss_x = m.loss_from_embeddings(Ex, pos, masked)
    loss_x.backward()
    ops.raise_on_bad_indices()
    assert torch.equal(_bits(loss_x.detach()), _bits(loss.detach()))
    terms = Ex.grad[1:].double()
    used = (pos.permute(0, 2, 1).reshape(-1) != 0) & (flat != 0)
    keep = used.double()[:, None]
    z = lambda: torch.zeros(M, D, dtype=torch.float64, device="cuda")
    d64, dabs = z().index_add_(0, flat, terms * keep), z().index_add_(0, flat, terms.abs() * keep)
    k = torch.zeros(M, dtype=torch.float64, device="cuda").index_add_(0, flat, keep[:, 0])
    over = (E.grad.double() - d64).abs() - (k[:, None] + 1) * U32 * dabs
    print("dE against the summed copies", float((E.grad.double() - d64).abs().max()), "most copies", int(k.max()))
    assert float(over.max()) <= 0 and float(Ex.grad[0].abs().max()) == 0 and int(k.max()) > 8
    assert float(Ex.grad[1:][~used].abs().max()) == 0               # copies the mapping does not point at receive nothing


# ------------------------------------------------------------------------------------------------------------ 7. BERT4Rec's launches
def test_loss_and_gradients_are_bert4recs_bit_for_bit():
    """A BERT4Rec with item_num + 1 = M whose table is E and whose block weights are the model's, on the same [B, 3, P] rows, at
    dropout 0, on the first step of a fresh model: both go through the same launches, so the loss, the 35 block gradients and the
    sparse table-gradient rows against dE are bit-identical."""
    from pixelrec_amd.model import BERT4Rec

    m, index, masked, E = _head_case()
    M = E.shape[0]

    class DL:
        item_num = M - 1

    cfg = {k: v for k, v in _config(HEAD["D"], HEAD["L"], 37).items() if not k.startswith(("encoder_", "fine_tune", "pretrain"))}
    bert = BERT4Rec(cfg, DL())
    bert.load_state_dict({"item_embedding.weight": E.detach().cpu(), **{k: v.cpu() for k, v in _block(m, torch.float32).items()}}, strict=True)
    bert = bert.cuda().train()
    E = E.requires_grad_(True)
    loss = m.loss_from_embeddings(E, index, masked)
    loss.backward()
    loss_b = bert((index, masked))
    loss_b.backward()
    ops.raise_on_bad_indices()
    assert torch.equal(_bits(loss.detach()), _bits(loss_b.detach()))
    for k in R.names(m.n_layers):
        a, b = m.get_parameter(k).grad, bert.get_parameter(k).grad
        assert (float(a.abs().max()) > 0 or ".key.bias" in k) and torch.equal(_bits(a), _bits(b)), k
    sp = bert.sparse_table_grad
    assert torch.equal(_bits(sp.to_dense(M)), _bits(E.grad)) and sp.count() > 2


# ------------------------------------------------------------------------------------------------------------ 8. the fixture
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "mobert4rec_tiny.npz"))


class _Store:
    """ImageStore's surface over the fixture's normalised images."""

    def __init__(self, images):
        self.images = images

    def batch(self, ids):
        return self.images[ids]


def _inputs(m, g, j, store, form):
    items, masked = g[f"b{j}.items"], torch.from_numpy(g[f"b{j}.masked_index"]).cuda()
    I = int(g["meta"][0])
    if form == "positions":                                         # what MoBert4RecTrainBatcher.make_batch builds, then modal_inputs
        from pixelrec_amd.data.dataset import positions_into_distinct_images_masked

        index, image_ids = positions_into_distinct_images_masked(items, I)
        return m.modal_inputs(_Store(store), (torch.from_numpy(index).cuda(), masked, torch.from_numpy(image_ids).cuda()))
    # mobert4rec.py:79 with MOBERT4RecTrainDataset's images: (input, positive, negative) per position; the ones image at mask and
    # padded input positions, the zero image (store row 0) at ids 0 of the other two planes
    it = torch.from_numpy(items).cuda()
    ones = torch.ones_like(store[:1])
    ext = torch.cat((store, ones))                                  # row I: the ones image
    inp = torch.where(it[:, 0] == 0, torch.full_like(it[:, 0], I), it[:, 0])
    modal = torch.stack((ext[inp], ext[it[:, 1]], ext[it[:, 2]]), dim=2).flatten(1, 2)      # [B, 3 P, 3, H, W]
    return it[:, 0].contiguous(), modal, masked


def _step(m, g, j, store, form):
    loss = m(_inputs(m, g, j, store, form))
    loss.backward()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad and p.grad is not None}


@pytest.mark.parametrize("form", ["positions", "reference"])
def test_model_matches_the_reference_fixture(gold, form):
    """Loss, all 53 gradients, compute_item including the mask row and predict against the stored results of the reference's
    MOBERT4Rec, with the batch in the batcher's form and in the reference's 5-D form.  Budgets: the project's recorded ones for this
    tiny tower -- loss 3e-5 max(1, |loss|), block gradients 5e-6 + 3e-4 max|g|, encoder gradients 5e-6 + 5e-4 max|g|, item features
    3e-5, scores 1e-4 -- each plus the quantity's stored ref_err.  Then the generic fused path: encode_last + score_topk on
    scoring_item_matrix() with history masks returns the ids of predict + masks + topk and never the mask row's id."""
    g = gold
    I = int(g["meta"][0])
    m = build_from_fixture(g).cuda().train()
    store = R.golden_store(g).cuda()
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
            rel = 5e-4 if k.startswith("visual_encoder.") else 3e-4
            budget = 5e-6 + rel * float(want.abs().max()) + float(g[f"ref_err.b{j}.grad." + k])
            print(form, "batch", j, "grad", k, err, "budget", budget)
            assert err <= budget, (k, err)
        assert len(names) == len(grads) == N_BLOCK + 18
    m.eval()
    feat = m.compute_item(torch.cat((store, m.extra_item_images(*store.shape[2:], "cuda"))))
    err = float((feat.cpu() - torch.from_numpy(g["eval.item_feature"])).abs().max())
    print("item features", err, "budget", 3e-5 + float(g["ref_err.item_feature"]))
    assert tuple(feat.shape) == (I + 1, int(g["meta"][1])) and err <= 3e-5 + float(g["ref_err.item_feature"])
    win = torch.from_numpy(g["eval.windows"]).cuda()
    scores = m.predict(win, feat)
    err = float((scores.cpu() - torch.from_numpy(g["eval.scores"])).abs().max())
    print("scores", err, "budget", 1e-4 + float(g["ref_err.scores"]))
    assert tuple(scores.shape) == (len(win), I) and err <= 1e-4 + float(g["ref_err.scores"])
    # the generic fused path (Trainer._full_sort_batch_topk) against predict + masks + topk
    K, Bw = 5, len(win)
    hist = [sorted(set(w[w != 0].tolist())) for w in g["eval.windows"]]
    hu = torch.tensor([b for b in range(Bw) for _ in hist[b]], dtype=torch.int64)
    hi = torch.tensor([i for b in range(Bw) for i in hist[b]], dtype=torch.int64)
    ptr, hitems = ops.history_csr(hu, hi, Bw, "cuda")
    m.set_item_feature(feat)
    sm = m.scoring_item_matrix()
    assert tuple(sm.shape) == (I, feat.shape[1]) and sm.is_contiguous()
    out, last = m.encode_last(win, feat)
    idx, _ = ops.score_topk(last, last.stride(0), Bw, sm, K, ptr, hitems)
    ops.raise_on_bad_indices()
    s = scores.clone()
    s[:, 0] = float("-inf")
    for b, h in enumerate(hist):
        s[b, torch.tensor(h, device="cuda")] = float("-inf")
    assert torch.equal(idx, torch.topk(s, K, dim=-1).indices) and int(idx.max()) < I and int(idx.min()) >= 1
    with pytest.raises(ValueError):
        m.encode_last(win, feat[:I].contiguous())                   # a matrix without the mask row


def test_two_fresh_models_give_the_same_bits(gold):
    store = R.golden_store(gold).cuda()
    assert_two_fresh_models_agree(lambda: build_from_fixture(gold).cuda().train(), lambda m, j: _step(m, gold, j, store, "positions"),
                                  1 + N_BLOCK + 18)


# ------------------------------------------------------------------------------------------------------------ 10. dropout
def test_dropout_runs_reproducibly_and_draws_fresh_masks(gold):
    """At 0.1 the step runs; two models with the same seed give the same loss bits; the second step's loss (the same batch, the
    weights untouched) differs from the first: the masks are a function of the step counter."""
    store = R.golden_store(gold).cuda()
    losses = []
    for _ in range(2):
        m = build_from_fixture(gold, p_drop=0.1).cuda().train()
        seq = []
        for _step_no in range(2):
            loss, grads = _step(m, gold, 0, store, "positions")
            assert np.isfinite(float(loss)) and all(bool(torch.isfinite(v).all()) for v in grads.values())
            seq.append(loss)
        losses.append(seq)
    ops.raise_on_bad_indices()
    assert torch.equal(_bits(losses[0][0]), _bits(losses[1][0])) and torch.equal(_bits(losses[0][1]), _bits(losses[1][1]))
    assert float(losses[0][0]) != float(losses[0][1])
    quiet = build_from_fixture(gold).cuda().train()
    assert float(_step(quiet, gold, 0, store, "positions")[0]) != float(losses[0][0])


# ------------------------------------------------------------------------------------------------------------ optimizer, end to end
def test_optimizer_steps_both_groups_and_its_state_round_trips(gold):
    """Four optim_args: the encoder group and a rec group without a table, [18, 35] parameters; one step moves both; the torch-layout
    state loads into torch.optim.AdamW over the reference's two groups and back."""
    store = R.golden_store(gold).cuda()
    blk = R.names(2)

    def moved(moved, trainable):
        # (a key projection's bias has a zero gradient by the softmax's shift invariance: it may stay where it is)
        assert moved <= trainable and {k for k in blk if ".key.bias" not in k} <= moved and any("visual_encoder" in k for k in moved)

    assert_optimizer_state_round_trips(lambda: build_from_fixture(gold).cuda().train(), lambda m: _step(m, gold, 0, store, "positions"),
                                       [18, N_BLOCK], list(range(18 + N_BLOCK)), moved=moved,
                                       rec=lambda m: [m.get_parameter(k) for k in blk])     # the reference's registration order


def test_main_py_trains_evaluates_and_the_checkpoint_reloads(tmp_path):
    """main.py on TinyInter with synthetic 64 x 64 images and the tiny tower, two epochs at mask_ratio 0.6, through the fused
    evaluation: finite losses that change, Recall@10 and NDCG@10 reported from the reloaded checkpoint, whose state_dict loads with
    strict=True."""
    from pixelrec_amd.utils import get_model

    _, _, ck, config, data = run_main_py(
        tmp_path, "model: MOBERT4Rec\nembedding_size: 32\nn_layers: 2\nn_heads: 2\ninner_size: 2\nhidden_dropout_prob: 0.1\n"
                  "attn_dropout_prob: 0.1\nhidden_act: 'gelu'\nlayer_norm_eps: 1e-12\ninitializer_range: 0.02\nmask_ratio: 0.6\n")
    assert list(ck["state_dict"])[-N_BLOCK:] == R.names(2)
    assert [len(x["params"]) for x in ck["optimizer"]["param_groups"]] == [18, N_BLOCK]    # the reference's two groups
    fresh = get_model("MOBERT4Rec")(config, data)
    fresh.load_state_dict(ck["state_dict"], strict=True)
