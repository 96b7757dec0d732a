"""The BPR loss head (csrc/bpr_loss.hip; fused into the last LayerNorm in csrc/layernorm.hip) against a float64 restatement of the
reference's formulas (sasrec.py:88-92):
    pos = <out, E[target]>,  neg = <out, E[negative]>,  loss = mean_b( -sum_t log(sigmoid(pos - neg) + 1e-8) * mask[b,t] )
and autograd's coefficient d loss / d(pos - neg) = -(mask/B) * s(1-s)/(s+1e-8) * upstream, d out = coef * (E[target] - E[negative]);
in both id layouts (SASRec's shifted [B, 2, L+1] windows, BERT4Rec's aligned [B, 3, L] planes), through sigmoid saturation both ways.
Then the fused entries against the unfused pair, bit for bit, and ids outside the table raising IndexError like nn.Embedding does.

Tolerances come from fp32 rounding: U = 8 unit roundoffs per elementwise step, U * sqrt(D) * sum|products| for a dot product."""
import math

import numpy as np
import pytest
import torch

from oracle import sasrec_oracle as O

pytestmark = pytest.mark.gpu

U = 8 * 2.0 ** -24
N_TABLE = 211
GAPS = (0.0, 5.0, 20.0, 40.0, 100.0)


def _close(got, ref, tol, what):
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} beyond tolerance; at {i}: got {got[i].item()!r}, "
                             f"fp64 {ref[i].item()!r}, tol {tol[i].item()!r}")


def _layout(kind, L):
    """(items shape, layout argument of ops, (id_bstride, pos_off, neg_off))"""
    if kind == "sasrec":
        return (2, L + 1), None, (2 * (L + 1), 1, L + 2)
    return (3, L), (3 * L, L, 2 * L), (3 * L, L, 2 * L)


def _ids(items, lay, L):
    B = items.shape[0]
    flat = items.reshape(B, -1)
    bs, po, no = lay
    return flat[:, po:po + L], flat[:, no:no + L]


def _case(kind, B, L, D, seed, gap=None):
    """(out [B,L,D], table, items, mask) with pos - neg near +-GAPS (or near `gap` [B, L]), a mask with zeros and (B > 1) an
    all-zero row."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(seed)
    shape, layout, lay = _layout(kind, L)
    table = torch.randn(N_TABLE, D, device=dev, generator=g, dtype=torch.float64) / math.sqrt(D)
    items = torch.randint(1, N_TABLE, (B, *shape), device=dev, generator=g)
    pid, nid = _ids(items, lay, L)
    dvec = table[pid] - table[nid]                                   # [B, L, D]
    o = torch.randn(B, L, D, device=dev, generator=g, dtype=torch.float64)
    if gap is None:
        gap = torch.tensor(GAPS, device=dev, dtype=torch.float64)[torch.randint(0, len(GAPS), (B, L), device=dev, generator=g)]
        gap = gap * (torch.randint(0, 2, (B, L), device=dev, generator=g) * 2 - 1)
    nrm = (dvec * dvec).sum(-1, keepdim=True).clamp_min(1e-30)
    o = o - (o * dvec).sum(-1, keepdim=True) / nrm * dvec + gap[..., None] / nrm * dvec    # <o, E[pos] - E[neg]> = gap
    nid_eq = pid == nid
    o[nid_eq] = o[nid_eq] * 0.1                                       # (same row twice: x = 0 whatever o is)
    mask = (torch.rand(B, L, device=dev, generator=g) < 0.7).long()
    if B > 1:
        mask[1] = 0
    return o.float().contiguous(), table.float().contiguous(), items, mask, layout, lay


def _loss64(pos, neg, mask, B):
    x = pos - neg
    term = -torch.log(torch.sigmoid(x) + 1e-8) * mask.double()
    return term.sum() / B, term


def _coef64(pos, neg, mask, B, scale):
    x = pos.double() - neg.double()
    s = torch.sigmoid(x)
    return -(mask.double() / B) * (s * (1 - s)) / (s + 1e-8) * scale, x


@pytest.mark.parametrize("kind", ("sasrec", "bert4rec"))
@pytest.mark.parametrize("D", (4, 68, 512, 1028))
def test_bpr_loss_fwd_bwd_match_fp64(kind, D):
    from pixelrec_amd import ops

    for B in (1, 300):
        for L in (1, 50):
            out, table, items, mask, layout, lay = _case(kind, B, L, D, seed=D * 1000 + B + L)
            what = f"{kind} B={B} L={L} D={D}"
            loss, pos, neg = ops.bpr_loss_fwd(out, table, items, mask, layout=layout)
            pid, nid = _ids(items, lay, L)
            o64, t64 = out.double(), table.double()
            pp, nn_ = o64 * t64[pid], o64 * t64[nid]
            pos_ref, neg_ref = pp.sum(-1), nn_.sum(-1)
            t_pos = U * math.sqrt(D) * pp.abs().sum(-1)
            t_neg = U * math.sqrt(D) * nn_.abs().sum(-1)
            _close(pos, pos_ref, t_pos, f"{what} pos")
            _close(neg, neg_ref, t_neg, f"{what} neg")
            loss_ref, term = _loss64(pos_ref, neg_ref, mask, B)
            # |d term / dx| <= 1; each term one expf / logf (U); the sum in L + 8 levels of fp32 adds
            t_loss = ((t_pos + t_neg) * mask + U * term.abs()).sum() / B + (L + 16) * 2.0 ** -24 * term.abs().sum() / B
            _close(loss, loss_ref.view(1), t_loss.view(1), f"{what} loss")
            for gs, gsd in ((1.0, None), (0.37, torch.tensor([2.5], device="cuda"))):
                dout, coef = ops.bpr_loss_bwd(pos, neg, table, items, mask, D, gs, gsd, layout=layout)
                scale = gs * (2.5 if gsd is not None else 1.0)
                cref, x = _coef64(pos, neg, mask, B, scale)
                # from the given fp32 scores: x = pos - neg rounds (U |x|), |d coef / dx| <= 1/2 * |mask/B * scale|, expf / divisions U
                t_coef = (mask.double() / B) * abs(scale) * U * (2.0 + x.abs()) + U * cref.abs()
                assert bool(torch.isfinite(coef).all())
                _close(coef, cref, t_coef, f"{what} gs={gs} gsd={gsd is not None} coef")
                dvec = t64[pid] - t64[nid]
                _close(dout, cref[..., None] * dvec, t_coef[..., None] * dvec.abs() + 2 * U * (cref[..., None] * dvec).abs(),
                       f"{what} gs={gs} gsd={gsd is not None} dout")
    ops.raise_on_bad_indices("cuda")


@pytest.mark.parametrize("kind", ("sasrec", "bert4rec"))
def test_bpr_loss_saturation_edges(kind):
    """One position per launch at pos - neg = +-{0, 5, 20, 40, 100}: sigmoid underflows to 0 below about -88 and rounds to 1 above
    about 17 in fp32.  At the bottom the loss is -log(1e-8) (the +1e-8 term), at the top the coefficient is 0 to within rounding, and
    in between both follow the formula; the coefficient is finite everywhere."""
    from pixelrec_amd import ops

    D = 68
    for v in sorted({s * g for g in GAPS for s in (-1.0, 1.0)}):
        out, table, items, mask, layout, lay = _case(kind, 1, 1, D, seed=17, gap=torch.full((1, 1), v, device="cuda",
                                                                                          dtype=torch.float64))
        mask.fill_(1)
        loss, pos, neg = ops.bpr_loss_fwd(out, table, items, mask, layout=layout)
        x = float(pos) - float(neg)
        assert abs(x - v) <= 1e-4 * (1 + abs(v)), (v, x)
        ref = -math.log(1.0 / (1.0 + math.exp(-x)) + 1e-8)
        assert abs(float(loss) - ref) <= U * (1 + abs(ref)), (v, float(loss), ref)
        if v <= -40:
            assert abs(float(loss) - (-math.log(1e-8))) <= 4 * 2.0 ** -24 * 18.5, (v, float(loss))
        _, coef = ops.bpr_loss_bwd(pos, neg, table, items, mask, D, 1.0, None, layout=layout)
        s = 1.0 / (1.0 + math.exp(-x))
        cref = -(s * (1 - s)) / (s + 1e-8)
        c = float(coef)
        assert math.isfinite(c) and abs(c - cref) <= U * (2.0 + abs(x)) + U * abs(cref), (v, c, cref)


# ---- fused == unfused ----------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), f"{what}: fused and unfused differ in {int((_bits(a) != _bits(b)).sum())} elements"


@pytest.mark.parametrize("kind", ("sasrec", "bert4rec"))
@pytest.mark.parametrize("p", (0.0, 0.1))
def test_fused_head_is_bit_identical_to_unfused(kind, p):
    """ln_residual_bpr_fwd is ln_residual_fwd + bpr_loss_fwd bit for bit up to D = 1024 (VEC <= 4); beyond, y / xhat / rstd still
    are, and the scores and the loss agree to within the fp32 rounding of the D-term dot product (layernorm.hip's header says why).
    bpr_ln_bwd is bpr_loss_bwd + ln_bwd(0, ...) bit for bit at every D."""
    from pixelrec_amd import ops

    dev = "cuda"
    for (B, L, D) in ((7, 50, 64), (300, 1, 512), (3, 13, 768), (3, 13, 1028), (2, 5, 4096)):
        g = torch.Generator(device=dev).manual_seed(B * L + D)
        x = torch.randn(B, L, D, device=dev, generator=g)
        res = torch.randn(B, L, D, device=dev, generator=g)
        gamma = torch.randn(D, device=dev, generator=g) * 0.5 + 1.0
        beta = torch.randn(D, device=dev, generator=g) * 0.1
        table = torch.randn(N_TABLE, D, device=dev, generator=g) * 0.3
        shape, layout, _ = _layout(kind, L)
        items = torch.randint(0, N_TABLE, (B, *shape), device=dev, generator=g)
        mask = (torch.rand(B, L, device=dev, generator=g) < 0.7).long()
        what = f"{kind} p={p} B={B} L={L} D={D}"
        fy, fxh, frs, floss, fpos, fneg = ops.ln_residual_bpr_fwd(x, res, gamma, beta, 1e-12, table, items, mask, p, 21, 4, layout=layout)
        uy, uxh, urs = ops.ln_residual_fwd(x, res, gamma, beta, 1e-12, p, 21, 4)
        uloss, upos, uneg = ops.bpr_loss_fwd(uy, table, items, mask, layout=layout)
        for a, b, n in ((fy, uy, "y"), (fxh, uxh, "xhat"), (frs, urs, "rstd")):
            _assert_same(a, b, f"{what} forward {n}")
        if D <= 1024:
            for a, b, n in ((fpos, upos, "pos"), (fneg, uneg, "neg"), (floss, uloss, "loss")):
                _assert_same(a, b, f"{what} forward {n}")
        else:
            pid, nid = _ids(items, _layout(kind, L)[2], L)
            y64, t64 = uy.double(), table.double()
            t_sc = []
            for a, b, ids, n in ((fpos, upos, pid, "pos"), (fneg, uneg, nid, "neg")):
                prod = y64 * t64[ids]
                t_sc.append(U * math.sqrt(D) * prod.abs().sum(-1))
                _close(a, prod.sum(-1), t_sc[-1], f"{what} fused {n}")
                _close(b, prod.sum(-1), t_sc[-1], f"{what} unfused {n}")
            t_loss = ((t_sc[0] + t_sc[1]) * mask).sum() / B * 2 + U * uloss.abs().double()
            _close(floss, uloss.double(), t_loss, f"{what} fused vs unfused loss")
        gsd = torch.tensor([0.75], device=dev)
        fdg, fdb = torch.empty(D, device=dev), torch.empty(D, device=dev)
        fdz, fdx, _, fcoef = ops.bpr_ln_bwd(fpos, fneg, table, items, mask, 1.3, gsd, fxh, frs, gamma, fdg, fdb, p, 33, 6,
                                            need_dx=p > 0, layout=layout)
        dout, ucoef = ops.bpr_loss_bwd(fpos, fneg, table, items, mask, D, 1.3, gsd, layout=layout)   # (the same scores)
        udg, udb = torch.empty(D, device=dev), torch.empty(D, device=dev)
        udz, udx = ops.ln_bwd(0, dout, uxh, urs, gamma, udg, udb, p, 33, 6, need_dx=p > 0)
        pairs = [(fcoef, ucoef, "coef"), (fdz, udz, "dz"), (fdg, udg, "dgamma"), (fdb, udb, "dbeta")]
        if p > 0:
            pairs.append((fdx, udx, "dx"))
        for a, b, n in pairs:
            _assert_same(a, b, f"{what} backward {n}")
    ops.raise_on_bad_indices("cuda")


# ---- ids outside the table ---------------------------------------------------------------------------------------------------------
def _clean_slate():
    from pixelrec_amd import ops

    torch.cuda.synchronize()
    ops.raise_on_bad_indices("cuda")


def test_bpr_loss_fwd_flags_target_and_negative_ids_outside_the_table():
    """nn.Embedding raises on every id of `items` (sasrec.py:68); the head flags the status word (and clamps: nothing faults)."""
    from pixelrec_amd import ops

    B, L, D = 3, 5, 64
    out, table, items, mask, layout, lay = _case("sasrec", B, L, D, seed=5)
    _clean_slate()
    ops.bpr_loss_fwd(out, table, items, mask)
    ops.raise_on_bad_indices("cuda")                                    # in range: nothing flagged
    for (j, k, v) in ((0, L, N_TABLE), (1, 2, N_TABLE + 7), (1, L, -1)):   # last target; a negative; a negative id < 0
        bad = items.clone()
        bad[2, j, k] = v
        ops.bpr_loss_fwd(out, table, bad, mask)
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices("cuda")
    out, table, items, mask, layout, lay = _case("bert4rec", B, L, D, seed=6)
    bad = items.clone()
    bad[1, 1, 3] = N_TABLE                                              # an original (target) id of the aligned layout
    ops.bpr_loss_fwd(out, table, bad, mask, layout=layout)
    with pytest.raises(IndexError):
        ops.raise_on_bad_indices("cuda")


def test_fused_head_flags_ids_outside_the_table():
    from pixelrec_amd import ops

    B, L, D = 4, 6, 128
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(8)
    x, res = torch.randn(B, L, D, device=dev, generator=g), torch.randn(B, L, D, device=dev, generator=g)
    gamma, beta = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    table = torch.randn(N_TABLE, D, device=dev, generator=g)
    items = torch.randint(1, N_TABLE, (B, 2, L + 1), device=dev, generator=g)
    mask = torch.ones(B, L, dtype=torch.long, device=dev)
    _clean_slate()
    ops.ln_residual_bpr_fwd(x, res, gamma, beta, 1e-12, table, items, mask)
    ops.raise_on_bad_indices("cuda")
    for (j, k) in ((0, L), (1, 1)):
        bad = items.clone()
        bad[3, j, k] = N_TABLE
        ops.ln_residual_bpr_fwd(x, res, gamma, beta, 1e-12, table, bad, mask)
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices("cuda")


@pytest.mark.parametrize("B", (5, 500))       # 3*B*L occurrences: the fused sort passes / the multi-launch radix sort
def test_occurrence_sort_flags_ids_outside_the_table(B):
    from pixelrec_amd import ops

    L = 50
    items = torch.randint(1, N_TABLE, (B, 2, L + 1), device="cuda")
    sp = ops.SparseRows(B * (2 * L + 1), 1, "cuda")
    ws = torch.empty(ops.occ_ws_bytes(B, L), dtype=torch.uint8, device="cuda")
    _clean_slate()
    ops.occ_sort(items, L, None, N_TABLE, sp, ws)
    ops.raise_on_bad_indices("cuda")
    bad = items.clone()
    bad[B - 1, 1, L] = N_TABLE
    ops.occ_sort(bad, L, None, N_TABLE, sp, ws)
    with pytest.raises(IndexError):
        ops.raise_on_bad_indices("cuda")


N, DM, LM, H, BM = 300, 64, 8, 2, 5
CFG = {"n_layers": 2, "n_heads": H, "embedding_size": DM, "inner_size": 2, "hidden_dropout_prob": 0.0,
       "attn_dropout_prob": 0.0, "hidden_act": "gelu", "layer_norm_eps": 1e-12, "initializer_range": 0.02,
       "MAX_ITEM_LIST_LENGTH": LM, "seed": 2020}


@pytest.mark.parametrize("fused", ("1", "0"))
def test_sasrec_step_raises_on_target_or_negative_outside_the_catalogue(fused, monkeypatch):
    """items[b, 0, L] (the last target) and items[b, 1, t+1] (a negative) are read by no input gather; the reference embeds them
    (sasrec.py:68) and raises.  (items[b, 1, 0] is read by no kernel here: not checked, see ops._sasrec_layout.)"""
    from pixelrec_amd import synth
    from pixelrec_amd.model import SASRec

    monkeypatch.setenv("PXR_FUSED_HEAD", fused)

    class DL:
        item_num = N

    m = SASRec(CFG, DL())
    m.load_state_dict(O.synth_params(N, DM, LM, 2, 2, seed=3), strict=True)
    m = m.cuda().train()
    rng = np.random.default_rng(4)
    items, mask = (torch.from_numpy(a).cuda() for a in synth.train_batch(N, BM, LM, rng, synth.ZipfItems(N, seed=4)))
    _clean_slate()
    m((items, mask)).backward()
    torch.cuda.synchronize()
    from pixelrec_amd import ops

    ops.raise_on_bad_indices("cuda")                                    # a clean batch: nothing flagged
    for (j, k) in ((0, LM), (1, 4)):
        bad = items.clone()
        bad[2, j, k] = N
        m((bad, mask)).backward()
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices("cuda")


def test_bert4rec_step_raises_on_masked_original_id_outside_the_table():
    import os

    from pixelrec_amd import ops
    from pixelrec_amd.model import BERT4Rec
    from tests import bert4rec_restate as R

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bert4rec_tiny.npz"), allow_pickle=False)
    meta = dict(zip(("item_num", "D", "L", "H", "inner", "n_layers", "B", "seed"), [int(v) for v in z["meta"]]))
    cfg = {"n_layers": meta["n_layers"], "n_heads": meta["H"], "embedding_size": meta["D"], "inner_size": meta["inner"],
           "hidden_dropout_prob": 0.0, "attn_dropout_prob": 0.0, "hidden_act": "gelu", "layer_norm_eps": 1e-12,
           "initializer_range": 0.02, "MAX_ITEM_LIST_LENGTH": meta["L"], "mask_ratio": 0.4, "seed": 2020}

    class DL:
        item_num = meta["item_num"]

    m = BERT4Rec(cfg, DL())
    m.load_state_dict(R.golden_params(z), strict=True)
    m = m.cuda().train()
    items, mask = torch.from_numpy(z["items"]).cuda(), torch.from_numpy(z["masked_index"]).cuda()
    _clean_slate()
    m((items, mask)).backward()
    ops.raise_on_bad_indices("cuda")
    b, t = [int(v) for v in mask.nonzero()[0]]
    bad = items.clone()
    bad[b, 1, t] = meta["item_num"] + 1                                 # the table has item_num + 1 rows (the mask token is the last)
    m((bad, mask)).backward()
    with pytest.raises(IndexError):
        ops.raise_on_bad_indices("cuda")
