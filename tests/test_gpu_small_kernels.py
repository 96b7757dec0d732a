"""The small element-wise kernels -- csrc/gru.hip, conv1d.hip, pixel.hip, the small kernels of vit.hip -- and the row gather, each
called directly and compared with the float64 restatements of tests/small_kernels_restate.py (pinned on the CPU by
tests/test_small_kernels_cpu.py), at tiny shapes AND at the smallest shape past the clamp of its grid, where every thread of the
grid-stride loop makes a second trip.  Outputs are pre-filled with NaN where the wrapper lets the caller pass them, so an element
the second trip never reached fails the comparison.

Bars: moves and single float32 operations are bit equality; sums carry the derived bound written next to them.  The GRU gates
go through expf / tanhf, which are not correctly rounded on the device, so their bar is measured: GRU_MEASURED is the largest
|got - want| / max(1, max |want|) over every output of every GRU case of this file (forward h and the four save planes, backward
dgi, dgh, dh_prev; the saturation case included), and the tests assert four times that.  Each test also asserts that its bar does
not exceed the bar tests/test_gpu_gru4rec.py already holds this block to, 2e-6 + 2e-5 max |want|."""
import functools

import pytest
import torch

from tests import small_kernels_restate as R

pytestmark = pytest.mark.gpu

# Measured on an MI355X on 2026-10-20: 1.7633e-7, taken by dgh of the saturation case ((B, H) = (28, 4), max |want| 1.145); next
# the forward save plane n = tanh(.) at (B, H) = (1028, 1021) with 1.7544e-7 and h there with 1.66e-7.  4 x = 7.06e-7 < 2e-6.
GRU_MEASURED = 1.7633e-7
GRU_TOL = 4 * GRU_MEASURED


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def gru_figure(name, got, want):
    """-> (max |got - want| / max(1, max |want|), max |want|) of a device float32 output against its float64 restatement."""
    m = want.abs().max().item()
    err = (got.cpu().double() - want).abs().max().item() / max(1.0, m)
    print(f"gru {name}: err / max(1, max|want|) = {err:.3e}  (max|want| {m:.3e})")
    return err, m


def _gru_check(outputs):
    """Every (name, got, want): |got - want| <= GRU_TOL max(1, max |want|), a bar inside the model-level one."""
    for name, got, want in outputs:
        err, m = gru_figure(name, got, want)
        assert torch.isfinite(got).all(), name
        assert GRU_TOL * max(1.0, m) <= 2e-6 + 2e-5 * m, name
        assert err <= GRU_TOL, (name, err)


@functools.lru_cache(maxsize=None)
def _gru_ref(B, H, with_h_prev):
    c = R.gru_case(B, H)
    hp = c["h_prev"] if with_h_prev else None
    h, save = R.gru_fwd(c["gi"], c["gh"], hp)
    save32 = save.float()                                   # the backward's input: the float64 planes rounded once
    return c, hp, h, save, save32, R.gru_bwd(c["dh"], save32, hp)


def gru_forward_outputs(B, H, with_h_prev):
    """Runs the forward (with and without save) -> [(name, got, want)] of the outputs that carry device arithmetic."""
    from pixelrec_amd import ops

    c, hp, want_h, want_save, _, _ = _gru_ref(B, H, with_h_prev)
    gi, gh = c["gi"].cuda(), c["gh"].cuda()
    hp_d = None if hp is None else hp.cuda()
    h, save = _nan(B, H), _nan(B, 4 * H)
    ops.gru_gates_fwd(gi, gh, hp_d, h, save)
    assert torch.equal(save[:, 3 * H:], gh[:, 2 * H:])                          # gh_n is copied
    h2 = _nan(B, H)
    ops.gru_gates_fwd(gi, gh, hp_d, h2)                                         # without save: the same h, bit for bit
    assert torch.equal(h2, h)
    return [("h", h, want_h)] + [("save." + plane, save[:, i * H:(i + 1) * H], want_save[:, i * H:(i + 1) * H])
                                 for i, plane in enumerate(("r", "z", "n"))]


def gru_backward_outputs(B, H, with_h_prev):
    """Runs the backward on the float32-rounded restated save planes -> [(name, got, want)]."""
    from pixelrec_amd import ops

    c, hp, _, _, save32, want = _gru_ref(B, H, with_h_prev)
    dgi, dgh, dhp = _nan(B, 3 * H), _nan(B, 3 * H), _nan(B, H)
    ops.gru_gates_bwd(c["dh"].cuda(), save32.cuda(), None if hp is None else hp.cuda(), dgi, dgh, dhp)
    return list(zip(("dgi", "dgh", "dh_prev"), (dgi, dgh, dhp), want))


@pytest.mark.parametrize("with_h_prev", [True, False], ids=["h_prev", "first_step"])
@pytest.mark.parametrize("shape", R.GRU_SHAPES, ids=str)
def test_gru_gates_forward_matches_fp64(shape, with_h_prev):
    _gru_check(gru_forward_outputs(*shape, with_h_prev))


@pytest.mark.parametrize("with_h_prev", [True, False], ids=["h_prev", "first_step"])
@pytest.mark.parametrize("shape", R.GRU_SHAPES, ids=str)
def test_gru_gates_backward_matches_fp64(shape, with_h_prev):
    _gru_check(gru_backward_outputs(*shape, with_h_prev))


def gru_saturation_outputs():
    """Runs the saturation case forward and, on the device's own save planes, backward; asserts the exactness statements
    -> [(name, got, want)] for the value bar."""
    from pixelrec_amd import ops

    c = R.gru_saturation_case()
    B, H = c["dh"].shape
    want_h, want_save = R.gru_fwd(c["gi"], c["gh"], c["h_prev"])
    h, save = _nan(B, H), _nan(B, 4 * H)
    ops.gru_gates_fwd(c["gi"].cuda(), c["gh"].cuda(), c["h_prev"].cuda(), h, save)
    outputs = [("saturation h", h, want_h)] + [("saturation save." + plane, save[:, i * H:(i + 1) * H],
                                                want_save[:, i * H:(i + 1) * H]) for i, plane in enumerate(("r", "z", "n"))]
    assert torch.isfinite(h).all() and torch.isfinite(save).all()
    got, w32 = save.cpu()[:, :2 * H], want_save.float()[:, :2 * H]
    exact = (w32 == 0) | (w32 == 1)                                             # where float64 rounds to exactly 0 or 1: r and z too
    assert exact.any() and torch.equal(got[exact], w32[exact])
    # backward on the DEVICE's own save planes: exact zeros, never NaN, where r (1 - r), z (1 - z) or 1 - n^2 vanish
    dgi, dgh, dhp = _nan(B, 3 * H), _nan(B, 3 * H), _nan(B, H)
    ops.gru_gates_bwd(c["dh"].cuda(), save, c["h_prev"].cuda(), dgi, dgh, dhp)
    want = R.gru_bwd(c["dh"], save.cpu(), c["h_prev"])
    s = save.cpu().double()
    r, z, n = s[:, :H], s[:, H:2 * H], s[:, 2 * H:3 * H]
    assert (r * (1 - r) == 0).any() and (z * (1 - z) == 0).any() and (1 - n * n == 0).any()
    for name, g, w in zip(("dgi", "dgh", "dh_prev"), (dgi, dgh, dhp), want):
        assert torch.isfinite(g).all(), name
        assert not g.cpu()[w == 0].any(), name
        outputs.append(("saturation " + name, g, w))
    assert (want[0] == 0).any() and (want[1] == 0).any()
    return outputs


def test_gru_gates_saturate_to_exact_zeros_and_ones():
    _gru_check(gru_saturation_outputs())


def test_gru_wrappers_refuse_strided_float64_and_wrong_width_operands():
    from pixelrec_amd import ops
    from pixelrec_amd.lib import PxrError

    B, H = 3, 8
    f = lambda *s: torch.randn(*s, device="cuda")
    good = dict(gi=f(B, 3 * H), gh=f(B, 3 * H), h_prev=f(B, H), h_out=_nan(B, H), save=_nan(B, 4 * H))
    bad = {"transposed gi": dict(gi=f(3 * H, B).t()), "transposed save": dict(save=f(4 * H, B).t()),
           "float64 gh": dict(gh=f(B, 3 * H).double()), "float64 h_prev": dict(h_prev=f(B, H).double()),
           "wide gi": dict(gi=f(B, 4 * H)), "narrow save": dict(save=f(B, 3 * H)), "wide h_prev": dict(h_prev=f(B, 2 * H)),
           "host gh": dict(gh=torch.randn(B, 3 * H)), "transposed h_out": dict(h_out=f(H, B).t())}
    for name, over in bad.items():
        a = {**good, **over}
        with pytest.raises(PxrError):
            ops.gru_gates_fwd(a["gi"], a["gh"], a["h_prev"], a["h_out"], a["save"])
        assert torch.isnan(good["h_out"]).all() and torch.isnan(good["save"]).all(), name       # nothing was launched
    ops.gru_gates_fwd(good["gi"], good["gh"], None, good["h_out"], None)                        # None where the ABI allows it
    assert torch.isfinite(good["h_out"]).all()
    good = dict(dh=f(B, H), save=f(B, 4 * H), h_prev=f(B, H), dgi=_nan(B, 3 * H), dgh=_nan(B, 3 * H), dh_prev=_nan(B, H))
    bad = {"transposed dh": dict(dh=f(H, B).t()), "transposed dgi": dict(dgi=f(3 * H, B).t()), "float64 save": dict(save=f(B, 4 * H).double()),
           "float64 dgh": dict(dgh=f(B, 3 * H).double()), "wide dgh": dict(dgh=f(B, 4 * H)), "narrow save": dict(save=f(B, 3 * H)),
           "wide dh_prev": dict(dh_prev=f(B, H + 1)), "missing save": dict(save=None), "missing dh_prev": dict(dh_prev=None)}
    for name, over in bad.items():
        a = {**good, **over}
        with pytest.raises(PxrError):
            ops.gru_gates_bwd(a["dh"], a["save"], a["h_prev"], a["dgi"], a["dgh"], a["dh_prev"])
        assert all(torch.isnan(good[k]).all() for k in ("dgi", "dgh", "dh_prev")), name
    ops.gru_gates_bwd(good["dh"], good["save"], None, good["dgi"], good["dgh"], good["dh_prev"])
    assert all(torch.isfinite(good[k]).all() for k in ("dgi", "dgh", "dh_prev"))


# ------------------------------------------------------------------------------------------------- im2col and col2im
@pytest.mark.parametrize("shape", R.C1D_SMALL + (R.IM2COL_PAST_CAP,), ids=str)
def test_causal_im2col_is_a_pure_move(shape):
    from pixelrec_amd import ops

    B, L, C, k, d = shape
    x = R.im2col_case(shape)
    got = ops.causal_im2col(x.cuda(), k, d)
    assert got.shape == (B, L, C * k) and torch.equal(got.cpu(), R.causal_im2col(x, k, d))


@pytest.mark.parametrize("shape", R.C1D_SMALL + (R.COL2IM_PAST_CAP,), ids=str)
def test_causal_col2im_on_integers_is_exact(shape):
    """Integer-valued dxcol in [-8, 8]: every partial sum is exact in float32, so the float64 sum is the only right answer."""
    from pixelrec_amd import ops

    B, L, C, k, d = shape
    y = R.col2im_case(shape)
    got = ops.causal_col2im(y.cuda(), k, d)
    assert got.shape == (B, L, C) and torch.equal(got.cpu().double(), R.causal_col2im(y, k, d))


def test_causal_col2im_on_gaussians_stays_inside_the_summation_bound():
    """k taps summed in float32: k - 1 rounded additions (the first adds to 0), each off by at most 2^-24 of a partial sum that is
    at most sum |terms|."""
    from pixelrec_amd import ops

    shape = R.C1D_SMALL[3]
    B, L, C, k, d = shape
    y = R.col2im_case(shape, integers=False)
    err = (ops.causal_col2im(y.cuda(), k, d).cpu().double() - R.causal_col2im(y, k, d)).abs()
    bound = (k - 1) * R.U24 * R.causal_col2im_abs(y, k, d)
    print("col2im gaussian: max err / bound =", (err / bound.clamp_min(1e-300)).max().item())
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------------ image transform
@pytest.mark.parametrize("case", R.IMAGE_SHAPES, ids=str)
def test_image_transform_matches_fp64(case):
    """(float) u8 is exact; / 255, - 0.5 and / 0.5 are three float32 roundings of values in [-1, 1]: 4 x 2^-24 with the doubling of
    the last division."""
    from pixelrec_amd import ops

    store, ids = R.image_case(*case)
    ops.raise_on_bad_indices()
    got = ops.image_u8_to_f32(store.cuda(), ids.cuda()).cpu()
    ops.raise_on_bad_indices()                                                  # ids in range, the pad id included: nothing flagged
    want = R.image_u8_to_f64(store, ids)
    assert got.shape == want.shape
    err = (got.double() - want).abs().max().item()
    print("image: max err =", err, "bar", 4 * R.U24)
    assert err <= 4 * R.U24
    pad = got[ids == 0]
    assert pad.numel() and not pad.any() and not torch.signbit(pad).any()        # the pad rows are exactly +0.0


def test_image_transform_flags_ids_outside_the_store():
    """An id outside [0, n_store) is an error like in every other gather: the zero image is written, nothing else of the call
    changes, and the host raises IndexError at its next check.  Id 0 is the pad image, not an error."""
    from pixelrec_amd import ops

    store, ids = R.image_case(*R.IMAGE_SHAPES[0])
    n_store = store.shape[0]
    store_d = store.cuda()
    ops.raise_on_bad_indices()                                                  # clean slate
    clean = ops.image_u8_to_f32(store_d, ids.cuda())
    assert int(ops.device_status(store_d.device).item()) == 0
    ops.raise_on_bad_indices()
    for bad_id in (n_store, -3):
        bad = ids.clone()
        bad[1, 1] = bad_id
        got = ops.image_u8_to_f32(store_d, bad.cuda())
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices()
        ops.raise_on_bad_indices()                                              # the flag was consumed
        keep = torch.ones_like(ids, dtype=torch.bool)
        keep[1, 1] = False
        assert torch.equal(got[keep.cuda()], clean[keep.cuda()]) and not got[1, 1].any()
    zeros = ops.image_u8_to_f32(store_d, torch.zeros(4, dtype=torch.int64, device="cuda"))
    ops.raise_on_bad_indices()                                                  # pad ids alone: nothing flagged
    assert not zeros.any()


# --------------------------------------------------------------------------------------------------- mosasrec_emb_grad
@pytest.mark.parametrize("shape", R.EMB_GRAD_SHAPES, ids=str)
def test_mosasrec_emb_grad_matches_fp64(shape):
    """One multiply-add chain per element: the product and the sum round once each, both at most 2^-24 of |dx0| + |coef out|."""
    from pixelrec_amd import ops

    B, L, D = shape
    c = R.emb_grad_case(B, L, D)
    buf = c["dx0_buf"].cuda()
    out, coef = c["out"].cuda(), c["coef"].cuda()
    got = ops.mosasrec_emb_grad(R.emb_grad_dx0(buf, B, L), out, coef)
    dx0 = R.emb_grad_dx0(c["dx0_buf"], B, L)
    want = R.mosasrec_emb_grad(dx0, c["out"], c["coef"])
    assert got.shape == (B, L + 1, 2, D)
    err = (got.cpu().double() - want).abs()
    bound = 2 * R.U24 * R.mosasrec_emb_grad_scale(dx0, c["out"], c["coef"])
    print("emb_grad: max err / bound =", (err / bound.clamp_min(1e-300)).max().item())
    assert (err <= bound).all()
    assert not got[:, 0, 1].any()                                               # the negative of position 0 is used nowhere
    # rows (b, L, 0) carry no dx0 term: one float32 product, bit for bit -- nothing past dx0's [B, L] rows was read (the next
    # sequence's first row, or the sentinel row behind the last one)
    last = coef[:, L - 1, None] * out[:, L - 1]
    assert torch.equal(got[:, L, 0], last) and torch.equal(got[:, L, 1], -last)
    assert float(got.abs().max()) < 1e3 < R.EMB_GRAD_SENTINEL
    assert bool((buf[B * L] == R.EMB_GRAD_SENTINEL).all())


def test_mosasrec_emb_grad_refuses_strided_float64_and_wrong_width_operands():
    from pixelrec_amd import ops
    from pixelrec_amd.lib import PxrError

    B, L, D = 3, 5, 8
    f = lambda *s: torch.randn(*s, device="cuda")
    good = dict(dx0=f(B, L, D), out=f(B, L, D), coef=f(B, L))
    bad = {"transposed out": dict(out=f(L, B, D).transpose(0, 1)), "transposed dx0": dict(dx0=f(B, D, L).transpose(1, 2)),
           "transposed coef": dict(coef=f(L, B).t()), "float64 dx0": dict(dx0=f(B, L, D).double()),
           "float64 coef": dict(coef=f(B, L).double()), "D % 4": dict(dx0=f(B, L, 6), out=f(B, L, 6)),
           "short coef": dict(coef=f(B, L - 1)), "wide dx0": dict(dx0=f(B, L, 2 * D)), "host out": dict(out=torch.randn(B, L, D))}
    for name, over in bad.items():
        a = {**good, **over}
        with pytest.raises(PxrError) as e:
            ops.mosasrec_emb_grad(a["dx0"], a["out"], a["coef"])
        assert "failed (rc=" not in str(e.value), name                          # refused by the wrapper: the entry point never ran
    assert ops.mosasrec_emb_grad(good["dx0"], good["out"], good["coef"].view(-1)).shape == (B, L + 1, 2, D)   # coef [B L] is fine


# --------------------------------------------------------------------------------------------------- ViT small kernels
@pytest.mark.parametrize("shape", (R.VIT_TINY, R.VIT_EMBED_PAST_CAP), ids=str)
def test_vit_embed_and_relu_mean_backward_are_bit_exact(shape):
    """vit_embed is one float32 addition per element; the ReLU-mean backward one rounded reciprocal and one rounded product."""
    from pixelrec_amd import ops

    c = R.vit_case(*shape)
    got = ops.vit_embed(c["patches"].cuda(), c["cls"].cuda(), c["pos"].cuda())
    assert torch.equal(got.cpu(), R.vit_embed(c["patches"], c["cls"], c["pos"]))
    got = ops.token_mean_relu_bwd(c["dout"].cuda(), c["act"].cuda())
    assert torch.equal(got.cpu(), R.token_mean_relu_bwd(c["dout"], c["act"]))


@pytest.mark.parametrize("shape", (R.VIT_TINY, R.TOKEN_MEAN_PAST_CAP), ids=str)
def test_token_mean_matches_fp64(shape):
    """T rounded operations on partial sums of at most sum_t |x|, then the 1 / T: T 2^-24 sum |x| / T."""
    from pixelrec_amd import ops

    n, T, D = shape
    x = R.token_mean_case(n, T, D)
    got = ops.token_mean(x.cuda())
    assert got.shape == (n, D)
    err = (got.cpu().double() - R.token_mean(x)).abs()
    bound = T * R.U24 * x.double().abs().sum(1) / T
    print("token_mean: max err / bound =", (err / bound).max().item())
    assert (err <= bound).all()


@pytest.mark.parametrize("n", (R.ADD_TINY, R.ADD_PAST_CAP))
def test_add_is_bit_exact(n):
    from pixelrec_amd import ops

    a, b = R.flat_case(n)
    assert torch.equal(ops.add(a.cuda(), b.cuda()).cpu(), R.add(a, b))


@pytest.mark.parametrize("with_step", [False, True], ids=["no_step", "step5"])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("n", (R.ADD_TINY, R.ADD_PAST_CAP))
def test_dropout_keeps_the_oracle_mask_and_scales_bit_exactly(n, p, with_step):
    from pixelrec_amd import ops

    x, _ = R.flat_case(n)
    x = x.abs() + 0.5                                                           # no zeros: the kept set is read off the output
    step = R.DROPOUT_STEP if with_step else None
    step_dev = torch.tensor([R.DROPOUT_STEP], dtype=torch.int64, device="cuda") if with_step else None
    got = ops.dropout(x.cuda(), p, R.DROPOUT_SEED, R.DROPOUT_STREAM, step_dev).cpu()
    keep = R.dropout_keep(n, p, R.DROPOUT_SEED, R.DROPOUT_STREAM, step)
    assert torch.equal(got != 0, keep)                                          # element for element
    assert torch.equal(got[keep], x[keep] * torch.tensor(R.dropout_inv_keep_f32(p)))
    assert not got[~keep].any()
    err = (got.double() - R.dropout(x, p, R.DROPOUT_SEED, R.DROPOUT_STREAM, step)).abs().max().item()
    assert err <= 2 * R.U24 * float(x.max()) / (1.0 - p)                        # 1 / (1 - p) and the product: two roundings
    if p == 0.0:
        assert keep.all() and torch.equal(got, x)


def test_dropout_refusals():
    from pixelrec_amd import ops
    from pixelrec_amd.lib import PxrError

    with pytest.raises(PxrError):
        ops.dropout(torch.ones(1002, device="cuda"), 0.3, 1, 0)                 # n % 4 != 0
    with pytest.raises(PxrError):
        ops.dropout(torch.ones(1000, device="cuda"), 1.0, 1, 0)                 # p = 1
    with pytest.raises(PxrError):
        ops.add(torch.ones(1002, device="cuda"), torch.ones(1002, device="cuda"))


# ------------------------------------------------------------------------------------------------------- embed_gather
@pytest.mark.parametrize("D", R.GATHER_DIMS)
@pytest.mark.parametrize("chunks", R.GATHER_CHUNKS)
def test_embed_gather_around_its_block_of_1024_chunks(chunks, D):
    """The default variant: a block owns 4 x 256 consecutive float4 chunks; totals one short of, at and one past a block, and
    past four blocks, with rows narrower and wider than a wave."""
    from pixelrec_amd import ops

    table, idx = R.gather_case(chunks, D)
    ops.raise_on_bad_indices()
    got = ops.embed_gather(table.cuda(), idx.cuda())
    ops.raise_on_bad_indices()
    assert got.shape == (idx.numel(), D) and torch.equal(got.cpu(), table[idx])
