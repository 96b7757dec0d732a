"""The yardsticks of tests/test_gpu_small_kernels.py, pinned without a GPU (tests/small_kernels_restate.py), so that a GPU failure
points at the kernel and not at its reference:
  * the GRU gate restatement chained over L steps is torch.nn.GRU(bias=False, batch_first=True) in float64, and its closed-form
    backward is autograd of its forward;
  * causal im2col times the weight view is torch's conv2d on the left-padded input, and col2im is its exact transpose;
  * the two-term embedding-gradient formula is autograd through MOSASRec's slices of the encoder output;
  * every case the GPU tests call "past the cap" exceeds the cap of its launch, by arithmetic on its shape."""
import numpy as np
import pytest
import torch

from tests import small_kernels_restate as R


# ----------------------------------------------------------------------------------------------------------------- GRU
@pytest.mark.parametrize("L", [1, 5])
@pytest.mark.parametrize("layers", [1, 2])
def test_gru_forward_restatement_chained_is_torch_gru(L, layers):
    B, E, H = 3, 6, 5
    torch.manual_seed(7 + L + layers)
    gru = torch.nn.GRU(E, H, num_layers=layers, bias=False, batch_first=True).double()
    x = torch.randn(B, L, E, dtype=torch.float64)
    want, want_last = gru(x)
    inp = x
    for k in range(layers):
        w_ih, w_hh = getattr(gru, f"weight_ih_l{k}").detach(), getattr(gru, f"weight_hh_l{k}").detach()
        h, outs = None, []
        for t in range(L):
            gi = inp[:, t] @ w_ih.t()
            gh = torch.zeros(B, 3 * H, dtype=torch.float64) if h is None else h @ w_hh.t()
            h_new, save = R.gru_fwd(gi, gh, h)
            assert save.shape == (B, 4 * H) and torch.equal(save[:, 3 * H:], gh[:, 2 * H:])
            h = h_new
            outs.append(h)
        inp = torch.stack(outs, dim=1)
        assert (h - want_last[k].detach()).abs().max().item() <= 1e-12
    assert (inp - want.detach()).abs().max().item() <= 1e-12


@pytest.mark.parametrize("with_h_prev", [True, False])
def test_gru_closed_form_backward_is_autograd_of_the_forward(with_h_prev):
    for (B, H) in R.GRU_SHAPES[:3]:
        c = R.gru_case(B, H)
        hp = c["h_prev"] if with_h_prev else None
        _, save = R.gru_fwd(c["gi"], c["gh"], hp)
        got = R.gru_bwd(c["dh"], save, hp)
        want = R.gru_bwd_autograd(c["dh"], c["gi"], c["gh"], hp)
        for name, g, w in zip(("dgi", "dgh", "dh_prev"), got, want):
            assert g.shape == w.shape and (g - w).abs().max().item() <= 1e-12, (B, H, name)


def test_gru_saturation_case_holds_what_it_says():
    c = R.gru_saturation_case()
    H = c["dh"].shape[1]
    assert len(c["rows"]) == 4 * len(R.SATURATION_VALUES)
    for i, (gate, v, which) in enumerate(c["rows"]):
        cols = slice(gate * H, (gate + 1) * H)
        if gate < 2:
            assert torch.equal(c["gi"][i, cols] + c["gh"][i, cols], torch.full((H,), v))        # exact in float32
        elif which == "gi":
            assert torch.equal(c["gi"][i, cols], torch.full((H,), v))
        else:
            assert torch.equal(c["gh"][i, cols], torch.full((H,), v)) and not c["gi"][i, cols].any()
    _, save = R.gru_fwd(c["gi"], c["gh"], c["h_prev"])
    s32 = save.float()
    # the float64 gates rounded to float32 really reach 0 and 1: the exactness statements of the GPU test are not vacuous
    assert (s32[:, :H] == 1).any() and (s32[:, :H] == 0).any() and (s32[:, H:2 * H] == 1).any() and (s32[:, H:2 * H] == 0).any()
    assert (s32[:, 2 * H:3 * H].abs() == 1).any()
    dgi, dgh, _ = R.gru_bwd(c["dh"], s32, c["h_prev"])
    assert torch.isfinite(dgi).all() and torch.isfinite(dgh).all() and (dgi == 0).any()


# --------------------------------------------------------------------------------------------------------- convolution
CONV_SHAPES = [(B, L, C, k, d) for (B, L, C) in ((2, 5, 3), (1, 9, 4)) for k in (1, 2, 3, 4) for d in (1, 4, 8)] + list(R.C1D_SMALL)


def test_conv_shapes_include_taps_that_only_see_the_padding():
    assert any(d * (k - 1) >= L for (_, L, _, k, d) in CONV_SHAPES) and any(0 < d * (k - 1) < L for (_, L, _, k, d) in CONV_SHAPES)


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=str)
def test_im2col_times_the_weight_view_is_conv2d_on_the_left_padded_input(shape):
    B, L, C, k, d = shape
    g = torch.Generator().manual_seed(sum(shape))
    C_out = C + 1
    x = torch.randn(B, L, C, generator=g, dtype=torch.float64)
    w = torch.randn(C_out, C, 1, k, generator=g, dtype=torch.float64)
    bias = torch.randn(C_out, generator=g, dtype=torch.float64)
    got = R.causal_im2col(x, k, d) @ w.view(C_out, C * k).t() + bias
    padded = torch.nn.functional.pad(x.permute(0, 2, 1).unsqueeze(2), ((k - 1) * d, 0, 0, 0))           # [B, C, 1, pad + L]
    want = torch.nn.functional.conv2d(padded, w, bias, dilation=(1, d)).squeeze(2).permute(0, 2, 1)    # [B, L, C_out]
    assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=str)
def test_col2im_is_the_exact_transpose_of_im2col(shape):
    B, L, C, k, d = shape
    g = torch.Generator().manual_seed(1 + sum(shape))
    x = torch.randn(B, L, C, generator=g, dtype=torch.float64)
    y = torch.randn(B, L, C * k, generator=g, dtype=torch.float64)
    lhs, rhs = (R.causal_im2col(x, k, d) * y).sum().item(), (x * R.causal_col2im(y, k, d)).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


def test_col2im_integer_cases_are_exact_in_float32():
    """|partial sum| <= 8 k < 2^24: float32 adds of the GPU kernel commit no rounding, in any order."""
    for shape in R.C1D_SMALL + (R.COL2IM_PAST_CAP,):
        y = R.col2im_case(shape)
        assert torch.equal(y, y.round()) and float(y.abs().max()) <= 8
        want = R.causal_col2im(y, shape[3], shape[4])
        assert torch.equal(want.float().double(), want)


# ---------------------------------------------------------------------------------------------------------- emb_grad
@pytest.mark.parametrize("shape", R.EMB_GRAD_SHAPES[:2] + ((2, 3, 4),), ids=str)
def test_emb_grad_formula_is_autograd_through_the_slices_of_the_encoder_output(shape):
    B, L, D = shape
    c = R.emb_grad_case(B, L, D)
    dx0, out, coef = R.emb_grad_dx0(c["dx0_buf"], B, L).double(), c["out"].double(), c["coef"].double()
    emb = torch.randn(B, L + 1, 2, D, dtype=torch.float64, generator=torch.Generator().manual_seed(5)).requires_grad_(True)
    pos, neg = emb[:, :, 0], emb[:, :, 1]
    inputs, target_pos, target_neg = pos[:, :-1], pos[:, 1:], neg[:, 1:]
    # dx0 = d loss / d inputs (through the sequence block), coef = d loss / d pos_score = -d loss / d neg_score, out held fixed
    pos_score, neg_score = (out * target_pos).sum(-1), (out * target_neg).sum(-1)
    (inputs * dx0).sum().add((coef * (pos_score - neg_score)).sum()).backward()
    got = R.mosasrec_emb_grad(dx0, out, coef)
    assert (got - emb.grad).abs().max().item() <= 1e-12
    assert not got[:, 0, 1].any()
    scale = R.mosasrec_emb_grad_scale(dx0, out, coef)
    assert (scale >= got.abs() - 1e-12).all() and torch.equal(scale[:, L, 0], (coef[:, L - 1, None] * out[:, L - 1]).abs())


def test_emb_grad_case_plants_its_sentinel_behind_dx0():
    B, L, D = R.EMB_GRAD_SHAPES[1]
    c = R.emb_grad_case(B, L, D)
    assert c["dx0_buf"].shape == (B * L + 1, D) and bool((c["dx0_buf"][B * L] == R.EMB_GRAD_SENTINEL).all())
    dx0 = R.emb_grad_dx0(c["dx0_buf"], B, L)
    assert dx0.shape == (B, L, D) and dx0.is_contiguous() and float(dx0.abs().max()) < 10


# ------------------------------------------------------------------------------------------------- image, ViT, dropout
def test_image_restatement_and_case():
    for n_store, H, W, ids_shape in R.IMAGE_SHAPES:
        store, ids = R.image_case(n_store, H, W, ids_shape)
        flat = ids.view(-1)
        assert 0 in flat and n_store - 1 in flat and len(set(flat.tolist())) < flat.numel()
        assert int(flat.min()) >= 0 and int(flat.max()) < n_store
        out = R.image_u8_to_f64(store, ids)
        assert out.shape == (*ids_shape, 3, H, W) and not out[ids == 0].any()
        i = int((flat > 0).nonzero()[0])
        want = (store[flat[i]].permute(2, 0, 1).double() / 255.0 - 0.5) / 0.5
        assert torch.equal(out.view(-1, 3, H, W)[i], want) and float(out.abs().max()) <= 1.0
    store, _ = R.image_case(*R.IMAGE_SHAPES[0])
    bad = torch.tensor([1, store.shape[0], -3, 2])
    out = R.image_u8_to_f64(store, bad)
    assert not out[1].any() and not out[2].any() and out[0].any() and out[3].any()


def test_vit_restatements():
    c = R.vit_case(*R.VIT_TINY)
    n, T, H = R.VIT_TINY
    tok = R.vit_embed(c["patches"], c["cls"], c["pos"])
    assert tok.shape == (n, T, H) and torch.equal(tok[:, 0], (c["cls"] + c["pos"][0]).expand(n, -1))
    assert torch.equal(tok[2, 5], c["patches"][2, 4] + c["pos"][5])
    assert (R.token_mean(c["act"]) - c["act"].double().mean(1)).abs().max().item() <= 1e-15
    # the float64 form of the ReLU-mean backward is autograd of mean_t relu(act)
    act = c["act"].double().requires_grad_(True)
    torch.relu(act).mean(1).backward(c["dout"].double())
    assert (R.token_mean_relu_bwd(c["dout"].double(), c["act"].double()) - act.grad).abs().max().item() <= 1e-15
    assert R.token_mean_relu_bwd(c["dout"], c["act"]).dtype == torch.float32


def test_dropout_restatement():
    x, _ = R.flat_case(R.ADD_TINY)
    assert torch.equal(R.dropout(x, 0.0, R.DROPOUT_SEED, R.DROPOUT_STREAM), x.double())
    keep = R.dropout_keep(x.numel(), 0.3, R.DROPOUT_SEED, R.DROPOUT_STREAM)
    y = R.dropout(x, 0.3, R.DROPOUT_SEED, R.DROPOUT_STREAM)
    assert 0.6 < keep.float().mean().item() < 0.8 and not y[~keep].any()
    assert (y[keep] - x.double()[keep] / (1.0 - float(np.float32(0.3)))).abs().max().item() == 0.0
    stepped = R.dropout_keep(x.numel(), 0.3, R.DROPOUT_SEED, R.DROPOUT_STREAM, R.DROPOUT_STEP)
    assert torch.equal(stepped, R.dropout_keep(x.numel(), 0.3, R.DROPOUT_SEED + R.DROPOUT_STEP, R.DROPOUT_STREAM))
    assert not torch.equal(stepped, keep)
    assert abs(float(R.dropout_inv_keep_f32(0.3)) - 1.0 / 0.7) < 1e-6 and R.dropout_inv_keep_f32(0.0) == 1.0


def test_gather_cases():
    for chunks in R.GATHER_CHUNKS:
        for D in R.GATHER_DIMS:
            table, idx = R.gather_case(chunks, D)
            n, dv = idx.numel(), D // 4
            assert chunks <= n * dv < chunks + dv and int(idx.min()) >= 0 and int(idx.max()) == table.shape[0] - 1
            if D == 4:
                assert n * dv == chunks
            if n > 1:
                assert 0 in idx
            if n > 3:
                assert len(set(idx.tolist())) < n
    totals = {R.gather_case(c, 4)[1].numel() for c in R.GATHER_CHUNKS}
    assert {R.GATHER_BLOCK - 1, R.GATHER_BLOCK, R.GATHER_BLOCK + 1, 4 * R.GATHER_BLOCK + 3} <= totals


# ------------------------------------------------------------------------------------------------------------ grid caps
def test_every_past_the_cap_case_exceeds_its_cap():
    """Work items of each "past the cap" launch, as its kernel counts them, against the first trip of its grid-stride loop; the
    small cases stay inside it (so both sides of every clamp are run)."""
    B, H = R.GRU_PAST_CAP
    assert B * H == 1049588 > R.GRU_CAP == 1048576 and H % 2 == 1
    assert all(b * h <= R.GRU_CAP for (b, h) in R.GRU_SHAPES[:3])
    B, L, C, k, d = R.IM2COL_PAST_CAP
    assert B * L * C * k == 2109000 > R.C1D_CAP == 2097152
    B, L, C, k, d = R.COL2IM_PAST_CAP
    assert B * L * C == 2109000 > R.C1D_CAP
    assert all(b * l * c * k <= R.C1D_CAP for (b, l, c, k, d) in R.C1D_SMALL)
    n_store, H, W, ids_shape = R.IMAGE_PAST_CAP
    assert int(np.prod(ids_shape)) * 3 * H * W == 2098788 > R.IMAGE_CAP == 2097152
    n_store, H, W, ids_shape = R.IMAGE_SHAPES[0]
    assert int(np.prod(ids_shape)) * 3 * H * W <= R.IMAGE_CAP
    B, L, D = R.EMB_GRAD_PAST_CAP
    assert D % 4 == 0 and B * (L + 1) * 2 * (D // 4) == 1049600 > R.EMB_GRAD_CAP == 1048576
    assert all(b * (l + 1) * 2 * (dd // 4) <= R.EMB_GRAD_CAP for (b, l, dd) in R.EMB_GRAD_SHAPES[:2])
    n, T, H = R.VIT_EMBED_PAST_CAP                      # vit_embed and token_mean_relu_bwd: one float4 of [n, T, H] per item
    assert H % 4 == 0 and n * T * (H // 4) == 1049600 > R.VIT_CAP == 1048576
    n, T, D = R.TOKEN_MEAN_PAST_CAP                     # token_mean: one OUTPUT float4 per item
    assert D % 4 == 0 and n * (D // 4) == 1051137 > R.VIT_CAP
    assert R.ADD_PAST_CAP % 4 == 0 and R.ADD_PAST_CAP // 4 == 1048577 > R.VIT_CAP         # add and dropout
    n, T, H = R.VIT_TINY
    assert n * T * (H // 4) <= R.VIT_CAP and R.ADD_TINY // 4 <= R.VIT_CAP
