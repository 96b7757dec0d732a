"""The conv2d / max-pool family of csrc/conv2d.hip alone, on the MI355X: im2col bit-equal to F.unfold, the convolution (im2col + the
library GEMMs + col2im, ops.conv2d_relu_fwd / ops.conv2d_bwd) against float64 F.conv2d in both GEMM modes, chunked against
unchunked, the pool against torch bit for bit, bad geometry, determinism.  Shapes: tests/test_dvbpr_cpu.py, where the index maps
themselves are checked without a GPU.

Bounds.  Forward: the project's GEMM bound tests/test_gpu_gemm_epilogues.py::_tol = 2e-6 sqrt(K) max|ref| + 1e-6 with K = Cin kh kw.
Weight (and bias) gradient: the same with K = n Ho Wo.  Data gradient: an element is a sum of at most kh kw entries of dcol = dz W,
each inside the GEMM bound with K = Cout, added in float32: kh kw _tol(dcol, Cout) + kh kw 2^-24 sum|terms|; an element no window
reads is exactly +0.0.

Chunking (measured on the MI355X, shape (5, 4, 20, 19, 8, 3, 3, 1, 1) cut into 2 + 2 + 1 images): the forward and the data gradient
have the unchunked run's bits -- a row of the GEMM does not depend on which other rows are in the launch --; the weight gradient is
summed chunk by chunk, which is NOT the one-launch summation order, so it is checked against the bound, not bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pixelrec_amd import lib as _l
from pixelrec_amd import ops
from tests import dvbpr_restate as R
from tests.mo_common import bits
from tests.test_dvbpr_cpu import CONV_SHAPES, POOL_SHAPES, conv_input, pool_input
from tests.test_gpu_gemm_epilogues import _tol

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("bf16x3", "f32")


def nhwc(t):
    """A logical [n, C, H, W] view over NHWC storage holding t's values."""
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def weights(shape, seed=3):
    n, C, H, W, Cout, kh, kw, sh, sw = shape
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(Cout, C, kh, kw, generator=g) / (C * kh * kw) ** 0.5
    b = torch.randn(Cout, generator=g)
    K = C * kh * kw
    wp = torch.zeros(Cout, ops.conv2d_ldk(C, kh, kw))
    wp[:, :K] = w.view(Cout, K)
    return w, b, wp


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_im2col_is_unfold_bit_for_bit(shape, layout):
    n, C, H, W, _, kh, kw, sh, sw = shape
    x = conv_input(shape)
    K, ldk = C * kh * kw, ops.conv2d_ldk(C, kh, kw)
    ref = F.unfold(x, (kh, kw), stride=(sh, sw)).transpose(1, 2).reshape(-1, K)
    rows, G = ref.shape[0], 3
    buf = torch.full((rows + 2 * G, ldk), float("nan"), device=DEV)
    xd = x.to(DEV) if layout == "nchw" else nhwc(x.to(DEV))
    col = ops.conv2d_im2col(xd, kh, kw, sh, sw, buf[G:G + rows], ldk).cpu()
    assert torch.equal(bits(col[:, :K]), bits(ref))
    assert torch.equal(bits(col[:, K:]), torch.zeros(rows, ldk - K, dtype=torch.int32))               # the pad columns are +0.0
    assert np.array_equal(col.numpy().view(np.int32), R.im2col_map(x.numpy(), kh, kw, sh, sw).view(np.int32))
    guards = torch.cat((buf[:G], buf[G + rows:])).cpu()
    assert bool(torch.isnan(guards).all())                                                             # nothing outside the buffer


def conv_case(shape, ws_bytes=1 << 30):
    """One forward and backward of the convolution over NHWC storage -> (y, dWp, db, dx) on the host."""
    n, C, H, W, Cout, kh, kw, sh, sw = shape
    x = conv_input(shape)
    w, b, wp = weights(shape)
    Ho, Wo = R.out_hw(H, W, kh, kw, sh, sw)
    dz = torch.randn(n, Cout, Ho, Wo, generator=torch.Generator().manual_seed(5))
    xd, wd, bd = nhwc(x.to(DEV)), wp.to(DEV), b.to(DEV)
    y, der = ops.conv2d_relu_fwd(xd, wd, bd, kh, kw, sh, sw, ws_bytes, save_der=True)
    y2, none = ops.conv2d_relu_fwd(xd, wd, bd, kh, kw, sh, sw, ws_bytes, save_der=False)
    assert none is None and torch.equal(bits(y), bits(y2))                       # the two epilogues that apply the ReLU agree
    assert torch.equal(der, (y > 0).to(torch.float32))
    dwp, db = torch.full_like(wd, float("nan")), torch.full_like(bd, float("nan"))
    dx = ops.conv2d_bwd(nhwc(dz.to(DEV)), xd, wd, kh, kw, sh, sw, dwp, db, ws_bytes)
    assert dx.permute(0, 2, 3, 1).is_contiguous() and y.permute(0, 2, 3, 1).is_contiguous()          # NHWC storage
    return (x, w, b, dz), (y.cpu(), dwp.cpu(), db.cpu(), dx.cpu())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv_against_float64(shape, mode):
    n, C, H, W, Cout, kh, kw, sh, sw = shape
    prev = ops.set_gemm_mode(mode)
    try:
        (x, w, b, dz), (y, dwp, db, dx) = conv_case(shape)
    finally:
        ops.set_gemm_mode(prev)
    K = C * kh * kw
    x64, w64, b64 = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    z64 = F.conv2d(x64, w64, b64, stride=(sh, sw))
    err = float((y.double() - torch.relu(z64)).abs().max())
    print(f"CONV2D {mode} {shape} fwd err {err:.3e} tol {_tol(z64.detach(), K):.3e}")
    assert err <= _tol(z64.detach(), K)
    z64.backward(dz.double())
    rows = n * z64.shape[2] * z64.shape[3]
    err = float((dwp[:, :K].double() - w64.grad.view(Cout, K)).abs().max())
    print(f"CONV2D {mode} {shape} dW err {err:.3e} tol {_tol(w64.grad, rows):.3e}")
    assert err <= _tol(w64.grad, rows)
    assert not dwp[:, K:].any()                                                   # the pad column's gradient is zero
    assert float((db.double() - b64.grad).abs().max()) <= _tol(b64.grad, rows)
    # data gradient: dcol64 = dz W per (row, k); the elements' sums of |terms| through the same gather
    dzm = dz.double().permute(0, 2, 3, 1).reshape(rows, Cout)
    dcol64 = (dzm @ w64.detach().view(Cout, K)).numpy()
    ldk = dwp.shape[1]
    pad = np.zeros((rows, ldk))
    pad[:, :K] = np.abs(dcol64)
    sum_abs = torch.from_numpy(R.col2im_map(pad, n, C, H, W, kh, kw, sh, sw))
    bound = kh * kw * _tol(torch.from_numpy(dcol64), Cout) + kh * kw * 2.0 ** -24 * sum_abs
    diff = (dx.double() - x64.grad).abs()
    print(f"CONV2D {mode} {shape} dx err {float(diff.max()):.3e} bound {float(bound.min()):.3e}")
    assert bool((diff <= bound).all())
    unread = torch.from_numpy(~R.covered(H, W, kh, kw, sh, sw))
    assert torch.equal(bits(dx[:, :, unread]), torch.zeros_like(dx[:, :, unread], dtype=torch.int32))  # exactly +0.0


@pytest.mark.parametrize("mode", MODES)
def test_chunked_convolution(mode):
    shape = CONV_SHAPES[4]
    n, C, H, W, Cout, kh, kw, sh, sw = shape
    Ho, Wo = R.out_hw(H, W, kh, kw, sh, sw)
    budget = 2 * Ho * Wo * ops.conv2d_ldk(C, kh, kw) * 4 + 100        # two images' columns and a little: chunks of 2, 2 and 1
    assert ops.conv2d_chunk_images(n, Ho * Wo, ops.conv2d_ldk(C, kh, kw), budget) == 2 and n == 5
    prev = ops.set_gemm_mode(mode)
    try:
        (x, w, b, dz), whole = conv_case(shape)
        _, parts = conv_case(shape, budget)
    finally:
        ops.set_gemm_mode(prev)
    assert torch.equal(bits(whole[0]), bits(parts[0]))                # forward: the same bits
    assert torch.equal(bits(whole[3]), bits(parts[3]))                # data gradient: the same bits
    w64 = w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    F.conv2d(x.double(), w64, b64, stride=(sh, sw)).backward(dz.double())
    K, rows = C * kh * kw, n * Ho * Wo
    same = torch.equal(bits(whole[1]), bits(parts[1]))
    print(f"CONV2D {mode} chunked dW bit-equal to unchunked: {same}")
    assert float((parts[1][:, :K].double() - w64.grad.view(Cout, K)).abs().max()) <= _tol(w64.grad, rows)
    assert float((parts[2].double() - b64.grad).abs().max()) <= _tol(b64.grad, rows)


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_pool_is_torch_bit_for_bit(shape, ties):
    y = pool_input(shape, ties=ties)
    x = y.clone().requires_grad_(True)
    p_ref = F.max_pool2d(torch.relu(x), 2)
    dp = torch.randn(p_ref.shape, generator=torch.Generator().manual_seed(2))
    p_ref.backward(dp)
    yd = nhwc(y.to(DEV))
    p = ops.maxpool2x2_fwd(yd)
    p_chw = ops.maxpool2x2_fwd(yd, chw=True)
    assert p.permute(0, 2, 3, 1).is_contiguous() and p_chw.is_contiguous()
    assert torch.equal(bits(p.cpu()), bits(p_ref.detach())) and torch.equal(bits(p_chw.cpu()), bits(p_ref.detach()))
    for dpd in (nhwc(dp.to(DEV)), dp.to(DEV)):                        # dp over NHWC storage, and in (c, h, w) order as fcs.0 hands it back
        dy = ops.maxpool2x2_relu_bwd(yd, dpd).cpu()
        assert torch.equal(bits(dy), bits(x.grad))
        n, C, H, W = shape
        tail = torch.cat((dy[:, :, 2 * (H // 2):, :].reshape(-1), dy[:, :, :, 2 * (W // 2):].reshape(-1)))
        assert torch.equal(bits(tail), torch.zeros_like(tail, dtype=torch.int32))     # dropped rows / columns: +0.0
    dy_nchw = ops.maxpool2x2_relu_bwd(y.to(DEV), dp.to(DEV)).cpu()    # the scalar path (NCHW storage)
    assert torch.equal(bits(dy_nchw), bits(x.grad))


def test_bad_geometry_is_refused_without_a_launch():
    x = torch.randn(1, 4, 3, 3, device=DEV)
    col = torch.full((4, 36), float("nan"), device=DEV)
    for args, word in (((4, 3, 1, 1), "larger"), ((3, 4, 1, 1), "larger"), ((3, 3, 0, 1), "stride"), ((3, 3, 1, -1), "stride")):
        with pytest.raises(_l.PxrError, match=word):
            ops.conv2d_im2col(x, *args, col=col[:1], ldk=36)
        with pytest.raises(_l.PxrError, match=word):
            ops.conv2d_col2im(col[:1], torch.empty_like(x), *args, ldk=36)
    x3 = torch.randn(1, 3, 3, 3, device=DEV)                          # K = 27: ldk must be 28
    for ldk in (27, 29, 32):
        with pytest.raises(_l.PxrError, match="ldk"):
            ops.conv2d_im2col(x3, 3, 3, 1, 1, col=col.view(-1)[:ldk].view(1, ldk), ldk=ldk)
        with pytest.raises(_l.PxrError, match="ldk"):
            ops.conv2d_col2im(col.view(-1)[:ldk].view(1, ldk), torch.empty_like(x3), 3, 3, 1, 1, ldk=ldk)
    with pytest.raises(_l.PxrError, match="H, W >= 2"):
        ops.maxpool2x2_fwd(torch.randn(1, 4, 1, 4, device=DEV))
    with pytest.raises(_l.PxrError):
        ops.conv2d_relu_fwd(x, torch.zeros(4, 40, device=DEV), torch.zeros(4, device=DEV), 3, 3, 1, 1)      # a weight operand of the wrong width
    torch.cuda.synchronize()
    assert bool(torch.isnan(col).all())                               # nothing was launched on the buffer


def test_two_runs_give_the_same_bits():
    for shape in (CONV_SHAPES[0], CONV_SHAPES[4]):
        a, b = conv_case(shape)[1], conv_case(shape)[1]
        for s, t in zip(a, b):
            assert torch.equal(bits(s), bits(t))
