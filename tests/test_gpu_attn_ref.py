"""Every sequence-attention family (csrc/attention.hip; the rows path of ops = batched GEMMs + csrc/vit.hip's row kernels) against a
float64 restatement of the same operation (reference layers.py:590-612, sasrec.py:119-126, IDNet/bert4rec.py:150-155), computed from
the exact fp32 inputs each kernel was given, attention dropout included:

  attn_*_mfma2_kernel       L <= 51, d <= 128, d % 8 == 0 (default)
  attn_*_mfma1_kernel<8>    52 <= L <= 64, or PXR_ATTN_TWO=0 (read per call)
  attn_*_mfma1_kernel<4>    PXR_ATTN_MFMA_WAVES=4                              (child process)
  attn_*_mfma_kernel        L <= 64, d > 128, d % 8 == 0 (d-chunked)
  attn_*_kernel<NW>         d % 8 != 0, or PXR_ATTN_MFMA=0; NW = PXR_ATTN_WAVES (child processes for the knobs)
  attn_*_long_kernel        65 <= L <= 128, d % 8 == 0
  rows path                 L > 128, or 65..128 with d % 8 != 0 or with PXR_ATTN_MFMA=0

each in its causal and bidirectional form, p_drop in {0, 0.1, 0.5}.  The fused entries are called through the C ABI directly with
every output pre-filled with NaN (an element nothing writes fails), q / k / v inside a wider buffer, ctx / dctx / dq|dk|dv at strides of
their own with sentinels in the gap columns (they must come back unchanged; the input gaps hold NaN, so reading one shows), and the key
mask as an offset view with a batch stride of 3L (BERT4Rec's [B, 3, L] layout).

Bars: err < max(C * max|ref|, 3 * err32), err32 = how far the same restatement run in fp32 lands from fp64 on the same inputs (the
pattern of test_gpu_tower_attn.py).  One constant per output, the same for every case."""
import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.dropout_rng import keep_mask

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_CTX, C_P, C_GRAD = 3e-6, 3e-6, 3e-6       # per output: ctx, probabilities (scale 1), dq | dk | dv
SPREADS = (1.0, 4.0)                          # |scaled score| up to ~ 5 and ~ 80
PS = (0.0, 0.1, 0.5)
SENT = 7777.0                                 # sentinel of the gap columns of the outputs
KNOBS = ("PXR_ATTN_MFMA", "PXR_ATTN_WAVES", "PXR_ATTN_MFMA_WAVES", "PXR_ATTN_TWO")


# ---- the fp64 restatement ---------------------------------------------------------------------------------------------------------
def inv_keep(p, dtype=torch.float64):
    """1 / (1 - p) as the kernels scale kept probabilities: p is the fp32 dropout rate; in fp32 for the fp32 restatement."""
    if dtype == torch.float32:
        return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return 1.0 / (1.0 - float(np.float32(p)))


def attn_keep(seed, stream, B, H, L, p, device):
    """The kernels' keep mask of the [B, H, L, L] probabilities: counter ((b*H + h)*L + i)*L + j (oracle/dropout_rng.py)."""
    if p == 0.0:
        return None
    return torch.from_numpy(keep_mask(seed % 2 ** 64, stream, (B, H, L, L), p)).to(device)


def restate(qkv, km, H, d, causal, keep=None, p=0.0, dtype=torch.float64):
    """qkv [B, L, 3*H*d] (q | k | v), km [B, L] (key real iff != 0) -> (ctx [B, L, H*d], P [B, H, L, L] before dropout), in `dtype`.

    The reference's arithmetic: score = q.k / sqrt(d) rounded to fp32, plus the additive -1e9 in fp32 -- so score + (-1e9) == -1e9
    exactly while |score| < 32 and a fully masked query row is uniform over all L keys; causal: key j <= query i and key real,
    bidirectional: key real.  Softmax, dropout (kept entries * 1 / (1 - p)) and P.V in `dtype`."""
    B, L, _ = qkv.shape
    D = H * d
    q, k, v = (qkv[..., i * D:(i + 1) * D].reshape(B, L, H, d).permute(0, 2, 1, 3).to(dtype) for i in range(3))
    allowed = (km != 0)[:, None, None, :].expand(B, 1, L, L)
    if causal:
        allowed = allowed & torch.ones(L, L, dtype=torch.bool, device=qkv.device).tril()
    s = (q @ k.transpose(-1, -2) / math.sqrt(d)).float() + torch.where(allowed, 0.0, -1e9).float()
    P = torch.softmax(s.to(dtype), -1)
    PD = P if keep is None else P * keep.to(dtype) * inv_keep(p, dtype)
    return (PD @ v).permute(0, 2, 1, 3).reshape(B, L, D), P


def reference(qkv, km, H, d, causal, keep, p, dctx):
    """-> fp64 (ctx, P, dqkv) and the fp32 restatement's distance from them (ctx, P, dqkv)."""
    out = {}
    for dt in (torch.float64, torch.float32):
        x = qkv.detach().to(dt).requires_grad_(True)
        ctx, P = restate(x, km, H, d, causal, keep, p, dt)
        ctx.backward(dctx.to(dt))
        out[dt] = (ctx.detach(), P.detach(), x.grad)
    ref = out[torch.float64]
    err32 = tuple(float((a.double() - b).abs().max()) for a, b in zip(out[torch.float32], ref))
    return ref, err32


def _check(got, ref, c, err32, what):
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = (got.double() - ref).abs()
    bar = max(c * scale, 3.0 * err32)
    bad = ~(err <= bar)                 # a NaN (an element nothing wrote) fails too
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} beyond {bar:.3g} (scale {scale:.3g}, err32 {err32:.3g}); "
                             f"at {i}: got {got[i].item()!r}, fp64 {ref[i].item()!r}")


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def make_inputs(B, H, L, d, spread, causal, tag=0):
    """qkv [B, L, 3D], dctx [B, L, D], key mask [B, L]: left padding of varying length, one fully padded sequence (B > 2), random
    holes elsewhere, sequence 0 unpadded."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(((B * 31 + H) * 257 + L) * 1009 + d * 7 + int(spread * 10) + tag)
    D = H * d
    qkv = torch.randn(B, L, 3 * D, device=dev, generator=g) * spread
    dctx = torch.randn(B, L, D, device=dev, generator=g)
    km = (torch.rand(B, L, device=dev, generator=g) > 0.15).to(torch.int64)
    for b in range(B):
        km[b, :(b * 5) % (L // 2 + 1)] = 0
    km[0] = 1
    if B > 2:
        km[2] = 0
    # a fully masked query row is uniform only while |score| < 32: the fp32 ulp of 1e9 is 64, so beyond that the rounding of
    # score + (-1e9) decides the row in the kernel and in the restatement alike.  Sequences with such a row keep their scores below
    # 24: q and k of the sequence are scaled down together.
    allowed = (km != 0)[:, None, :].expand(B, L, L)
    if causal:
        allowed = allowed & torch.ones(L, L, dtype=torch.bool, device=dev).tril()
    has_dead = ~allowed.any(-1).all(-1)                                  # [B]
    q = qkv[..., :D].reshape(B, L, H, d).double()
    k = qkv[..., D:2 * D].reshape(B, L, H, d).double()
    smax = torch.einsum("bihc,bjhc->bhij", q, k).abs().amax(dim=(1, 2, 3)) / math.sqrt(d)
    shrink = torch.where(has_dead & (smax > 24.0), torch.sqrt(24.0 / smax.clamp(min=1e-30)), torch.ones_like(smax)).float()
    qkv[..., :2 * D] *= shrink[:, None, None]
    return qkv, dctx, km


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _digest(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(_bits(t).cpu().numpy().tobytes())
    return h.hexdigest()[:16]


# ---- direct ABI calls -------------------------------------------------------------------------------------------------------------
def wide_keymask(km):
    """km as the middle row of a [B, 3, L] buffer: (view, batch stride 3L); the rows around it hold its complement."""
    B, L = km.shape
    buf = torch.empty(B, 3, L, dtype=torch.int64, device=km.device)
    buf[:, 0], buf[:, 1], buf[:, 2] = 1 - km, km, 1 - km
    return buf[:, 1], 3 * L


def abi_attn(qkv, km, dctx, B, H, L, d, causal, p, seed, stream, step_dev=None):
    """pxr_attn_fwd_f32 + pxr_attn_bwd_f32 the way ops calls them, at strides of their own, outputs pre-filled with NaN and gaps holding
    sentinels.  -> ctx [B, L, D], probs [B, H, L, L], dqkv [B, L, 3D] (fp32, contiguous copies)."""
    from pixelrec_amd import lib as _l

    Lb = _l.load()
    D = H * d
    nan = float("nan")
    # q | k | v at columns 4, D + 8, 2D + 12 of rows of 3D + 16; the gaps hold NaN (an input a kernel must never read)
    ldq, oq, ok, ov = 3 * D + 16, 4, D + 8, 2 * D + 12
    xb = torch.full((B, L, ldq), nan, device="cuda")
    xb[..., oq:oq + D], xb[..., ok:ok + D], xb[..., ov:ov + D] = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    kmv, kms = wide_keymask(km)
    ldc, oc = D + 8, 4                                  # ctx / dctx at column 4 of rows of D + 8
    cb = torch.full((B, L, ldc), SENT, device="cuda")
    cb[..., oc:oc + D] = nan
    probs = torch.full((B, H, L, L), nan, device="cuda")
    cp, ep = _l.c_void_p, lambda t, o: _l.c_void_p(t.data_ptr() + 4 * o)
    sd = _l.ptr(step_dev)
    _l.check(Lb.pxr_attn_fwd_f32(ep(xb, oq), ep(xb, ok), ep(xb, ov), ldq, _l.ptr(kmv), kms, B, H, L, d, ep(cb, oc), ldc, _l.ptr(probs),
                                 p, seed, stream, sd, None, 0, 0, 0, int(causal), _l.stream_ptr()), "pxr_attn_fwd_f32")
    db = torch.full((B, L, ldc), nan, device="cuda")
    db[..., oc:oc + D] = dctx
    ldd, gq, gk, gv = 3 * D + 20, 0, D + 4, 2 * D + 12   # dq | dk | dv: ld_d != ld, gaps of 4 and 8 columns
    gb = torch.full((B, L, ldd), SENT, device="cuda")
    for o in (gq, gk, gv):
        gb[..., o:o + D] = nan
    _l.check(Lb.pxr_attn_bwd_f32(ep(db, oc), ldc, ep(xb, oq), ep(xb, ok), ep(xb, ov), ldq, _l.ptr(probs), B, H, L, d, ep(gb, gq),
                                 ep(gb, gk), ep(gb, gv), ldd, p, seed, stream, sd, None, 0, 0, 0, 0, 0, 0, _l.stream_ptr()),
             "pxr_attn_bwd_f32")
    torch.cuda.synchronize()
    gap_c = torch.ones(ldc, dtype=torch.bool)
    gap_c[oc:oc + D] = False
    gap_g = torch.ones(ldd, dtype=torch.bool)
    for o in (gq, gk, gv):
        gap_g[o:o + D] = False
    assert bool((cb[..., gap_c.cuda()] == SENT).all()), "ctx: a gap column was written"
    assert bool((gb[..., gap_g.cuda()] == SENT).all()), "dq | dk | dv: a gap column was written"
    ctx = cb[..., oc:oc + D].contiguous()
    dqkv = torch.cat([gb[..., o:o + D] for o in (gq, gk, gv)], -1)
    return ctx, probs, dqkv


def rows_attn(qkv, km, dctx, B, H, L, d, causal, p, seed, stream, step_dev=None):
    """The rows path through ops (batched GEMMs + pxr_attn_rows_{fwd,bwd}_f32), key mask as an offset view.  Also checks the saved
    PD against the saved P: exactly 0 where the mask drops, P * inv_keep (the fp32 product) where it keeps; columns L..Lp zero."""
    from pixelrec_amd import ops

    assert ops._attn_takes_gemm_path(L, d)
    kmv, kms = wide_keymask(km)
    ctx, saved = ops.attn_fwd(qkv, kmv, kms, B, H, L, d, p, seed, stream, step_dev=step_dev, causal=causal)
    P, PD = saved
    Lp = (L + 3) & ~3
    assert P.shape == (B * H, L, Lp)
    assert bool((P[..., L:] == 0).all())
    if p > 0:
        keep = attn_keep(seed + (int(step_dev[0]) if step_dev is not None else 0), stream, B, H, L, p, "cuda").view(B * H, L, L)
        want = torch.where(keep, P[..., :L] * torch.tensor(inv_keep(p, torch.float32), device="cuda"), torch.zeros((), device="cuda"))
        assert torch.equal(_bits(PD[..., :L]), _bits(want)), "rows path: PD is not keep * (P * inv_keep)"
        assert bool((PD[..., L:] == 0).all())
    else:
        assert PD is None
    dqkv = ops.attn_bwd(dctx, qkv, saved, B, H, L, d, p, seed, stream, step_dev=step_dev)
    torch.cuda.synchronize()
    return ctx, P[..., :L].reshape(B, H, L, L), dqkv


def run_case(B, H, L, d, causal, p, spread, seed=11, stream=2, tag=0):
    """One shape through whatever the dispatcher picks, checked against fp64 -> digest of ctx, probs, dqkv."""
    from pixelrec_amd import ops

    qkv, dctx, km = make_inputs(B, H, L, d, spread, causal, tag)
    run = rows_attn if ops._attn_takes_gemm_path(L, d) else abi_attn
    ctx, probs, dqkv = run(qkv, km, dctx, B, H, L, d, causal, p, seed, stream)
    keep = attn_keep(seed, stream, B, H, L, p, "cuda")
    (rc, rp, rg), (e_c, e_p, e_g) = reference(qkv, km, H, d, causal, keep, p, dctx)
    what = f"B={B} H={H} L={L} d={d} causal={causal} p={p} spread={spread}"
    _check(ctx, rc, C_CTX, e_c, "ctx " + what)
    _check(probs, rp, C_P, e_p, "probs " + what)
    _check(dqkv, rg, C_GRAD, e_g, "dqkv " + what)
    return ":".join(_digest(t) for t in (ctx, probs, dqkv))


def run_matrix(shapes, ps=PS, spreads=SPREADS):
    out = []
    for (B, H, L, d) in shapes:
        for causal in (True, False):
            for p in ps:
                for spread in spreads:
                    out.append(run_case(B, H, L, d, causal, p, spread))
    from pixelrec_amd import ops
    ops.raise_on_bad_indices()
    return out


# ---- the matrix of the default process --------------------------------------------------------------------------------------------
# (B, H, L, d): B*H never a multiple of 8
FAMILIES = {
    "mfma2": [(3, 3, 1, 8), (5, 3, 2, 64), (3, 5, 51, 128), (5, 1, 37, 8)],
    "mfma1_8": [(5, 3, 52, 64), (3, 3, 63, 8), (3, 5, 64, 128)],
    "mfma_dchunk": [(3, 3, 2, 136), (5, 1, 51, 256), (3, 3, 64, 136)],
    "valu": [(3, 3, 1, 4), (3, 3, 2, 20), (5, 3, 51, 36), (3, 5, 63, 20), (3, 3, 64, 132)],
    "long": [(5, 3, 65, 64), (3, 3, 100, 8), (3, 3, 127, 72), (3, 5, 128, 200)],
    "rows": [(3, 3, 65, 4), (5, 3, 127, 20), (3, 3, 129, 64), (3, 1, 200, 36), (3, 3, 150, 8)],
}
# one grid per family with B*H >= 2048: the grid covers the chip several times over (xcd_remap)
LARGE = {"mfma2": (683, 3, 20, 8), "mfma1_8": (683, 3, 60, 8), "mfma_dchunk": (2049, 1, 12, 136), "valu": (683, 3, 33, 4),
         "long": (2049, 1, 100, 8), "rows": (683, 3, 130, 4)}


def _two(v):
    prev = os.environ.get("PXR_ATTN_TWO")
    os.environ["PXR_ATTN_TWO"] = v
    return prev


def _restore_two(prev):
    if prev is None:
        os.environ.pop("PXR_ATTN_TWO", None)
    else:
        os.environ["PXR_ATTN_TWO"] = prev


@pytest.fixture
def f32_gemms():
    """The rows path's GEMMs on the f32-input MFMA: exact fp32 products, the yardstick of this module."""
    from pixelrec_amd import ops

    prev = ops.set_gemm_mode("f32")
    try:
        yield
    finally:
        ops.set_gemm_mode(prev)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_family_matches_fp64(family, f32_gemms):
    for (B, H, L, d) in FAMILIES[family]:
        assert _family_of(L, d) == family, (family, L, d)
    run_matrix(FAMILIES[family])


def test_mfma1_at_short_lengths_matches_fp64():
    """PXR_ATTN_TWO=0 (read per call): the single-phase kernels at lengths the two-per-CU kernels serve by default."""
    prev = _two("0")
    try:
        run_matrix([(3, 3, 1, 8), (5, 3, 51, 64), (3, 1, 17, 128)])
    finally:
        _restore_two(prev)


@pytest.mark.parametrize("family", list(LARGE))
def test_large_grid_matches_fp64(family, f32_gemms):
    B, H, L, d = LARGE[family]
    assert B * H >= 2048 and _family_of(L, d) == family
    run_matrix([LARGE[family]], ps=(0.1,), spreads=(1.0,))


def test_rows_path_in_default_gemm_mode():
    """The rows path in the process's default GEMM mode (bf16x3 on the exact three-way split) meets the same bars."""
    run_matrix([(3, 3, 129, 64), (3, 3, 65, 4)], ps=(0.1,), spreads=(1.0,))


def _family_of(L, d):
    from pixelrec_amd import ops

    if ops._attn_takes_gemm_path(L, d):
        return "rows"
    if L > 64:
        return "long"
    if d % 8:
        return "valu"
    if d > 128:
        return "mfma_dchunk"
    return "mfma2" if L <= 51 else "mfma1_8"


# ---- seeds ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,L,d", [(3, 3, 40, 64), (3, 3, 60, 8), (3, 1, 50, 136), (3, 3, 33, 20), (3, 3, 100, 64), (3, 3, 140, 8)])
def test_step_dev_is_seed_plus_counter(B, H, L, d, f32_gemms):
    """step_dev = s gives the bits of seed + s without a counter, and the keep mask of seed + s -- also where seed + s wraps past
    2^64; a different stream id gives a different mask."""
    from pixelrec_amd import ops

    p, causal = 0.5, True
    qkv, dctx, km = make_inputs(B, H, L, d, 1.0, causal)
    run = rows_attn if ops._attn_takes_gemm_path(L, d) else abi_attn
    for seed, s in ((11, 5), (2 ** 64 - 3, 7)):
        step = torch.tensor([s], dtype=torch.int64, device="cuda")
        a = run(qkv, km, dctx, B, H, L, d, causal, p, seed, 2, step_dev=step)
        b = run(qkv, km, dctx, B, H, L, d, causal, p, (seed + s) % 2 ** 64, 2)
        for x, y, nm in zip(a, b, ("ctx", "probs", "dqkv")):
            assert torch.equal(_bits(x), _bits(y)), (seed, s, nm)
        keep = attn_keep(seed + s, 2, B, H, L, p, "cuda")
        (rc, rp, rg), (e_c, e_p, e_g) = reference(qkv, km, H, d, causal, keep, p, dctx)
        _check(a[0], rc, C_CTX, e_c, f"ctx seed={seed}+{s}")
        _check(a[2], rg, C_GRAD, e_g, f"dqkv seed={seed}+{s}")
    other = run(qkv, km, dctx, B, H, L, d, causal, p, 11 + 5, 3)
    keep = attn_keep(16, 3, B, H, L, p, "cuda")
    assert not torch.equal(keep, attn_keep(16, 2, B, H, L, p, "cuda"))
    (rc, _, rg), (e_c, _, e_g) = reference(qkv, km, H, d, causal, keep, p, dctx)
    _check(other[0], rc, C_CTX, e_c, "ctx stream 3")
    _check(other[2], rg, C_GRAD, e_g, "dqkv stream 3")
    first = run(qkv, km, dctx, B, H, L, d, causal, p, 16, 2)
    assert not torch.equal(other[0], first[0])


# ---- other output forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,L,d", [(5, 3, 40, 64), (3, 4, 60, 8), (3, 1, 64, 128)])
@pytest.mark.parametrize("causal", [True, False])
def test_planes_and_stat_forms(B, H, L, d, causal):
    """Shapes with attn_planes_supported, dropout on: bf16x3 ctx / dqkv planes are split_planes of the fp32 outputs bit for bit, h2 ctx
    planes within the two-plane fp16 bound, and the stat form leaves exactly max |dqkv|."""
    from pixelrec_amd import ops

    assert ops.attn_planes_supported(L, d) and (H * d) % 32 == 0
    p, seed, stream = 0.1, 21, 4
    qkv, dctx, km = make_inputs(B, H, L, d, 1.0, causal)
    D = H * d
    ctx, probs = ops.attn_fwd(qkv, km, L, B, H, L, d, p, seed, stream, causal=causal)
    keep = attn_keep(seed, stream, B, H, L, p, "cuda")
    (rc, rp, rg), (e_c, e_p, e_g) = reference(qkv, km, H, d, causal, keep, p, dctx)
    _check(ctx, rc, C_CTX, e_c, "ctx")
    cp, _ = ops.attn_fwd(qkv, km, L, B, H, L, d, p, seed, stream, planes=True, causal=causal)
    assert torch.equal(cp.buf, ops.split_planes(ctx.view(B * L, D)).buf)
    h2, _ = ops.attn_fwd(qkv, km, L, B, H, L, d, p, seed, stream, planes="h2", causal=causal)
    assert (h2.to_dense() - ctx.view(B * L, D)).abs().max().item() <= 2.0 ** -21 * float(ctx.abs().max()) + 2.0 ** -24
    dqkv = ops.attn_bwd(dctx, qkv, probs, B, H, L, d, p, seed, stream)
    _check(dqkv, rg, C_GRAD, e_g, "dqkv")
    if (3 * D) % 32 == 0:
        gp = ops.attn_bwd(dctx, qkv, probs, B, H, L, d, p, seed, stream, planes=True)
        assert torch.equal(gp.buf, ops.split_planes(dqkv.view(B * L, 3 * D)).buf)
    st = torch.zeros(ops.ATTN_STAT_SLOTS, device="cuda")
    ds = ops.attn_bwd(dctx, qkv, probs, B, H, L, d, p, seed, stream, stat=st)
    assert torch.equal(_bits(ds), _bits(dqkv))
    assert float(st.max()) == float(dqkv.abs().max())
    ops.raise_on_bad_indices()


# ---- launch knobs (read once per process: each runs in a child) ---------------------------------------------------------------------
VALU_SLICE = [(3, 3, 1, 8), (5, 3, 51, 64), (3, 3, 64, 128), (3, 1, 40, 136), (3, 3, 64, 4)]
ROUTED_SLICE = [(3, 3, 100, 64), (3, 1, 65, 8)]          # 65..128 positions with the MFMA kernels off: the rows path
MFMA1_SLICE = [(3, 3, 1, 8), (5, 3, 51, 64), (3, 3, 52, 8), (3, 5, 64, 128)]


def knob_outputs(kind):
    """A child's slice of the matrix, each case checked against fp64 -> digests."""
    from pixelrec_amd import ops

    if kind == "valu":
        assert not ops.attn_planes_supported(1, 8)              # PXR_ATTN_MFMA=0 took effect
        prev = ops.set_gemm_mode("f32")
        try:
            for (B, H, L, d) in ROUTED_SLICE:
                assert ops._attn_takes_gemm_path(L, d)
            run_matrix(ROUTED_SLICE, ps=(0.0, 0.1), spreads=(1.0,))
        finally:
            ops.set_gemm_mode(prev)
        return run_matrix(VALU_SLICE, spreads=(1.0,))
    return run_matrix(MFMA1_SLICE, spreads=(1.0,))


CHILD = r"""
import sys
sys.path.insert(0, %r)
from tests.test_gpu_attn_ref import knob_outputs
print("DIGESTS " + " ".join(knob_outputs(sys.argv[1])))
""" % ROOT

CHILDREN = {"valu8": ("valu", {"PXR_ATTN_MFMA": "0"}), "valu4": ("valu", {"PXR_ATTN_MFMA": "0", "PXR_ATTN_WAVES": "4"}),
            "valu16": ("valu", {"PXR_ATTN_MFMA": "0", "PXR_ATTN_WAVES": "16"}), "mfma1_4": ("mfma1", {"PXR_ATTN_MFMA_WAVES": "4"})}


def test_launch_knobs_match_fp64_and_each_other():
    """Four children (at most four at once, no retries): the VALU kernels at NW = 8 / 4 / 16 (PXR_ATTN_MFMA=0, PXR_ATTN_WAVES) and
    mfma1<4> (PXR_ATTN_MFMA_WAVES=4), each against fp64 in the child; mfma1<4> agrees with mfma1<8> (run here, PXR_ATTN_TWO=0) bit for
    bit.  The VALU kernels at different NW are held to the fp64 bars only: the source gives each row the same operations in the same
    order whichever wave owns it, but the build lets the compiler contract a * b + c * d into an FMA around either product, and it
    vectorises the three instantiations differently (packed FMAs over row pairs), so the roundings differ.  With contraction off
    (`#pragma clang fp contract(off)` over attention.hip) NW = 4 / 8 / 16 do agree bit for bit."""
    procs = {}
    for name, (kind, extra) in CHILDREN.items():
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(extra)
        procs[name] = subprocess.Popen([sys.executable, "-c", CHILD, kind], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                                       stderr=subprocess.PIPE, text=True)
    prev = _two("0")
    try:
        mfma1_8 = run_matrix(MFMA1_SLICE, spreads=(1.0,))
    except BaseException:
        for q in procs.values():
            q.kill()
        raise
    finally:
        _restore_two(prev)
    digests = {}
    for name, pr in procs.items():
        try:
            so, se = pr.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs.values():
                q.kill()
            raise
        assert pr.returncode == 0, f"child {name}: {se[-3000:]}"
        digests[name] = [l for l in so.splitlines() if l.startswith("DIGESTS ")][-1].split()[1:]
    for name in ("valu4", "valu8", "valu16"):
        assert len(digests[name]) == 2 * len(PS) * len(VALU_SLICE), name
    differ = [(i, x, y) for i, (x, y) in enumerate(zip(digests["mfma1_4"], mfma1_8)) if x != y]
    assert len(digests["mfma1_4"]) == len(mfma1_8) and not differ, differ
