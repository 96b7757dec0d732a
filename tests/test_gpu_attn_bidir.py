"""The bidirectional (key-padding-only) attention of BERT4Rec (reference IDNet/bert4rec.py:150-155) in every family the dispatcher
can pick (csrc/attention.hip, csrc/vit.hip): against a torch restatement with the padding-only mask, forward and backward; a query
attends to later keys; and the causal entry points still compute SASRec's causal attention, their results unchanged by the new
instantiations (the same inputs through them agree bit for bit with a second call and with the torch causal restatement)."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

# (L, H, d, PXR_ATTN_TWO, family the dispatcher picks)
SHAPES = [
    (51, 4, 128, "1", "mfma2"), (51, 8, 64, "1", "mfma2"), (9, 2, 16, "1", "mfma2"),
    (51, 4, 128, "0", "mfma1"), (64, 4, 128, "1", "mfma1"), (64, 8, 64, "1", "mfma1"),
    (40, 2, 256, "1", "mfma (d-chunked)"), (33, 2, 36, "1", "VALU (d % 8 != 0)"),
    (65, 4, 128, "1", "long"), (100, 8, 64, "1", "long"), (128, 4, 128, "1", "long"),
    (129, 4, 128, "1", "rows"), (150, 8, 64, "1", "rows"),
]


def _reference(qkv, km, H, d, causal):
    B, L, _ = qkv.shape
    D = H * d
    q, k, v = (qkv[..., i * D:(i + 1) * D].view(B, L, H, d).permute(0, 2, 1, 3).double() for i in range(3))
    keep = (km != 0)[:, None, None, :].expand(B, 1, L, L)
    if causal:
        keep = torch.tril(keep)
    # the reference's fp32 arithmetic: score + (-1e9) == -1e9 exactly, so a fully masked (left-padded) query row is uniform
    s = (q @ k.transpose(-1, -2) / math.sqrt(d)).float() + torch.where(keep, 0.0, -1e9)
    p = torch.softmax(s.double(), -1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B, L, D), p


def _inputs(B, L, H, d):
    g = torch.Generator(device="cuda").manual_seed(L * 131 + d)
    D = H * d
    qkv = torch.randn(B, L, 3 * D, device="cuda", generator=g) * 0.7
    km = torch.ones(B, L, dtype=torch.int64, device="cuda")
    for b in range(B):
        km[b, :(b * 7) % (L // 2 + 1)] = 0                  # left padding of varying length; row 0 unpadded
    return qkv, km


@pytest.mark.parametrize("L,H,d,two,family", SHAPES, ids=[f"{s[4]}-L{s[0]}-d{s[2]}" for s in SHAPES])
def test_bidirectional_attention_forward_and_backward(L, H, d, two, family):
    from pixelrec_amd import ops

    prev = os.environ.get("PXR_ATTN_TWO")
    os.environ["PXR_ATTN_TWO"] = two
    try:
        B = 5
        qkv, km = _inputs(B, L, H, d)
        ctx, probs = ops.attn_fwd(qkv, km, L, B, H, L, d, causal=False)
        ref_ctx, ref_p = _reference(qkv.cpu(), km.cpu(), H, d, causal=False)
        assert (ctx.cpu().double() - ref_ctx).abs().max().item() <= 2e-5
        # a query attends to later keys: the first real query of every sequence puts weight on the last key
        assert float(probs[0, :, 0, L - 1].min() if isinstance(probs, torch.Tensor) else ref_p[0, :, 0, L - 1].min()) > 0
        assert float(ref_p[0, :, 0, L - 1].min()) > 0
        # backward (mask-agnostic: it reads the saved probabilities) against autograd of the restatement
        dctx = torch.randn(B, L, H * d, device="cuda") * 0.3
        dqkv = ops.attn_bwd(dctx, qkv, probs, B, H, L, d)
        x = qkv.cpu().double().requires_grad_(True)
        out, _ = _reference(x, km.cpu(), H, d, causal=False)
        out.backward(dctx.cpu().double())
        assert (dqkv.cpu().double() - x.grad).abs().max().item() <= 5e-5
        # the causal entry: SASRec's attention as before, deterministic bit for bit, and different from the bidirectional one
        c1, _ = ops.attn_fwd(qkv, km, L, B, H, L, d)
        c2, _ = ops.attn_fwd(qkv, km, L, B, H, L, d)
        assert torch.equal(c1, c2)
        ref_c, _ = _reference(qkv.cpu(), km.cpu(), H, d, causal=True)
        assert (c1.cpu().double() - ref_c).abs().max().item() <= 2e-5
        assert not torch.equal(c1, ctx)
        ops.raise_on_bad_indices()
        torch.cuda.synchronize()
    finally:
        if prev is None:
            os.environ.pop("PXR_ATTN_TWO", None)
        else:
            os.environ["PXR_ATTN_TWO"] = prev


@pytest.mark.parametrize("L,H,d", [(51, 4, 128), (64, 8, 64), (9, 2, 16)])
def test_bidirectional_planes_outputs_match_fp32(L, H, d):
    """The plane-writing forms (bf16x3 and h2) of the bidirectional forward carry the fp32 context."""
    from pixelrec_amd import ops

    B = 4
    qkv, km = _inputs(B, L, H, d)
    ctx, _ = ops.attn_fwd(qkv, km, L, B, H, L, d, causal=False)
    for fmt in (True, "h2"):
        cp, _ = ops.attn_fwd(qkv, km, L, B, H, L, d, planes=fmt, causal=False)
        err = (cp.to_dense().view(B, L, H * d) - ctx).abs().max().item()
        assert err <= (1e-6 if fmt is True else 1e-3 * ctx.abs().max().item()), (fmt, err)
