"""The yardstick of tests/test_gpu_attn_ref.py, pinned without a GPU: its float64 restatement of the sequence attention agrees with
torch's scaled_dot_product_attention, keeps the reference's uniform fully masked rows, applies the kernels' dropout mask in the kernels'
index order and scale; and ops routes each shape to the family the dispatcher table names."""
import math

import numpy as np
import pytest
import torch

from oracle.dropout_rng import keep_mask
from tests.test_gpu_attn_ref import attn_keep, inv_keep, restate


def _inputs(B, H, L, d, spread, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, L, 3 * H * d, generator=g) * spread
    km = (torch.rand(B, L, generator=g) > 0.3).to(torch.int64)
    for b in range(B):
        km[b, :b % (L // 2 + 1)] = 0
    km[0] = 1
    return qkv, km


def _allowed(km, L, causal):
    a = (km != 0)[:, None, None, :].expand(km.shape[0], 1, L, L)
    return a & torch.ones(L, L, dtype=torch.bool).tril() if causal else a


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B,H,L,d", [(3, 2, 1, 4), (4, 3, 17, 8), (3, 2, 70, 20)])
def test_restatement_matches_sdpa_on_live_rows(B, H, L, d, causal):
    qkv, km = _inputs(B, H, L, d, 1.0, L * 7 + d)
    ctx, P = restate(qkv, km, H, d, causal)
    D = H * d
    q, k, v = (qkv[..., i * D:(i + 1) * D].reshape(B, L, H, d).permute(0, 2, 1, 3).double() for i in range(3))
    allowed = _allowed(km, L, causal)
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=torch.where(allowed, 0.0, -1e9).double())
    ref = ref.permute(0, 2, 1, 3).reshape(B, L, D)
    live = allowed.any(-1)[:, 0].unsqueeze(-1)                                  # [B, L, 1]: query rows with a real key
    assert bool(live.any())
    # the restatement rounds q.k / sqrt(d) to fp32 before the mask: agreement to fp32 resolution of the scores
    assert float(((ctx - ref) * live).abs().max()) < 1e-5
    assert torch.allclose(P.sum(-1), torch.ones((), dtype=torch.float64))


@pytest.mark.parametrize("causal", [True, False])
def test_fully_masked_rows_are_uniform_below_score_32(causal):
    B, H, L, d = 3, 2, 9, 8
    qkv, km = _inputs(B, H, L, d, 1.0, 5)
    km[1] = 0                                                      # a fully padded sequence
    km[2, :4] = 0                                                  # left padding: causal rows 0..3 are fully masked
    D = H * d
    s = torch.einsum("bihc,bjhc->bhij", qkv[..., :D].reshape(B, L, H, d).double(), qkv[..., D:2 * D].reshape(B, L, H, d).double())
    assert float(s.abs().max()) / math.sqrt(d) < 32
    _, P = restate(qkv, km, H, d, causal)
    dead = ~_allowed(km, L, causal).any(-1)[:, 0]                 # [B, L]
    assert bool(dead[1].all()) and (not causal or bool(dead[2, :4].all()))
    rows = P.permute(0, 2, 1, 3)[dead]                              # [n, H, L]
    assert torch.equal(rows, torch.full_like(rows, 1.0 / L))
    # beyond 32 the fp32 rounding of score + (-1e9) decides: the row is no longer uniform
    big = qkv.clone()
    big[1, :, :2 * D] *= 20.0
    _, Pb = restate(big, km, H, d, causal)
    assert not torch.equal(Pb[1], torch.full_like(Pb[1], 1.0 / L))


def test_dropout_scaling_and_index_order_match_the_counter_hash():
    B, H, L, d = 2, 3, 5, 4
    qkv, km = _inputs(B, H, L, d, 1.0, 9)
    p, seed, stream = 0.5, 123, 4
    keep = attn_keep(seed, stream, B, H, L, p, "cpu")
    flat = keep_mask(seed, stream, (B * H * L * L,), p)
    for (b, h, i, j) in ((0, 0, 0, 0), (1, 2, 4, 3), (0, 1, 3, 2), (1, 0, 2, 4)):
        assert bool(keep[b, h, i, j]) == bool(flat[((b * H + h) * L + i) * L + j])
    assert 0 < int(keep.sum()) < keep.numel()
    ctx, P = restate(qkv, km, H, d, True, keep, p)
    ctx0, P0 = restate(qkv, km, H, d, True)
    assert torch.equal(P, P0)                                        # the saved probabilities are the pre-dropout ones
    assert inv_keep(p) == 1.0 / (1.0 - float(np.float32(p))) == 2.0
    assert inv_keep(0.1) == 1.0 / (1.0 - float(np.float32(0.1))) and inv_keep(0.1) != 1.0 / 0.9
    D = H * d
    v = qkv[..., 2 * D:].reshape(B, L, H, d).permute(0, 2, 1, 3).double()
    want = torch.zeros(B, H, L, d, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            for i in range(L):
                for j in range(L):
                    if flat[((b * H + h) * L + i) * L + j]:
                        want[b, h, i] += P0[b, h, i, j] * 2.0 * v[b, h, j]
    assert torch.allclose(ctx, want.permute(0, 2, 1, 3).reshape(B, L, D), rtol=0, atol=1e-13)
    assert attn_keep(seed, stream, B, H, L, 0.0, "cpu") is None


@pytest.mark.parametrize("mfma", [True, False])
def test_routing_follows_the_dispatch_table(mfma, monkeypatch):
    from pixelrec_amd import ops

    monkeypatch.setattr(ops, "attn_planes_supported", lambda L, d: mfma and L <= 64 and d <= 128 and d % 8 == 0)
    for L in (1, 2, 51, 52, 63, 64):
        for d in (4, 8, 20, 64, 128, 136, 256):
            assert not ops._attn_takes_gemm_path(L, d), (L, d)             # fused: mfma2 / mfma1 / d-chunked / VALU
    for L in (65, 100, 127, 128):
        for d in (8, 64, 72, 200):
            assert ops._attn_takes_gemm_path(L, d) is (not mfma), (L, d)  # long kernel; rows path with the MFMA kernels off
        for d in (4, 20, 36):
            assert ops._attn_takes_gemm_path(L, d), (L, d)                 # d % 8 != 0: rows path
    for L in (129, 200, 513):
        for d in (4, 8, 64, 136):
            assert ops._attn_takes_gemm_path(L, d), (L, d)
