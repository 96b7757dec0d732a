"""The LayerNorm entries (csrc/layernorm.hip) against a float64 restatement of the same operation, computed from the exact fp32 inputs
each kernel was given: the gather site (ops.input_ln_fwd), the residual site (ops.ln_residual_fwd, with and without `res`) and the
backward of both (ops.ln_bwd, both gather modes and the `res=` form).  Shapes reach every VEC branch of ln_vec_for, partial float4
groups (D not a multiple of 256), idle waves (rows not a multiple of 4), partial last blocks of the two-stage dgamma / dbeta reduction
(rows_per_block = 4 and > 4, and a stage 2 over ~1 000 partials), SASRec's id stride 2(L+1) with padding ids, and the launch policies
PXR_LN_RPW2_ROWS / PXR_LN_STAGE_ROWS / PXR_LN_NT (read once per process: each runs in a child process).

Tolerances come from fp32 rounding, not from what passes: U = 4 unit roundoffs (2^-24) per operation, times sqrt(D) for a row
reduction; the mean's rounding is charged relative to the row's spread (rstd * mean|z|), so a catastrophic cancellation shows; the
column sums dgamma / dbeta get 1e-5 * sum|terms| per column."""
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
U = 4 * 2.0 ** -24
DS = (4, 12, 36, 100, 260, 512, 768, 1028, 2052, 4096)   # VEC 1, 1, 1, 1, 2, 2, 4, 8, 16, 16
ROWS = ((1, 1), (1, 3), (5, 1), (17, 241))               # (B, L): rows 1, 3, 5, 4097
BIG = (2002, 50)                                         # 100 100 rows: rows_per_block 98, 1 022 partials, the last one partial
EPS = (1e-12, 1e-5)


def _close(got, ref, tol, what):
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)              # a NaN fails too
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} beyond tolerance; at {i}: got {got[i].item()!r}, "
                             f"fp64 {ref[i].item()!r}, tol {tol[i].item() if torch.is_tensor(tol) else tol!r}")


def _keep(seed, stream, rows, D, p, dev):
    if p == 0.0:
        return None
    return torch.from_numpy(keep_mask(seed, stream, (rows, D), p)).to(dev)


def _inv_keep(p):
    return 1.0 / (1.0 - float(np.float32(p)))


def _ln64(z, gamma, beta, eps):
    """nn.LayerNorm in float64 (biased variance, two-pass) -> (y, xhat, rstd, tolerances of y / xhat / rstd)."""
    D = z.shape[-1]
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + float(np.float32(eps)))
    xhat = (z - mean) * rstd
    g, b = gamma.double(), beta.double()
    y = xhat * g + b
    s = U * math.sqrt(D)
    m = rstd * z.abs().mean(-1, keepdim=True)       # the rounding of the fp32 mean, in units of the row's spread
    t_xhat = s * (xhat.abs() + 1.0 + m)
    t_y = t_xhat * g.abs() + U * (y.abs() + b.abs())
    t_rstd = rstd * (s + (s * m) ** 2)              # (a mean off by d adds d^2 to the two-pass variance)
    return y, xhat, rstd.squeeze(-1), t_y, t_xhat, t_rstd.squeeze(-1)


def _check_fwd(y, xhat, rstd, z64, gamma, beta, eps, keep=None, p=0.0, what=""):
    rows, D = z64.shape
    yr, xr, rr, ty, tx, tr = _ln64(z64, gamma, beta, eps)
    if keep is not None:         # the gather site: dropout AFTER the LayerNorm
        k = _inv_keep(p)
        yr = torch.where(keep, yr * k, torch.zeros_like(yr))
        ty = (ty + U * yr.abs()) * k
    _close(rstd.view(rows), rr, tr, f"{what} rstd")
    _close(xhat.reshape(rows, D), xr, tx, f"{what} xhat")
    _close(y.reshape(rows, D), yr, ty, f"{what} y")


def _params(D, dev, g):
    gamma = torch.randn(D, device=dev, generator=g) * 0.8 + 0.2
    beta = torch.randn(D, device=dev, generator=g) * 0.5
    return gamma, beta


def _items(B, L, N, dev, g):
    """SASRec's [B, 2, L+1] windows (the gather reads items[b, 0, t], stride 2(L+1)), a share of them padding id 0."""
    items = torch.randint(0, N, (B, 2, L + 1), device=dev, generator=g)
    items[torch.rand(items.shape, device=dev, generator=g) < 0.15] = 0
    items[0, 0, 0] = 0
    return items


def _gather_case(B, L, D, eps, p, seed=0, planes=False):
    from pixelrec_amd import ops

    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1000 * D + 7 * B + L)
    N = 97
    table = torch.randn(N, D, device=dev, generator=g) + 0.5
    table[0] = 0.0                                  # padding_idx row
    pos = torch.randn(L, D, device=dev, generator=g) * 0.5
    gamma, beta = _params(D, dev, g)
    items = _items(B, L, N, dev, g)
    out = ops.input_ln_fwd(table, items, 2 * (L + 1), B, L, pos, gamma, beta, eps, p, seed, 0, planes=planes)
    ids = items[:, 0, :L]
    z64 = (table.double()[ids] + pos.double()[None]).reshape(B * L, D)
    _check_fwd(*out[:3], z64, gamma, beta, eps, _keep(seed, 0, B * L, D, p, dev), p, f"input_ln_fwd B={B} L={L} D={D} eps={eps} p={p}")
    return out


def _residual_case(rows, D, eps, p, with_res, seed=0, planes=False, cancel=False):
    from pixelrec_amd import ops

    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(3000 * D + rows + int(with_res))
    if cancel:                                      # rows of 1e3 + N(0, 1e-2)
        x = 1e3 + torch.randn(rows, D, device=dev, generator=g) * 1e-2
        res = torch.randn(rows, D, device=dev, generator=g) * 1e-2 if with_res else None
    else:
        x = torch.randn(rows, D, device=dev, generator=g) + 0.3
        res = torch.randn(rows, D, device=dev, generator=g) if with_res else None
    gamma, beta = _params(D, dev, g)
    out = ops.ln_residual_fwd(x, res, gamma, beta, eps, p, seed, 5, planes=planes)
    keep = _keep(seed, 5, rows, D, p, dev)
    if cancel:                                      # z exactly as the kernel forms it (one fp32 add), the LayerNorm in fp64
        z64 = (x if res is None else x + res).double()
    else:
        z64 = x.double()
        if keep is not None:                        # the residual site: dropout on x BEFORE the residual add
            z64 = torch.where(keep, z64 * _inv_keep(p), torch.zeros_like(z64))
        if res is not None:
            z64 = z64 + res.double()
    _check_fwd(*out[:3], z64, gamma, beta, eps, what=f"ln_residual_fwd rows={rows} D={D} eps={eps} p={p} res={with_res}")
    return out, z64


@pytest.mark.parametrize("D", DS)
def test_input_ln_fwd_matches_fp64(D):
    for B, L in ROWS:
        for eps in EPS:
            _gather_case(B, L, D, eps, 0.0)


def test_input_ln_fwd_dropout_and_many_rows_match_fp64():
    _gather_case(17, 241, 260, 1e-12, 0.1, seed=99)
    _gather_case(*BIG, 36, 1e-12, 0.0)


@pytest.mark.parametrize("D", DS)
def test_ln_residual_fwd_matches_fp64(D):
    for B, L in ROWS:
        for with_res in (True, False):
            for eps in EPS:
                _residual_case(B * L, D, eps, 0.0, with_res)


def test_ln_residual_fwd_dropout_and_many_rows_match_fp64():
    _residual_case(4097, 100, 1e-12, 0.1, True, seed=123)
    _residual_case(BIG[0] * BIG[1], 36, 1e-5, 0.0, True)


@pytest.mark.parametrize("D", (100, 512, 4096))
def test_ln_residual_fwd_no_variance_cancellation(D):
    """Rows of 1e3 + N(0, 1e-2): E[z^2] - mean^2 in fp32 is all rounding here (ulp(1e6) = 0.06 against a variance of 1e-4); the
    header promises a two-pass variance from registers.  rstd within 1e-3 of fp64, xhat / y within the rounding bound."""
    for with_res in (False, True):
        (y, xhat, rstd), z64 = _residual_case(37, D, 1e-12, 0.0, with_res, cancel=True)
        rr = 1.0 / torch.sqrt(z64.var(-1, unbiased=False) + float(np.float32(1e-12)))
        rel = ((rstd.double() - rr) / rr).abs()
        assert bool(torch.isfinite(rstd).all()) and rel.max().item() <= 1e-3, rel.max().item()


def _bwd_inputs(rows, D, dev, g):
    """xhat (normalised rows, as fp32), rstd > 0, gamma, the upstream gradient."""
    z = torch.randn(rows, D, device=dev, generator=g, dtype=torch.float64)
    xhat = ((z - z.mean(-1, keepdim=True)) / z.std(-1, unbiased=False, keepdim=True).clamp_min(1e-3)).float()
    rstd = (torch.rand(rows, device=dev, generator=g) * 1.5 + 0.5)
    gamma = torch.randn(D, device=dev, generator=g) * 0.8 + 0.2
    dy = torch.randn(rows, D, device=dev, generator=g)
    return xhat, rstd, gamma, dy


def _bwd64(d, xhat, rstd, gamma):
    """LayerNorm backward in float64 from the kernel's fp32 inputs -> (dz, its tolerance)."""
    D = d.shape[-1]
    a = d * gamma.double()
    ax = a * xhat.double()
    c1, c2 = a.mean(-1, keepdim=True), ax.mean(-1, keepdim=True)
    r = rstd.double()[:, None]
    dz = r * (a - c1 - xhat.double() * c2)
    tol = U * math.sqrt(D) * r * (a.abs() + a.abs().mean(-1, keepdim=True) + xhat.double().abs() * ax.abs().mean(-1, keepdim=True))
    return dz, tol


def _bwd_case(gather_mode, rows, D, p=0.0, with_res=False, seed=0):
    from pixelrec_amd import ops

    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(5000 * D + rows + 2 * gather_mode + int(with_res))
    xhat, rstd, gamma, dy = _bwd_inputs(rows, D, dev, g)
    res = torch.randn(rows, D, device=dev, generator=g) if with_res else None
    dgamma, dbeta = torch.empty(D, device=dev), torch.empty(D, device=dev)
    dz, dx = ops.ln_bwd(gather_mode, dy, xhat, rstd, gamma, dgamma, dbeta, p, seed, 3, need_dx=(gather_mode == 0 and p > 0), res=res)
    what = f"ln_bwd(gather_mode={gather_mode}) rows={rows} D={D} p={p} res={with_res}"
    keep = _keep(seed, 3, rows, D, p, dev)
    d = dy.double()
    if gather_mode and keep is not None:            # dy is w.r.t. dropout(LN(z)): the mask goes on dy
        d = torch.where(keep, d * _inv_keep(p), torch.zeros_like(d))
    dz_ref, tol = _bwd64(d, xhat, rstd, gamma)
    if res is not None:                             # dz = res + LayerNorm-backward
        dz_ref = res.double() + dz_ref
        tol = tol + U * dz_ref.abs()
    _close(dz, dz_ref, tol, f"{what} dz")
    if gather_mode == 0 and keep is not None:       # dx = dropout-mask(dz) / (1 - p): the gradient w.r.t. the sub-layer output
        k = _inv_keep(p)
        _close(dx, torch.where(keep, dz_ref * k, torch.zeros_like(dz_ref)), (tol + U * dz_ref.abs()) * k, f"{what} dx")
    else:
        assert dx is None
    gx = d * xhat.double()
    _close(dgamma, gx.sum(0), 1e-5 * gx.abs().sum(0) + 1e-30, f"{what} dgamma")
    _close(dbeta, d.sum(0), 1e-5 * d.abs().sum(0) + 1e-30, f"{what} dbeta")


@pytest.mark.parametrize("D", DS)
def test_ln_bwd_matches_fp64(D):
    for B, L in ROWS:
        for gm in (0, 1):
            _bwd_case(gm, B * L, D)
    _bwd_case(0, 5, D, with_res=True)


def test_ln_bwd_dropout_res_and_many_rows_match_fp64():
    for gm in (0, 1):
        _bwd_case(gm, 4097, 260, p=0.1, seed=77)
        _bwd_case(gm, BIG[0] * BIG[1], 36)
        _bwd_case(gm, BIG[0] * BIG[1] + 3, 4)
    _bwd_case(0, 4097, 1028, with_res=True)
    _bwd_case(0, BIG[0] * BIG[1], 36, with_res=True)


# ---- launch policies ---------------------------------------------------------------------------------------------------------------
def _digest(*ts):
    h = hashlib.sha256()
    for t in ts:
        if t is not None:
            h.update(t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def policy_outputs():
    """Every case of a policy run, each checked against fp64; -> sha256 of each case's fp32 outputs (and the planes of y).  Covers
    RPW = 2 (D <= 1024; rows % 8 != 0 leaves idle waves), the staged planes (planes, D % 32 == 0, 256 <= D <= 1024) and the
    streaming stores, on both forward sites, the fused loss head and the backward."""
    from pixelrec_amd import ops

    out = []
    for (B, L, D, p, planes) in ((5, 1, 36, 0.0, False), (17, 241, 260, 0.1, False), (17, 241, 512, 0.0, True),
                                 (1, 3, 768, 0.0, True), (17, 241, 768, 0.1, "h2"), (3, 1, 1028, 0.0, False)):
        r = _gather_case(B, L, D, 1e-12, p, seed=4, planes=planes)
        out.append(_digest(*r[:3], r[3].to_dense() if planes else None))
        (y, xhat, rstd, *yp), _ = _residual_case(B * L, D, 1e-5, p, True, seed=6, planes=planes)
        out.append(_digest(y, xhat, rstd, yp[0].to_dense() if planes else None))
    dev = "cuda"
    for (B, L, D, p) in ((17, 241, 512, 0.1), (5, 1, 100, 0.0)):
        g = torch.Generator(device=dev).manual_seed(D + B)
        x, res = torch.randn(B, L, D, device=dev, generator=g), torch.randn(B, L, D, device=dev, generator=g)
        gamma, beta = _params(D, dev, g)
        table = torch.randn(300, D, device=dev, generator=g) * 0.1
        items = _items(B, L, 300, dev, g)
        mask = (torch.rand(B, L, device=dev, generator=g) < 0.8).long()
        y, xhat, rstd, loss, pos, neg = ops.ln_residual_bpr_fwd(x, res, gamma, beta, 1e-12, table, items, mask, p, 8, 2)
        z64 = torch.where(_keep(8, 2, B * L, D, p, dev), x.double().view(B * L, D) * _inv_keep(p), torch.zeros(1, device=dev,
                          dtype=torch.float64)) if p else x.double().view(B * L, D)
        _check_fwd(y, xhat, rstd, z64 + res.double().view(B * L, D), gamma, beta, 1e-12, what=f"ln_residual_bpr_fwd B={B} L={L} D={D}")
        out.append(_digest(y, xhat, rstd, loss, pos, neg))
    for (rows, D) in ((4097, 260), (5, 1028)):
        for gm in (0, 1):
            _bwd_case(gm, rows, D, p=0.1, seed=9)
    ops.raise_on_bad_indices("cuda")
    return out


CHILD = r"""
import sys
sys.path.insert(0, %r)
from tests.test_gpu_ln_ref import policy_outputs
print("DIGESTS " + " ".join(policy_outputs()))
""" % ROOT

POLICIES = {"default": {}, "rpw2": {"PXR_LN_RPW2_ROWS": "0"}, "stage": {"PXR_LN_STAGE_ROWS": "0"}, "nt": {"PXR_LN_NT": "7"}}


def test_launch_policies_match_fp64_and_default_bit_for_bit():
    procs = {}
    for name, extra in POLICIES.items():
        env = {k: v for k, v in os.environ.items() if k not in ("PXR_LN_RPW2_ROWS", "PXR_LN_STAGE_ROWS", "PXR_LN_NT")}
        env.update(extra)
        procs[name] = subprocess.Popen([sys.executable, "-c", CHILD], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                                       stderr=subprocess.PIPE, text=True)
    digests = {}
    for name, pr in procs.items():
        try:
            so, se = pr.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs.values():
                q.kill()
            raise
        assert pr.returncode == 0, f"policy {name}: {se[-3000:]}"
        digests[name] = [l for l in so.splitlines() if l.startswith("DIGESTS ")][-1].split()[1:]
    for name in ("rpw2", "stage", "nt"):
        assert digests[name] == digests["default"], name
