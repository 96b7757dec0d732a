"""The polynomial erf of the GELU epilogues (pixelrec_amd/csrc/gemm_epi.cuh::pxr_erff), restated in numpy with the SAME
coefficients (read out of the header, so that the two cannot drift apart) and fp32 FMAs emulated through fp64: maximum error
against the fp64 erf over [-6, 6] below 1 ulp / 6e-8 absolute -- the error class of the library erff it replaces, far inside the
+-2e-5 activation / +-1e-4 logit budgets (BASELINE.json).  Reference: REC/model/layers.py:651-660 (erf-GELU).  The kernels
themselves are held to the reference's activations on the GPU (tests/test_gpu_sasrec.py, sasrec_act.npz)."""
import os
import re

import numpy as np
from scipy.special import erf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _coefficients():
    src = open(os.path.join(ROOT, "pixelrec_amd", "csrc", "gemm_epi.cuh")).read()
    body = src[src.index("float pxr_erff(float a)"):src.index("// erf-GELU as the reference writes it")]
    hexes = [float.fromhex(h) for h in re.findall(r"-?0x1\.[0-9a-f]+p[+-]?\d+", body)]
    assert len(hexes) == 13, hexes         # 7 of the large branch (incl. the switch point's neighbours), 6 of the small one
    return body, hexes


def _erf_poly(a, c):
    a = a.astype(F)
    t, s = np.abs(a), (a * a).astype(F)
    r = _fma(F(c[0]), t, F(c[1]))
    u = _fma(F(c[2]), t, F(c[3]))
    r = _fma(r, s, u)
    for k in (4, 5, 6):
        r = _fma(r, t, F(c[k]))
    r = _fma(r, t, t)
    big = np.copysign((F(1.0) - np.exp2(-1.44269504088896340736 * r.astype(np.float64)).astype(F)).astype(F), a)
    q = np.full_like(a, F(c[7]))
    for k in range(8, 13):
        q = _fma(q, s, F(c[k]))
    small = _fma(q, a, a)
    return np.where(t > F(0.921875), big, small)


def test_erf_polynomial_is_below_one_ulp():
    body, c = _coefficients()
    assert "0.921875f" in body
    x = np.linspace(-6.0, 6.0, 2_000_001).astype(F)
    ref = erf(x.astype(np.float64))
    got = _erf_poly(x, c).astype(np.float64)
    err = np.abs(got - ref)
    ulp = np.spacing(np.abs(ref).astype(F)).astype(np.float64)
    assert err.max() < 6e-8 and (err / ulp).max() < 1.0, (err.max(), (err / ulp).max())
    # odd, saturating, exact zero
    assert _erf_poly(np.array([0.0], F), c)[0] == 0.0 and _erf_poly(np.array([9.0, -9.0], F), c).tolist() == [1.0, -1.0]


def test_gelu_and_its_derivative_from_the_polynomial():
    """gelu(x) = x/2 (1 + erf(x/sqrt 2)) and gelu'(x) = Phi(x) + x phi(x) as the epilogue forms them: against fp64."""
    _, c = _coefficients()
    x = np.linspace(-8.0, 8.0, 400_001).astype(F)
    e = _erf_poly((x * F(0.70710678118654752440)).astype(F), c)
    g = (x * F(0.5) * (F(1.0) + e)).astype(F)
    cdf = (F(0.5) * (F(1.0) + e)).astype(F)
    pdf = (F(0.39894228040143267794) * np.exp2((F(-0.72134752044448170368) * x * x).astype(np.float64)).astype(F)).astype(F)
    dg = (cdf + x * pdf).astype(F)
    x64 = x.astype(np.float64)
    g_ref = x64 * 0.5 * (1.0 + erf(x64 / np.sqrt(2.0)))
    dg_ref = 0.5 * (1.0 + erf(x64 / np.sqrt(2.0))) + x64 * np.exp(-0.5 * x64 * x64) / np.sqrt(2.0 * np.pi)
    assert np.abs(g - g_ref).max() < 5e-7 and np.abs(dg - dg_ref).max() < 3e-7, (np.abs(g - g_ref).max(), np.abs(dg - dg_ref).max())
