"""tests/gemm_epi_restate.py (the fp64 reference of tests/test_gpu_gemm_epilogues.py) against torch itself: the restated
activations equal torch.nn.functional's, and every restated closed-form derivative equals fp64 autograd of the restated
activation on a grid that straddles 0 and reaches |v| = 8 (without 0 itself for relu and selu, whose derivative jumps there)."""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_epi_restate as R


def _grid(with_zero):
    # k / 256 for k = -2048 .. 2048 (exact in fp64: 0 and both end points are on the grid); without 0: the same grid minus k = 0
    k = torch.arange(-2048, 2049, dtype=torch.float64)
    v = (k if with_zero else k[k != 0]) / 256.0
    assert float(v.abs().max()) == 8.0 and bool((v < 0).any()) and bool((v > 0).any())
    assert bool((v == 0).any()) == with_zero
    return v


def _autograd(fn, v):
    v = v.clone().requires_grad_(True)
    fn(v).sum().backward()
    return v.grad


def test_codes_are_the_librarys():
    from pixelrec_amd import ops

    for name in ("EPI_NONE", "EPI_BIAS", "EPI_BIAS_GELU", "EPI_MUL_DGELU", "EPI_ADD", "EPI_BIAS_GELU_GRAD", "EPI_MUL", "EPI_BIAS_ADD",
                 "EPI_BIAS_QGELU_GRAD", "EPI_BIAS_RELU", "EPI_BIAS_ACT_GRAD", "EPI_BIAS_QGELU"):
        assert getattr(R, name) == getattr(ops, name), name
    assert {"relu": R.ACT_RELU, "swish": R.ACT_SWISH, "tanh": R.ACT_TANH, "sigmoid": R.ACT_SIGMOID, "selu": R.ACT_SELU} == ops.ACT_CODES
    assert len(set(R.ACTS)) == 5


def test_activations_are_torchs():
    v = _grid(True)
    assert (R.gelu(v) - F.gelu(v)).abs().max().item() < 1e-15
    assert (R.qgelu(v) - v * torch.sigmoid(1.702 * v)).abs().max().item() == 0.0
    assert torch.equal(R.act_fn(v, R.ACT_RELU), F.relu(v))
    assert (R.act_fn(v, R.ACT_SWISH) - F.silu(v)).abs().max().item() < 1e-15
    assert torch.equal(R.act_fn(v, R.ACT_TANH), torch.tanh(v))
    assert torch.equal(R.act_fn(v, R.ACT_SIGMOID), torch.sigmoid(v))
    assert (R.act_fn(v, R.ACT_SELU) - F.selu(v)).abs().max().item() < 1e-15


@pytest.mark.parametrize("name,fn,dfn,with_zero", [
    ("gelu", R.gelu, R.dgelu, True),
    ("quick_gelu", R.qgelu, R.dqgelu, True),
    ("relu", lambda v: R.act_fn(v, R.ACT_RELU), lambda v: R.act_grad(v, R.ACT_RELU), False),
    ("swish", lambda v: R.act_fn(v, R.ACT_SWISH), lambda v: R.act_grad(v, R.ACT_SWISH), True),
    ("tanh", lambda v: R.act_fn(v, R.ACT_TANH), lambda v: R.act_grad(v, R.ACT_TANH), True),
    ("sigmoid", lambda v: R.act_fn(v, R.ACT_SIGMOID), lambda v: R.act_grad(v, R.ACT_SIGMOID), True),
    ("selu", lambda v: R.act_fn(v, R.ACT_SELU), lambda v: R.act_grad(v, R.ACT_SELU), False),
])
def test_restated_derivative_is_fp64_autograd_of_the_restated_activation(name, fn, dfn, with_zero):
    v = _grid(with_zero)
    got, ref = dfn(v), _autograd(fn, v)
    # two fp64 evaluations of one smooth function of |v| <= 8, |f'| <= 1.13 (gelu') and a few roundings each
    assert (got - ref).abs().max().item() <= 1e-14, name


def test_selu_and_relu_take_the_negative_branch_at_zero():
    """torch's backward gives relu'(0) = 0 and selu'(0) = scale * alpha; so do the kernels (v > 0 decides)."""
    z = torch.zeros(1, dtype=torch.float64)
    assert R.act_grad(z, R.ACT_RELU).item() == 0.0 == _autograd(F.relu, z).item()
    assert R.act_grad(z, R.ACT_SELU).item() == R.SELU_SCALE * R.SELU_ALPHA
    assert abs(_autograd(F.selu, z).item() - R.SELU_SCALE * R.SELU_ALPHA) < 1e-15


def test_epilogue_table():
    g = torch.Generator().manual_seed(0)
    pre, aux = torch.randn(5, 7, generator=g, dtype=torch.float64), torch.randn(5, 7, generator=g, dtype=torch.float64)
    b = torch.randn(7, generator=g, dtype=torch.float64)
    v = pre + b
    for epi, (c, a) in {
        R.EPI_NONE: (pre, None), R.EPI_BIAS: (v, None), R.EPI_BIAS_GELU: (F.gelu(v), v), R.EPI_BIAS_GELU_GRAD: (F.gelu(v), R.dgelu(v)),
        R.EPI_MUL_DGELU: (pre * R.dgelu(aux), None), R.EPI_ADD: (pre + aux, None), R.EPI_MUL: (pre * aux, None),
        R.EPI_BIAS_ADD: (v + aux, None), R.EPI_BIAS_QGELU_GRAD: (R.qgelu(v), R.dqgelu(v)), R.EPI_BIAS_QGELU: (R.qgelu(v), None),
        R.EPI_BIAS_RELU: (F.relu(v), None),
    }.items():
        C, ao = R.epilogue(epi, pre, b, aux)
        assert (C - c).abs().max().item() < 1e-15, epi
        assert (ao is None) == (a is None) == (epi not in R.WRITES_AUX), epi
        if a is not None:
            assert torch.equal(ao, a), epi
    for act in R.ACTS:
        C, ao = R.epilogue(R.EPI_BIAS_ACT_GRAD, pre, b, None, act)
        assert torch.equal(C, R.act_fn(v, act)) and torch.equal(ao, R.act_grad(v, act))
    # the same formulas in fp32 (the yardstick of the GPU test) stay fp32
    C, ao = R.epilogue(R.EPI_BIAS_GELU_GRAD, pre.float(), b.float())
    assert C.dtype == torch.float32 and ao.dtype == torch.float32
    with pytest.raises(ValueError):
        R.epilogue(R.EPI_ADD, pre)
