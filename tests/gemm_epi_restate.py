"""Plain torch restatements of every GEMM epilogue (pixelrec_amd/csrc/gemm_epi.cuh::epi_elem, which all four GEMM families call) as functions of (pre, bias, aux, act) -> (C, aux_out): `pre` is the accumulator (the product), `bias` a row vector or None, `aux`
the operand the epilogue reads (residual / saved derivative / saved pre-activation) or None, `act` one of the ACT_* codes of
EPI_BIAS_ACT_GRAD.  aux_out is what the epilogue WRITES to aux (None when it writes nothing).

Every formula works in the dtype of its input: on fp64 inputs it is the reference, on fp32 inputs it is the yardstick "the
same formula evaluated by torch in fp32" of tests/test_gpu_gemm_epilogues.py.  The closed-form derivatives are held to fp64
autograd of the activations in tests/test_gemm_epi_restate_cpu.py.

Reference: erf-GELU REC/model/layers.py:651-660, swish :662-663, ACT2FN :642-649, F.selu (ViNet/curatornet.py:67-82), CLIP's
quick_gelu x * sigmoid(1.702 x)."""
import math

import torch

EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_MUL_DGELU, EPI_ADD = 0, 1, 2, 3, 4
EPI_BIAS_GELU_GRAD, EPI_MUL, EPI_BIAS_ADD, EPI_BIAS_QGELU_GRAD, EPI_BIAS_RELU, EPI_BIAS_ACT_GRAD = 5, 6, 7, 8, 9, 10
EPI_BIAS_QGELU = 11
ACT_RELU, ACT_SWISH, ACT_TANH, ACT_SIGMOID, ACT_SELU = 3, 4, 5, 6, 7
ACTS = (ACT_RELU, ACT_SWISH, ACT_TANH, ACT_SIGMOID, ACT_SELU)

SELU_SCALE = 1.0507009873554804934193349852946
SELU_ALPHA = 1.6732632423543772848170429916717
QGELU_SLOPE = 1.702

READS_AUX = (EPI_MUL_DGELU, EPI_ADD, EPI_MUL, EPI_BIAS_ADD)
WRITES_AUX = (EPI_BIAS_GELU, EPI_BIAS_GELU_GRAD, EPI_BIAS_QGELU_GRAD, EPI_BIAS_ACT_GRAD)
HAS_BIAS = (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_GRAD, EPI_BIAS_ADD, EPI_BIAS_QGELU_GRAD, EPI_BIAS_RELU, EPI_BIAS_ACT_GRAD,
            EPI_BIAS_QGELU)
# results that go through erf / exp / tanh: compared with a tolerance, everything else is exact fp32 arithmetic
TRANSCENDENTAL = (EPI_BIAS_GELU, EPI_MUL_DGELU, EPI_BIAS_GELU_GRAD, EPI_BIAS_QGELU_GRAD, EPI_BIAS_QGELU)


def gelu(v):
    return v * 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0)))


def dgelu(v):
    """gelu'(v) = Phi(v) + v phi(v)"""
    return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def qgelu(v):
    return v * torch.sigmoid(QGELU_SLOPE * v)


def dqgelu(v):
    s = torch.sigmoid(QGELU_SLOPE * v)
    return s + QGELU_SLOPE * v * s * (1.0 - s)


def act_fn(v, act):
    if act == ACT_RELU:
        return torch.clamp_min(v, 0.0)
    if act == ACT_SWISH:
        return v * torch.sigmoid(v)
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    if act == ACT_SELU:       # the exponential of min(v, 0) only, like the kernels (and no inf * 0 in autograd)
        return torch.where(v > 0, SELU_SCALE * v, SELU_SCALE * SELU_ALPHA * (torch.exp(torch.clamp_max(v, 0.0)) - 1.0))
    raise ValueError(f"act {act}")


def act_grad(v, act):
    if act == ACT_RELU:
        return (v > 0).to(v.dtype)
    if act == ACT_SWISH:
        s = torch.sigmoid(v)
        return s + v * s * (1.0 - s)
    if act == ACT_TANH:
        t = torch.tanh(v)
        return 1.0 - t * t
    if act == ACT_SIGMOID:
        s = torch.sigmoid(v)
        return s * (1.0 - s)
    if act == ACT_SELU:       # torch's backward takes the negative branch at v == 0
        return torch.where(v > 0, torch.full_like(v, SELU_SCALE), SELU_SCALE * SELU_ALPHA * torch.exp(torch.clamp_max(v, 0.0)))
    raise ValueError(f"act {act}")


def epilogue(epi, pre, bias=None, aux=None, act=0):
    """(C, aux_out) of epilogue `epi`."""
    if epi in HAS_BIAS and bias is not None:
        v = pre + bias
    else:
        v = pre
    if epi in READS_AUX and aux is None:
        raise ValueError(f"epilogue {epi} reads aux")
    if epi == EPI_NONE or epi == EPI_BIAS:
        return v, None
    if epi == EPI_BIAS_GELU:
        return gelu(v), v
    if epi == EPI_BIAS_GELU_GRAD:
        return gelu(v), dgelu(v)
    if epi == EPI_MUL_DGELU:
        return v * dgelu(aux), None
    if epi == EPI_ADD:
        return v + aux, None
    if epi == EPI_MUL:
        return v * aux, None
    if epi == EPI_BIAS_ADD:
        return v + aux, None
    if epi == EPI_BIAS_QGELU_GRAD:
        return qgelu(v), dqgelu(v)
    if epi == EPI_BIAS_QGELU:
        return qgelu(v), None
    if epi == EPI_BIAS_RELU:
        return torch.clamp_min(v, 0.0), None
    if epi == EPI_BIAS_ACT_GRAD:
        return act_fn(v, act), act_grad(v, act)
    raise ValueError(f"epilogue {epi}")
