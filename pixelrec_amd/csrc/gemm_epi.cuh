// gemm_epi.cuh -- everything about the GEMM epilogues, in one place: the codes, which operands each one needs, the element
// formulas, the epilogues each operand flavour is instantiated for and the host-side operand check.  Shared by the four GEMM
// families (gemm_f32.hip incl. stream-K, gemm_b3.hip, the planes and fp16 two-plane kernels of gemm_p3.hip) and score_topk.hip.
// A new epilogue is one line in PXR_EPI_TABLE, one branch in epi_elem and one entry in the flavour lists below.
#pragma once
#include "pxr_common.h"

namespace pxr {

enum { EPI_NONE = 0, EPI_BIAS = 1, EPI_BIAS_GELU = 2, EPI_MUL_DGELU = 3, EPI_ADD = 4, EPI_BIAS_GELU_GRAD = 5, EPI_MUL = 6,
       // the ViT blocks of the PixelNet image encoder (HF CLIPEncoderLayer; reference load.py:90-120):
       EPI_BIAS_ADD = 7,          // C = acc + bias + aux            (out_proj / fc2 + residual stream)
       EPI_BIAS_QGELU_GRAD = 8,   // C = quick_gelu(acc + bias), aux = quick_gelu'(acc + bias)   (CLIP MLP fc1)
       EPI_BIAS_RELU = 9,         // C = relu(acc + bias)            (rec_fc of MeanItemEncoder, layers.py:121-128)
       // the other hidden_act choices of the reference's FeedForward (layers.py:642-649: relu / swish / tanh / sigmoid):
       EPI_BIAS_ACT_GRAD = 10,    // C = act(acc + bias), aux = act'(acc + bias); act = GemmBatch::act
       EPI_LAST = 10,
       // planes GEMMs only (gemm_p3.hip): quick_gelu(acc + bias) without the derivative -- the frozen blocks of the image tower
       EPI_BIAS_QGELU = 11 };
enum { ACT_RELU = 3, ACT_SWISH = 4, ACT_TANH = 5, ACT_SIGMOID = 6,
       ACT_SELU = 7 };      // F.selu (model/ViNet/curatornet.py:67-82), not one of ACT2FN
// selu(x) = s x for x > 0, else s a (exp(x) - 1); torch's backward takes the negative branch at x == 0 (derivative s a)
#define PXR_SELU_SCALE 1.0507009873554804934193349852946f
#define PXR_SELU_ALPHA 1.6732632423543772848170429916717f

// ---- which operands an epilogue needs: X(code, adds bias[col], reads aux, writes aux) -------------------------------------------
#define PXR_EPI_TABLE(X)          \
  X(EPI_NONE, 0, 0, 0)            \
  X(EPI_BIAS, 1, 0, 0)            \
  X(EPI_BIAS_GELU, 1, 0, 1)       \
  X(EPI_MUL_DGELU, 0, 1, 0)       \
  X(EPI_ADD, 0, 1, 0)             \
  X(EPI_BIAS_GELU_GRAD, 1, 0, 1)  \
  X(EPI_MUL, 0, 1, 0)             \
  X(EPI_BIAS_ADD, 1, 1, 0)        \
  X(EPI_BIAS_QGELU_GRAD, 1, 0, 1) \
  X(EPI_BIAS_RELU, 1, 0, 0)       \
  X(EPI_BIAS_ACT_GRAD, 1, 0, 1)   \
  X(EPI_BIAS_QGELU, 1, 0, 0)
struct EpiOperands {
  bool has_bias, reads_aux, writes_aux;
};
// by epilogue code, for host code (an unknown code needs nothing: the dispatchers reject it)
constexpr EpiOperands epi_operands(int epilogue) {
  switch (epilogue) {
#define PXR_EPI_ROW(E, B, R, W) \
  case E: return EpiOperands{B != 0, R != 0, W != 0};
    PXR_EPI_TABLE(PXR_EPI_ROW)
#undef PXR_EPI_ROW
  }
  return EpiOperands{false, false, false};
}
template <int EPI>
struct EpiTraits {
  static constexpr bool HAS_BIAS = epi_operands(EPI).has_bias;
  static constexpr bool READS_AUX = epi_operands(EPI).reads_aux;
  static constexpr bool WRITES_AUX = epi_operands(EPI).writes_aux;
};
// the check of every GEMM entry point, before any HIP call: a missing operand never reaches a kernel
static inline bool epi_operands_ok(const char* who, int epilogue, const float* bias, const float* aux) {
  const EpiOperands o = epi_operands(epilogue);
  if (o.has_bias && !bias) {
    pxr_set_error("%s: epilogue %d needs a bias", who, epilogue);
    return false;
  }
  if ((o.reads_aux || o.writes_aux) && !aux) {
    pxr_set_error("%s: epilogue %d reads / writes aux", who, epilogue);
    return false;
  }
  return true;
}

// ---- the epilogues each operand flavour is instantiated for: X(code) ---------------------------------------------------------------
// forward (KC,KC): Y = X W^T;  input gradient (KC,XC): dX = dY W.  The families differ in two codes, stated once each.
#define PXR_EPI_FWD(X)                                                                                             \
  X(EPI_NONE) X(EPI_BIAS) X(EPI_BIAS_GELU) X(EPI_BIAS_GELU_GRAD) X(EPI_BIAS_ADD) X(EPI_BIAS_QGELU_GRAD) X(EPI_BIAS_RELU) \
  X(EPI_BIAS_ACT_GRAD)
#define PXR_EPI_BWD(X) X(EPI_NONE) X(EPI_ADD) X(EPI_MUL)
#define PXR_EPI_FWD_PLANES(X) PXR_EPI_FWD(X) X(EPI_BIAS_QGELU)      // planes / h2: + quick_gelu without its derivative
#define PXR_EPI_BWD_F32(X) PXR_EPI_BWD(X) X(EPI_MUL_DGELU)          // f32 / bf16x3: + the product with gelu'(saved pre-activation)

// erf for the GELU epilogues: two branch-free polynomial pieces (|x| <= 0.921875: x + x P(x^2); beyond: 1 - exp(-Q(|x|)), one
// v_exp_f32), both evaluated and selected -- 16 FMAs + one exponential per element where the library erff costs ~60 VALU
// slots with its divergent ranges.  The fc1 epilogue (3.3 M elements per launch at B = 64) is pure VALU time behind the last
// MFMA: profiles/r05.  Maximum error 0.97 ulp = 5.8e-8 absolute against the fp64 erf over [-6, 6] (4 M points, the committed
// check tests/test_erf_poly_cpu.py restates this function in numpy) -- the library's own error class.
__device__ __forceinline__ float pxr_erff(float a) {
  // (every product / sum is an explicit single operation: the result must not depend on what the compiler contracts into FMAs
  // in the epilogue it is inlined into -- gelu'(x) saved by the forward equals gelu'(x) recomputed by the backward bit for bit)
  const float t = fabsf(a), s = __fmul_rn(a, a);
  float r = fmaf(0x1.222900p-16f, t, -0x1.91d2ccp-12f);
  const float u = fmaf(0x1.fd1336p-09f, t, -0x1.8d6300p-06f);
  r = fmaf(r, s, u);
  r = fmaf(r, t, 0x1.b55cb0p-4f);
  r = fmaf(r, t, 0x1.450aa0p-1f);
  r = fmaf(r, t, 0x1.079d0cp-3f);
  r = fmaf(r, t, t);
  const float big = copysignf(__fsub_rn(1.0f, __builtin_amdgcn_exp2f(__fmul_rn(-1.44269504088896340736f, r))), a);
  float q = -0x1.3a1a82p-11f;
  q = fmaf(q, s, 0x1.473f48p-08f);
  q = fmaf(q, s, -0x1.b68bd2p-06f);
  q = fmaf(q, s, 0x1.ce1a46p-04f);
  q = fmaf(q, s, -0x1.8126e0p-02f);
  q = fmaf(q, s, 0x1.06eba6p-03f);
  const float small = fmaf(q, a, a);
  return t > 0.921875f ? big : small;
}
// erf-GELU as the reference writes it: x * 0.5 * (1 + erf(x / sqrt(2)))  (layers.py:651-660)
__device__ __forceinline__ float gelu_erf(float x) {
  return __fmul_rn(__fmul_rn(x, 0.5f), __fadd_rn(1.0f, pxr_erff(__fmul_rn(x, 0.70710678118654752440f))));
}
// CLIP's quick_gelu: x * sigmoid(1.702 x), and its derivative s + 1.702 x s (1 - s)
__device__ __forceinline__ float sigmoid_1702(float x) { return 1.0f / (1.0f + __expf(-1.702f * x)); }
__device__ __forceinline__ float dgelu_erf(float x) {
  const float cdf = __fmul_rn(0.5f, __fadd_rn(1.0f, pxr_erff(__fmul_rn(x, 0.70710678118654752440f))));
  const float pdf = __fmul_rn(0.39894228040143267794f, __builtin_amdgcn_exp2f(__fmul_rn(-0.72134752044448170368f, __fmul_rn(x, x))));
  return fmaf(x, pdf, cdf);
}

// One element of epilogue EPI: v = the accumulator, bv = bias[col], av = the aux operand where the epilogue reads one; returns
// C and sets aux_out where EpiTraits<EPI>::WRITES_AUX.  The only statement of the formulas: every family calls it.
template <int EPI>
__device__ __forceinline__ float epi_elem(float v, float bv, float av, float& aux_out, int act) {
  if constexpr (EPI == EPI_BIAS) {
    v += bv;
  } else if constexpr (EPI == EPI_BIAS_GELU) {
    v += bv;
    aux_out = v;                  // pre-activation, kept for the backward pass
    v = gelu_erf(v);
  } else if constexpr (EPI == EPI_BIAS_GELU_GRAD) {
    v += bv;
    aux_out = dgelu_erf(v);       // gelu'(pre-activation): the backward is then one multiply
    v = gelu_erf(v);
  } else if constexpr (EPI == EPI_MUL) {
    v *= av;
  } else if constexpr (EPI == EPI_MUL_DGELU) {
    v *= dgelu_erf(av);
  } else if constexpr (EPI == EPI_ADD) {
    v += av;                      // residual-branch gradient joins here
  } else if constexpr (EPI == EPI_BIAS_ADD) {
    v = (v + bv) + av;
  } else if constexpr (EPI == EPI_BIAS_QGELU_GRAD) {
    v += bv;
    const float sg = sigmoid_1702(v);
    aux_out = sg + 1.702f * v * sg * (1.0f - sg);
    v = v * sg;
  } else if constexpr (EPI == EPI_BIAS_RELU) {
    v = fmaxf(v + bv, 0.f);
  } else if constexpr (EPI == EPI_BIAS_QGELU) {
    v += bv;
    v = v * sigmoid_1702(v);
  } else if constexpr (EPI == EPI_BIAS_ACT_GRAD) {
    v += bv;
    float dv;
    if (act == ACT_RELU) {                    // F.relu
      dv = v > 0.f ? 1.f : 0.f; v = fmaxf(v, 0.f);
    } else if (act == ACT_SWISH) {            // x * sigmoid(x)   (layers.py:662-663)
      const float sg = 1.0f / (1.0f + __expf(-v));
      dv = sg + v * sg * (1.0f - sg); v = v * sg;
    } else if (act == ACT_TANH) {
      const float th = tanhf(v);
      dv = 1.0f - th * th; v = th;
    } else if (act == ACT_SELU) {             // exp of min(x, 0) only: a large positive x never makes an inf
      const float sa = PXR_SELU_SCALE * PXR_SELU_ALPHA, ex = __expf(fminf(v, 0.f));
      dv = v > 0.f ? PXR_SELU_SCALE : sa * ex;
      v = v > 0.f ? PXR_SELU_SCALE * v : sa * (ex - 1.0f);
    } else {                                  // sigmoid
      const float sg = 1.0f / (1.0f + __expf(-v));
      dv = sg * (1.0f - sg); v = sg;
    }
    aux_out = dv;
  }
  return v;
}

}  // namespace pxr
