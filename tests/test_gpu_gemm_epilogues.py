"""Every GEMM epilogue on every tile the dispatchers accept, on ragged shapes, in dense and strided output layouts, for the four
GEMM families (pxr_gemm_f32 on the f32-input MFMA incl. stream-K, the bf16x3 kernels of gemm_b3, the planes GEMMs of gemm_p3 /
gemm_p4, the fp16 two-plane pxr_gemm_h2_f32); and pxr_gemm_batched_f32 called directly, across its launch cut at 65 535 problems.

What is asserted, per (family, tile, shape):
  * P = this tile's own fp32 result of EPI_BIAS (forward flavour) / EPI_NONE (input-gradient flavour) against fp64 matmul, with
    the bound of tests/test_gpu_gemm*.py (2e-6 sqrt(K) max|ref| + 1e-6; h2: 4e-6 sqrt(K) max|ref| + 1e-9 as tests/test_gpu_h2.py).
  * the kernels are deterministic, so every other epilogue of the same tile starts from the same accumulator bits.  Epilogues that
    are plain fp32 arithmetic are therefore held to torch's fp32 arithmetic on P BIT FOR BIT (bias+add, add, mul, relu, the saved
    pre-activation, ACT_RELU and its 0/1 derivative).
  * epilogues that go through erf / exp / tanh are compared with the fp64 restatement (tests/gemm_epi_restate.py) evaluated ON P
    -- only the activation's own fp32 evaluation is measured, not the GEMM.  Yardstick: the same restatement evaluated by torch in
    fp32 on P.  The kernel is allowed 4x the yardstick's maximum error (the factor tests/test_gpu_gemm_b3.py gives one fp32 path
    over another), no floor.  W is scaled so that max |P| = 7.5 < 8: branches are decided on P itself, nothing is excluded.
  * four layouts per case: dense, (ldc, ldaux) = (N + 4, N + 8) (16-byte rows: the vector path stays on), (N + 1, N + 3) (rows
    lose their alignment: the planes kernels must fall back to scalar stores) and (N + 4, N + 3) (only aux loses it: one unaligned
    operand must switch BOTH off).  C and aux are views of [M + 2, ld] buffers pre-filled with a NaN pattern: pad columns and the
    two extra rows must keep that pattern bit for bit, operands the epilogue only reads must come back unchanged, and the
    layouts must agree bit for bit.  Output planes (N % 32 == 0): to_dense() == C.

Shapes are the smallest that reach the edges: (300, N, K) gives 2x2 tiles of the largest tile (256x256), ragged in both
directions, and the ragged column edge of the 256-wide tiles lies in their SECOND epilogue pass (EPI_COLS = 128 of gemm_p4.cuh:
columns 384 ..); N = 456 (N % 8 == 0: vector path), 452 (N % 8 == 4: scalar path, 4-wide last chunk), 451 (N % 4 != 0), 448
(N % 32 == 0: the x-contiguous B of the planes input gradient, output planes) and (1, 8, 32).  The stream-K tile 6464 runs the
same shapes at K = 128 with 37 workers (the entry point hands fewer than 4 K tiles to the tile-per-workgroup kernel).

(family, tile, epilogue) triples covered: f32 13 tiles (stream-K 6464 included) x (8 forward + 4 input-gradient) = 156,
bf16x3 3 x 12 = 36, planes 12 x (9 + 3) = 144, h2 7 x (9 + 3) = 84: 420, each on ragged shapes in all four layouts.
EPI_BIAS_ACT_GRAD: the planes / h2 entry points take `act`, all five activations run on every tile; pxr_gemm_f32 has no such
argument, a direct call runs the kernel's last branch (sigmoid) -- that is what every f32 / bf16x3 tile is held to -- and the
five activations go through ops.linear_fwd(act=...) in both GEMM modes at a shape of the 64x64 tile and one of the 128x128 tile
(1281).  Left out: the (XC, XC) weight-gradient flavour (EPI_NONE only; tests/test_gpu_gemm*.py and the split-K / grouped tests
hold it bit for bit).

Measured on an MI355X, largest kernel error / yardstick error over all families, tiles and shapes (the bound is 4; no floor was
needed): gelu 1.00, gelu' 1.00, mul_dgelu 2.71 (the 8 elements of (1, 8, 128) on the stream-K tile; at most 1.08 elsewhere),
qgelu 1.11, qgelu' 1.00, swish 1.13, swish' 1.00, tanh 1.00, tanh' 1.09, sigmoid 1.09, sigmoid' 1.05, selu 1.00, selu' 1.01.
Each test prints its own ratios (`pytest -s`: lines starting with EPI_RATIO).  The determinism premise -- two epilogues on one
tile see the same accumulators -- held on every tile."""
import functools

import pytest
import torch

from tests import gemm_epi_restate as R
from tests.test_gpu_gemm import TILES as _F32_LIST
from tests.test_gpu_gemm_b3 import B3_TILES as _B3_LIST
from tests.test_gpu_gemm_p3 import TILES as _P3_LIST
from tests.test_gpu_h2 import H2_TILES as _H2_LIST

pytestmark = pytest.mark.gpu

SK_TILE = 6464
F32_TILES = sorted(set(_F32_LIST) | {0, 641, 128611, SK_TILE})
B3_TILES = sorted(set(_B3_LIST) | {0, 9064, 91281})
P3_TILES = sorted(set(_P3_LIST) | {0, 406406461, 412806441})
H2_TILES = sorted(set(_H2_LIST) | {0})

FWD_SHAPES = [(300, 456, 64), (300, 452, 32), (300, 451, 32), (300, 448, 64), (1, 8, 32)]
BWD_SHAPES_F32 = [(300, 456, 64), (300, 452, 32), (300, 448, 64), (1, 8, 32)]      # B is [K, N] with ldb = N: N % 4 == 0
BWD_SHAPES_PLANES = [(300, 448, 64), (1, 32, 32)]                                  # B planes [K, N]: N % 32 == 0
LAYOUTS = [(0, 0), (4, 8), (1, 3), (4, 3)]                                        # (ldc - N, ldaux - N)
SENTINEL = 0x7FC0BEEF                                                               # a quiet NaN with a payload
P_MAX = 7.5

FWD_EPIS_F32 = [R.EPI_NONE, R.EPI_BIAS_GELU, R.EPI_BIAS_GELU_GRAD, R.EPI_BIAS_ADD, R.EPI_BIAS_QGELU_GRAD, R.EPI_BIAS_RELU,
                R.EPI_BIAS_ACT_GRAD]                                                # (+ EPI_BIAS: the launch that gives P)
FWD_EPIS_PLANES = FWD_EPIS_F32 + [R.EPI_BIAS_QGELU]
BWD_EPIS_F32 = [R.EPI_MUL_DGELU, R.EPI_ADD, R.EPI_MUL]                              # (+ EPI_NONE: P)
BWD_EPIS_PLANES = [R.EPI_ADD, R.EPI_MUL]
NAMES = {R.ACT_SWISH: "swish", R.ACT_TANH: "tanh", R.ACT_SIGMOID: "sigmoid", R.ACT_SELU: "selu"}


def _tol(ref, K):
    return 2e-6 * (K ** 0.5) * float(ref.abs().max()) + 1e-6


def _tol_h2(ref, K):
    return 4e-6 * (K ** 0.5) * float(ref.abs().max()) + 1e-9


@functools.lru_cache(maxsize=None)
def _inputs(M, N, K, b_kc):
    """Operands of one shape (shared by every tile and family, never modified), scaled so that the fp64 result peaks at P_MAX."""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K + (0 if b_kc else 5))
    x = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) if b_kc else torch.randn(K, N, generator=g)
    b = torch.randn(N, generator=g) if b_kc else None
    aux = (torch.randn(M, N, generator=g) * 2.0).clamp_(-P_MAX, P_MAX)               # residual / saved derivative / saved pre-activation
    pre = x.double() @ (W.double().t() if b_kc else W.double())
    if b_kc:
        pre = pre + b.double()
    s = P_MAX / float(pre.abs().max())
    W = (W * s).cuda()
    b = (b * s).cuda() if b_kc else None
    x, aux = x.cuda(), aux.cuda()
    prod = x.double() @ (W.double().t() if b_kc else W.double())                     # the fp64 product of the fp32 operands
    return {"x": x, "W": W, "b": b, "aux": aux, "prod": prod, "pre": prod + b.double() if b_kc else prod}


@functools.lru_cache(maxsize=None)
def _planes(M, N, K, b_kc, h2):
    from pixelrec_amd import ops

    d = _inputs(M, N, K, b_kc)
    if h2:
        return tuple(ops.split_planes_multi([d["x"], d["W"]], h2=True))
    return ops.split_planes(d["x"]), ops.split_planes(d["W"])


def _sentinel_buf(rows, ld):
    t = torch.empty(rows, ld, device="cuda")
    t.view(torch.int32).fill_(SENTINEL)
    return t


def _pad_untouched(buf, M, N):
    iv = buf.view(torch.int32)
    return bool((iv[M:] == SENTINEL).all()) and bool((iv[:M, N:] == SENTINEL).all())


class _Case:
    """One (family, tile, shape, flavour): launches epilogues into sentinel buffers and returns views of what they wrote."""

    def __init__(self, family, tile, M, N, K, b_kc):
        self.family, self.tile, self.M, self.N, self.K, self.b_kc = family, tile, M, N, K, b_kc
        self.d = _inputs(M, N, K, b_kc)
        self.planes = family in ("planes", "h2")
        if self.planes:
            self.Ap, self.Bp = _planes(M, N, K, b_kc, family == "h2")
        self.want_cp = self.planes and N % 32 == 0
        self.tag = f"{family} tile {tile} ({M},{N},{K}) b_kc={b_kc}"

    def run(self, epi, layout, act=0):
        """-> (C, aux_out): views [M, N] of fresh sentinel buffers (aux_out: None unless the epilogue writes aux).  Checks the
        canaries, that an aux the epilogue only reads comes back unchanged, and the output planes."""
        from pixelrec_amd import ops

        M, N, K, d = self.M, self.N, self.K, self.d
        ldc, ldaux = N + layout[0], N + layout[1]
        what = f"{self.tag} epi {epi} act {act} layout {layout}"
        cbuf = _sentinel_buf(M + 2, ldc)
        C = cbuf[:M, :N]
        abuf = aux = None
        if epi in R.READS_AUX or epi in R.WRITES_AUX:
            abuf = _sentinel_buf(M + 2, ldaux)
            aux = abuf[:M, :N]
            if epi in R.READS_AUX:
                aux.copy_(d["aux"])
        bias = d["b"] if epi in R.HAS_BIAS else None
        if self.planes:
            Cp = ops.Planes.alloc(M, N, "cuda") if self.want_cp else None
            ops.gemm_planes(self.Ap, self.Bp, C, epi, bias=bias, aux=aux, act=act, tile_hint=self.tile, b_kc=self.b_kc, Cp=Cp)
            if Cp is not None:
                assert torch.equal(Cp.to_dense(), C), what + ": output planes != C"
        else:
            sk = self.tile == SK_TILE
            ops.gemm(True, self.b_kc, M, N, K, d["x"], K, d["W"], K if self.b_kc else N, C, ldc, epi, bias=bias, aux=aux,
                     ldaux=ldaux if aux is not None else 0, use_ws=False, tile_hint=self.tile, split_hint=37 if sk else 0)
        assert _pad_untouched(cbuf, M, N), what + ": C written outside [M, N]"
        assert not bool(torch.isnan(C).any()), what + ": C not (fully) written"
        if abuf is not None:
            assert _pad_untouched(abuf, M, N), what + ": aux written outside [M, N]"
            if epi in R.READS_AUX:
                assert torch.equal(aux, d["aux"]), what + ": a read-only aux was modified"
            else:
                assert not bool(torch.isnan(aux).any()), what + ": aux not (fully) written"
        return C, (aux if epi in R.WRITES_AUX else None)


def _record(name, e_k, e_y, seen):
    seen[name] = max(seen.get(name, 0.0), e_k / e_y if e_y > 0 else float("inf") if e_k > 0 else 0.0)


def _check_transcendental(what, name, got, fn, args, seen):
    """got against fn(fp64 args); allowed 4x the error of fn(fp32 args) -- the same formula, by torch, in fp32."""
    ref = fn(*[a.double() for a in args])
    yard = fn(*args)
    assert yard.dtype == torch.float32
    e_k, e_y = torch.stack([(got.double() - ref).abs().max(), (yard.double() - ref).abs().max()]).tolist()
    _record(name, e_k, e_y, seen)
    assert e_k <= 4.0 * e_y, f"{what}: {name} kernel error {e_k:.3e} > 4 x yardstick error {e_y:.3e}"


def _check_epilogue(tag, a, epi, act, P, C, aux_out, seen):
    """One epilogue's dense-layout result against P = the same tile's pre-activation (forward) / plain product (input gradient);
    a = the aux operand the reading epilogues were given."""
    what = f"{tag} epi {epi} act {act}"
    if epi == R.EPI_BIAS_ADD or epi == R.EPI_ADD:
        assert torch.equal(C, P + a), what
    elif epi == R.EPI_MUL:
        assert torch.equal(C, P * a), what
    elif epi == R.EPI_BIAS_RELU:
        assert torch.equal(C, torch.clamp_min(P, 0.0)), what
    elif epi == R.EPI_MUL_DGELU:
        _check_transcendental(what, "mul_dgelu", C, lambda p, s: p * R.dgelu(s), (P, a), seen)
    elif epi == R.EPI_BIAS_GELU:
        assert torch.equal(aux_out, P), what + ": saved pre-activation"
        _check_transcendental(what, "gelu", C, R.gelu, (P,), seen)
    elif epi == R.EPI_BIAS_GELU_GRAD:
        _check_transcendental(what, "gelu", C, R.gelu, (P,), seen)
        _check_transcendental(what, "gelu'", aux_out, R.dgelu, (P,), seen)
    elif epi == R.EPI_BIAS_QGELU_GRAD:
        _check_transcendental(what, "qgelu", C, R.qgelu, (P,), seen)
        _check_transcendental(what, "qgelu'", aux_out, R.dqgelu, (P,), seen)
    elif epi == R.EPI_BIAS_QGELU:
        assert aux_out is None
        _check_transcendental(what, "qgelu", C, R.qgelu, (P,), seen)
    elif epi == R.EPI_BIAS_ACT_GRAD:
        if act == R.ACT_RELU:
            assert torch.equal(C, torch.clamp_min(P, 0.0)), what
            assert torch.equal(aux_out, (P > 0).float()), what + ": relu'"
        else:
            n = NAMES[act]
            _check_transcendental(what, n, C, lambda p: R.act_fn(p, act), (P,), seen)
            _check_transcendental(what, n + "'", aux_out, lambda p: R.act_grad(p, act), (P,), seen)
    else:
        raise AssertionError(f"no check for epilogue {epi}")


def _run_case(family, tile, M, N, K, b_kc):
    from pixelrec_amd import ops

    if tile == SK_TILE:
        K = 128             # stream-K needs at least 4 K tiles of 32
    case = _Case(family, tile, M, N, K, b_kc)
    d = case.d
    planes = case.planes
    if b_kc:
        epis = FWD_EPIS_PLANES if planes else FWD_EPIS_F32
        base = R.EPI_BIAS
    else:
        epis = BWD_EPIS_PLANES if planes else BWD_EPIS_F32
        base = R.EPI_NONE
    # pxr_gemm_f32 takes no `act`: a direct EPI_BIAS_ACT_GRAD launch runs the kernel's last branch, sigmoid
    acts = R.ACTS if planes else (R.ACT_SIGMOID,)
    todo = [(e, 0) for e in epis if e != R.EPI_BIAS_ACT_GRAD] + [(R.EPI_BIAS_ACT_GRAD, a) for a in acts if R.EPI_BIAS_ACT_GRAD in epis]
    seen, dense = {}, {}
    tol = _tol_h2 if family == "h2" else _tol
    # tile 0 = the heuristic of the family under test: pxr_gemm_f32 picks the f32 or the bf16x3 kernels by the process mode
    prev = ops.set_gemm_mode("f32" if family == "f32" else "bf16x3")
    try:
        for layout in LAYOUTS:
            P, _ = case.run(base, layout)
            if layout == LAYOUTS[0]:
                err = (P.double() - d["pre"]).abs().max().item()
                assert err <= tol(d["pre"], K), f"{case.tag}: product error {err:.3e}"
                assert float(P.abs().max()) < 8.0
                dense[(base, 0)] = (P, None)
            else:
                assert torch.equal(P, dense[(base, 0)][0]), f"{case.tag} layout {layout}: P differs from the dense layout"
            for epi, act in todo:
                C, aux_out = case.run(epi, layout, act if planes else 0)
                if layout != LAYOUTS[0]:
                    C0, a0 = dense[(epi, act)]
                    assert torch.equal(C, C0), f"{case.tag} epi {epi} act {act} layout {layout}: C differs from the dense layout"
                    assert aux_out is None or torch.equal(aux_out, a0), f"{case.tag} epi {epi} act {act} layout {layout}: aux differs"
                    continue
                dense[(epi, act)] = (C, aux_out)
                if epi == R.EPI_NONE:            # forward flavour without a bias: the product itself, and P = it + b exactly
                    err = (C.double() - d["prod"]).abs().max().item()
                    assert err <= tol(d["prod"], K), f"{case.tag}: EPI_NONE product error {err:.3e}"
                    assert torch.equal(P, C + d["b"]), f"{case.tag}: EPI_BIAS != EPI_NONE + b (the accumulators differ between epilogues)"
                else:
                    _check_epilogue(case.tag, d["aux"], epi, act, P, C, aux_out, seen)
    finally:
        ops.set_gemm_mode(prev)
    print("EPI_RATIO", family, tile, (M, N, K), "fwd" if b_kc else "bwd", {k: round(v, 3) for k, v in sorted(seen.items())})


@pytest.mark.parametrize("M,N,K", FWD_SHAPES)
@pytest.mark.parametrize("tile", F32_TILES)
def test_f32_forward_epilogues(tile, M, N, K):
    _run_case("f32", tile, M, N, K, True)


@pytest.mark.parametrize("M,N,K", BWD_SHAPES_F32)
@pytest.mark.parametrize("tile", F32_TILES)
def test_f32_input_gradient_epilogues(tile, M, N, K):
    _run_case("f32", tile, M, N, K, False)


@pytest.mark.parametrize("M,N,K", FWD_SHAPES)
@pytest.mark.parametrize("tile", B3_TILES)
def test_b3_forward_epilogues(tile, M, N, K):
    _run_case("b3", tile, M, N, K, True)


@pytest.mark.parametrize("M,N,K", BWD_SHAPES_F32)
@pytest.mark.parametrize("tile", B3_TILES)
def test_b3_input_gradient_epilogues(tile, M, N, K):
    _run_case("b3", tile, M, N, K, False)


@pytest.mark.parametrize("M,N,K", FWD_SHAPES)
@pytest.mark.parametrize("tile", P3_TILES)
def test_planes_forward_epilogues(tile, M, N, K):
    _run_case("planes", tile, M, N, K, True)


@pytest.mark.parametrize("M,N,K", BWD_SHAPES_PLANES)
@pytest.mark.parametrize("tile", P3_TILES)
def test_planes_input_gradient_epilogues(tile, M, N, K):
    _run_case("planes", tile, M, N, K, False)


@pytest.mark.parametrize("M,N,K", FWD_SHAPES)
@pytest.mark.parametrize("tile", H2_TILES)
def test_h2_forward_epilogues(tile, M, N, K):
    _run_case("h2", tile, M, N, K, True)


@pytest.mark.parametrize("M,N,K", BWD_SHAPES_PLANES)
@pytest.mark.parametrize("tile", H2_TILES)
def test_h2_input_gradient_epilogues(tile, M, N, K):
    _run_case("h2", tile, M, N, K, False)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("M,N,K", [(300, 452, 32), (3200, 1024, 32)])
def test_linear_fwd_activations_both_modes(mode, M, N, K):
    """EPI_BIAS_ACT_GRAD of pxr_gemm_f32 with each of its five activations (ops.linear_fwd(act=...) sets the activation), in
    both GEMM modes, at a shape of the 64x64 tile and one of the 128x128 tile 1281 ((3200, 1024): 25 x 8 = 200 tiles of 128).
    P = linear_fwd without an activation: the same heuristic, the same tile, the same accumulators."""
    from pixelrec_amd import ops

    d = _inputs(M, N, K, True)
    seen = {}
    prev = ops.set_gemm_mode(mode)
    try:
        P = ops.linear_fwd(d["x"], d["W"], d["b"])
        err = (P.double() - d["pre"]).abs().max().item()
        assert err <= _tol(d["pre"], K) and float(P.abs().max()) < 8.0
        tag = f"linear_fwd {mode} ({M},{N},{K})"
        for name, act in ops.ACT_CODES.items():
            y, dv = ops.linear_fwd(d["x"], d["W"], d["b"], act=name)
            _check_epilogue(tag, None, R.EPI_BIAS_ACT_GRAD, act, P, y, dv, seen)
        y, pre = ops.linear_fwd(d["x"], d["W"], d["b"], gelu=True)
        _check_epilogue(tag, None, R.EPI_BIAS_GELU, 0, P, y, pre, seen)
        y, dg = ops.linear_fwd(d["x"], d["W"], d["b"], gelu=True, save_grad=True)
        _check_epilogue(tag, None, R.EPI_BIAS_GELU_GRAD, 0, P, y, dg, seen)
    finally:
        ops.set_gemm_mode(prev)
    print("EPI_RATIO", "linear_fwd", mode, (M, N, K), "fwd", {k: round(v, 3) for k, v in sorted(seen.items())})


# ---- pxr_gemm_batched_f32, direct -------------------------------------------------------------------------------------------
def _r4(n):
    return (n + 3) // 4 * 4


def _batched_case(a_kc, b_kc, M, N, K, G, nb2, tile, seed, overlap=False):
    """One launch of G * nb2 problems with padded leading dimensions, non-zero offsets and two-level strides; C is a sentinel
    buffer: every problem against fp64 bmm, everything between the problems untouched.  overlap: the (read-only) operands of
    different problems overlap, so that the inputs of a huge batch stay small."""
    from pixelrec_amd import ops

    g = torch.Generator().manual_seed(seed)
    batch = G * nb2

    def operand(rows, cols, off):
        ld = _r4(cols) + 4                                   # padded rows, 16-byte aligned; the pad holds finite values
        if overlap:
            s2, s1 = rows * ld + 4, 8                        # problem (z1, z2) at z1 * 8 + z2 * s2: windows of one small buffer
            total = off + (G - 1) * s1 + nb2 * s2
        else:
            s2 = rows * ld + 8
            s1 = nb2 * s2 + 12
            total = off + G * s1
        buf = torch.randn(total + 256, generator=g).cuda()      # (slack behind the last problem)
        view = torch.as_strided(buf.double(), (G, nb2, rows, cols), (s1, s2, ld, 1), off)
        return buf, view, ld, (s1, s2)

    A, Av, lda, a12 = operand(M if a_kc else K, K if a_kc else M, 8)
    B, Bv, ldb, b12 = operand((N if b_kc else K), (K if b_kc else N), 4)
    ldc, c_off = N + 1, 3
    c2 = M * ldc + 3
    c1 = nb2 * c2 + 5
    c_total = c_off + G * c1 + 7
    C = torch.empty(c_total, device="cuda")
    C.view(torch.int32).fill_(SENTINEL)
    ops.gemm_batched(a_kc, b_kc, M, N, K, A, 8, lda, B, 4, ldb, C, c_off, ldc, batch, nb2, a12, b12, (c1, c2), tile_hint=tile)
    ref = (Av if a_kc else Av.transpose(-1, -2)) @ (Bv.transpose(-1, -2) if b_kc else Bv)           # [G, nb2, M, N] fp64
    got = torch.as_strided(C, (G, nb2, M, N), (c1, c2, ldc, 1), c_off)
    what = f"batched a_kc={a_kc} b_kc={b_kc} ({M},{N},{K}) G={G} nb2={nb2} tile={tile}"
    assert not bool(torch.isnan(got).any()), what + ": a problem was not (fully) written"
    # per problem: the bound of its own reference
    err = (got.double() - ref).abs().amax(dim=(-1, -2))
    bound = 2e-6 * (K ** 0.5) * ref.abs().amax(dim=(-1, -2)) + 1e-6
    bad = (err > bound).nonzero()
    assert bad.numel() == 0, what + f": problems {bad[:4].tolist()} wrong (err {float(err.max()):.3e})"
    mask = torch.ones(c_total, dtype=torch.bool, device="cuda")
    torch.as_strided(mask, (G, nb2, M, N), (c1, c2, ldc, 1), c_off).fill_(False)
    assert bool((C.view(torch.int32)[mask] == SENTINEL).all()), what + ": C written between the problems"


BATCH_FLAVOURS = [(True, True), (True, False), (False, False)]           # S = Q K^T, O = P V, dV = P^T dO
BATCH_MODES = [("f32", 0), ("bf16x3", 0), ("bf16x3", 1281), ("f32", 91281)]     # the mode's default tile; an explicit f32 / b3 tile


@pytest.mark.parametrize("mode,tile", BATCH_MODES)
@pytest.mark.parametrize("a_kc,b_kc", BATCH_FLAVOURS)
def test_batched_gemm_direct(a_kc, b_kc, mode, tile):
    from pixelrec_amd import ops

    prev = ops.set_gemm_mode(mode)
    try:
        for M, N, K in ((5, 8, 12), (70, 130, 36)):
            for nb2 in (1, 3, 12):
                _batched_case(a_kc, b_kc, M, N, K, 3, nb2, tile, seed=M + nb2)
    finally:
        ops.set_gemm_mode(prev)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("a_kc,b_kc", BATCH_FLAVOURS)
def test_batched_gemm_across_the_launch_cut(a_kc, b_kc, mode):
    """batch = 65 532 + 24 with nb2 = 12: grid.z holds 65 532 = 5 461 whole groups, problems 65 532 .. 65 555 are a second launch
    whose operands are rebased by 5 461 first-level strides."""
    from pixelrec_amd import ops

    nb2, batch = 12, 65532 + 24
    assert batch % nb2 == 0 and 65535 // nb2 * nb2 == 65532
    prev = ops.set_gemm_mode(mode)
    try:
        _batched_case(a_kc, b_kc, 4, 8, 8, batch // nb2, nb2, 0, seed=7, overlap=True)
    finally:
        ops.set_gemm_mode(prev)
