"""Thin torch-tensor wrappers over the C-ABI (include/pxr.h).  No arithmetic happens in Python here: each
function checks device/dtype/layout, allocates outputs through torch's caching allocator, and launches the HIP
kernel on torch's current stream.  Every function raises if the inputs are not CUDA(HIP) tensors -- there is
no CPU path.
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import lib as _l

_CHECK_IDX = os.environ.get("PXR_CHECK_INDICES", "0") == "1"


def _req(t: torch.Tensor, dtype, name: str, contiguous: bool = True):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _l.PxrError(f"{name}: expected a CUDA/HIP tensor (pixelrec_amd has no CPU fallback)")
    if t.dtype != dtype:
        raise _l.PxrError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise _l.PxrError(f"{name}: expected a contiguous tensor")
    return t


class Workspace:
    """Grow-only scratch buffer (bytes) per (device, stream), reused by kernels that need temporary storage.
    Keyed by the CURRENT stream so that work issued on a side stream never shares scratch with the main stream."""

    def __init__(self):
        self._buf = {}
        self._retired = []

    def get(self, nbytes: int, device) -> torch.Tensor:
        device = torch.device(device)
        stream = _l.raw_stream() if device.type == "cuda" else 0
        key = (device.type, device.index, stream)
        b = self._buf.get(key)
        if b is None or b.numel() < nbytes:
            if b is not None:
                self._retired.append(b)   # a captured hipGraph may still hold this pointer: never free it
            b = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
            self._buf[key] = b
        return b


_ws = Workspace()

# bench.py: set to a list to collect (start_event, end_event, work, tag) around kernel launches: every fp32-MFMA GEMM
# launch (work = flops) and the tagged HBM-side kernels (lazy AdamW rows, fused gather+LN, dense table sweep; work =
# algorithmic bytes, 0 when it is data dependent).  Events are recorded on the stream the kernel is launched on.
GEMM_TIMING = None


class _gemm_timer:
    def __init__(self, flops, tag="gemm"):
        self.flops = flops
        self.tag = tag          # names the kernel instantiation the launch resolves to (see bench.py's roofline)
        self.on = GEMM_TIMING is not None
        if self.on and tag.startswith(("gemm_kernel", "grouped_dw_kernel")) and _l.load().pxr_get_gemm_mode():
            # bf16x3 GEMM mode: the same launch sites resolve to the bf16-pipe kernels (csrc/gemm_b3.hip)
            self.tag = tag.replace("gemm_kernel", "gemm_b3_kernel", 1).replace("grouped_dw_kernel", "grouped_dw_b3_kernel", 1)

    def __enter__(self):
        if self.on:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record()

    def __exit__(self, *exc):
        if self.on:
            self.ev[1].record()
            GEMM_TIMING.append((self.ev[0], self.ev[1], self.flops, self.tag))


# ------------------------------------------------------------------------------------------------ bad-index flag
_status = {}


def device_status(device=None) -> torch.Tensor:
    """The int32 device status word of this process' GPU (created and registered with the library on first use)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index is None:            # "cuda" without an index names the current device, not a second status word
        dev = torch.device("cuda", torch.cuda.current_device())
    t = _status.get(dev.index)
    if t is None:
        t = _status[dev.index] = torch.zeros(1, dtype=torch.int32, device=dev)
        _l.check(_l.load().pxr_set_status_word(_l.ptr(t)), "pxr_set_status_word")
    return t


STATUS_SHARD_OVERFLOW = 16      # PXR_STATUS_SHARD_OVERFLOW (csrc/pxr_common.h)
STATUS_ROWS_STALE = 256         # PXR_STATUS_ROWS_STALE


def clear_status_bits(device, bits: int):
    """Drop `bits` from the device status word (stream-ordered; for a condition the caller has just handled itself)."""
    if torch.device(device).type != "cuda":
        return
    device_status(device).bitwise_and_(~int(bits))


class StatusPoll:
    """The status word watched WITHOUT stalling the stream: start() enqueues a 4-byte copy into pinned host memory behind the work
    issued so far; check() looks at the copy of an EARLIER start() once its event has completed (a query, no wait) and raises through
    raise_on_bad_indices when a bit is set.  A condition is therefore reported at most two polling intervals after the kernel that
    flagged it (graph.GraphedTrainStep polls every PXR_H2_REFRESH_STEPS replays), not at the end of the epoch."""

    def __init__(self, device=None):
        self.device = device
        self._host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._ev = None

    def start(self):
        self._host.copy_(device_status(self.device), non_blocking=True)
        self._ev = torch.cuda.Event()
        self._ev.record()

    def check(self):
        if self._ev is None or not self._ev.query():
            return
        self._ev = None
        if int(self._host[0]):
            raise_on_bad_indices(self.device)


def raise_on_bad_indices(device=None):
    """Host check of the status word (synchronises): IndexError if a gather kernel met an item id outside the table
    since the last check -- what nn.Embedding raises in the reference (sasrec.py:68).  Called where the host
    synchronises anyway: once per training epoch (with the loss), after predict / evaluate, by embed_gather under
    PXR_CHECK_INDICES=1."""
    t = device_status(device)
    v = int(t.item())
    if v:
        t.zero_()
    if v & 8:
        _l.load().pxr_gemm_reset_flags()     # the flag words are in an unknown state: zero them before anything launches again
        raise RuntimeError("stream-K / split-K GEMM: a worker timed out waiting for a partial tile (results are wrong; the flag "
                           "words were reset); set PXR_GEMM_SK=0 PXR_DW_SPLITK=0 and report")
    if v & 1:
        raise IndexError("index out of range in self (an item id outside [0, item_num) reached an embedding gather)")
    if v & 4:
        raise RuntimeError("fused scoring + top-k: the per-user candidate buffer of the threshold pass overflowed (results may miss "
                           "items); with PXR_TOPK_PRODUCTS=1 first go back to 3 or 6 (a tighter threshold margin admits fewer "
                           "candidates), else set PXR_TOPK_VARIANT=2 (register lists, no candidate buffer)")
    if v & 32:
        raise RuntimeError("fused scoring + top-k: a user ended with fewer than K candidates above its threshold (non-finite scores "
                           "or embeddings?); the affected rows of the result hold id -1")
    if v & 64:
        raise RuntimeError("fp16 two-plane operands (image tower, or the sequence block of batches >= PXR_SEQ_H2_MIN_TOKENS "
                           "tokens): an activation, a gradient or a scaled weight was NaN or left the fp16 range (|x| > 65504) "
                           "-- the affected outputs are inf / nan; set PXR_TOWER_H2=0 and / or PXR_SEQ_H2=0 (the six-product "
                           "bf16x3 GEMMs have fp32's range)")
    if v & 128:
        raise H2StaleOverflow("fp16 two-plane gradients under the recent steps' scale (PXR_SEQ_H2_STALE): a gradient exceeded the "
                              f"decaying maximum of the last steps more than 2^{H2_STALE_HEADROOM + 2}-fold; its largest elements were "
                              "saturated in that step (no inf / nan was written).  The Trainer goes on with per-step exact scales "
                              "(PXR_SEQ_H2_STALE=0: six more launches per step)")
    if v & 16:
        raise RuntimeError("row-sharded table: one rank owned more of a batch's hit rows than the per-pair request capacity "
                           "(ShardedSASRec.pair_slack); rows were dropped -- raise the slack or use row_exchange='reduce_scatter'")
    if v & 2:
        raise RuntimeError("data-parallel row exchange: a rank's batch touched more unique table rows than the configured "
                           "exchange capacity (GradSync(exchange_rows=...)); gradient rows were dropped -- raise the bound")
    if v & STATUS_ROWS_STALE:
        raise RuntimeError("fused segment sum + row update: a table row of the batch was not current through the previous step "
                           "when its gradient was applied (its update was skipped, nothing was written from stale state); the "
                           "rows of a batch must be caught up before its backward pass -- set PXR_ROWS_FUSED=0 for the two-launch "
                           "path, which replays such rows")


# ------------------------------------------------------------------------------------------------ K1 gather
def embed_gather(table: torch.Tensor, idx: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """out[..., :] = table[idx[...], :]  (reference: nn.Embedding forward, sasrec.py:68,101).  out: a contiguous buffer of
    idx.numel() * D floats to write into (default: a new tensor)."""
    L = _l.load()
    _req(table, torch.float32, "table")
    _req(idx, torch.int64, "idx")
    N, D = table.shape
    device_status(table.device)       # out-of-range ids are flagged on the device (and clamped), raised at the next check
    if out is None:
        out = torch.empty(*idx.shape, D, dtype=torch.float32, device=table.device)
    elif out.numel() != idx.numel() * D or not out.is_contiguous() or out.dtype != torch.float32:
        raise _l.PxrError("embed_gather: out must be a contiguous fp32 buffer of idx.numel() * D elements")
    _l.check(L.pxr_embed_gather_f32(_l.ptr(table), N, D, _l.ptr(idx), idx.numel(), _l.ptr(out), _l.stream_ptr()),
             "pxr_embed_gather_f32")
    if _CHECK_IDX:
        raise_on_bad_indices(table.device)
    return out


# ------------------------------------------------------------------------------------------------ GEMMs
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_MUL_DGELU, EPI_ADD = 0, 1, 2, 3, 4
EPI_BIAS_GELU_GRAD, EPI_MUL, EPI_BIAS_ADD, EPI_BIAS_QGELU_GRAD, EPI_BIAS_RELU, EPI_BIAS_ACT_GRAD = 5, 6, 7, 8, 9, 10
EPI_BIAS_QGELU = 11         # planes GEMMs only: quick_gelu(x W^T + b), no derivative


def gemm(a_kc: bool, b_kc: bool, M: int, N: int, K: int, A, lda, B, ldb, C, ldc, epilogue=EPI_NONE, bias=None,
         aux=None, ldaux=0, use_ws=True, tile_hint=0, split_hint=0):
    """Raw pxr_gemm_f32 (see gemm_f32.cuh for the operand flavours).  Used by tests and the bench."""
    L = _l.load()
    ws = None
    ws_bytes = 0
    if use_ws:
        ws_bytes = int(L.pxr_gemm_ws_bytes(int(a_kc), int(b_kc), M, N, K))
        ws_bytes = min(ws_bytes, 1 << 30)
        ws = _ws.get(ws_bytes, C.device)
    with _gemm_timer(2.0 * M * N * K):
        _l.check(L.pxr_gemm_f32(int(a_kc), int(b_kc), M, N, K, _l.ptr(A), lda, _l.ptr(B), ldb, _l.ptr(C), ldc,
                                epilogue, _l.ptr(bias), _l.ptr(aux), ldaux, _l.ptr(ws), ws_bytes, tile_hint,
                                split_hint, _l.stream_ptr()), "pxr_gemm_f32")
    return C


class Planes:
    """An fp32 matrix [rows, cols] pre-split into planes in PANEL layout (include/pxr.h, csrc/planes.cuh): the operand format of
    gemm_planes.  fmt 0: three bf16 planes (x = hi + mid + lo exactly); fmt 1 ("h2"): two fp16 planes of x * 2^exp (22 significant
    bits; the forward-only blocks of the image tower).  `buf` is a flat 2-byte-element tensor; `off` / `pr` / `ps` are the element
    offset of plane 0, the rows per panel and the plane stride, so row / column ranges are views of the same buffer."""
    __slots__ = ("buf", "rows", "cols", "pr", "ps", "off", "fmt", "exp", "exp_dev", "stats", "pre_bound")

    def __init__(self, buf, rows, cols, pr, ps, off=0, fmt=0, exp=0, exp_dev=None, stats=None):
        self.buf, self.rows, self.cols, self.pr, self.ps, self.off, self.fmt, self.exp = buf, rows, cols, pr, ps, off, fmt, exp
        # fmt 1 with a scale chosen on the device (split_h2_auto / a bound): int32 [1] holding the exponent (then `exp` is unused)
        # and float32 [2] = (max |x|, for weights the largest column sum of |x|)
        self.exp_dev, self.stats = exp_dev, stats
        self.pre_bound = None      # (W.stats address, factor, int32 [1]): an h2_bound_exp its split launch already computed

    @staticmethod
    def alloc(rows: int, cols: int, device, fmt: int = 0) -> "Planes":
        if cols % 32:
            raise _l.PxrError(f"planes need a multiple of 32 columns, got {cols}")
        pr = (rows + 31) // 32 * 32
        ps = pr * cols
        # rows past `rows` of a panel are read by edge tiles and, when the rows are a GEMM's reduction dimension (weight
        # gradients), multiplied in: they must be zero.  Producers never write them, so one fill at allocation is enough.
        mk = torch.empty if pr == rows else torch.zeros
        if fmt:
            return Planes(mk(2 * ps, dtype=torch.float16, device=device), rows, cols, pr, ps, fmt=1)
        return Planes(mk(3 * ps, dtype=torch.bfloat16, device=device), rows, cols, pr, ps)

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 2 * self.off)

    def row_range(self, r0: int, r1: int) -> "Planes":
        assert r0 % 16 == 0 and r0 <= r1 <= self.rows
        return Planes(self.buf, r1 - r0, self.cols, self.pr, self.ps, self.off + 32 * r0, self.fmt, self.exp, self.exp_dev, self.stats)

    def col_range(self, c0: int, c1: int) -> "Planes":
        assert c0 % 32 == 0 and c1 % 32 == 0 and c0 <= c1 <= self.cols
        return Planes(self.buf, self.rows, c1 - c0, self.pr, self.ps, self.off + (c0 // 32) * self.pr * 32, self.fmt, self.exp,
                      self.exp_dev, self.stats)

    def to_dense(self) -> torch.Tensor:
        """fp32 [rows, cols] = the sum of the planes (exact for fmt 0; x rounded to 22 bits for fmt 1).  For tests; not on the
        product path."""
        dev = self.buf.device
        r = torch.arange(self.rows, device=dev).view(-1, 1)
        c = torch.arange(self.cols, device=dev).view(1, -1)
        idx = ((c // 32) * self.pr + r) * 32 + ((((c // 8) % 4) ^ ((r // 4) % 4)) * 8) + c % 8 + self.off
        out = None
        for q in range(2 if self.fmt else 3):
            t = self.buf[(idx + q * self.ps).reshape(-1)].view(self.rows, self.cols).float()
            out = t if out is None else out + t
        if self.fmt:
            out = out * (2.0 ** -(int(self.exp_dev.item()) if self.exp_dev is not None else self.exp))
        return out


def split_planes(x: torch.Tensor, out: Planes | None = None) -> Planes:
    """fp32 [rows, cols] -> Planes with x = hi + mid + lo exactly (pxr_split_planes_f32)."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32
    rows, cols = x.shape
    if out is None:
        out = Planes.alloc(rows, cols, x.device)
    assert (out.rows, out.cols) == (rows, cols)
    _l.check(_l.load().pxr_split_planes_f32(_l.ptr(x), rows, cols, x.stride(0), out.ptr(), out.ps, out.pr,
                                            _l.stream_ptr()), "pxr_split_planes_f32")
    return out


def gemm_planes(Ap: Planes, Bp: Planes, C: torch.Tensor | None, epilogue=EPI_NONE, bias=None, aux=None, act=0, tile_hint=0,
                b_kc=True, Cp: Planes | None = None):
    """C[M,N] = A[M,K] x B from planes (pxr_gemm_planes_f32): Bp is [N,K] (b_kc) or [K,N]; C (fp32) and / or Cp (planes of
    the result) are written."""
    M, K = Ap.rows, Ap.cols
    N = Bp.rows if b_kc else Bp.cols
    assert (Bp.cols if b_kc else Bp.rows) == K
    assert C is None or C.shape == (M, N)
    if Ap.fmt or Bp.fmt:
        # two fp16 planes per operand, three products per multiply (pxr_gemm_h2_f32)
        if not (Ap.fmt and Bp.fmt):
            raise _l.PxrError("gemm_planes: fp16 two-plane operands need BOTH operands in that format")
        device_status(Ap.buf.device)      # the producers' fp16 range check reports through the status word
        with _gemm_timer(2.0 * M * N * K, "gemm_p3_kernel<P4Cfg<..., HALF>> (fp16 two-plane operands, 3 products)"):
            _l.check(_l.load().pxr_gemm_h2_f32(int(b_kc), M, N, K, Ap.ptr(), Ap.ps, Ap.pr, Ap.exp, _l.ptr(Ap.exp_dev), Bp.ptr(), Bp.ps,
                                               Bp.pr, Bp.exp, _l.ptr(Bp.exp_dev), _l.ptr(C), C.stride(0) if C is not None else 0,
                                               epilogue, _l.ptr(bias), _l.ptr(aux), aux.stride(0) if aux is not None else 0, *_pl(Cp),
                                               Cp.fmt if Cp is not None else 0,
                                               _l.ptr(Cp.exp_dev) if (Cp is not None and Cp.fmt) else None, act, tile_hint,
                                               _l.stream_ptr()), "pxr_gemm_h2_f32")
        return C
    assert Cp is None or Cp.fmt == 0, "the bf16x3 GEMMs write bf16x3 planes"
    with _gemm_timer(2.0 * M * N * K):
        _l.check(_l.load().pxr_gemm_planes_f32(int(b_kc), M, N, K, Ap.ptr(), Ap.ps, Ap.pr, Bp.ptr(), Bp.ps, Bp.pr, _l.ptr(C),
                                               C.stride(0) if C is not None else 0, epilogue, _l.ptr(bias), _l.ptr(aux),
                                               aux.stride(0) if aux is not None else 0,
                                               Cp.ptr() if Cp is not None else None, Cp.ps if Cp is not None else 0,
                                               Cp.pr if Cp is not None else 0, act, tile_hint, _l.stream_ptr()),
                 "pxr_gemm_planes_f32")
    return C


def set_gemm_mode(mode: str):
    """"bf16x3" (default; PXR_GEMM_MODE) = the heuristic's GEMM choices run on the bf16 matrix pipe through the exact
    3 x bf16 operand split (csrc/gemm_b3.cuh), "f32" = on the f32-input MFMA.  Process-wide; returns the previous mode."""
    L = _l.load()
    prev = "bf16x3" if L.pxr_get_gemm_mode() else "f32"
    if mode not in ("bf16x3", "f32"):
        raise ValueError(f"gemm mode must be 'bf16x3' or 'f32', got {mode!r}")
    _l.check(L.pxr_set_gemm_mode(1 if mode == "bf16x3" else 0), "pxr_set_gemm_mode")
    return prev


def gemm_mode() -> str:
    return "bf16x3" if _l.load().pxr_get_gemm_mode() else "f32"


# the reference's ACT2FN besides gelu (layers.py:642-649), and F.selu (ViNet/curatornet.py:67-82)
ACT_CODES = {"relu": 3, "swish": 4, "tanh": 5, "sigmoid": 6, "selu": 7}


def linear_fwd(x: torch.Tensor, W: torch.Tensor, b: torch.Tensor | None, gelu: bool = False, save_grad: bool = False,
               act: str | None = None):
    """y = x W^T + b (nn.Linear, layers.py:586-588,613,666,669).  gelu=True also returns the pre-activation, or with
    save_grad=True gelu'(pre-activation) (what linear_bwd_input(mul=...) multiplies by).  act in ACT_CODES: that
    activation instead of erf-GELU, always with its derivative returned second."""
    if act is not None and act != "gelu":
        gelu, code = True, ACT_CODES[act]
    else:
        code = None
    L = _l.load()
    _req(x, torch.float32, "x"); _req(W, torch.float32, "W")
    N, K = W.shape
    M = x.numel() // K
    y = torch.empty(*x.shape[:-1], N, dtype=torch.float32, device=x.device)
    pre = torch.empty_like(y) if gelu else None
    with _gemm_timer(2.0 * M * N * K, "gemm_kernel<KC,KC,EPI_BIAS_GELU*> (fwd + erf-GELU)" if gelu else
                     "gemm_kernel<KC,KC,EPI_BIAS> (fwd)"):
        _l.check(L.pxr_linear_fwd_f32(_l.ptr(x), _l.ptr(W), _l.ptr(b), _l.ptr(y), _l.ptr(pre), M, N, K,
                                      code if code is not None else ((2 if save_grad else 1) if gelu else 0),
                                      _l.stream_ptr()), "pxr_linear_fwd_f32")
    return (y, pre) if gelu else y


def linear_epi(x: torch.Tensor, W: torch.Tensor, b: torch.Tensor, epi: int, aux: torch.Tensor | None = None,
               tag: str = "gemm_kernel<KC,KC,*> (ViT linear)", out: torch.Tensor | None = None):
    """y = epilogue(x W^T + b) for the ViT-block epilogues (gemm_f32.hip): EPI_BIAS_ADD (aux = residual stream, read),
    EPI_BIAS_QGELU_GRAD (aux = quick_gelu' saved for the backward, written; returned second), EPI_BIAS_RELU.
    out: a contiguous fp32 buffer of y's shape to write into (default: a new tensor)."""
    L = _l.load()
    _req(x, torch.float32, "x"); _req(W, torch.float32, "W")
    N, K = W.shape
    M = x.numel() // K
    if out is not None:
        _req(out, torch.float32, "out")
        assert out.shape == (*x.shape[:-1], N)
    y = out if out is not None else torch.empty(*x.shape[:-1], N, dtype=torch.float32, device=x.device)
    out_aux = None
    if epi == EPI_BIAS_QGELU_GRAD:
        aux = out_aux = torch.empty_like(y)
    elif epi == EPI_BIAS_ADD:
        _req(aux, torch.float32, "aux")
    with _gemm_timer(2.0 * M * N * K, tag):
        _l.check(L.pxr_gemm_f32(1, 1, M, N, K, _l.ptr(x), K, _l.ptr(W), K, _l.ptr(y), N, epi, _l.ptr(b), _l.ptr(aux), N,
                                None, 0, 0, 0, _l.stream_ptr()), "pxr_gemm_f32")
    return (y, out_aux) if out_aux is not None else y


def gemm_batched(a_kc: bool, b_kc: bool, M: int, N: int, K: int, A, a_off, lda, B, b_off, ldb, C, c_off, ldc, batch, nb2,
                 a12, b12, c12, tile_hint=0):
    """`batch` GEMMs in one launch (pxr_gemm_batched_f32).  A/B/C are tensors, *_off element offsets of problem 0,
    x12 = (stride1, stride2) in elements for the two batch levels (z // nb2, z % nb2).  tile_hint: 0 = the mode's default
    tile (bf16x3 64x64 / f32 64x64), otherwise a tile code of pxr_gemm_f32."""
    L = _l.load()
    cp = _l.c_void_p
    with _gemm_timer(2.0 * M * N * K * batch, "gemm_kernel (batched: attention contraction of the ViT encoder)"):
        _l.check(L.pxr_gemm_batched_f32(int(a_kc), int(b_kc), M, N, K, cp(A.data_ptr() + 4 * a_off), lda,
                                        cp(B.data_ptr() + 4 * b_off), ldb, cp(C.data_ptr() + 4 * c_off), ldc, batch, nb2,
                                        a12[0], a12[1], b12[0], b12[1], c12[0], c12[1], tile_hint, _l.stream_ptr()),
                 "pxr_gemm_batched_f32")


def tower_attn_supported(T: int, d: int) -> bool:
    return os.environ.get("PXR_TOWER_ATTN", "1") != "0" and bool(_l.load().pxr_tower_attn_supported(int(T), int(d)))


def tower_attn_fwd(qkv: torch.Tensor, n: int, T: int, heads: int, d: int, q_off: int, k_off: int, v_off: int, scale: float,
                   ctx: bool = True, planes: bool = False, lse: bool = False):
    """Fused attention of a tower block (pxr_tower_attn_fwd_f32) on the fused projection output qkv [n*T, ld]: q / k / v start at
    columns q_off / k_off / v_off.  Returns (ctx fp32 [n, T, heads*d] | None, ctx Planes | None, lse [n*heads, T] | None)."""
    _req(qkv, torch.float32, "qkv")
    ld = qkv.shape[-1]
    H = heads * d
    out = torch.empty(n, T, H, dtype=torch.float32, device=qkv.device) if ctx else None
    h2 = planes == "h2"               # context planes in the two-plane fp16 format (the operand of the h2 out-projection GEMM)
    op = Planes.alloc(n * T, H, qkv.device, fmt=int(h2)) if planes else None
    ls = torch.empty(n * heads, T, dtype=torch.float32, device=qkv.device) if lse else None
    cp = _l.c_void_p
    base = qkv.data_ptr()
    if h2:
        device_status(qkv.device)
    with _gemm_timer(4.0 * T * T * d * n * heads, "tower_attn_fwd_kernel (fused QK^T / softmax / PV of a tower block)"):
        _l.check(_l.load().pxr_tower_attn_fwd_f32(cp(base + 4 * q_off), cp(base + 4 * k_off), cp(base + 4 * v_off), ld, n, heads, T,
                                                  d, float(scale), _l.ptr(out) if ctx else None, H, *_pl(op), int(h2),
                                                  _l.ptr(ls) if lse else None, _l.stream_ptr()), "pxr_tower_attn_fwd_f32")
    return out, op, ls


def tower_attn_bwd(qkv: torch.Tensor, dctx: torch.Tensor, ctx: torch.Tensor, lse: torch.Tensor, n: int, T: int, heads: int, d: int,
                   q_off: int, k_off: int, v_off: int, scale: float) -> torch.Tensor:
    """Backward of tower_attn_fwd (pxr_tower_attn_bwd_f32): -> dqkv with the layout of qkv (every column of the q / k / v
    ranges is written).  ctx / lse: the forward's fp32 context and log-sum-exp."""
    _req(qkv, torch.float32, "qkv"); _req(dctx, torch.float32, "dctx"); _req(ctx, torch.float32, "ctx"); _req(lse, torch.float32, "lse")
    ld, H = qkv.shape[-1], heads * d
    dqkv = torch.empty_like(qkv)
    ws = torch.empty(n * heads * T, dtype=torch.float32, device=qkv.device)
    cp = _l.c_void_p
    b, g = qkv.data_ptr(), dqkv.data_ptr()
    with _gemm_timer(10.0 * T * T * d * n * heads, "tower_attn_bwd_{dq,dkv}_kernel (fused attention backward of a tower block)"):
        _l.check(_l.load().pxr_tower_attn_bwd_f32(cp(b + 4 * q_off), cp(b + 4 * k_off), cp(b + 4 * v_off), ld, _l.ptr(dctx),
                                                  _l.ptr(ctx), H, _l.ptr(lse), n, heads, T, d, float(scale), cp(g + 4 * q_off),
                                                  cp(g + 4 * k_off), cp(g + 4 * v_off), ld, _l.ptr(ws), _l.stream_ptr()),
                 "pxr_tower_attn_bwd_f32")
    return dqkv


def causal_im2col(x: torch.Tensor, k: int, dilation: int) -> torch.Tensor:
    """x [B, L, C] -> xcol [B, L, C*k] with xcol[b, t, c*k + j] = x[b, t - (k-1-j)*dilation, c] (pxr_causal_im2col_f32)."""
    _req(x, torch.float32, "x")
    B, L, C = x.shape
    out = torch.empty(B, L, C * k, dtype=torch.float32, device=x.device)
    _l.check(_l.load().pxr_causal_im2col_f32(_l.ptr(x), _l.ptr(out), B, L, C, k, dilation, _l.stream_ptr()), "pxr_causal_im2col_f32")
    return out


def causal_col2im(dxcol: torch.Tensor, k: int, dilation: int) -> torch.Tensor:
    """The transpose of causal_im2col: dxcol [B, L, C*k] -> dx [B, L, C] (pxr_causal_col2im_f32)."""
    _req(dxcol, torch.float32, "dxcol")
    B, L, Ck = dxcol.shape
    out = torch.empty(B, L, Ck // k, dtype=torch.float32, device=dxcol.device)
    _l.check(_l.load().pxr_causal_col2im_f32(_l.ptr(dxcol), _l.ptr(out), B, L, Ck // k, k, dilation, _l.stream_ptr()),
             "pxr_causal_col2im_f32")
    return out


def _gru_operands(who: str, B: int, H: int, operands):
    """The operands of one GRU step beside its [B, H] anchor, as (name, tensor, width, optional): each contiguous fp32 [B, width]
    on the device, None only where the entry point takes a null pointer."""
    for name, t, width, optional in operands:
        if t is None and optional:
            continue
        _req(t, torch.float32, name)
        if tuple(t.shape) != (B, width):
            raise _l.PxrError(f"{who}: {name} must be [{B}, {width}], got {list(t.shape)}")


def gru_gates_fwd(gi, gh, h_prev, h_out, save=None):
    """One GRU step's gates (pxr_gru_gates_fwd_f32): gi, gh [B, 3H]; h_prev [B, H] | None; writes h_out [B, H] (and save [B, 4H])."""
    _req(h_out, torch.float32, "h_out")
    if h_out.dim() != 2:
        raise _l.PxrError("gru_gates_fwd: h_out must be [B, H]")
    B, H = h_out.shape
    _gru_operands("gru_gates_fwd", B, H, (("gi", gi, 3 * H, False), ("gh", gh, 3 * H, False), ("h_prev", h_prev, H, True),
                                          ("save", save, 4 * H, True)))
    _l.check(_l.load().pxr_gru_gates_fwd_f32(_l.ptr(gi), _l.ptr(gh), _l.ptr(h_prev), _l.ptr(h_out), _l.ptr(save), B, H,
                                             _l.stream_ptr()), "pxr_gru_gates_fwd_f32")


def gru_gates_bwd(dh, save, h_prev, dgi, dgh, dh_prev):
    """Backward of gru_gates_fwd (pxr_gru_gates_bwd_f32): dh [B, H] -> dgi, dgh [B, 3H], dh_prev [B, H] = dh * z."""
    _req(dh, torch.float32, "dh")
    if dh.dim() != 2:
        raise _l.PxrError("gru_gates_bwd: dh must be [B, H]")
    B, H = dh.shape
    _gru_operands("gru_gates_bwd", B, H, (("save", save, 4 * H, False), ("h_prev", h_prev, H, True), ("dgi", dgi, 3 * H, False),
                                          ("dgh", dgh, 3 * H, False), ("dh_prev", dh_prev, H, False)))
    _l.check(_l.load().pxr_gru_gates_bwd_f32(_l.ptr(dh), _l.ptr(save), _l.ptr(h_prev), _l.ptr(dgi), _l.ptr(dgh), _l.ptr(dh_prev),
                                             B, H, _l.stream_ptr()), "pxr_gru_gates_bwd_f32")


def softmax_rows(S: torch.Tensor, rows: int, T: int, ld: int, scale: float):
    _l.check(_l.load().pxr_softmax_rows_f32(_l.ptr(S), rows, T, ld, float(scale), _l.stream_ptr()), "pxr_softmax_rows_f32")


def softmax_rows_bwd(P: torch.Tensor, dP: torch.Tensor, rows: int, T: int, ld: int, scale: float):
    _l.check(_l.load().pxr_softmax_rows_bwd_f32(_l.ptr(P), _l.ptr(dP), rows, T, ld, float(scale), _l.stream_ptr()),
             "pxr_softmax_rows_bwd_f32")


def vit_embed(patches: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """patches [n, T-1, H] -> tokens [n, T, H] = [cls | patches] + pos."""
    _req(patches, torch.float32, "patches"); _req(cls, torch.float32, "cls"); _req(pos, torch.float32, "pos")
    n, Tm1, H = patches.shape
    out = torch.empty(n, Tm1 + 1, H, dtype=torch.float32, device=patches.device)
    _l.check(_l.load().pxr_vit_embed_f32(_l.ptr(patches), _l.ptr(cls), _l.ptr(pos), _l.ptr(out), n, Tm1 + 1, H,
                                         _l.stream_ptr()), "pxr_vit_embed_f32")
    return out


def token_mean(x: torch.Tensor) -> torch.Tensor:
    _req(x, torch.float32, "x")
    n, T, D = x.shape
    out = torch.empty(n, D, dtype=torch.float32, device=x.device)
    _l.check(_l.load().pxr_token_mean_f32(_l.ptr(x), _l.ptr(out), n, T, D, _l.stream_ptr()), "pxr_token_mean_f32")
    return out


def token_mean_relu_bwd(dout: torch.Tensor, act: torch.Tensor) -> torch.Tensor:
    _req(dout, torch.float32, "dout"); _req(act, torch.float32, "act")
    n, T, D = act.shape
    dact = torch.empty_like(act)
    _l.check(_l.load().pxr_token_mean_relu_bwd_f32(_l.ptr(dout), _l.ptr(act), _l.ptr(dact), n, T, D, _l.stream_ptr()),
             "pxr_token_mean_relu_bwd_f32")
    return dact


def add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    _req(a, torch.float32, "a"); _req(b, torch.float32, "b")
    out = torch.empty_like(a)
    _l.check(_l.load().pxr_add_f32(_l.ptr(a), _l.ptr(b), _l.ptr(out), a.numel(), _l.stream_ptr()), "pxr_add_f32")
    return out


def dropout(x: torch.Tensor, p: float, seed: int, stream_id: int, step_dev=None) -> torch.Tensor:
    """x / (1 - p) where the library's counter hash keeps the element, else 0 (pxr_dropout_f32); on the upstream gradient with the
    same (seed, stream_id, step_dev) it is the backward of itself."""
    _req(x, torch.float32, "x")
    y = torch.empty_like(x)
    _l.check(_l.load().pxr_dropout_f32(_l.ptr(x), _l.ptr(y), x.numel(), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id),
                                       _l.ptr(step_dev), _l.stream_ptr()), "pxr_dropout_f32")
    return y


def linear_bwd_input(dy: torch.Tensor, W: torch.Tensor, dgelu_pre: torch.Tensor | None = None,
                     add: torch.Tensor | None = None, mul: torch.Tensor | None = None, out: torch.Tensor | None = None):
    """dx = dy W, optionally times gelu'(pre) (from the saved pre-activation), times `mul` (gelu' saved by the forward),
    or plus `add` (residual gradient).  out: a contiguous buffer to write dx into (default: a new tensor)."""
    L = _l.load()
    _req(dy, torch.float32, "dy"); _req(W, torch.float32, "W")
    N, K = W.shape
    M = dy.numel() // N
    if out is None:
        dx = torch.empty(*dy.shape[:-1], K, dtype=torch.float32, device=dy.device)
    else:
        _req(out, torch.float32, "out")
        if out.numel() != M * K:
            raise _l.PxrError(f"linear_bwd_input: out has {out.numel()} elements, expected {M * K}")
        dx = out
    tag = ("gemm_kernel<KC,XC,EPI_MUL_DGELU> (dX through GELU)" if dgelu_pre is not None else
           "gemm_kernel<KC,XC,EPI_MUL> (dX x saved gelu')" if mul is not None else
           "gemm_kernel<KC,XC,EPI_ADD> (dX + residual grad)" if add is not None else "gemm_kernel<KC,XC,EPI_NONE> (dX)")
    with _gemm_timer(2.0 * M * N * K, tag):
        _l.check(L.pxr_linear_bwd_input_f32(_l.ptr(dy), _l.ptr(W), _l.ptr(dx), _l.ptr(dgelu_pre), _l.ptr(add),
                                            _l.ptr(mul), M, N, K, _l.stream_ptr()), "pxr_linear_bwd_input_f32")
    return dx


def linear_bwd_weight(dy: torch.Tensor, x: torch.Tensor, out: torch.Tensor | None = None):
    """dW = dy^T x   ([N,K], reduction over all tokens)."""
    L = _l.load()
    _req(dy, torch.float32, "dy"); _req(x, torch.float32, "x")
    N, K = dy.shape[-1], x.shape[-1]
    M = dy.numel() // N
    dW = out if out is not None else torch.empty(N, K, dtype=torch.float32, device=dy.device)
    ws_bytes = min(int(L.pxr_gemm_ws_bytes(0, 0, N, K, M)), 1 << 30)
    ws = _ws.get(ws_bytes, dy.device)
    with _gemm_timer(2.0 * M * N * K, "gemm_kernel<XC,XC> (dW, split-K)"):
        _l.check(L.pxr_linear_bwd_weight_f32(_l.ptr(dy), _l.ptr(x), _l.ptr(dW), M, N, K, _l.ptr(ws), ws_bytes,
                                             _l.stream_ptr()), "pxr_linear_bwd_weight_f32")
    return dW


def grouped_linear_bwd_weight(problems):
    """problems: list of (dy2d [M,N], x2d [M,K], dW [N,K] out, db [N] out | None).  One launch for all of them (one per MULTI_MAX
    of them: blocks deeper than 4 layers)."""
    import ctypes

    if len(problems) > MULTI_MAX:
        for lo in range(0, len(problems), MULTI_MAX):
            grouped_linear_bwd_weight(problems[lo:lo + MULTI_MAX])
        return
    if len(problems) == 1:
        # ONE small weight under a long token reduction (the image tower's head: a 512 x 768 weight over 69 344 tokens is 24 tiles
        # of 128 x 128, each 69 344 tokens deep -- 1.5 ms on a tenth of the chip): the token range is cut into parts that run as
        # the problems of ONE grouped launch into a workspace, and a column-sum launch adds the parts in part order
        dy, x, dW, db = problems[0]
        M, N, K = dy.shape[0], dy.shape[1], x.shape[1]
        S = _dw_token_parts(M, N, K)
        # (N % 4: part i starts i * (N K + N) floats into the workspace -- 16-byte aligned for the kernels' vector accesses only then)
        if S > 1 and N % 4 == 0 and K % 4 == 0 and dy.is_contiguous() and x.is_contiguous() and dW.is_contiguous():
            step = (-(-M // S) + 63) // 64 * 64
            S = -(-M // step)
            # one workspace per (stream, shape): the side stream of fork_pending / overlap_weight_grads may run this route beside
            # the main stream's
            row = N * K + N
            key = (dy.device, _l.raw_stream(), S, N, K)
            ws = _dw_split_ws.get(key)
            if ws is None:
                if len(_dw_split_ws) >= 8:       # a handful of (stream, shape) pairs exist in practice: never grow without bound
                    _dw_split_ws.clear()
                ws = _dw_split_ws[key] = torch.empty(S, row, dtype=torch.float32, device=dy.device)
            grouped_linear_bwd_weight([(dy[i * step:(i + 1) * step], x[i * step:(i + 1) * step], ws[i, :N * K].view(N, K), ws[i, N * K:])
                                       for i in range(S)])
            red = DeferredReductions()
            red.add(ws, S, N * K + N, dW, db if db is not None else ws.new_empty(N), N * K)
            red.flush()
            return
    L = _l.load()
    n = len(problems)
    P, I = ctypes.c_void_p * n, ctypes.c_int * n
    dy = P(*[p[0].data_ptr() for p in problems])
    x = P(*[p[1].data_ptr() for p in problems])
    dW = P(*[p[2].data_ptr() for p in problems])
    db = P(*[(p[3].data_ptr() if p[3] is not None else None) for p in problems])
    M = I(*[p[0].shape[0] for p in problems])
    N = I(*[p[0].shape[1] for p in problems])
    K = I(*[p[1].shape[1] for p in problems])
    flops = sum(2.0 * p[0].shape[0] * p[0].shape[1] * p[1].shape[1] for p in problems)
    with _gemm_timer(flops, "grouped_dw_kernel (all dW + db of the step)"):
        _l.check(L.pxr_grouped_linear_bwd_weight_f32(n, dy, x, dW, db, M, N, K, _l.stream_ptr()),
                 "pxr_grouped_linear_bwd_weight_f32")


_dw_split_ws: dict = {}


def _dw_token_parts(M: int, N: int, K: int) -> int:
    """Parts of the token range for a single weight gradient (grouped_linear_bwd_weight): 1 unless its 128 x 128 tiles cover less
    than a third of the chip under a reduction of >= 16 384 tokens; then enough parts for 192 tiles, each >= 2 048 tokens deep."""
    if os.environ.get("PXR_DW_TOKEN_SPLIT", "1") == "0":
        return 1
    t128 = ((N + 127) // 128) * ((K + 127) // 128)
    if M < 16384 or t128 >= 96:
        return 1
    return max(1, min(MULTI_MAX, -(-192 // t128), M // 2048))


MULTI_MAX = 16      # matrices per pxr_split_planes_multi_f32 launch / plane segments per pxr_adamw_flat_tab_f32 launch


def h2_exponent(max_abs: float) -> int:
    """The power-of-two exponent e that puts max_abs * 2^e into [2^13, 2^14): a factor 4 below the fp16 maximum, 38 binades above
    its smallest subnormal (csrc/planes.cuh "h2")."""
    import math

    if not (max_abs > 0.0) or math.isinf(max_abs):
        return 0
    return max(-60, min(60, 14 - math.frexp(max_abs)[1]))


def split_h2_auto(mats, col_stats: bool = False, stats: torch.Tensor | None = None, outs=None, with_buffers: bool = False, top: int = 0):
    """fp32 matrices -> h2 Planes whose power-of-two scales are chosen ON THE DEVICE (pxr_h2_split_auto_multi_f32): no host
    synchronisation -- gradients, weights that an optimizer step just moved.  Each result carries `exp_dev` (int32 [1]) and
    `stats` (float32 [2]: max |x|; then the largest column sum of |x| with col_stats, else rows * max |x| -- what h2_bound_exp needs
    of a weight).  `stats` ([len(mats), 2] float32): the producers of the matrices already gathered max |x| into stats[:, 0]
    (ln_bwd / attn_bwd with stat=...): no statistics pass at all.  top (8..15; default 14): the largest scaled value lands in
    [2^(top-1), 2^top) -- more headroom below the fp16 limit for tensors rewritten in place with the same exponent."""
    res = []
    if stats is not None:
        assert len(mats) <= MULTI_MAX and tuple(stats.shape) == (len(mats), 2) and stats.dtype == torch.float32 and stats.is_contiguous()
    for lo in range(0, len(mats), MULTI_MAX):
        ms = mats[lo:lo + MULTI_MAX]
        n = len(ms)
        for m in ms:
            assert m.dim() == 2 and m.stride(1) == 1 and m.dtype == torch.float32
        dev = ms[0].device
        device_status(dev)
        # outs = (planes list, stats [n, 2], exps [n]) of an earlier call on the same matrices: overwritten in place (the optimizer
        # keeps writing into these buffers between re-splits: seqcore._weight_planes_h2)
        if outs is not None:
            assert lo == 0 and len(mats) <= MULTI_MAX and stats is None
            os_, st, exps = outs
        else:
            os_ = [Planes.alloc(m.shape[0], m.shape[1], dev, fmt=1) for m in ms]
            st = stats if stats is not None else torch.empty(n, 2, dtype=torch.float32, device=dev)
            exps = torch.empty(n, dtype=torch.int32, device=dev)
        P, I64 = ctypes.c_void_p * n, ctypes.c_int64 * n
        _l.check(_l.load().pxr_h2_split_auto_multi_f32(
            n, P(*[m.data_ptr() for m in ms]), I64(*[m.shape[0] for m in ms]), I64(*[m.shape[1] for m in ms]),
            I64(*[m.stride(0) for m in ms]), P(*[o.ptr().value for o in os_]), I64(*[o.ps for o in os_]), I64(*[o.pr for o in os_]),
            (2 if stats is not None else int(col_stats)) | (int(top) << 8), _l.ptr(st), _l.ptr(exps), _l.stream_ptr()),
            "pxr_h2_split_auto_multi_f32")
        for i, o in enumerate(os_):
            o.exp_dev, o.stats = exps[i:i + 1], st[i]
        res += os_
    if with_buffers:          # (planes, stats [n, 2], exps [n]): what `outs=` takes back to overwrite the same buffers in place
        assert len(mats) <= MULTI_MAX
        return res, st, exps
    return res


ATTN_STAT_SLOTS = 64        # PXR_ATTN_STAT_SLOTS (csrc/attention.hip): words of attn_bwd's `stat` buffer


def ln_bwd_stat_parts(rows: int) -> int:
    """How many partial maxima ln_bwd(stat=...) / bpr_ln_bwd(stat=...) write for `rows` rows (one per workgroup)."""
    return int(_l.load().pxr_ln_bwd_partial_rows(rows))


def split_h2_parts(x: torch.Tensor, parts: torch.Tensor, n_parts: int, bound_with=None) -> Planes:
    """One fp32 matrix -> h2 Planes, its maximum taken from `n_parts` partial maxima its producer left in `parts` (ln_bwd /
    bpr_ln_bwd / attn_bwd with stat=...): no statistics pass, no single-word atomics (pxr_h2_split_parts_f32).
    bound_with = (W Planes, factor): the launch also computes h2_bound_exp(result, W, factor) -- linear_bwd_input_planes(result, W,
    want_planes=True, mul_bound=factor) then finds it on the result and skips its one-thread launch."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32 and parts.dtype == torch.float32 and parts.numel() >= n_parts
    dev = x.device
    device_status(dev)
    o = Planes.alloc(x.shape[0], x.shape[1], dev, fmt=1)
    st = torch.empty(2, dtype=torch.float32, device=dev)
    exps = torch.empty(1, dtype=torch.int32, device=dev)
    bexp = bcol = None
    factor = 1.0
    if bound_with is not None:
        Wp, factor = bound_with
        assert Wp.stats is not None
        bexp = torch.empty(1, dtype=torch.int32, device=dev)
        bcol = ctypes.c_void_p(Wp.stats.data_ptr() + 4)
    _l.check(_l.load().pxr_h2_split_parts_f32(_l.ptr(x), x.shape[0], x.shape[1], x.stride(0), o.ptr(), o.ps, o.pr, _l.ptr(parts),
                                              int(n_parts), _l.ptr(st), _l.ptr(exps), bcol, float(factor), _l.ptr(bexp),
                                              _l.stream_ptr()), "pxr_h2_split_parts_f32")
    o.exp_dev, o.stats = exps, st
    if bound_with is not None:
        o.pre_bound = (bound_with[0].stats.data_ptr(), float(factor), bexp)
    return o


H2_STALE_HEADROOM = 3      # binades between the recent maximum and its placement in the planes (csrc/h2.hip "stale scales")
H2_STALE_DECAY = 0.99      # per-step decay of the running maximum the scales follow (half-life 69 steps)


class H2StaleOverflow(RuntimeError):
    """PXR_STATUS_H2_STALE: a gradient outgrew the headroom of its stale scale and was saturated in one step."""


class H2Sites:
    """Persistent scale state of the gradients a backward pass hands to its GEMMs as h2 planes ("sites": per layer the LayerNorm-2
    backward's output, the LayerNorm-1 backward's output, dqkv).  exps[s] is the exponent site s's producer uses in the NEXT step,
    stats[s] = (max, rows * max) with the headroom applied, bexp[s] the exponent of the planes a GEMM epilogue writes from site s and
    its weight (du).  `update()` -- one launch after the last consumer of a step -- derives all of it from the step's partial maxima
    (pxr_h2_sites_update).  seeded_for: the batch geometry the state was derived from (a different one re-seeds through an exact pass)."""

    def __init__(self, n: int, device):
        assert 1 <= n <= 16
        self.n = n
        self.exps = torch.zeros(n, dtype=torch.int32, device=device)
        self.stats = torch.zeros(n, 2, dtype=torch.float32, device=device)
        self.bexp = torch.zeros(n, dtype=torch.int32, device=device)
        self.run_max = torch.zeros(n, dtype=torch.float32, device=device)
        self.seeded_for = None

    def planes_like(self, s: int, rows: int, cols: int, bound_with=None) -> Planes:
        """Fresh h2 Planes [rows, cols] whose exponent / statistics are site s's (views of the persistent arrays)."""
        o = Planes.alloc(rows, cols, self.exps.device, fmt=1)
        o.exp_dev, o.stats = self.exps[s:s + 1], self.stats[s]
        if bound_with is not None:
            o.pre_bound = (bound_with[0].stats.data_ptr(), float(bound_with[1]), self.bexp[s:s + 1])
        return o

    def update(self, parts, n_parts, rows, bound_b, bound_factor: float):
        """parts[s]: tensor holding site s's partial maxima (first n_parts[s] words); bound_b[s]: None or the weight Planes whose
        column-sum statistic bounds the GEMM output written from site s."""
        n = self.n
        assert len(parts) == len(n_parts) == len(rows) == len(bound_b) == n
        P, I = ctypes.c_void_p * n, ctypes.c_int * n
        bb = [(w.stats.data_ptr() + 4) if w is not None else None for w in bound_b]
        _l.check(_l.load().pxr_h2_sites_update(n, P(*[t.data_ptr() for t in parts]), I(*[int(x) for x in n_parts]), I(*[int(r) for r in rows]),
                                               P(*bb), float(bound_factor), H2_STALE_HEADROOM, H2_STALE_DECAY, _l.ptr(self.run_max),
                                               _l.ptr(self.exps), _l.ptr(self.stats), _l.ptr(self.bexp), _l.stream_ptr()),
                 "pxr_h2_sites_update")


def ln_bwd_h2s(dy, xhat, rstd, gamma, dgamma, dbeta, sites: H2Sites, site: int, stat: torch.Tensor, p_drop=0.0, seed=0, stream_id=0,
               step_dev=None, defer=None, zero: torch.Tensor | None = None, bound_with=None, head=None, layout=None):
    """A residual LayerNorm site's backward whose GEMM-facing gradient leaves ONLY as h2 planes under the site's stale scale
    (pxr_ln_bwd_h2s_f32), + this step's partial maxima in `stat`.  head = (pos, neg, table, items, masked_index, grad_scale,
    grad_scale_dev): the loss head's backward fused in (dy unused).  layout = (id_bstride, pos_off, neg_off) of the head's ids (None:
    SASRec's shifted windows).  -> (dz, Planes, coef | None)."""
    Lb = _l.load()
    D = xhat.shape[-1]
    rows = xhat.numel() // D
    dz = torch.empty_like(xhat)
    ws_bytes = int(Lb.pxr_ln_bwd_ws_bytes(rows, D))
    if defer is not None:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=xhat.device)   # must outlive this call
        defer.add(ws, int(Lb.pxr_ln_bwd_partial_rows(rows)), 2 * D, dgamma, dbeta, D)
        dgamma = dbeta = None
    else:
        ws = _ws.get(ws_bytes, xhat.device)
    assert stat.numel() >= ln_bwd_stat_parts(rows) and (zero is None or zero.numel() <= 256)
    device_status(xhat.device)
    gp = sites.planes_like(site, rows, D, bound_with=bound_with)
    coef = None
    if head is not None:
        pos, neg, table, items, masked_index, grad_scale, grad_scale_dev = head
        B, L = pos.shape
        coef = torch.empty(B, L, dtype=torch.float32, device=pos.device)
        hargs = (_l.ptr(pos), _l.ptr(neg), _l.ptr(table), table.shape[0], _l.ptr(items), _l.ptr(masked_index), B, L, float(grad_scale),
                 _l.ptr(grad_scale_dev), _l.ptr(coef))
    else:
        B = L = 0
        hargs = (None, None, None, 0, None, None, B, L, 1.0, None, None)
    _l.check(Lb.pxr_ln_bwd_h2s_f32(*hargs, _l.ptr(dy), _l.ptr(xhat), _l.ptr(rstd), _l.ptr(gamma), rows, D, _l.ptr(dz), _l.ptr(dgamma),
                                   _l.ptr(dbeta), p_drop, seed, stream_id, _l.ptr(step_dev), _l.ptr(ws), ws_bytes, *_pl(gp),
                                   _l.ptr(gp.exp_dev), _l.ptr(stat), _l.ptr(zero), zero.numel() if zero is not None else 0,
                                   *_head_layout(L, layout), _l.stream_ptr()), "pxr_ln_bwd_h2s_f32")
    return dz, gp, coef


def attn_bwd_h2s(dctx, qkv, probs, B, H, L, d, sites: H2Sites, site: int, stat: torch.Tensor, p_drop=0.0, seed=0, stream_id=0,
                 step_dev=None) -> Planes:
    """dqkv ONLY as h2 Planes [B*L, 3*H*d] under the site's stale scale (pxr_attn_bwd_h2s_f32); `stat`: ATTN_STAT_SLOTS zeroed words."""
    D = H * d
    assert attn_planes_supported(L, d) and (3 * D) % 32 == 0 and stat.numel() >= ATTN_STAT_SLOTS
    _req(dctx, torch.float32, "dctx"); _req(qkv, torch.float32, "qkv"); _req(probs, torch.float32, "probs")
    device_status(qkv.device)
    gp = sites.planes_like(site, B * L, 3 * D)
    cp, base = _l.c_void_p, qkv.data_ptr()
    _l.check(_l.load().pxr_attn_bwd_h2s_f32(_l.ptr(dctx), D, cp(base), cp(base + 4 * D), cp(base + 8 * D), 3 * D, _l.ptr(probs), B, H, L, d,
                                            p_drop, seed, stream_id, _l.ptr(step_dev), *_pl(gp), 3 * D, 0, D, 2 * D, _l.ptr(gp.exp_dev),
                                            _l.ptr(stat), _l.stream_ptr()), "pxr_attn_bwd_h2s_f32")
    return gp


def h2_bound_exp(dy: Planes, W: Planes, factor: float = 1.0) -> torch.Tensor:
    """int32 [1] on the device: the exponent e with |dy W| * factor * 2^e < 2^15 for EVERY element, from max |dy| and the largest
    column sum of |W| (both gathered by split_h2_auto) -- for an input gradient a GEMM epilogue writes as planes before its own
    maximum can be known (pxr_h2_bound_exp)."""
    assert dy.stats is not None and W.stats is not None
    out = torch.empty(1, dtype=torch.int32, device=dy.buf.device)
    _l.check(_l.load().pxr_h2_bound_exp(_l.ptr(dy.stats), ctypes.c_void_p(W.stats.data_ptr() + 4), float(factor), _l.ptr(out),
                                        _l.stream_ptr()), "pxr_h2_bound_exp")
    return out


def split_planes_multi(mats, outs=None, h2: bool = False):
    """Several fp32 matrices -> Planes in ONE launch (pxr_split_planes_multi_f32); `outs`: existing Planes to overwrite.
    h2=True: the two-plane fp16 format, each matrix scaled by its own power of two (h2_exponent of its max |x|: ONE host
    synchronisation for all of them -- meant for weights that are split once)."""
    for m in mats:
        assert m.dim() == 2 and m.stride(1) == 1 and m.dtype == torch.float32
    if h2:
        assert outs is None
        mx = torch.stack([m.abs().max() for m in mats]).tolist()
        outs = [Planes.alloc(m.shape[0], m.shape[1], m.device, fmt=1) for m in mats]
        device_status(mats[0].device)
        for lo in range(0, len(mats), MULTI_MAX):
            ms, os_ = mats[lo:lo + MULTI_MAX], outs[lo:lo + MULTI_MAX]
            n = len(ms)
            for o, v in zip(os_, mx[lo:lo + MULTI_MAX]):
                o.exp = h2_exponent(float(v))
            P, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
            _l.check(_l.load().pxr_split_h2_multi_f32(
                n, P(*[m.data_ptr() for m in ms]), I64(*[m.shape[0] for m in ms]), I64(*[m.shape[1] for m in ms]),
                I64(*[m.stride(0) for m in ms]), P(*[o.ptr().value for o in os_]), I64(*[o.ps for o in os_]),
                I64(*[o.pr for o in os_]), I32(*[o.exp for o in os_]), _l.stream_ptr()), "pxr_split_h2_multi_f32")
        return outs
    if outs is None:
        outs = [Planes.alloc(m.shape[0], m.shape[1], m.device) for m in mats]
    # the entry point takes at most MULTI_MAX matrices per launch (its argument block is a fixed-size struct): deeper models
    # (4 matrices per layer: n_layers >= 5) take one launch per group
    for lo in range(0, len(mats), MULTI_MAX):
        ms, os_ = mats[lo:lo + MULTI_MAX], outs[lo:lo + MULTI_MAX]
        n = len(ms)
        P, I64 = ctypes.c_void_p * n, ctypes.c_int64 * n
        _l.check(_l.load().pxr_split_planes_multi_f32(
            n, P(*[m.data_ptr() for m in ms]), I64(*[m.shape[0] for m in ms]), I64(*[m.shape[1] for m in ms]),
            I64(*[m.stride(0) for m in ms]), P(*[o.ptr().value for o in os_]), I64(*[o.ps for o in os_]),
            I64(*[o.pr for o in os_]), _l.stream_ptr()), "pxr_split_planes_multi_f32")
    return outs


def linear_fwd_planes(xp: Planes, Wp: Planes, b, gelu: bool = False, save_grad: bool = False, act: str | None = None,
                      want_fp32: bool = True, want_planes: bool = False, lead_shape=None):
    """linear_fwd from planes: y = x W^T + b (xp [M,K], Wp [N,K]).  Returns (y | None, y Planes | None, aux | None) where aux
    is the saved pre-activation / activation derivative of the gelu / act variants (as linear_fwd's second value)."""
    M, K, N = xp.rows, xp.cols, Wp.rows
    dev = xp.buf.device
    shape = tuple(lead_shape) + (N,) if lead_shape is not None else (M, N)
    y = torch.empty(shape, dtype=torch.float32, device=dev) if want_fp32 else None
    yp = Planes.alloc(M, N, dev, fmt=xp.fmt) if want_planes else None
    aux, epi, code = None, EPI_BIAS, 0
    if act is not None and act != "gelu":
        epi, code = EPI_BIAS_ACT_GRAD, ACT_CODES[act]
    elif gelu:
        epi = EPI_BIAS_GELU_GRAD if save_grad else EPI_BIAS_GELU
    if epi != EPI_BIAS:
        aux = torch.empty(shape, dtype=torch.float32, device=dev)
    if xp.fmt:           # fp16 two-plane operands (the output planes, activations, at unit scale)
        gemm_planes(xp, Wp, y.view(M, N) if y is not None else None, epi, bias=b, aux=aux.view(M, N) if aux is not None else None,
                    act=code, Cp=yp)
        return y, yp, aux
    tag = "gemm_p3_kernel<KC,KC,EPI_BIAS_GELU*> (fwd + activation)" if epi != EPI_BIAS else "gemm_p3_kernel<KC,KC,EPI_BIAS> (fwd)"
    with _gemm_timer(2.0 * M * N * K, tag):
        _l.check(_l.load().pxr_gemm_planes_f32(1, M, N, K, xp.ptr(), xp.ps, xp.pr, Wp.ptr(), Wp.ps, Wp.pr, _l.ptr(y), N, epi,
                                               _l.ptr(b), _l.ptr(aux), N, *_pl(yp), code, 0, _l.stream_ptr()),
                 "pxr_gemm_planes_f32")
    return y, yp, aux


def linear_bwd_input_planes(dyp: Planes, Wp: Planes, add: torch.Tensor | None = None, mul: torch.Tensor | None = None,
                            want_fp32: bool = True, want_planes: bool = False, lead_shape=None, mul_bound: float = 1.0):
    """linear_bwd_input from planes: dx = dy W (dyp [M,N], Wp [N,K]) (+ add | * mul).  Returns (dx | None, dx Planes | None).
    h2 operands (both from split_h2_auto): `mul_bound` >= max |mul| enters the bound that fixes the output planes' scale."""
    M, N, K = dyp.rows, dyp.cols, Wp.cols
    assert Wp.rows == N
    dev = dyp.buf.device
    shape = tuple(lead_shape) + (K,) if lead_shape is not None else (M, K)
    dx = torch.empty(shape, dtype=torch.float32, device=dev) if want_fp32 else None
    aux = mul if mul is not None else add
    epi = EPI_MUL if mul is not None else (EPI_ADD if add is not None else EPI_NONE)
    if dyp.fmt:
        # fp16 two-plane operands; the output planes' scale comes from the bound |dy W| * mul_bound (h2_bound_exp)
        dxp = None
        if want_planes:
            dxp = Planes.alloc(M, K, dev, fmt=1)
            pb = dyp.pre_bound
            if pb is not None and Wp.stats is not None and pb[0] == Wp.stats.data_ptr() and pb[1] == float(mul_bound):
                dxp.exp_dev = pb[2]            # the split launch that made dyp computed this bound
            else:
                dxp.exp_dev = h2_bound_exp(dyp, Wp, mul_bound)
        gemm_planes(dyp, Wp, dx.view(M, K) if dx is not None else None, epi, aux=aux.view(M, K) if aux is not None else None, b_kc=False,
                    Cp=dxp)
        return dx, dxp
    dxp = Planes.alloc(M, K, dev) if want_planes else None
    tag = ("gemm_p3_kernel<KC,XC,EPI_MUL> (dX x saved gelu')" if mul is not None else
           "gemm_p3_kernel<KC,XC,EPI_ADD> (dX + residual grad)" if add is not None else "gemm_p3_kernel<KC,XC,EPI_NONE> (dX)")
    with _gemm_timer(2.0 * M * N * K, tag):
        _l.check(_l.load().pxr_gemm_planes_f32(0, M, K, N, dyp.ptr(), dyp.ps, dyp.pr, Wp.ptr(), Wp.ps, Wp.pr, _l.ptr(dx), K,
                                               epi, None, _l.ptr(aux), K, *_pl(dxp), 0, 0, _l.stream_ptr()),
                 "pxr_gemm_planes_f32")
    return dx, dxp


def grouped_dw_planes(problems, tile_hint=0):
    """problems: list of (dy Planes [T,N], x Planes [T,K], dW [N,K] out, db [N] out | None).  One launch for all of them
    (pxr_grouped_dw_planes_f32; one per MULTI_MAX of them: blocks deeper than 4 layers)."""
    if len(problems) > MULTI_MAX:
        for lo in range(0, len(problems), MULTI_MAX):
            grouped_dw_planes(problems[lo:lo + MULTI_MAX], tile_hint)
        return
    L = _l.load()
    n = len(problems)
    P, I, I64 = ctypes.c_void_p * n, ctypes.c_int * n, ctypes.c_int64 * n
    for dy, x, _, _ in problems:
        assert dy.rows == x.rows
    if any(p[0].fmt or p[1].fmt for p in problems):
        if not all(p[0].fmt and p[1].fmt for p in problems):
            raise _l.PxrError("grouped_dw_planes: fp16 two-plane operands need every operand of the launch in that format")
        edev = lambda pl: (pl.exp_dev.data_ptr() if pl.exp_dev is not None else None)
        flops = sum(2.0 * p[0].rows * p[0].cols * p[1].cols for p in problems)
        with _gemm_timer(flops, "grouped_dw_p3_kernel<P4Cfg<..., HALF>> (all dW + db of a block, fp16 two-plane operands)"):
            _l.check(L.pxr_grouped_dw_h2_f32(
                n, P(*[p[0].ptr().value for p in problems]), I64(*[p[0].ps for p in problems]), I64(*[p[0].pr for p in problems]),
                I(*[p[0].exp for p in problems]), P(*[edev(p[0]) for p in problems]),
                P(*[p[1].ptr().value for p in problems]), I64(*[p[1].ps for p in problems]), I64(*[p[1].pr for p in problems]),
                I(*[p[1].exp for p in problems]), P(*[edev(p[1]) for p in problems]),
                P(*[p[2].data_ptr() for p in problems]), P(*[(p[3].data_ptr() if p[3] is not None else None) for p in problems]),
                I(*[p[0].rows for p in problems]), I(*[p[0].cols for p in problems]), I(*[p[1].cols for p in problems]), tile_hint,
                _l.stream_ptr()), "pxr_grouped_dw_h2_f32")
        return
    args = (P(*[p[0].ptr().value for p in problems]), I64(*[p[0].ps for p in problems]), I64(*[p[0].pr for p in problems]),
            P(*[p[1].ptr().value for p in problems]), I64(*[p[1].ps for p in problems]), I64(*[p[1].pr for p in problems]),
            P(*[p[2].data_ptr() for p in problems]), P(*[(p[3].data_ptr() if p[3] is not None else None) for p in problems]),
            I(*[p[0].rows for p in problems]), I(*[p[0].cols for p in problems]), I(*[p[1].cols for p in problems]))
    flops = sum(2.0 * p[0].rows * p[0].cols * p[1].cols for p in problems)
    if tile_hint == 0 and os.environ.get("PXR_P3_DW_TILE"):
        tile_hint = int(os.environ["PXR_P3_DW_TILE"])        # A/B knob (tools/p3_sweep.py)
    with _gemm_timer(flops, "grouped_dw_p3_kernel (all dW + db of the step, from planes)"):
        _l.check(L.pxr_grouped_dw_planes_f32(n, *args, tile_hint, _l.stream_ptr()), "pxr_grouped_dw_planes_f32")


COLSUM_DIRECT_ROWS = int(os.environ.get("PXR_COLSUM_DIRECT_ROWS", "128"))


def colsum(x2d: torch.Tensor, out: torch.Tensor | None = None, defer=None):
    """out[n] = sum_m x[m, n] (deterministic two-stage reduction; second stage deferred when `defer` is given)."""
    L = _l.load()
    _req(x2d, torch.float32, "x")
    M, N = x2d.shape
    o = out if out is not None else torch.empty(N, dtype=torch.float32, device=x2d.device)
    ws_bytes = int(L.pxr_colsum_ws_bytes(M, N))
    if defer is not None and M <= COLSUM_DIRECT_ROWS and x2d.is_contiguous():
        # few rows (the position-embedding gradient of a B = 64 step: 64 rows of L*D): the deferred launch sums the rows themselves --
        # they ARE its partials -- and the first-stage launch is saved
        defer.add(x2d, M, N, o)
        return o
    if defer is not None:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x2d.device)
        defer.add(ws, int(L.pxr_colsum_partial_rows(M)), N, o)
        _l.check(L.pxr_colsum_f32(_l.ptr(x2d), N, M, N, None, _l.ptr(ws), ws_bytes, _l.stream_ptr()), "pxr_colsum_f32")
        return o
    ws = _ws.get(ws_bytes, x2d.device)
    _l.check(L.pxr_colsum_f32(_l.ptr(x2d), N, M, N, _l.ptr(o), _l.ptr(ws), ws_bytes, _l.stream_ptr()), "pxr_colsum_f32")
    return o


# ------------------------------------------------------------------------------------------------ LayerNorm sites
def _pl(p):
    """(ptr, plane stride, panel rows) of an optional Planes"""
    return (p.ptr(), p.ps, p.pr) if p is not None else (None, 0, 0)


def input_ln_fwd(table, idx, idx_bstride, B, L, pos, gamma, beta, eps, p_drop=0.0, seed=0, stream_id=0, save=True,
                 step_dev=None, planes: bool = False):
    """y = dropout(LN(table[idx[b,t]] + pos[t]))  (sasrec.py:68,77-82 / :99-104).  Returns (y, xhat, rstd); with
    planes=True a 4th value: y as Planes [B*L, D] (written by the same kernel)."""
    Lb = _l.load()
    _req(table, torch.float32, "table"); _req(idx, torch.int64, "idx", contiguous=False)
    N, D = table.shape
    device_status(table.device)
    y = torch.empty(B, L, D, dtype=torch.float32, device=table.device)
    xhat = torch.empty_like(y) if save else None
    rstd = torch.empty(B * L, dtype=torch.float32, device=table.device) if save else None
    # algorithmic bytes: B*L table rows read once + y (+ xhat when saved) written; the [B,2,L+1,D] gather of the
    # reference never exists (SURVEY.md §8d "fused" rule)
    h2 = planes == "h2"
    yp = Planes.alloc(B * L, D, table.device, fmt=int(h2)) if planes else None
    # (+ the planes of y -- three bf16 ones, 6 B per element, or two fp16 ones -- when the kernel also writes them for the QKV GEMM)
    with _gemm_timer(B * L * D * (4.0 * (3 if save else 2) + ((4.0 if h2 else 6.0) if planes else 0.0)), "ln_fwd_kernel<GATHER> (gather + pos + LN + dropout)"):
        _l.check(Lb.pxr_input_ln_fwd_f32(_l.ptr(table), N, _l.ptr(idx), idx_bstride, _l.ptr(pos), _l.ptr(gamma),
                                         _l.ptr(beta), eps, B, L, D, _l.ptr(y), _l.ptr(xhat), _l.ptr(rstd), p_drop,
                                         seed, stream_id, _l.ptr(step_dev), *_pl(yp), int(h2), _l.stream_ptr()),
                 "pxr_input_ln_fwd_f32")
    return (y, xhat, rstd, yp) if planes else (y, xhat, rstd)


def ln_residual_fwd(x, res, gamma, beta, eps, p_drop=0.0, seed=0, stream_id=0, save=True, step_dev=None, planes: bool = False,
                    want_y: bool = True):
    """y = LN(dropout(x) + res)  (layers.py:614-615, :670-671).  Returns (y, xhat, rstd) (+ y as Planes with planes=True;
    want_y=False then skips the fp32 copy of y)."""
    Lb = _l.load()
    _req(x, torch.float32, "x")
    D = x.shape[-1]
    rows = x.numel() // D
    assert want_y or planes
    y = torch.empty_like(x) if want_y else None
    xhat = torch.empty_like(x) if save else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save else None
    h2 = planes == "h2"               # y as two fp16 planes (the image tower, the sequence block of large batches)
    yp = Planes.alloc(rows, D, x.device, fmt=int(h2)) if planes else None
    if h2:
        device_status(x.device)
    _l.check(Lb.pxr_ln_residual_fwd_f32(_l.ptr(x), _l.ptr(res), _l.ptr(gamma), _l.ptr(beta), eps, rows, D, _l.ptr(y), _l.ptr(xhat),
                                        _l.ptr(rstd), p_drop, seed, stream_id, _l.ptr(step_dev), *_pl(yp), int(h2), _l.stream_ptr()),
             "pxr_ln_residual_fwd_f32")
    return (y, xhat, rstd, yp) if planes else (y, xhat, rstd)


def ln_gather_fwd(cache, ids, T, gamma, beta, eps, save=True, planes: bool = False, want_y: bool = True):
    """x[i, t, :] = cache[ids[i], t, :] and y = LN(x) in one launch (pxr_ln_gather_fwd_f32): cache fp32 [N, T*D], ids int64 [n].
    Returns (x [n, T, D], y, xhat, rstd) (+ y as Planes with planes=True / "h2"; want_y=False then skips the fp32 copy of y) --
    embed_gather(cache, ids) followed by ln_residual_fwd, bit for bit.  An id outside [0, N) is flagged and clamped."""
    Lb = _l.load()
    _req(cache, torch.float32, "cache"); _req(ids, torch.int64, "ids")
    D = gamma.numel()
    N, n = cache.shape[0], ids.numel()
    if cache.dim() != 2 or cache.shape[1] != T * D or ids.dim() != 1:
        raise _l.PxrError(f"ln_gather_fwd: cache must be [N, T*D = {T * D}] and ids [n], got {tuple(cache.shape)} / {tuple(ids.shape)}")
    assert want_y or planes
    device_status(cache.device)
    x = torch.empty(n, T, D, dtype=torch.float32, device=cache.device)
    y = torch.empty_like(x) if want_y else None
    xhat = torch.empty_like(x) if save else None
    rstd = torch.empty(n * T, dtype=torch.float32, device=cache.device) if save else None
    h2 = planes == "h2"
    yp = Planes.alloc(n * T, D, cache.device, fmt=int(h2)) if planes else None
    _l.check(Lb.pxr_ln_gather_fwd_f32(_l.ptr(cache), N, _l.ptr(ids), n, T, _l.ptr(gamma), _l.ptr(beta), eps, D, _l.ptr(x), _l.ptr(y),
                                      _l.ptr(xhat), _l.ptr(rstd), *_pl(yp), int(h2), _l.stream_ptr()), "pxr_ln_gather_fwd_f32")
    return (x, y, xhat, rstd, yp) if planes else (x, y, xhat, rstd)


def ln_residual_bpr_fwd(x, res, gamma, beta, eps, table, items, masked_index, p_drop=0.0, seed=0, stream_id=0, save=True,
                        step_dev=None, layout=None, defer_loss: list | None = None):
    """The block's last LayerNorm with the loss head's forward fused in (pxr_ln_residual_bpr_fwd_f32):
    -> (y [B,L,D], xhat, rstd, loss [1], pos [B,L], neg [B,L]) -- what ln_residual_fwd + bpr_loss_fwd return, bit for bit for
    D <= 1024; beyond, y / xhat / rstd bit for bit and the scores / loss within the fp32 rounding of the dot product.
    layout = (id_bstride, pos_off, neg_off) of the target / negative ids in `items` (None: SASRec's shifted [B, 2, L+1] windows;
    BERT4Rec's aligned [B, 3, L]: (3L, L, 2L)).
    defer_loss (a list): the one-workgroup sum over the per-position terms is NOT launched; the returned loss tensor stays unwritten
    until the problem (lossrow, B, L, loss) appended to the list has run -- as part of a TailRider in the same step's backward."""
    Lb = _l.load()
    _req(x, torch.float32, "x"); _req(table, torch.float32, "table")
    _req(items, torch.int64, "items"); _req(masked_index, torch.int64, "masked_index")
    B, L, D = x.shape
    dev = x.device
    y = torch.empty_like(x)
    xhat = torch.empty_like(x) if save else None
    rstd = torch.empty(B * L, dtype=torch.float32, device=dev) if save else None
    pos = torch.empty(B, L, dtype=torch.float32, device=dev)
    neg = torch.empty(B, L, dtype=torch.float32, device=dev)
    lossrow = torch.empty(B * L, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    device_status(dev)                # an id outside the table flags the status word (raise_on_bad_indices)
    with _gemm_timer(0.0, "ln_fwd_kernel<RESIDUAL + loss head>"):
        _l.check(Lb.pxr_ln_residual_bpr_fwd_f32(_l.ptr(x), _l.ptr(res), _l.ptr(gamma), _l.ptr(beta), eps, B, L, D, _l.ptr(y),
                                                _l.ptr(xhat), _l.ptr(rstd), p_drop, seed, stream_id, _l.ptr(step_dev), _l.ptr(table),
                                                table.shape[0], _l.ptr(items), _l.ptr(masked_index), _l.ptr(pos), _l.ptr(neg),
                                                _l.ptr(lossrow), None if defer_loss is not None else _l.ptr(loss),
                                                *_head_layout(L, layout), _l.stream_ptr()),
                 "pxr_ln_residual_bpr_fwd_f32")
    if defer_loss is not None:
        defer_loss.append((lossrow, B, L, loss))
    return y, xhat, rstd, loss, pos, neg


def bpr_ln_bwd(pos, neg, table, items, masked_index, grad_scale, grad_scale_dev, xhat, rstd, gamma, dgamma, dbeta, p_drop=0.0,
               seed=0, stream_id=0, need_dx=False, step_dev=None, defer=None, planes: bool = False, stat: torch.Tensor | None = None,
               layout=None):
    """bpr_loss_bwd + ln_bwd(0, ...) of the block's last LayerNorm in one launch (pxr_bpr_ln_bwd_f32): the gradient w.r.t. the
    block's output never reaches HBM.  -> (dz, dx | None, planes of the gradient the next GEMMs read | None, coef [B,L]).
    layout: as ln_residual_bpr_fwd."""
    Lb = _l.load()
    B, L = pos.shape
    D = xhat.shape[-1]
    rows = B * L
    dz = torch.empty_like(xhat)
    dx = torch.empty_like(xhat) if need_dx else None
    coef = torch.empty(B, L, dtype=torch.float32, device=pos.device)
    ws_bytes = int(Lb.pxr_ln_bwd_ws_bytes(rows, D))
    if defer is not None:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=xhat.device)   # must outlive this call
        defer.add(ws, int(Lb.pxr_ln_bwd_partial_rows(rows)), 2 * D, dgamma, dbeta, D)
        dgamma = dbeta = None
    else:
        ws = _ws.get(ws_bytes, xhat.device)
    assert not (planes and stat is not None)
    gp = Planes.alloc(rows, D, xhat.device) if planes else None
    _l.check(Lb.pxr_bpr_ln_bwd_f32(_l.ptr(pos), _l.ptr(neg), _l.ptr(table), table.shape[0], _l.ptr(items), _l.ptr(masked_index), B, L,
                                   float(grad_scale), _l.ptr(grad_scale_dev), _l.ptr(coef), _l.ptr(xhat), _l.ptr(rstd), _l.ptr(gamma), D,
                                   _l.ptr(dz), _l.ptr(dx), _l.ptr(dgamma), _l.ptr(dbeta), p_drop, seed, stream_id, _l.ptr(step_dev),
                                   _l.ptr(ws), ws_bytes, *_pl(gp), _l.ptr(stat), *_head_layout(L, layout), _l.stream_ptr()),
             "pxr_bpr_ln_bwd_f32")
    return dz, dx, gp, coef


def tail_riders_on() -> bool:
    """The knob PXR_TAIL_RIDERS (default 1), read per call: the reductions that close a backward pass ride in the segment-sum launch
    of the table gradient (TailRider) instead of running as launches of their own."""
    return os.environ.get("PXR_TAIL_RIDERS", "1") != "0"


class _CTailRider(ctypes.Structure):
    """include/pxr.h: pxr_tail_rider."""
    _fields_ = [("n", ctypes.c_int32), ("B", ctypes.c_int32), ("L", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("part", ctypes.c_void_p * 16), ("out_a", ctypes.c_void_p * 16), ("out_b", ctypes.c_void_p * 16),
                ("P", ctypes.c_int32 * 16), ("N", ctypes.c_int32 * 16), ("split", ctypes.c_int32 * 16),
                ("bump_counter", ctypes.c_void_p), ("lossrow", ctypes.c_void_p), ("loss", ctypes.c_void_p)]


class TailRider:
    """Small reductions prepared for a launch that runs anyway (the segment sums of the table gradient: sasrec_occ_segsum /
    sasrec_occ_segsum_apply take one as `rider`): up to 16 problems of DeferredReductions, the counter bump that travels with them,
    and the loss sum a forward left undone (ln_residual_bpr_fwd(defer_loss=...)).  Holds its tensors until it is handed over."""

    def __init__(self, items=(), bump=None, loss=None):
        assert len(items) <= 16 and (bump is None or items)
        self.items, self.bump, self.loss = list(items), bump, loss     # loss: (lossrow, B, L, loss) | None

    def __bool__(self):
        return bool(self.items) or self.loss is not None

    def c_arg(self):
        """(pointer argument for the entry point, the structure to keep alive across the call)."""
        if not self:
            return None, None
        r = _CTailRider()
        r.n = len(self.items)
        for i, (part, P, N, out_a, out_b, split) in enumerate(self.items):
            r.part[i], r.out_a[i], r.out_b[i] = part.data_ptr(), out_a.data_ptr(), (out_b.data_ptr() if out_b is not None else None)
            r.P[i], r.N[i], r.split[i] = P, N, split
        r.bump_counter = self.bump.data_ptr() if self.bump is not None else None
        if self.loss is not None:
            lossrow, B, L, loss = self.loss
            r.lossrow, r.B, r.L, r.loss = lossrow.data_ptr(), B, L, loss.data_ptr()
        return ctypes.cast(ctypes.pointer(r), ctypes.c_void_p), r


class DeferredReductions:
    """Collects the second stage of several partial reductions (LayerNorm dgamma|dbeta, column sums) so that one
    launch finishes all of them at the end of a backward pass."""

    def __init__(self):
        self.items = []      # (part tensor, P, N, out_a, out_b | None, split)

    def add(self, part, P, N, out_a, out_b=None, split=0):
        self.items.append((part, P, N, out_a, out_b, split))

    def flush(self, bump: torch.Tensor | None = None, prepare: bool = False):
        """One launch (per 16 problems).  `bump`: an int64 device counter the LAST launch increments by one; returns
        whether it did (False when there was nothing to reduce: the caller then bumps it itself).
        prepare=True launches NOTHING: the collected problems (and the bump) are returned as a TailRider for a launch that will
        carry them, and the collector is left empty -- or None, with the collector untouched, when one rider cannot hold them
        (none, or more than 16): the caller then flushes as usual."""
        if prepare:
            if not self.items or len(self.items) > 16:
                return None
            rider, self.items = TailRider(self.items, bump), []
            return rider
        if not self.items:
            return False
        Lb = _l.load()
        for c0 in range(0, len(self.items), 16):
            it = self.items[c0:c0 + 16]
            n = len(it)
            last = c0 + 16 >= len(self.items)
            Pp, I = ctypes.c_void_p * n, ctypes.c_int * n
            _l.check(Lb.pxr_reduce_partials_multi_f32(
                n, Pp(*[x[0].data_ptr() for x in it]), I(*[x[1] for x in it]), I(*[x[2] for x in it]),
                Pp(*[x[3].data_ptr() for x in it]), Pp(*[(x[4].data_ptr() if x[4] is not None else None) for x in it]),
                I(*[x[5] for x in it]), _l.ptr(bump) if (bump is not None and last) else None, _l.stream_ptr()),
                "pxr_reduce_partials_multi_f32")
        self.items = []
        return bump is not None


def ln_bwd(gather_mode, dy, xhat, rstd, gamma, dgamma, dbeta, p_drop=0.0, seed=0, stream_id=0, need_dx=False,
           step_dev=None, defer: DeferredReductions | None = None, planes: bool = False, stat: torch.Tensor | None = None,
           zero: torch.Tensor | None = None, res: torch.Tensor | None = None):
    """Backward of either LN site; dgamma/dbeta ([D] tensors) are overwritten (by `defer.flush()` when a
    DeferredReductions collector is given).  Returns (dz, dx|None) (+ with planes=True the Planes of dx when it exists,
    else of dz: what the following GEMMs read).  res (a residual site without dropout -- a pre-LN block of the image tower): the
    launch returns dz = res + LayerNorm-backward(dy), and `stat` then holds the partial maxima of that sum (pxr_ln_bwd_res_f32)."""
    Lb = _l.load()
    _req(dy, torch.float32, "dy")
    D = dy.shape[-1]
    rows = dy.numel() // D
    dz = torch.empty_like(dy)
    dx = torch.empty_like(dy) if need_dx else None
    ws_bytes = int(Lb.pxr_ln_bwd_ws_bytes(rows, D))
    if defer is not None:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dy.device)   # must outlive this call
        defer.add(ws, int(Lb.pxr_ln_bwd_partial_rows(rows)), 2 * D, dgamma, dbeta, D)
        dgamma = dbeta = None
    else:
        ws = _ws.get(ws_bytes, dy.device)
    if res is not None:
        assert not gather_mode and not planes and not need_dx and p_drop == 0.0 and zero is None
        _req(res, torch.float32, "res")
        assert res.numel() == dy.numel() and (stat is None or stat.numel() >= ln_bwd_stat_parts(rows))
        _l.check(Lb.pxr_ln_bwd_res_f32(_l.ptr(dy), _l.ptr(xhat), _l.ptr(rstd), _l.ptr(gamma), _l.ptr(res), rows, D, _l.ptr(dz),
                                       _l.ptr(dgamma), _l.ptr(dbeta), _l.ptr(ws), ws_bytes, _l.ptr(stat), _l.stream_ptr()),
                 "pxr_ln_bwd_res_f32")
        return dz, None
    if stat is not None:        # also: per-workgroup partial maxima of |gradient the next GEMMs read| into stat[:ln_bwd_stat_parts(rows)];
        assert not planes and not gather_mode       # `zero` (<= 256 floats): cleared by the launch (attn_bwd's spread slots)
        assert stat.numel() >= ln_bwd_stat_parts(rows) and (zero is None or zero.numel() <= 256)
        _l.check(Lb.pxr_ln_bwd_stat_f32(_l.ptr(dy), _l.ptr(xhat), _l.ptr(rstd), _l.ptr(gamma), rows, D, _l.ptr(dz), _l.ptr(dx),
                                        _l.ptr(dgamma), _l.ptr(dbeta), p_drop, seed, stream_id, _l.ptr(step_dev), _l.ptr(ws), ws_bytes,
                                        _l.ptr(stat), _l.ptr(zero), zero.numel() if zero is not None else 0, _l.stream_ptr()),
                 "pxr_ln_bwd_stat_f32")
        return dz, dx
    gp = Planes.alloc(rows, D, dy.device) if planes else None
    _l.check(Lb.pxr_ln_bwd_f32(int(gather_mode), _l.ptr(dy), _l.ptr(xhat), _l.ptr(rstd), _l.ptr(gamma), rows, D,
                               _l.ptr(dz), _l.ptr(dx), _l.ptr(dgamma), _l.ptr(dbeta), p_drop, seed, stream_id,
                               _l.ptr(step_dev), _l.ptr(ws), ws_bytes, *_pl(gp), _l.stream_ptr()), "pxr_ln_bwd_f32")
    return (dz, dx, gp) if planes else (dz, dx)


# ------------------------------------------------------------------------------------------------ attention
ATTN_FUSED_MAX_L = 128     # sequences beyond this take the batched-GEMM path below (any length)


def _attn_takes_gemm_path(L, d):
    """Beyond 128 positions -- or 65..128 with a head size that is not a multiple of 8, which the two-keys-per-lane fused
    kernels need, or with the MFMA kernels turned off (PXR_ATTN_MFMA=0: attn_planes_supported(1, 8) is false exactly then) --
    the attention runs as batched GEMMs + the row kernel (any length, head size % 4 == 0)."""
    return L > ATTN_FUSED_MAX_L or (L > 64 and (d % 8 != 0 or not attn_planes_supported(1, 8)))


def _attn_long_fwd(qkv, keymask, km_bstride, B, H, L, d, p_drop, seed, stream_id, step_dev, causal=True):
    """MAX_ITEM_LIST_LENGTH > 128: S = Q K^T and O = PD V as batched fp32-MFMA GEMMs (grid.z = batch x head) around the
    row kernel pxr_attn_rows_fwd_f32 (mask + softmax + dropout).  Same arithmetic as the fused kernels."""
    Lb = _l.load()
    D, ld, Lp, bh = H * d, 3 * H * d, (L + 3) & ~3, B * H
    P = torch.empty(bh, L, Lp, dtype=torch.float32, device=qkv.device)
    sP, sQ, sC = (H * L * Lp, L * Lp), (L * ld, d), (L * D, d)
    gemm_batched(True, True, L, L, d, qkv, 0, ld, qkv, D, ld, P, 0, Lp, bh, H, sQ, sQ, sP)            # q at 0, k at D
    PD = torch.empty_like(P) if p_drop > 0 else None
    _l.check(Lb.pxr_attn_rows_fwd_f32(_l.ptr(P), _l.ptr(PD), _l.ptr(keymask), km_bstride, B, H, L, Lp, p_drop, seed, stream_id,
                                      _l.ptr(step_dev), d, int(causal), _l.stream_ptr()), "pxr_attn_rows_fwd_f32")
    ctx = torch.empty(B, L, D, dtype=torch.float32, device=qkv.device)
    gemm_batched(True, False, L, d, L, PD if PD is not None else P, 0, Lp, qkv, 2 * D, ld, ctx, 0, D, bh, H, sP, sQ, sC)
    return ctx, (P, PD)


def _attn_long_bwd(dctx, qkv, saved, B, H, L, d, p_drop, seed, stream_id, step_dev):
    Lb = _l.load()
    P, PD = saved
    D, ld, Lp, bh = H * d, 3 * H * d, (L + 3) & ~3, B * H
    sP, sQ, sC = (H * L * Lp, L * Lp), (L * ld, d), (L * D, d)
    dqkv = torch.empty_like(qkv)
    gemm_batched(False, False, L, d, L, PD if PD is not None else P, 0, Lp, dctx, 0, D, dqkv, 2 * D, ld, bh, H, sP, sC, sQ)  # dV
    dP = torch.empty_like(P)
    gemm_batched(True, True, L, L, d, dctx, 0, D, qkv, 2 * D, ld, dP, 0, Lp, bh, H, sC, sQ, sP)                         # dPD
    _l.check(Lb.pxr_attn_rows_bwd_f32(_l.ptr(P), _l.ptr(dP), B, H, L, Lp, p_drop, seed, stream_id, _l.ptr(step_dev), d,
                                      _l.stream_ptr()), "pxr_attn_rows_bwd_f32")
    gemm_batched(True, False, L, d, L, dP, 0, Lp, qkv, D, ld, dqkv, 0, ld, bh, H, sP, sQ, sQ)                           # dQ = dS K
    gemm_batched(False, False, L, d, L, dP, 0, Lp, qkv, 0, ld, dqkv, D, ld, bh, H, sP, sQ, sQ)                          # dK = dS^T Q
    return dqkv


def attn_planes_supported(L: int, d: int) -> bool:
    return bool(_l.load().pxr_attn_planes_supported(L, d))


def attn_fwd(qkv, keymask, km_bstride, B, H, L, d, p_drop=0.0, seed=0, stream_id=0, save=True, step_dev=None,
             planes: bool = False, causal: bool = True):
    """qkv [B,L,3*H*d] fused projection output -> (ctx [B,L,H*d], probs [B,H,L,L] | None).  planes=True: ctx is returned
    as Planes [B*L, H*d] INSTEAD of the fp32 tensor (written by the fused kernel where it serves the shape, by a split
    launch otherwise).  causal=False: the key-padding mask only (BERT4Rec); attn_bwd serves both masks (it works from the saved
    probabilities)."""
    Lb = _l.load()
    _req(qkv, torch.float32, "qkv"); _req(keymask, torch.int64, "keymask", contiguous=False)
    D = H * d
    if _attn_takes_gemm_path(L, d):
        ctx, saved = _attn_long_fwd(qkv, keymask, km_bstride, B, H, L, d, p_drop, seed, stream_id, step_dev, causal=causal)
        return (split_planes(ctx.view(B * L, D)) if planes else ctx), (saved if save else None)
    fused_p = planes and attn_planes_supported(L, d)
    h2 = planes == "h2"
    assert fused_p or not h2, "h2 context planes come from the fused kernel only (attn_planes_supported)"
    ctx = None if fused_p else torch.empty(B, L, D, dtype=torch.float32, device=qkv.device)
    cp_ = Planes.alloc(B * L, D, qkv.device, fmt=int(h2)) if fused_p else None
    probs = torch.empty(B, H, L, L, dtype=torch.float32, device=qkv.device) if save else None
    base = qkv.data_ptr()
    q, k, v = _l.c_void_p(base), _l.c_void_p(base + 4 * D), _l.c_void_p(base + 8 * D)
    _l.check(Lb.pxr_attn_fwd_f32(q, k, v, 3 * D, _l.ptr(keymask), km_bstride, B, H, L, d, _l.ptr(ctx), D, _l.ptr(probs), p_drop, seed,
                                 stream_id, _l.ptr(step_dev), *_pl(cp_), int(h2), int(causal), _l.stream_ptr()), "pxr_attn_fwd_f32")
    if planes and not fused_p:
        cp_ = split_planes(ctx.view(B * L, D))
    return (cp_ if planes else ctx), probs


def attn_bwd(dctx, qkv, probs, B, H, L, d, p_drop=0.0, seed=0, stream_id=0, step_dev=None, planes: bool = False,
             stat: torch.Tensor | None = None):
    """-> dqkv [B,L,3*H*d] laid out like qkv; planes=True: as Planes [B*L, 3*H*d] INSTEAD of the fp32 tensor.  stat (ATTN_STAT_SLOTS
    ZEROED float32 words; shapes of attn_planes_supported only): also max |dqkv|, spread over the words (one atomic per workgroup)."""
    Lb = _l.load()
    D = H * d
    if stat is not None:
        assert not planes and attn_planes_supported(L, d) and stat.numel() >= ATTN_STAT_SLOTS
        _req(dctx, torch.float32, "dctx"); _req(qkv, torch.float32, "qkv"); _req(probs, torch.float32, "probs")
        dqkv = torch.empty_like(qkv)
        cp = _l.c_void_p
        base, g = qkv.data_ptr(), dqkv.data_ptr()
        _l.check(Lb.pxr_attn_bwd_stat_f32(_l.ptr(dctx), D, cp(base), cp(base + 4 * D), cp(base + 8 * D), 3 * D, _l.ptr(probs), B, H, L, d,
                                          cp(g), cp(g + 4 * D), cp(g + 8 * D), 3 * D, p_drop, seed, stream_id, _l.ptr(step_dev),
                                          _l.ptr(stat), _l.stream_ptr()), "pxr_attn_bwd_stat_f32")
        return dqkv
    if _attn_takes_gemm_path(L, d):
        dqkv = _attn_long_bwd(dctx, qkv, probs, B, H, L, d, p_drop, seed, stream_id, step_dev)
        return split_planes(dqkv.view(B * L, 3 * D)) if planes else dqkv
    _req(dctx, torch.float32, "dctx"); _req(qkv, torch.float32, "qkv"); _req(probs, torch.float32, "probs")
    fused_p = planes and attn_planes_supported(L, d) and (3 * D) % 32 == 0
    dqkv = None if fused_p else torch.empty_like(qkv)
    gp = Planes.alloc(B * L, 3 * D, qkv.device) if fused_p else None
    base = qkv.data_ptr()
    cp = _l.c_void_p
    dptr = (lambda o: None) if fused_p else (lambda o: cp(dqkv.data_ptr() + o))
    _l.check(Lb.pxr_attn_bwd_f32(_l.ptr(dctx), D, cp(base), cp(base + 4 * D), cp(base + 8 * D), 3 * D, _l.ptr(probs),
                                 B, H, L, d, dptr(0), dptr(4 * D), dptr(8 * D), 3 * D, p_drop, seed,
                                 stream_id, _l.ptr(step_dev), *_pl(gp), 3 * D, 0, D, 2 * D, _l.stream_ptr()),
             "pxr_attn_bwd_f32")
    if planes and not fused_p:
        gp = split_planes(dqkv.view(B * L, 3 * D))
    return gp if planes else dqkv


# ------------------------------------------------------------------------------------------------ loss head
def _sasrec_layout(L: int):
    """SASRec's shifted [B, 2, L+1] id windows: (id_bstride, in_off, pos_off, neg_off) -- the inputs items[:, 0, t], the targets
    items[:, 0, t+1], the negatives items[:, 1, t+1] of the L positions.  What layout=None means throughout this module.
    items[:, 1, 0] is read by no kernel, so an id outside the table there is not flagged in the status word -- the reference embeds
    the whole items tensor (sasrec.py:68) and would raise on it."""
    return 2 * (L + 1), 0, 1, L + 2


def _head_layout(L: int, layout):
    """(id_bstride, pos_off, neg_off) of the loss head's target / negative ids: `layout`, or SASRec's windows when None."""
    if layout is not None:
        return tuple(layout)
    bstride, _, pos_off, neg_off = _sasrec_layout(L)
    return bstride, pos_off, neg_off


def bpr_loss_fwd(out, table, items, masked_index, layout=None):
    """-> (loss [1] on device, pos_score [B,L], neg_score [B,L])   (sasrec.py:88-92).  layout = (id_bstride, pos_off, neg_off) of the
    target / negative ids (None: SASRec's shifted windows; BERT4Rec: (3L, L, 2L), bert4rec.py:98-111)."""
    Lb = _l.load()
    _req(out, torch.float32, "out"); _req(table, torch.float32, "table")
    _req(items, torch.int64, "items"); _req(masked_index, torch.int64, "masked_index")
    B, L, D = out.shape
    dev = out.device
    pos = torch.empty(B, L, dtype=torch.float32, device=dev)
    neg = torch.empty(B, L, dtype=torch.float32, device=dev)
    lossrow = torch.empty(B * L, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    device_status(dev)                # an id outside the table flags the status word (raise_on_bad_indices)
    _l.check(Lb.pxr_bpr_loss_fwd_f32(_l.ptr(out), _l.ptr(table), table.shape[0], _l.ptr(items), _l.ptr(masked_index), B, L, D,
                                     _l.ptr(pos), _l.ptr(neg), _l.ptr(lossrow), _l.ptr(loss), *_head_layout(L, layout), _l.stream_ptr()),
             "pxr_bpr_loss_fwd_f32")
    return loss, pos, neg


def bpr_loss_bwd(pos, neg, table, items, masked_index, D, grad_scale=1.0, grad_scale_dev=None, layout=None):
    """-> (dout [B,L,D], coef [B,L])."""
    Lb = _l.load()
    B, L = pos.shape
    dout = torch.empty(B, L, D, dtype=torch.float32, device=pos.device)
    coef = torch.empty(B, L, dtype=torch.float32, device=pos.device)
    _l.check(Lb.pxr_bpr_loss_bwd_f32(_l.ptr(pos), _l.ptr(neg), _l.ptr(table), table.shape[0], _l.ptr(items), _l.ptr(masked_index), B, L,
                                     D, float(grad_scale), _l.ptr(grad_scale_dev), _l.ptr(dout), _l.ptr(coef), *_head_layout(L, layout),
                                     _l.stream_ptr()), "pxr_bpr_loss_bwd_f32")
    return dout, coef


# ------------------------------------------------------------------------------------------------ sparse table grad
class SparseRows:
    """(uniq_idx [cap] int64 ascending, rows [cap, D], n [1] int32 on device): the table gradient of one step."""

    def __init__(self, cap: int, D: int, device, packed: bool = False):
        self.cap = cap
        self.packed = None
        # True: this step's rows were applied to the table where they were summed (sasrec_occ_segsum_apply) -- `rows` was not
        # written and the optimizer's step() has no row launch left to do
        self.applied = False
        if packed:
            # idx | n | rows are views of ONE buffer laid out as pxr.h's packed block, so a data-parallel exchange
            # sends it with a single all-gather (parallel.GradSync) and pxr_merge_packed_rows_f32 reads it as it is
            Lb = _l.load()
            off = int(Lb.pxr_packed_rows_offset(cap))
            buf = torch.zeros(int(Lb.pxr_packed_rows_bytes(cap, D)), dtype=torch.uint8, device=device)
            self.idx = buf[:cap * 8].view(torch.int64)
            self.n = buf[cap * 8:cap * 8 + 4].view(torch.int32)
            self.rows = buf[off:].view(torch.float32).view(cap, D)
            self.packed = buf
            return
        self.idx = torch.zeros(cap, dtype=torch.int64, device=device)
        self.rows = torch.empty(cap, D, dtype=torch.float32, device=device)
        self.n = torch.zeros(1, dtype=torch.int32, device=device)

    def count(self) -> int:  # host sync; tests / logging only
        return int(self.n.item())

    def to_dense(self, n_table: int) -> torch.Tensor:  # tests only
        n = self.count()
        g = torch.zeros(n_table, self.rows.shape[1], dtype=torch.float32, device=self.rows.device)
        keep = self.idx[:n] > 0          # a merged (non-compacted) list marks its empty slots with id 0
        g[self.idx[:n][keep]] = self.rows[:n][keep]
        return g


def embed_grad_rows(idx, rows, n_table, scale=1.0, out: SparseRows | None = None) -> SparseRows:
    """Plain embedding backward in sparse form (see pxr.h)."""
    Lb = _l.load()
    _req(idx, torch.int64, "idx"); _req(rows, torch.float32, "rows")
    n, D = idx.numel(), rows.shape[-1]
    sp = out if out is not None else SparseRows(n, D, rows.device)
    ws_bytes = int(Lb.pxr_embed_grad_ws_bytes(n))
    ws = _ws.get(ws_bytes, rows.device)
    _l.check(Lb.pxr_embed_grad_rows_f32(_l.ptr(idx), n, _l.ptr(rows), D, n_table, float(scale), _l.ptr(sp.idx),
                                        _l.ptr(sp.rows), _l.ptr(sp.n), _l.ptr(ws), ws_bytes, _l.stream_ptr()),
             "pxr_embed_grad_rows_f32")
    return sp


def embed_grad_dense(idx, rows, n_rows: int, out=None):
    """embed_grad_rows (scale 1) as a dense block over a batch-local row space (pxr_embed_grad_dense_f32): idx int64 [n] holds rows
    of an [n_rows, D] matrix (0 = "no item", dropped; ids outside [0, n_rows) dropped), rows [n, D] one gradient row per occurrence
    -> d_rows float32 [n_rows, D]: embed_grad_rows' row sums, bit for bit, at their rows and exactly +0.0 everywhere else (row 0,
    unreferenced rows), whatever `out` held before."""
    Lb = _l.load()
    _req(idx, torch.int64, "idx"); _req(rows, torch.float32, "rows")
    n = idx.numel()
    if n < 1 or rows.dim() != 2 or rows.shape[0] != n or n_rows < 1:
        raise _l.PxrError(f"embed grad dense: need idx [n], rows [n, D] and n_rows >= 1, got idx {tuple(idx.shape)}, rows {tuple(rows.shape)}, "
                          f"n_rows={n_rows}")
    D = rows.shape[1]
    d_rows = _out_f32(out, (int(n_rows), D), rows.device, "embed grad dense", "d_rows")
    ws_bytes = int(Lb.pxr_embed_grad_ws_bytes(n))
    ws = _ws.get(ws_bytes, rows.device)
    _l.check(Lb.pxr_embed_grad_dense_f32(_l.ptr(idx), n, _l.ptr(rows), D, int(n_rows), _l.ptr(d_rows), _l.ptr(ws), ws_bytes,
                                         _l.stream_ptr()), "pxr_embed_grad_dense_f32")
    return d_rows


def merge_sorted_rows(idx_all, rows_all, world, n_table, scale=1.0, out: SparseRows | None = None) -> SparseRows:
    """Merge `world` sorted-unique sparse gradients (idx_all [world*cap] padded with ids >= n_table, rows_all
    [world*cap, D]) without re-sorting; the result keeps world*cap slots, empty ones carry id 0 (see pxr.h)."""
    Lb = _l.load()
    _req(idx_all, torch.int64, "idx_all"); _req(rows_all, torch.float32, "rows_all")
    E, D = idx_all.numel(), rows_all.shape[-1]
    cap = E // world
    sp = out if out is not None else SparseRows(E, D, rows_all.device)
    ws_bytes = int(Lb.pxr_merge_rows_ws_bytes(world, cap))
    ws = _ws.get(ws_bytes, rows_all.device)
    _l.check(Lb.pxr_merge_sorted_rows_f32(_l.ptr(idx_all), _l.ptr(rows_all), world, cap, D, n_table, float(scale),
                                          _l.ptr(sp.idx), _l.ptr(sp.rows), _l.ptr(sp.n), _l.ptr(ws), ws_bytes,
                                          _l.stream_ptr()), "pxr_merge_sorted_rows_f32")
    return sp


def merge_packed_rows(packed_all, world, cap, D, n_table, scale=1.0, out: SparseRows | None = None) -> SparseRows:
    """merge_sorted_rows on `world` packed blocks (SparseRows(packed=True).packed of every rank, concatenated by one
    all-gather): counts travel inside the blocks, so the lists need no PAD tail (see pxr.h)."""
    Lb = _l.load()
    _req(packed_all, torch.uint8, "packed_all")
    if packed_all.numel() != world * int(Lb.pxr_packed_rows_bytes(cap, D)):
        raise ValueError("merge_packed_rows: packed_all has the wrong size for (world, cap, D)")
    sp = out if out is not None else SparseRows(world * cap, D, packed_all.device)
    ws_bytes = int(Lb.pxr_merge_rows_ws_bytes(world, cap))
    ws = _ws.get(ws_bytes, packed_all.device)
    _l.check(Lb.pxr_merge_packed_rows_f32(_l.ptr(packed_all), world, cap, D, n_table, float(scale), _l.ptr(sp.idx),
                                          _l.ptr(sp.rows), _l.ptr(sp.n), _l.ptr(ws), ws_bytes, _l.stream_ptr()),
             "pxr_merge_packed_rows_f32")
    return sp


def merge_split_rows(heads_all, rows_all, world, cap, cap_x, D, n_table, scale=1.0, out: SparseRows | None = None):
    """merge on the two-collective exchange with a reduced row capacity (see pxr.h)."""
    Lb = _l.load()
    _req(heads_all, torch.uint8, "heads_all"); _req(rows_all, torch.float32, "rows_all")
    device_status(rows_all.device)
    sp = out if out is not None else SparseRows(world * cap_x, D, rows_all.device)
    ws_bytes = int(Lb.pxr_merge_rows_ws_bytes(world, cap_x))
    ws = _ws.get(ws_bytes, rows_all.device)
    _l.check(Lb.pxr_merge_split_rows_f32(_l.ptr(heads_all), _l.ptr(rows_all), world, cap, cap_x, D, n_table, float(scale),
                                         _l.ptr(sp.idx), _l.ptr(sp.rows), _l.ptr(sp.n), _l.ptr(ws), ws_bytes,
                                         _l.stream_ptr()), "pxr_merge_split_rows_f32")
    return sp


def sample_negatives(pos: torch.Tensor, n_items: int, seed: int, batch_counter: int):
    """pos int64 [B, L+1] left-padded positive windows -> (items [B,2,L+1], masked_index [B,L]) with one negative per
    target position drawn on the device (trainset.py:40-63 semantics; stream selected by (seed, batch_counter))."""
    Lb = _l.load()
    _req(pos, torch.int64, "pos")
    B, W = pos.shape
    items = torch.empty(B, 2, W, dtype=torch.int64, device=pos.device)
    mask = torch.empty(B, W - 1, dtype=torch.int64, device=pos.device)
    _l.check(Lb.pxr_sample_negatives_i64(_l.ptr(pos), B, W, n_items, seed & 0xFFFFFFFFFFFFFFFF,
                                         batch_counter & 0xFFFFFFFFFFFFFFFF, _l.ptr(items), _l.ptr(mask),
                                         _l.stream_ptr()), "pxr_sample_negatives_i64")
    return items, mask


def shard_local_rows(ids: torch.Tensor, world: int, rank: int, n_table: int) -> torch.Tensor:
    """Row-sharded table: local row (id // world + 1) of the ids this rank owns (id % world == rank), 0 elsewhere."""
    Lb = _l.load()
    _req(ids, torch.int64, "ids")
    out = torch.empty_like(ids)
    _l.check(Lb.pxr_shard_local_rows_i64(_l.ptr(ids), ids.numel(), world, rank, n_table, _l.ptr(out), _l.stream_ptr()),
             "pxr_shard_local_rows_i64")
    return out


def shard_bucket_ids(ids: torch.Tensor, n_dev: torch.Tensor, world: int, n_table: int, pp_cap: int, pad_id: int):
    """Ascending unique ids (count on the device) -> per-owner request lists: (req int64 [world, pp_cap], pos int32
    [world, pp_cap], counts int32 [world]) -- pxr_shard_bucket_ids_i64."""
    _req(ids, torch.int64, "ids"); _req(n_dev, torch.int32, "n_dev")
    device_status(ids.device)
    req = torch.empty(world, pp_cap, dtype=torch.int64, device=ids.device)
    pos = torch.empty(world, pp_cap, dtype=torch.int32, device=ids.device)
    counts = torch.empty(world, dtype=torch.int32, device=ids.device)
    _l.check(_l.load().pxr_shard_bucket_ids_i64(_l.ptr(ids), _l.ptr(n_dev), world, n_table, pp_cap, pad_id, _l.ptr(req),
                                                _l.ptr(pos), _l.ptr(counts), _l.stream_ptr()), "pxr_shard_bucket_ids_i64")
    return req, pos, counts


def scatter_rows(src: torch.Tensor, pos: torch.Tensor, dst: torch.Tensor, row_offset: int = 0):
    """dst[row_offset + pos[i], :] = src[i, :] where pos[i] >= 0 (pxr_scatter_rows_f32)."""
    _req(src, torch.float32, "src"); _req(pos, torch.int32, "pos"); _req(dst, torch.float32, "dst")
    D = src.shape[-1]
    assert dst.shape[-1] == D and pos.numel() == src.numel() // D
    _l.check(_l.load().pxr_scatter_rows_f32(_l.ptr(src), _l.ptr(pos), pos.numel(), D, _l.ptr(dst), dst.numel() // D, row_offset,
                                            _l.stream_ptr()), "pxr_scatter_rows_f32")
    return dst


def shard_first_rows(ids_all: torch.Tensor, world: int, rank: int, n_table: int) -> torch.Tensor:
    """shard_local_rows over `world` ascending request lists, keeping each owned id only where it is requested FIRST
    (lowest rank): a duplicate-free work list."""
    Lb = _l.load()
    _req(ids_all, torch.int64, "ids_all")
    out = torch.empty_like(ids_all)
    _l.check(Lb.pxr_shard_first_rows_i64(_l.ptr(ids_all), world, ids_all.numel() // world, rank, n_table, _l.ptr(out),
                                         _l.stream_ptr()), "pxr_shard_first_rows_i64")
    return out


def ids_to_compact(ids: torch.Tensor, uniq_idx: torch.Tensor, n_uniq: torch.Tensor) -> torch.Tensor:
    """1 + position of every id in the ascending unique list (0 for padding): indices into a fetched row block."""
    Lb = _l.load()
    _req(ids, torch.int64, "ids"); _req(uniq_idx, torch.int64, "uniq_idx"); _req(n_uniq, torch.int32, "n_uniq")
    out = torch.empty_like(ids)
    _l.check(Lb.pxr_ids_to_compact_i64(_l.ptr(ids), ids.numel(), _l.ptr(uniq_idx), _l.ptr(n_uniq), _l.ptr(out),
                                       _l.stream_ptr()), "pxr_ids_to_compact_i64")
    return out


def occ_ws_bytes(B: int, L: int) -> int:
    return int(_l.load().pxr_embed_grad_ws_bytes(3 * B * L))


def occ_sort(items, L: int, layout, n_table, sp: SparseRows, ws: torch.Tensor):
    """Phase 1 of the table gradient (ids only): fills sp.idx / sp.n, leaves the sorted occurrences in `ws` (occ_ws_bytes(B, L),
    caller-owned, persistent).  layout = (id_bstride, in_off, pos_off, neg_off) of the L positions of each sequence (None: SASRec's
    [B, 2, L+1] windows, _sasrec_layout; BERT4Rec's [B, 3, L]: (3L, 0, L, 2L)).  Phase 2 is sasrec_occ_segsum whatever the layout."""
    Lb = _l.load()
    _req(items, torch.int64, "items")
    B = items.shape[0]
    device_status(items.device)       # an id outside the table flags the status word (raise_on_bad_indices)
    _l.check(Lb.pxr_seq_occ_sort(_l.ptr(items), B, L, *(_sasrec_layout(L) if layout is None else layout), n_table, _l.ptr(sp.idx),
                                 _l.ptr(sp.n), _l.ptr(ws), ws.numel(), _l.stream_ptr()), "pxr_seq_occ_sort")


def seq_occ_dense_grad(items, layout, dx0, out, coef, n_rows: int, d_rows=None, ws: torch.Tensor | None = None):
    """occ_sort + sasrec_occ_segsum(scale=1) as a dense block over a batch-local row space (pxr_seq_occ_dense_f32): items int64
    [B, ...] holds rows of an [n_rows, D] matrix under layout = (id_bstride, in_off, pos_off, neg_off) (None: SASRec's windows),
    dx0 / out [B, L, D], coef [B, L] -> d_rows float32 [n_rows, D]: the sparse route's row sums, bit for bit, at their rows and
    exactly +0.0 everywhere else (row 0, unreferenced rows), whatever `d_rows` held before.  Key 0 is dropped; an id outside
    [0, n_rows) is dropped and flags the status word (raise_on_bad_indices).  ws: occ_ws_bytes(B, L) bytes (default: the shared
    workspace)."""
    Lb = _l.load()
    _req(items, torch.int64, "items"); _req(dx0, torch.float32, "dx0"); _req(out, torch.float32, "out"); _req(coef, torch.float32, "coef")
    if out.dim() != 3 or items.shape[0] != out.shape[0] or dx0.shape != out.shape or coef.numel() != out.shape[0] * out.shape[1] or \
            out.numel() < 1 or n_rows < 1:
        raise _l.PxrError(f"seq occ dense grad: need items [B, ...], dx0 / out [B, L, D], coef [B, L] and n_rows >= 1, got items "
                          f"{tuple(items.shape)}, dx0 {tuple(dx0.shape)}, out {tuple(out.shape)}, coef {tuple(coef.shape)}, n_rows={n_rows}")
    B, L, D = out.shape
    lay = _sasrec_layout(L) if layout is None else tuple(int(x) for x in layout)
    if items.numel() < B * lay[0]:
        raise _l.PxrError(f"seq occ dense grad: items {tuple(items.shape)} holds fewer than id_bstride={lay[0]} ids per sequence")
    d_rows = _out_f32(d_rows, (int(n_rows), D), out.device, "seq occ dense grad", "d_rows")
    if ws is None:
        ws = _ws.get(occ_ws_bytes(B, L), out.device)
    device_status(items.device)       # an id outside the row space flags the status word (raise_on_bad_indices)
    _l.check(Lb.pxr_seq_occ_dense_f32(_l.ptr(items), B, L, *lay, _l.ptr(dx0), _l.ptr(out), _l.ptr(coef), D, int(n_rows),
                                      _l.ptr(d_rows), _l.ptr(ws), ws.numel(), _l.stream_ptr()), "pxr_seq_occ_dense_f32")
    return d_rows


def occ_split_ws_bytes(B: int, L: int, D: int) -> int:
    """Bytes of the second workspace of sasrec_occ_segsum's split route (0: shape not served).  Allocate it with torch.zeros."""
    return int(_l.load().pxr_sasrec_occ_split_ws_bytes(B, L, D))


def sasrec_occ_segsum(ws: torch.Tensor, dx0, out, coef, n_table, sp: SparseRows, scale=1.0, ws2: torch.Tensor | None = None,
                      rider: TailRider | None = None):
    """Phase 2: sp.rows from the sorted occurrences in `ws`.  ws2 (occ_split_ws_bytes zero-initialised bytes, persistent): very long
    segments are summed by many workgroups (big batches: a popular item's thousands of occurrences).  rider: reductions the ONE
    launch of the plain route carries on extra workgroups (not with ws2)."""
    Lb = _l.load()
    B, L, D = out.shape
    rarg, rkeep = rider.c_arg() if rider is not None else (None, None)
    if ws2 is not None:
        if rarg is not None:
            raise _l.PxrError("sasrec_occ_segsum: the split route (ws2) is three launches and carries no rider")
        _l.check(Lb.pxr_sasrec_occ_segsum_split(_l.ptr(ws), ws.numel(), B, L, _l.ptr(dx0), _l.ptr(out), _l.ptr(coef), D, n_table,
                                                float(scale), _l.ptr(sp.n), _l.ptr(sp.rows), _l.ptr(ws2), ws2.numel(), _l.stream_ptr()),
                 "pxr_sasrec_occ_segsum_split")
        return
    _l.check(Lb.pxr_sasrec_occ_segsum(_l.ptr(ws), ws.numel(), B, L, _l.ptr(dx0), _l.ptr(out), _l.ptr(coef), D,
                                      n_table, float(scale), _l.ptr(sp.n), _l.ptr(sp.rows), _l.stream_ptr(), rarg),
             "pxr_sasrec_occ_segsum")
    del rkeep


def sasrec_occ_segsum_apply(ws: torch.Tensor, dx0, out, coef, n_table, sp: SparseRows, table, m, v, last, hyper, t_prev, beta1, beta2,
                            eps, step_dev=None, rider: TailRider | None = None):
    """Phase 2 and the lazy row update in ONE launch (pxr_sasrec_occ_segsum_apply): the sums sasrec_occ_segsum(scale=1) would leave
    in sp.rows are applied where they are formed -- adamw_rows(t_prev, t_prev + 1, rows=sp.idx, grows=sp.rows) on rows that are
    current through t_prev, bit for bit -- and sp.rows is NOT written.  A row that is not current is left untouched and raises
    STATUS_ROWS_STALE.  Segments of any length on one workgroup each (no split route).  rider: reductions the launch carries on
    extra workgroups."""
    Lb = _l.load()
    B, L, D = out.shape
    rarg, rkeep = rider.c_arg() if rider is not None else (None, None)
    device_status(table.device)       # a stale row flags the status word (raise_on_bad_indices)
    with _gemm_timer(0.0, "segsum_apply_kernel (segment sums + apply: batch rows)"):
        _l.check(Lb.pxr_sasrec_occ_segsum_apply(_l.ptr(ws), ws.numel(), B, L, _l.ptr(dx0), _l.ptr(out), _l.ptr(coef), D, n_table,
                                                _l.ptr(sp.n), _l.ptr(sp.idx), _l.ptr(table), _l.ptr(m), _l.ptr(v), _l.ptr(last),
                                                table.shape[0], _l.ptr(hyper), t_prev, _l.ptr(step_dev), beta1, beta2, eps,
                                                _l.stream_ptr(), rarg),
                 "pxr_sasrec_occ_segsum_apply")
    del rkeep


# ------------------------------------------------------------------------------------------------ PixelNet pieces
def mosasrec_emb_grad(dx0, out, coef):
    """-> d_emb [B, L+1, 2, D] (see pxr.h)."""
    Lb = _l.load()
    _req(dx0, torch.float32, "dx0"); _req(out, torch.float32, "out"); _req(coef, torch.float32, "coef")
    if out.dim() != 3:
        raise _l.PxrError("mosasrec_emb_grad: out must be [B, L, D]")
    B, L, D = out.shape
    if D % 4 != 0:
        raise _l.PxrError(f"mosasrec_emb_grad: D must be a multiple of 4 (D={D})")
    if dx0.numel() != B * L * D or coef.numel() != B * L:
        raise _l.PxrError(f"mosasrec_emb_grad: dx0 must hold B*L*D = {B * L * D} and coef B*L = {B * L} elements, got "
                          f"{dx0.numel()} and {coef.numel()}")
    d = torch.empty(B, L + 1, 2, D, dtype=torch.float32, device=out.device)
    _l.check(Lb.pxr_mosasrec_emb_grad_f32(_l.ptr(dx0), _l.ptr(out), _l.ptr(coef), B, L, D, _l.ptr(d), _l.stream_ptr()),
             "pxr_mosasrec_emb_grad_f32")
    return d


def image_u8_to_f32(store: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """store uint8 [n_store, H, W, 3] on device, ids int64 [...] -> fp32 [..., 3, H, W] normalised like the reference."""
    Lb = _l.load()
    _req(store, torch.uint8, "store"); _req(ids, torch.int64, "ids")
    n_store, H, W, C = store.shape
    if C != 3:
        raise _l.PxrError("image store must be HWC with 3 channels")
    device_status(store.device)       # an id outside the store is flagged on the device (zero image), raised at the next check
    out = torch.empty(*ids.shape, 3, H, W, dtype=torch.float32, device=store.device)
    _l.check(Lb.pxr_image_u8_to_f32(_l.ptr(store), n_store, H, W, _l.ptr(ids), ids.numel(), _l.ptr(out),
                                    _l.stream_ptr()), "pxr_image_u8_to_f32")
    return out


# ------------------------------------------------------------------------------------------------ full-sort eval
def history_csr(history_u: torch.Tensor, history_i: torch.Tensor, B: int, device):
    """(history_u, history_i) of seq_eval_collate (grouped by user, collate_fn.py:27-28) -> (hist_ptr int32 [B+1],
    hist_items int64) on `device`.  Host-side index plumbing (a bincount), not arithmetic."""
    counts = torch.bincount(history_u.cpu(), minlength=B)
    ptr = torch.zeros(B + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
    return ptr.to(device), history_i.to(device=device, dtype=torch.int64).contiguous()


def score_planes_supported(table: torch.Tensor) -> bool:
    """Whether the fused scoring can run its main pass on planes of this table (GEMM mode bf16x3, D % 32 == 0, three planes
    below 2 GiB)."""
    N, D = table.shape
    return gemm_mode() == "bf16x3" and D % 32 == 0 and ((N + 31) // 32 * 32) * D * 6 < 0x7FFFFFF0


def row_norm_max(x: torch.Tensor) -> torch.Tensor:
    """max_i ||x[i]||_2 as a 1-element device tensor (pxr_row_norm_max_f32): the table statistic of the reduced-product top-k."""
    _req(x, torch.float32, "x", contiguous=False)
    assert x.dim() == 2 and x.stride(1) == 1
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    _l.check(_l.load().pxr_row_norm_max_f32(_l.ptr(x), x.shape[0], x.shape[1], x.stride(0), _l.ptr(out), _l.stream_ptr()),
             "pxr_row_norm_max_f32")
    return out


def topk_products() -> int:
    """bf16 products of the top-k threshold pass: PXR_TOPK_PRODUCTS = 6 | 3 | 1 (default 3; results are identical, see pxr.h)."""
    v = int(os.environ.get("PXR_TOPK_PRODUCTS", "3"))
    return v if v in (1, 3, 6) else 3


def _topk_hist_csr(who: str, hist_ptr, hist_items, B: int):
    """The history CSR of a fused top-k call, where one is given: hist_ptr int32 [B + 1], hist_items int64."""
    if hist_ptr is not None:
        _req(hist_ptr, torch.int32, "hist_ptr"); _req(hist_items, torch.int64, "hist_items")
        if hist_ptr.numel() != B + 1:
            raise _l.PxrError(f"{who}: hist_ptr must have B + 1 = {B + 1} entries")


def _topk_out(B: int, K: int, device):
    """The outputs of a fused top-k call (topk_idx int64 [B, K], topk_val fp32 [B, K]); the device's status word, which the
    kernels flag bad ids in, is registered first."""
    device_status(device)
    return torch.empty(B, K, dtype=torch.int64, device=device), torch.empty(B, K, dtype=torch.float32, device=device)


def score_topk(users: torch.Tensor, ld_users: int, B: int, table: torch.Tensor, K: int, hist_ptr=None,
               hist_items=None, table_planes: Planes | None = None, table_norm_max: torch.Tensor | None = None):
    """Fused full-catalog scoring + masking + top-K (see pxr.h).  `users` may be a strided view (row stride
    ld_users floats).  Returns (topk_idx int64 [B,K], topk_val fp32 [B,K]).  table_planes: split_planes(table), made once
    per evaluation -- the main pass over the catalogue then runs on pre-split operands; table_norm_max: row_norm_max(table), made
    with them -- that pass then runs on topk_products() of the six bf16 products and the survivors are re-scored exactly: same
    ids, same bits (pxr_score_topk_f32)."""
    Lb = _l.load()
    _req(users, torch.float32, "users", contiguous=False); _req(table, torch.float32, "table")
    N, D = table.shape
    idx, val = _topk_out(B, K, table.device)
    ws_bytes = int(Lb.pxr_score_topk_ws_bytes(B, N, K))
    if ws_bytes < 0:
        raise _l.PxrError("score_topk: K must be in [1, 32]")
    ws = _ws.get(ws_bytes, table.device)
    up = None
    if table_planes is not None:
        u2 = torch.as_strided(users, (B, D), (ld_users, 1))
        up = split_planes(u2)
    products = topk_products() if (table_planes is not None and table_norm_max is not None) else 6
    _l.check(Lb.pxr_score_topk_f32(_l.ptr(users), ld_users, B, _l.ptr(table), N, D, *_pl(up), *_pl(table_planes),
                                   _l.ptr(table_norm_max) if products != 6 else None, products,
                                   _l.ptr(hist_ptr), _l.ptr(hist_items), K, _l.ptr(idx), _l.ptr(val), _l.ptr(ws),
                                   ws_bytes, _l.stream_ptr()), "pxr_score_topk_f32")
    return idx, val


# ------------------------------------------------------------------------------------------------ optimizer
def adamw_flat(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step):
    Lb = _l.load()
    for t, nm in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _req(t, torch.float32, nm)
    _l.check(Lb.pxr_adamw_flat_f32(_l.ptr(p), _l.ptr(g), _l.ptr(m), _l.ptr(v), p.numel(), lr, beta1, beta2, eps,
                                   weight_decay, step, _l.stream_ptr()), "pxr_adamw_flat_f32")


def slot_fill(slot, value=-1):
    Lb = _l.load()
    _req(slot, torch.int32, "slot")
    _l.check(Lb.pxr_slot_fill_i32(_l.ptr(slot), slot.numel(), value, _l.stream_ptr()), "pxr_slot_fill_i32")


def adamw_table(table, m, v, slot, sp: SparseRows | None, lr, beta1, beta2, eps, weight_decay, step):
    Lb = _l.load()
    _req(table, torch.float32, "table"); _req(m, torch.float32, "m"); _req(v, torch.float32, "v")
    _req(slot, torch.int32, "slot")
    N, D = table.shape
    with _gemm_timer(24.0 * N * D + 4.0 * N, "adamw_table_kernel (dense sweep)"):
        _l.check(Lb.pxr_adamw_table_f32(_l.ptr(table), _l.ptr(m), _l.ptr(v), N, D, _l.ptr(slot),
                                        _l.ptr(sp.idx) if sp else None, _l.ptr(sp.rows) if sp else None,
                                        _l.ptr(sp.n) if sp else None, sp.cap if sp else 0, lr, beta1, beta2, eps,
                                        weight_decay, step, _l.stream_ptr()), "pxr_adamw_table_f32")


def adamw_hyper_append(hyper, cumlog, step, lr, beta1, beta2, eps, weight_decay, step_dev=None, advance=False):
    """Append the per-step scalars of `step` (or of *step_dev + 1).  advance=True: end-of-step form -- count the finished
    step on the device first, then append the next step's entry (one launch)."""
    Lb = _l.load()
    _l.check(Lb.pxr_adamw_hyper_append(_l.ptr(hyper), _l.ptr(cumlog), cumlog.numel(), step, _l.ptr(step_dev), lr, beta1,
                                       beta2, eps, weight_decay, int(bool(advance)), _l.stream_ptr()),
             "pxr_adamw_hyper_append")


def adamw_rows(table, m, v, last, hyper, cumlog, t_prev, t_apply, beta1, beta2, eps, rows=None, n_rows=None,
               max_rows=0, grows=None, step_dev=None, step_dev_bias=0, max_blocks=0):
    """Lazy table AdamW: catch rows up through t_prev (+ apply step t_apply with gradient rows).  rows=None: all.
    step_dev (device int64 counter of completed steps) overrides t_prev / t_apply (hipGraph-replayable)."""
    Lb = _l.load()
    N, D = table.shape
    tag = ("adamw_rows_kernel (flush: every row)" if rows is None else
           "adamw_rows_kernel (apply: batch rows + gradient)" if t_apply else
           "adamw_rows_kernel (next batch's rows, beside the GEMMs)" if (step_dev_bias or max_blocks) else
           "adamw_rows_kernel (catch-up: batch rows)")
    with _gemm_timer(0.0, tag):
        _l.check(Lb.pxr_adamw_rows_f32(_l.ptr(table), _l.ptr(m), _l.ptr(v), _l.ptr(last), N, D, _l.ptr(rows),
                                       _l.ptr(n_rows), max_rows, _l.ptr(grows), _l.ptr(hyper), _l.ptr(cumlog), t_prev,
                                       t_apply, _l.ptr(step_dev), int(step_dev_bias), int(max_blocks), beta1, beta2, eps,
                                       _l.stream_ptr()),
                 "pxr_adamw_rows_f32")


def adamw_rows_ids(table, m, v, last, hyper, cumlog, t_prev, beta1, beta2, eps, ids, step_dev=None):
    """Catch-up of the rows named by a raw int64 id tensor (duplicates / 0 / out-of-range allowed): pxr_adamw_rows_ids_f32."""
    _req(ids, torch.int64, "ids")
    N, D = table.shape
    with _gemm_timer(0.0, "adamw_rows_kernel (catch-up: batch rows, claimed from the raw id list)"):
        _l.check(_l.load().pxr_adamw_rows_ids_f32(_l.ptr(table), _l.ptr(m), _l.ptr(v), _l.ptr(last), N, D, _l.ptr(ids),
                                                  ids.numel(), _l.ptr(hyper), _l.ptr(cumlog), t_prev, _l.ptr(step_dev), beta1,
                                                  beta2, eps, _l.stream_ptr()), "pxr_adamw_rows_ids_f32")


def adamw_rows_ids2d(table, m, v, last, hyper, cumlog, t_prev, beta1, beta2, eps, ids, n_lists, row_len, row_stride, step_dev=None,
                     cur_hyper_out=None):
    """adamw_rows_ids over a 2-D window of an int64 id tensor (n_lists rows of row_len ids, row stride row_stride elements):
    pxr_adamw_rows_ids2d_f32.  cur_hyper_out (float32 [4]): also receives the scalars of the step about to run."""
    _req(ids, torch.int64, "ids")
    N, D = table.shape
    assert (n_lists - 1) * row_stride + row_len <= ids.numel()
    with _gemm_timer(0.0, "adamw_rows_kernel (catch-up: input rows, claimed from the raw id window)"):
        _l.check(_l.load().pxr_adamw_rows_ids2d_f32(_l.ptr(table), _l.ptr(m), _l.ptr(v), _l.ptr(last), N, D, _l.ptr(ids), n_lists,
                                                    row_len, row_stride, _l.ptr(hyper), _l.ptr(cumlog), t_prev, _l.ptr(step_dev),
                                                    beta1, beta2, eps, _l.ptr(cur_hyper_out), _l.stream_ptr()),
                 "pxr_adamw_rows_ids2d_f32")


def adamw_flat_tab(p, g, m, v, hyper, step, beta1, beta2, eps, step_dev=None, plane_segments=None, close=None, planes_exps=None):
    """Flat AdamW with the step's scalars from the hyper table.  plane_segments: list of (flat element offset, rows, cols,
    Planes): weight matrices whose updated values are also written as planes by the same launch -- three bf16 planes, or (Planes of
    fmt 1 + planes_exps, an int32 device tensor with one exponent per segment) two fp16 planes scaled by 2^exponent.
    close = (cumlog, cur_hyper, lr, weight_decay): the launch reads this step's scalars from cur_hyper and closes the step itself
    (no adamw_hyper_append(advance=True) launch afterwards)."""
    Lb = _l.load()
    segs = plane_segments or []
    # the fused plane output serves MULTI_MAX matrices; the rest (models with more than 4 layers) are split from the updated flat
    # buffer by a launch of their own right behind the optimizer's
    h2 = bool(segs) and segs[0][3].fmt == 1
    assert not h2 or (planes_exps is not None and planes_exps.dtype == torch.int32 and planes_exps.numel() >= len(segs) and len(segs) <= MULTI_MAX)
    late = segs[MULTI_MAX:]
    segs = segs[:MULTI_MAX]
    n = len(segs)
    if n:
        P, I64 = ctypes.c_void_p * n, ctypes.c_int64 * n
        sa = (n, I64(*[s_[0] for s_ in segs]), I64(*[s_[1] for s_ in segs]), I64(*[s_[2] for s_ in segs]),
              P(*[s_[3].ptr().value for s_ in segs]), I64(*[s_[3].ps for s_ in segs]), I64(*[s_[3].pr for s_ in segs]))
    else:
        sa = (0, None, None, None, None, None, None)
    if close is not None or h2:
        cumlog, cur, lr, wd = close if close is not None else (None, None, 0.0, 0.0)
        with _gemm_timer(0.0, "adamw_flat_tab_kernel" + (" (+ closes the step)" if close is not None else "") + (" (h2 planes out)" if h2 else "")):
            _l.check(Lb.pxr_adamw_flat_tab_ex_f32(_l.ptr(p), _l.ptr(g), _l.ptr(m), _l.ptr(v), p.numel(), _l.ptr(hyper), _l.ptr(cumlog),
                                                  cumlog.numel() if cumlog is not None else 0, step, _l.ptr(step_dev), _l.ptr(cur), lr,
                                                  beta1, beta2, eps, wd, *sa, 1 if h2 else 0, _l.ptr(planes_exps) if h2 else None,
                                                  _l.stream_ptr()), "pxr_adamw_flat_tab_ex_f32")
    else:
        _l.check(Lb.pxr_adamw_flat_tab_f32(_l.ptr(p), _l.ptr(g), _l.ptr(m), _l.ptr(v), p.numel(), _l.ptr(hyper), step,
                                           _l.ptr(step_dev), beta1, beta2, eps, *sa, _l.stream_ptr()),
                 "pxr_adamw_flat_tab_f32")
    if late:
        split_planes_multi([p[o:o + r * c].view(r, c) for o, r, c, _ in late], [pl for _, _, _, pl in late])


class ScoreClock:
    """The shader clock the fused scoring's main-pass kernels sustain, measured inside them (pxr_score_topk_clock_out): a context
    manager; `.ghz()` after the block has synchronised.  Measurement only (bench.py, tools/eval_bench.py)."""

    def __init__(self, device="cuda"):
        self.buf = torch.zeros(2, dtype=torch.int64, device=device)

    def __enter__(self):
        self.buf.zero_()
        torch.cuda.synchronize()
        _l.check(_l.load().pxr_score_topk_clock_out(_l.ptr(self.buf)), "pxr_score_topk_clock_out")
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        _l.check(_l.load().pxr_score_topk_clock_out(None), "pxr_score_topk_clock_out")

    def ghz(self) -> float:
        c, r = (int(x) for x in self.buf.tolist())
        return c / r * 0.1 if r > 0 else float("nan")


def counter_add(counter, delta=1):
    Lb = _l.load()
    _req(counter, torch.int64, "counter")
    _l.check(Lb.pxr_counter_add_i64(_l.ptr(counter), delta, _l.stream_ptr()), "pxr_counter_add_i64")


# ------------------------------------------------------------------------------------------------ LightGCN (csrc/lightgcn.hip)
class LgcnGraph:
    """The normalised user-item graph on the device as CSR (row_ptr int64 [n+1], col int32, w fp32), plus the split plan of its
    long rows: rows of more than `part_len` edges are cut into parts of part_len edges that pxr_lgcn_spmm_f32 sums in part order.
    The plan is host arithmetic on row_ptr, made once per graph."""

    PART_LEN = 512

    def __init__(self, row_ptr, col, w, device, part_len: int | None = None):
        import numpy as np

        row_ptr = np.asarray(row_ptr, dtype=np.int64)
        col = np.asarray(col, dtype=np.int32)
        w = np.asarray(w, dtype=np.float32)
        n = len(row_ptr) - 1
        if n <= 0 or row_ptr[0] != 0 or row_ptr[-1] != len(col) or len(w) != len(col) or (np.diff(row_ptr) < 0).any():
            raise ValueError("LgcnGraph: not a CSR (row_ptr must start at 0, be non-decreasing and end at nnz = len(col) = len(w))")
        self.n_rows, self.nnz = n, len(col)
        self.part_len = int(part_len or self.PART_LEN)
        deg = np.diff(row_ptr)
        split = np.nonzero(deg > self.part_len)[0]
        n_parts = -(-deg[split] // self.part_len)
        part0 = np.zeros(len(split) + 1, dtype=np.int64)
        np.cumsum(n_parts, out=part0[1:])
        if part0[-1] >= (1 << 31):
            raise ValueError("LgcnGraph: too many parts")
        self.n_split, self.n_parts = len(split), int(part0[-1])
        dev = torch.device(device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.row_ptr, self.col, self.w = t(row_ptr), t(col), t(w)
        self.split_row = t(split.astype(np.int32))
        self.split_part0 = t(part0.astype(np.int32))
        self.part_owner = t(np.repeat(np.arange(len(split), dtype=np.int32), n_parts))
        self.device = dev

    def spmm(self, x, y=None, acc_in=None, acc_out=None, scale=1.0):
        """s = A x; y = s (if given); acc_out = (acc_in + s) * scale (if given; acc_in None = 0, may be acc_out).  One launch (two
        when the graph has split rows)."""
        Lb = _l.load()
        _req(x, torch.float32, "x")
        for t, nm in ((y, "y"), (acc_in, "acc_in"), (acc_out, "acc_out")):
            if t is not None:
                _req(t, torch.float32, nm)
                if t.shape != x.shape:
                    raise _l.PxrError(f"lgcn spmm: {nm} has shape {tuple(t.shape)}, x {tuple(x.shape)}")
        N, D = x.shape
        if N != self.n_rows:
            raise _l.PxrError(f"lgcn spmm: x has {N} rows, the graph {self.n_rows}")
        device_status(x.device)
        ws_bytes = int(Lb.pxr_lgcn_spmm_ws_bytes(self.n_parts, D))
        if ws_bytes < 0:
            raise _l.PxrError(f"lgcn spmm: D={D} must be a positive multiple of 4")
        ws = _ws.get(ws_bytes, x.device) if self.n_parts else None
        _l.check(Lb.pxr_lgcn_spmm_f32(_l.ptr(self.row_ptr), _l.ptr(self.col), _l.ptr(self.w), N, D, _l.ptr(self.split_row),
                                      _l.ptr(self.split_part0), self.n_split, _l.ptr(self.part_owner), self.n_parts, self.part_len,
                                      _l.ptr(x), _l.ptr(y), _l.ptr(acc_in), _l.ptr(acc_out), float(scale), _l.ptr(ws), ws_bytes,
                                      _l.stream_ptr()), "pxr_lgcn_spmm_f32")
        return y if acc_out is None else acc_out


def lgcn_pair_fwd(emb, n_users: int, n_items: int, user, item):
    """LightGCN's pair loss head (lightgcn.py:70-78) on E_final [n_users + n_items, D]: user int64 [B], item int64 [B, 2] ->
    (loss [1], diff [B] = x_b, coef [B] = d loss / d x_b, nodes int32 [3B])."""
    Lb = _l.load()
    _req(emb, torch.float32, "emb"); _req(user, torch.int64, "user"); _req(item, torch.int64, "item")
    B = user.numel()
    if item.numel() != 2 * B:
        raise _l.PxrError(f"lgcn pair head: item must be [B, 2] for B={B}, got {tuple(item.shape)}")
    N, D = emb.shape
    if N != n_users + n_items:
        raise _l.PxrError(f"lgcn pair head: emb has {N} rows, n_users + n_items = {n_users + n_items}")
    dev = emb.device
    f = torch.empty(3 * B + 1, dtype=torch.float32, device=dev)
    diff, coef, lossrow, loss = f[:B], f[B:2 * B], f[2 * B:3 * B], f[3 * B:]
    nodes = torch.empty(3 * B, dtype=torch.int32, device=dev)
    device_status(dev)
    _l.check(Lb.pxr_lgcn_pair_fwd_f32(_l.ptr(emb), n_users, n_items, D, _l.ptr(user), _l.ptr(item), B, _l.ptr(diff), _l.ptr(coef),
                                      _l.ptr(lossrow), _l.ptr(nodes), _l.ptr(loss), _l.stream_ptr()), "pxr_lgcn_pair_fwd_f32")
    return loss, diff, coef, nodes


def lgcn_pair_bwd(emb, nodes, coef, grad, grad_scale=1.0, grad_scale_dev=None):
    """grad [n, D] (overwritten) = d loss / d E_final of lgcn_pair_fwd, scaled by grad_scale * (*grad_scale_dev)."""
    Lb = _l.load()
    _req(emb, torch.float32, "emb"); _req(grad, torch.float32, "grad"); _req(nodes, torch.int32, "nodes")
    _req(coef, torch.float32, "coef")
    if grad.shape != emb.shape:
        raise _l.PxrError("lgcn pair head backward: grad must have emb's shape")
    N, D = emb.shape
    _l.check(Lb.pxr_lgcn_pair_bwd_f32(_l.ptr(emb), N, D, _l.ptr(nodes), _l.ptr(coef), coef.numel(), float(grad_scale),
                                      _l.ptr(grad_scale_dev), _l.ptr(grad), _l.stream_ptr()), "pxr_lgcn_pair_bwd_f32")
    return grad


# ------------------------------------------------------------------------------------------------ SRGNN (csrc/srgnn.hip)
SRGNN_MAX_L = 64


def srgnn_graph(seq, n_items: int, target=None, want_occ: bool = False, want_mask: bool = False, out=None):
    """Session graphs of seq int64 [B, L] (right-padded) at a fixed L nodes -> dict(nodes int64 [B, L], alias int32 [B, L],
    A fp32 [B, L, 2L], occ int64 [B, 3L] | None, mask int64 [B, L] | None).  `out`: a dict of persistent buffers to fill."""
    Lb = _l.load()
    _req(seq, torch.int64, "seq")
    B, L = seq.shape
    if L < 1 or L > SRGNN_MAX_L:
        raise _l.PxrError(f"srgnn graph: L={L} outside 1..{SRGNN_MAX_L} (the node bitmasks of one wave)")
    if want_occ:
        _req(target, torch.int64, "target")
        if target.numel() != 2 * B:
            raise _l.PxrError(f"srgnn graph: target must be [B, 2] for B={B}, got {tuple(target.shape)}")
    dev = seq.device
    o = out if out is not None else {}
    if o.get("nodes") is None or o["nodes"].shape != (B, L) or o["nodes"].device != dev:
        o.update(nodes=torch.empty(B, L, dtype=torch.int64, device=dev), alias=torch.empty(B, L, dtype=torch.int32, device=dev),
                 A=torch.empty(B, L, 2 * L, dtype=torch.float32, device=dev), occ=None, mask=None)
    if want_occ and o.get("occ") is None:
        o["occ"] = torch.empty(B, 3 * L, dtype=torch.int64, device=dev)
    if want_mask and o.get("mask") is None:
        o["mask"] = torch.empty(B, L, dtype=torch.int64, device=dev)
    device_status(dev)                # an id outside the table flags the status word (raise_on_bad_indices)
    _l.check(Lb.pxr_srgnn_graph_i64(_l.ptr(seq), B, L, n_items, _l.ptr(target) if want_occ else None, _l.ptr(o["nodes"]),
                                    _l.ptr(o["alias"]), _l.ptr(o["A"]), _l.ptr(o["occ"]) if want_occ else None,
                                    _l.ptr(o["mask"]) if want_mask else None, _l.stream_ptr()), "pxr_srgnn_graph_i64")
    return o


def srgnn_prop(A, x, y=None, bias=None, transpose: bool = False):
    """[A_in x_in | A_out x_out] (+ bias) per session, or its transpose (the backward): x, y [B*L, 2D]."""
    Lb = _l.load()
    _req(A, torch.float32, "A"); _req(x, torch.float32, "x")
    B, L, _ = A.shape
    D = x.shape[-1] // 2
    if x.numel() != B * L * 2 * D:
        raise _l.PxrError(f"srgnn prop: x has {x.numel()} elements, expected B*L*2D = {B * L * 2 * D}")
    y = y if y is not None else torch.empty_like(x)
    _l.check(Lb.pxr_srgnn_prop_f32(_l.ptr(A), B, L, D, _l.ptr(x), _l.ptr(y), _l.ptr(bias), int(transpose), _l.stream_ptr()),
             "pxr_srgnn_prop_f32")
    return y


def srgnn_readout_fwd(Hn, P, alias, mask, w3, cat=None, sig=None, alpha=None):
    """Attention readout: Hn [B*L, D], P [B*L, 2D] -> cat [B, 2D] = [a | ht] (sig [B, L, D] / alpha [B, L] saved when given)."""
    Lb = _l.load()
    _req(Hn, torch.float32, "Hn"); _req(P, torch.float32, "P"); _req(alias, torch.int32, "alias"); _req(mask, torch.int64, "mask")
    _req(w3, torch.float32, "w3")
    B, L = alias.shape
    D = Hn.shape[-1]
    cat = cat if cat is not None else torch.empty(B, 2 * D, dtype=torch.float32, device=Hn.device)
    _l.check(Lb.pxr_srgnn_readout_fwd_f32(_l.ptr(Hn), _l.ptr(P), _l.ptr(alias), _l.ptr(mask), _l.ptr(w3), B, L, D, _l.ptr(cat),
                                          _l.ptr(sig), _l.ptr(alpha), _l.stream_ptr()), "pxr_srgnn_readout_fwd_f32")
    return cat


def srgnn_readout_bwd(dcat, Hn, alias, mask, w3, sig, alpha, dP=None, dH=None, dw3p=None):
    """-> (dP [B*L, 2D], dH [B*L, D], dw3p [B, D]) from dcat [B, 2D]."""
    Lb = _l.load()
    _req(dcat, torch.float32, "dcat"); _req(sig, torch.float32, "sig"); _req(alpha, torch.float32, "alpha")
    B, L = alias.shape
    D = Hn.shape[-1]
    dev = Hn.device
    dP = dP if dP is not None else torch.empty(B * L, 2 * D, dtype=torch.float32, device=dev)
    dH = dH if dH is not None else torch.empty(B * L, D, dtype=torch.float32, device=dev)
    dw3p = dw3p if dw3p is not None else torch.empty(B, D, dtype=torch.float32, device=dev)
    _l.check(Lb.pxr_srgnn_readout_bwd_f32(_l.ptr(dcat), _l.ptr(Hn), _l.ptr(alias), _l.ptr(mask), _l.ptr(w3), _l.ptr(sig),
                                          _l.ptr(alpha), B, L, D, _l.ptr(dP), _l.ptr(dH), _l.ptr(dw3p), _l.stream_ptr()),
             "pxr_srgnn_readout_bwd_f32")
    return dP, dH, dw3p


def srgnn_pair_fwd(out, ld_out: int, table, target, B: int):
    """SRGNN's pair loss (srgnn.py:60-66): query rows out[b * ld_out : + D], target [B, 2] rows of the table ->
    (loss [1], coef [B] = d loss / d x_b)."""
    Lb = _l.load()
    _req(out, torch.float32, "out", contiguous=False); _req(table, torch.float32, "table"); _req(target, torch.int64, "target")
    N, D = table.shape
    if target.numel() != 2 * B:
        raise _l.PxrError(f"srgnn pair head: target must be [B, 2] for B={B}, got {tuple(target.shape)}")
    f = torch.empty(2 * B + 1, dtype=torch.float32, device=out.device)
    lossrow, coef, loss = f[:B], f[B:2 * B], f[2 * B:]
    device_status(out.device)
    _l.check(Lb.pxr_srgnn_pair_fwd_f32(_l.ptr(out), ld_out, _l.ptr(table), N, D, _l.ptr(target), B, _l.ptr(lossrow), _l.ptr(coef),
                                       _l.ptr(loss), _l.stream_ptr()), "pxr_srgnn_pair_fwd_f32")
    return loss, coef


def srgnn_pair_bwd(table, target, coef, dout, ld_dout: int, grad_scale=1.0, grad_scale_dev=None, coef_out=None, coef_stride: int = 1):
    """dout rows (ld_dout apart) = c_b (e[pos] - e[neg]); coef_out[b * coef_stride] = c_b when given."""
    Lb = _l.load()
    _req(table, torch.float32, "table"); _req(target, torch.int64, "target"); _req(coef, torch.float32, "coef")
    N, D = table.shape
    _l.check(Lb.pxr_srgnn_pair_bwd_f32(_l.ptr(table), N, D, _l.ptr(target), _l.ptr(coef), coef.numel(), float(grad_scale),
                                       _l.ptr(grad_scale_dev), _l.ptr(dout), ld_dout, _l.ptr(coef_out), coef_stride,
                                       _l.stream_ptr()), "pxr_srgnn_pair_bwd_f32")
    return dout


# ------------------------------------------------------------------------------------------------ LightSANs (csrc/lightsans.hip)
LIGHTSANS_MAX_L, LIGHTSANS_MAX_D, LIGHTSANS_MAX_K = 64, 1024, 16


def lightsans_shape_error(L: int, D: int, H: int, K: int):
    """The message the kernels would fail with for this shape, or None when they serve it (checked before any launch)."""
    if not 1 <= L <= LIGHTSANS_MAX_L:
        return f"MAX_ITEM_LIST_LENGTH={L} outside 1..{LIGHTSANS_MAX_L}"
    if H < 1 or D < 4 or D > LIGHTSANS_MAX_D or D % (4 * H):
        return f"embedding_size={D} with n_heads={H}: need D <= {LIGHTSANS_MAX_D} and D % (4 * n_heads) == 0"
    if not 1 <= K <= LIGHTSANS_MAX_K:
        return f"k_interests={K} outside 1..{LIGHTSANS_MAX_K}"
    return None


def lightsans_fwd(qkv, theta, A, B: int, L: int, H: int, K: int, p_drop=0.0, seed=0, stream_id=0, step_dev=None, save=True):
    """Low-rank interest attention (layers.py:784-790, 839-878): qkv [B*L, 3D], theta [2, D, K] (thK | thV), A [H, L, L] ->
    (ctx [B*L, D], saved dict(pi [B, 2, L, K], probs [B, H, L, K], KVp [B, 2K, D]) | None without save)."""
    Lb = _l.load()
    _req(qkv, torch.float32, "qkv"); _req(theta, torch.float32, "theta"); _req(A, torch.float32, "A")
    D = qkv.shape[-1] // 3
    if qkv.numel() != B * L * 3 * D or theta.numel() != 2 * D * K or A.numel() != H * L * L:
        raise _l.PxrError(f"lightsans fwd: qkv {tuple(qkv.shape)} / theta {tuple(theta.shape)} / A {tuple(A.shape)} do not match "
                          f"B={B}, L={L}, H={H}, K={K}")
    dev = qkv.device
    ctx = torch.empty(B * L, D, dtype=torch.float32, device=dev)
    KVp = torch.empty(B, 2 * K, D, dtype=torch.float32, device=dev)
    pi = torch.empty(B, 2, L, K, dtype=torch.float32, device=dev) if save else None
    probs = torch.empty(B, H, L, K, dtype=torch.float32, device=dev) if save else None
    _l.check(Lb.pxr_lightsans_fwd_f32(_l.ptr(qkv), _l.ptr(theta), _l.ptr(A), B, L, D, H, K, float(p_drop), seed & 0xFFFFFFFFFFFFFFFF,
                                      stream_id, _l.ptr(step_dev), _l.ptr(ctx), _l.ptr(pi), _l.ptr(probs), _l.ptr(KVp), _l.stream_ptr()),
             "pxr_lightsans_fwd_f32")
    return ctx, (dict(pi=pi, probs=probs, KVp=KVp) if save else None)


def lightsans_bwd(dctx, qkv, theta, A, saved, B: int, L: int, H: int, K: int, p_drop=0.0, seed=0, stream_id=0, step_dev=None):
    """-> (dqkv [B*L, 3D], dKVp [B, 2K, D], dtheta_part [B, 2DK], dA_part [B, HLL]); the parts are reduced with colsum."""
    Lb = _l.load()
    D = qkv.shape[-1] // 3
    want = {"dctx": (dctx, B * L * D), "qkv": (qkv, B * L * 3 * D), "theta": (theta, 2 * D * K), "A": (A, H * L * L),
            "pi": (saved["pi"], B * 2 * L * K), "probs": (saved["probs"], B * H * L * K), "KVp": (saved["KVp"], B * 2 * K * D)}
    for name, (t, n) in want.items():
        _req(t, torch.float32, name)
        if t.numel() != n:
            raise _l.PxrError(f"lightsans bwd: {name} has {t.numel()} elements, B={B}, L={L}, D={D}, H={H}, K={K} need {n}")
    dev = qkv.device
    dqkv = torch.empty(B * L, 3 * D, dtype=torch.float32, device=dev)
    dKVp = torch.empty(B, 2 * K, D, dtype=torch.float32, device=dev)
    dth = torch.empty(B, 2 * D * K, dtype=torch.float32, device=dev)
    dA = torch.empty(B, H * L * L, dtype=torch.float32, device=dev)
    _l.check(Lb.pxr_lightsans_bwd_f32(_l.ptr(dctx), _l.ptr(qkv), _l.ptr(theta), _l.ptr(A), _l.ptr(saved["pi"]), _l.ptr(saved["probs"]),
                                      _l.ptr(saved["KVp"]), B, L, D, H, K, float(p_drop), seed & 0xFFFFFFFFFFFFFFFF, stream_id,
                                      _l.ptr(step_dev), _l.ptr(dqkv), _l.ptr(dKVp), _l.ptr(dth), _l.ptr(dA), _l.stream_ptr()),
             "pxr_lightsans_bwd_f32")
    return dqkv, dKVp, dth, dA


def lightsans_pos_fwd(pqk, H: int):
    """pqk [L, 2D] = pq | pk (before pos_scaling) -> A [H, L, L], softmax over the queries (layers.py:862-868)."""
    Lb = _l.load()
    _req(pqk, torch.float32, "pqk")
    L, D2 = pqk.shape
    A = torch.empty(H, L, L, dtype=torch.float32, device=pqk.device)
    _l.check(Lb.pxr_lightsans_pos_fwd_f32(_l.ptr(pqk), L, D2 // 2, H, _l.ptr(A), _l.stream_ptr()), "pxr_lightsans_pos_fwd_f32")
    return A


def lightsans_pos_bwd(pqk, A, dA):
    """dA [H, L, L] -> dpqk [L, 2D] = d pq | d pk."""
    Lb = _l.load()
    _req(pqk, torch.float32, "pqk"); _req(A, torch.float32, "A"); _req(dA, torch.float32, "dA")
    L, D2 = pqk.shape
    H = A.shape[0]
    if A.numel() != H * L * L or dA.numel() != H * L * L:
        raise _l.PxrError(f"lightsans pos bwd: A {tuple(A.shape)} / dA {tuple(dA.shape)} do not match L={L}, H={H}")
    dpqk = torch.empty_like(pqk)
    _l.check(Lb.pxr_lightsans_pos_bwd_f32(_l.ptr(pqk), _l.ptr(A), _l.ptr(dA), L, D2 // 2, H, _l.ptr(dpqk), _l.stream_ptr()),
             "pxr_lightsans_pos_bwd_f32")
    return dpqk


# ------------------------------------------------------------------------------------------------ ids -> table rows (csrc/rows.hip)
class _CRowSegment(ctypes.Structure):
    """include/pxr.h: pxr_row_segment."""
    _fields_ = [("ids", ctypes.c_void_p), ("count", ctypes.c_int64), ("n", ctypes.c_int64), ("base", ctypes.c_int64),
                ("pad0", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def _table_rows(who: str, segments, out, shape, want_gidx: bool = False):
    """pxr_table_rows_i64 over segments = [(name, ids int64 tensor | None, n, base, pad0)] (None: left out) into `out` or a new
    int64 tensor of `shape` ([n]: the rows; [2, n]: rows | gidx).  Bad ids flag the status word and are clamped."""
    segments = [g for g in segments if g[1] is not None]
    for name, ids, *_ in segments:
        _req(ids, torch.int64, name)
    dev = segments[0][1].device
    buf = out if out is not None else torch.empty(*shape, dtype=torch.int64, device=dev)
    if tuple(buf.shape) != tuple(shape) or buf.dtype != torch.int64:
        raise _l.PxrError(f"{who}: out must be int64 {list(shape)}")
    c = (_CRowSegment * len(segments))()
    for g, (_, ids, n, base, pad0) in zip(c, segments):
        g.ids, g.count, g.n, g.base, g.pad0 = ids.data_ptr(), ids.numel(), int(n), int(base), int(pad0)
    two = len(shape) == 2
    device_status(dev)
    _l.check(_l.load().pxr_table_rows_i64(c, len(segments), _l.ptr(buf[0] if two else buf), _l.ptr(buf[1]) if want_gidx else None,
                                          _l.stream_ptr()), "pxr_table_rows_i64")
    return buf


def _pair_items(who: str, item, B: int):
    if item is not None and item.numel() != 2 * B:
        raise _l.PxrError(f"{who}: item must be [B, 2] for B={B}, got {tuple(item.shape)}")


# ------------------------------------------------------------------------------------------------ MF (csrc/mf.hip)
def mf_pair_rows(user, item, n_users: int, n_items: int, out=None):
    """user int64 [B], item int64 [B, 2] | None -> rows int64 [3B] (or [B]) of the [1 + U + I, D] table: [1 + user | 1 + U +
    item.view(-1)].  Bad ids flag the status word (ops.raise_on_bad_indices) and are clamped."""
    B = user.numel()
    _pair_items("mf pair rows", item, B)
    return _table_rows("mf pair rows", [("user", user, n_users, 1, 0), ("item", item, n_items, 1 + n_users, 0)], out,
                       (3 * B if item is not None else B,))


def mf_pair_fwd(ufeat, ifeat, B: int, rows=None, out=None, eps=1e-8):
    """MF's pair loss head (mf.py forward; pxr_mf_pair_fwd_eps_f32).  rows given: u read from ufeat at rows[:B] and i+- from ifeat at
    rows[B:] (MF: both the one table; MOMF: the user table and the encoder's output); else ufeat [B, H], ifeat [2B, H] (tower
    outputs).  eps: the shift outside the log, 1e-8 in mf.py and 0 in momf.py.  -> (loss [1], coef [B] = d loss / d x_b).  out: a
    float32 [2B + 1] buffer to reuse."""
    Lb = _l.load()
    _req(ufeat, torch.float32, "ufeat"); _req(ifeat, torch.float32, "ifeat")
    H = ufeat.shape[-1]
    if ifeat.shape[-1] != H:
        raise _l.PxrError("mf pair head: ufeat and ifeat widths differ")
    if rows is None and (ufeat.shape[0] != B or ifeat.shape[0] != 2 * B):
        raise _l.PxrError(f"mf pair head: tower outputs must be [B, H] and [2B, H] for B={B}")
    if rows is not None:
        _req(rows, torch.int64, "rows")
        if rows.numel() != 3 * B:
            raise _l.PxrError(f"mf pair head: rows must be [3B] for B={B}")
    f = out if out is not None else torch.empty(2 * B + 1, dtype=torch.float32, device=ufeat.device)
    coef, lossrow, loss = f[:B], f[B:2 * B], f[2 * B:]
    _l.check(Lb.pxr_mf_pair_fwd_eps_f32(_l.ptr(ufeat), _l.ptr(ifeat), _l.ptr(rows), H, B, float(eps), _l.ptr(coef), _l.ptr(lossrow),
                                        _l.ptr(loss), _l.stream_ptr()), "pxr_mf_pair_fwd_eps_f32")
    return loss, coef


def mf_pair_bwd(ufeat, ifeat, coef, du, di, grad_scale=1.0, grad_scale_dev=None):
    """du [B, H] / di [2B, H] (overwritten) = the head's gradient onto the tower outputs."""
    Lb = _l.load()
    for t, nm in ((ufeat, "ufeat"), (ifeat, "ifeat"), (coef, "coef"), (du, "du"), (di, "di")):
        _req(t, torch.float32, nm)
    B, H = ufeat.shape
    if ifeat.shape != (2 * B, H) or du.shape != (B, H) or di.shape != (2 * B, H) or coef.numel() != B:
        raise _l.PxrError("mf pair head backward: shapes must be [B, H], [2B, H], coef [B], du [B, H], di [2B, H]")
    _l.check(Lb.pxr_mf_pair_bwd_f32(_l.ptr(ufeat), _l.ptr(ifeat), _l.ptr(coef), H, B, float(grad_scale), _l.ptr(grad_scale_dev),
                                    _l.ptr(du), _l.ptr(di), _l.stream_ptr()), "pxr_mf_pair_bwd_f32")


def mf_table_grad(rows, B: int, sp: SparseRows, table=None, coef=None, occ=None, grad_scale=1.0, grad_scale_dev=None):
    """The step's table gradient in sparse form (pxr_mf_table_grad_f32): from the head's formula on `table` with `coef`, or from the
    per-occurrence rows occ [3B, D] (the towers' input gradients).  Writes sp (cap >= 3B) and returns it."""
    Lb = _l.load()
    _req(rows, torch.int64, "rows")
    if rows.numel() != 3 * B:
        raise _l.PxrError(f"mf table grad: rows must be [3B] for B={B}")
    D = sp.rows.shape[1]
    if occ is not None:
        _req(occ, torch.float32, "occ")
        if occ.shape != (3 * B, D):
            raise _l.PxrError(f"mf table grad: occ must be [3B, D] = [{3 * B}, {D}], got {tuple(occ.shape)}")
        n_table = 0
    else:
        _req(table, torch.float32, "table"); _req(coef, torch.float32, "coef")
        if table.shape[1] != D or coef.numel() != B:
            raise _l.PxrError("mf table grad: table width / coef length do not match")
        n_table = table.shape[0]
    _l.check(Lb.pxr_mf_table_grad_f32(_l.ptr(table), n_table, D, _l.ptr(rows), B, _l.ptr(coef), _l.ptr(occ), float(grad_scale),
                                      _l.ptr(grad_scale_dev), _l.ptr(sp.idx), _l.ptr(sp.rows), _l.ptr(sp.n), sp.cap,
                                      _l.stream_ptr()), "pxr_mf_table_grad_f32")
    return sp


def momf_pair_rows(user, index, n_users: int, n_rows: int, out=None):
    """user int64 [B], index int64 [B, 2] positions into the encoder's output [n_rows, D] -> rows int64 [3B] = [1 + user |
    index.view(-1)] (position base 0: MOMF has no padding position).  Bad ids flag the status word and are clamped."""
    B = user.numel()
    _pair_items("momf pair rows", index, B)
    return _table_rows("momf pair rows", [("user", user, n_users, 1, 0), ("index", index, n_rows, 0, 0)], out, (3 * B,))


def momf_pair_grad(rows, B: int, sp: SparseRows, n_rows: int, utable=None, E=None, coef=None, occ=None, grad_scale=1.0,
                   grad_scale_dev=None, out=None):
    """MOMF's backward into its two row spaces (pxr_momf_pair_grad_f32): the user rows' gradient as sparse rows in sp (cap >= B,
    count B) and d loss / d E as a dense [n_rows, D] block (`out` or a new tensor; zeroed by the entry), from the head's formula on
    `utable`, `E` and `coef`, or from the per-occurrence rows occ [3B, D].  -> dE."""
    Lb = _l.load()
    _req(rows, torch.int64, "rows")
    if rows.numel() != 3 * B:
        raise _l.PxrError(f"momf pair grad: rows must be [3B] for B={B}")
    D = sp.rows.shape[1]
    if sp.cap < B:
        raise _l.PxrError(f"momf pair grad: the sparse rows hold {sp.cap} slots, B={B}")
    n_utable = 0
    if occ is not None:
        _req(occ, torch.float32, "occ")
        if occ.shape != (3 * B, D):
            raise _l.PxrError(f"momf pair grad: occ must be [3B, D] = [{3 * B}, {D}], got {tuple(occ.shape)}")
        utable = E = coef = None
    else:
        _req(utable, torch.float32, "utable"); _req(E, torch.float32, "E"); _req(coef, torch.float32, "coef")
        if utable.dim() != 2 or utable.shape[1] != D or tuple(E.shape) != (n_rows, D) or coef.numel() != B:
            raise _l.PxrError(f"momf pair grad: need utable [*, {D}], E [{n_rows}, {D}] and coef [{B}]")
        n_utable = utable.shape[0]
    dE = out if out is not None else torch.empty(n_rows, D, dtype=torch.float32, device=rows.device)
    _req(dE, torch.float32, "dE")
    if tuple(dE.shape) != (n_rows, D):
        raise _l.PxrError(f"momf pair grad: dE must be [{n_rows}, {D}], got {tuple(dE.shape)}")
    _l.check(Lb.pxr_momf_pair_grad_f32(_l.ptr(utable), n_utable, _l.ptr(E), n_rows, D, _l.ptr(rows), B, _l.ptr(coef), _l.ptr(occ),
                                       float(grad_scale), _l.ptr(grad_scale_dev), _l.ptr(sp.idx), _l.ptr(sp.rows), _l.ptr(sp.n),
                                       sp.cap, _l.ptr(dE), _l.stream_ptr()), "pxr_momf_pair_grad_f32")
    return dE


def mf_bn_tanh_fwd(x, gamma, beta, running_mean, running_var, num_batches_tracked, eps=1e-5, momentum=0.1, y=None, stats=None):
    """Training BatchNorm1d + tanh over x [R, H] (running statistics updated on the device) -> (y, mean [H], rstd [H])."""
    Lb = _l.load()
    for t, nm in ((x, "x"), (gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _req(t, torch.float32, nm)
    R, H = x.shape
    y = y if y is not None else torch.empty_like(x)
    st = stats if stats is not None else torch.empty(2, H, dtype=torch.float32, device=x.device)
    _l.check(Lb.pxr_mf_bn_tanh_fwd_f32(_l.ptr(x), R, H, _l.ptr(gamma), _l.ptr(beta), float(eps), float(momentum),
                                       _l.ptr(running_mean), _l.ptr(running_var), _l.ptr(num_batches_tracked), _l.ptr(y),
                                       _l.ptr(st[0]), _l.ptr(st[1]), _l.stream_ptr()), "pxr_mf_bn_tanh_fwd_f32")
    return y, st[0], st[1]


def mf_bn_tanh_bwd(dy, x, y, mean, rstd, gamma, dgamma, dbeta, dx=None):
    """Backward of mf_bn_tanh_fwd: -> dx [R, H]; dgamma / dbeta [H] overwritten."""
    Lb = _l.load()
    for t, nm in ((dy, "dy"), (x, "x"), (y, "y"), (mean, "mean"), (rstd, "rstd"), (gamma, "gamma"), (dgamma, "dgamma"),
                  (dbeta, "dbeta")):
        _req(t, torch.float32, nm)
    R, H = x.shape
    if dy.shape != x.shape or y.shape != x.shape:
        raise _l.PxrError("mf bn backward: dy, x and y must have one shape")
    dx = dx if dx is not None else torch.empty_like(x)
    _l.check(Lb.pxr_mf_bn_tanh_bwd_f32(_l.ptr(dy), _l.ptr(x), _l.ptr(y), _l.ptr(mean), _l.ptr(rstd), _l.ptr(gamma), R, H, _l.ptr(dx),
                                       _l.ptr(dgamma), _l.ptr(dbeta), _l.stream_ptr()), "pxr_mf_bn_tanh_bwd_f32")
    return dx


def mf_bn_tanh_eval(x, gamma, beta, running_mean, running_var, eps=1e-5, y=None):
    """Eval-mode BatchNorm1d + tanh over x [R, H] (running statistics)."""
    Lb = _l.load()
    for t, nm in ((x, "x"), (gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _req(t, torch.float32, nm)
    R, H = x.shape
    y = y if y is not None else torch.empty_like(x)
    _l.check(Lb.pxr_mf_bn_tanh_eval_f32(_l.ptr(x), R, H, _l.ptr(gamma), _l.ptr(beta), _l.ptr(running_mean), _l.ptr(running_var),
                                        float(eps), _l.ptr(y), _l.stream_ptr()), "pxr_mf_bn_tanh_eval_f32")
    return y


# ------------------------------------------------------------------------------------------------ VBPR (csrc/vbpr.hip)
def vbpr_rows(user, item, n_users: int, n_items: int, out=None):
    """user int64 [B], item int64 [B, 2] | None -> rows int64 [4B] (or [2B]) of the [1 + U + I + U, Dh] table: [1 + user | 1 + U + I
    + user | 1 + U + item.view(-1)].  Bad ids flag the status word (ops.raise_on_bad_indices) and are clamped."""
    B = user.numel()
    _pair_items("vbpr rows", item, B)
    return _table_rows("vbpr rows", [("user", user, n_users, 1, 0), ("user", user, n_users, 1 + n_users + n_items, 0),
                                     ("item", item, n_items, 1 + n_users, 0)], out, (4 * B if item is not None else 2 * B,))


def vbpr_gather(feat, item, wb, out=None, beta=None, copy=True):
    """feat [I, F] (frozen features), item int64 [n] | None (every row), wb [F] -> (out [n, F] | None, beta [n] = rows . wb), the row
    read once.  copy=False: beta only.  Bad item ids flag the status word and are clamped."""
    Lb = _l.load()
    _req(feat, torch.float32, "feat"); _req(wb, torch.float32, "wb")
    I, F = feat.shape
    if wb.numel() != F:
        raise _l.PxrError(f"vbpr gather: wb must have F={F} elements, got {wb.numel()}")
    if item is not None:
        _req(item, torch.int64, "item")
    n = item.numel() if item is not None else I
    if copy:
        out = out if out is not None else torch.empty(n, F, dtype=torch.float32, device=feat.device)
        _req(out, torch.float32, "out")
        if out.numel() != n * F:
            raise _l.PxrError(f"vbpr gather: out must be [{n}, {F}]")
    else:
        out = None
    beta = beta if beta is not None else torch.empty(n, dtype=torch.float32, device=feat.device)
    _req(beta, torch.float32, "beta")
    if beta.numel() != n:
        raise _l.PxrError(f"vbpr gather: beta must be [{n}]")
    device_status(feat.device)
    _l.check(Lb.pxr_vbpr_gather_f32(_l.ptr(feat), I, F, _l.ptr(item), n, _l.ptr(wb), _l.ptr(out), _l.ptr(beta), _l.stream_ptr()),
             "pxr_vbpr_gather_f32")
    return out, beta


def vbpr_pair_fwd(table, rows, e, beta, B: int, out=None):
    """VBPR's pair loss head (vbpr.py forward) on the table rows at rows [4B], the projected features e [2B, Dh] and beta [2B]
    -> (loss [1], coef [B] = d loss / d x_b).  out: a float32 [2B + 1] buffer to reuse."""
    Lb = _l.load()
    _req(table, torch.float32, "table"); _req(rows, torch.int64, "rows"); _req(e, torch.float32, "e"); _req(beta, torch.float32, "beta")
    Dh = table.shape[1]
    if rows.numel() != 4 * B or tuple(e.shape) != (2 * B, Dh) or beta.numel() != 2 * B:
        raise _l.PxrError(f"vbpr pair head: need rows [4B], e [2B, Dh], beta [2B] for B={B}, Dh={Dh}")
    f = out if out is not None else torch.empty(2 * B + 1, dtype=torch.float32, device=table.device)
    coef, lossrow, loss = f[:B], f[B:2 * B], f[2 * B:]
    _l.check(Lb.pxr_vbpr_pair_fwd_f32(_l.ptr(table), _l.ptr(rows), _l.ptr(e), _l.ptr(beta), Dh, B, _l.ptr(coef), _l.ptr(lossrow),
                                      _l.ptr(loss), _l.stream_ptr()), "pxr_vbpr_pair_fwd_f32")
    return loss, coef


def vbpr_pair_bwd(table, rows, e, coef, B: int, de, csign, sp: SparseRows, grad_scale=1.0, grad_scale_dev=None):
    """The head's backward: de [2B, Dh] and csign [2B] overwritten, the tables' gradient written to sp (cap >= 4B) and returned."""
    Lb = _l.load()
    for t, nm in ((table, "table"), (e, "e"), (coef, "coef"), (de, "de"), (csign, "csign")):
        _req(t, torch.float32, nm)
    _req(rows, torch.int64, "rows")
    Dh = table.shape[1]
    if (rows.numel() != 4 * B or tuple(e.shape) != (2 * B, Dh) or tuple(de.shape) != (2 * B, Dh) or coef.numel() != B
            or csign.numel() != 2 * B or sp.rows.shape[1] != Dh):
        raise _l.PxrError(f"vbpr pair head backward: need rows [4B], e / de [2B, Dh], coef [B], csign [2B], sparse rows Dh wide "
                          f"(B={B}, Dh={Dh})")
    _l.check(Lb.pxr_vbpr_pair_bwd_f32(_l.ptr(table), _l.ptr(rows), _l.ptr(e), _l.ptr(coef), Dh, B, float(grad_scale),
                                      _l.ptr(grad_scale_dev), _l.ptr(de), _l.ptr(csign), _l.ptr(sp.idx), _l.ptr(sp.rows),
                                      _l.ptr(sp.n), sp.cap, _l.stream_ptr()), "pxr_vbpr_pair_bwd_f32")
    return sp


def vbpr_bias_grad(x, csign, out):
    """out [F] = sum_r csign[r] x[r, :] (the gradient of bias_projection.weight), fixed summation order."""
    Lb = _l.load()
    _req(x, torch.float32, "x"); _req(csign, torch.float32, "csign"); _req(out, torch.float32, "out")
    R, F = x.shape
    if csign.numel() != R or out.numel() != F:
        raise _l.PxrError(f"vbpr bias gradient: need csign [{R}] and out [{F}]")
    _l.check(Lb.pxr_vbpr_bias_grad_f32(_l.ptr(x), _l.ptr(csign), R, F, _l.ptr(out), _l.stream_ptr()), "pxr_vbpr_bias_grad_f32")
    return out


def vbpr_packed_width(Dh: int) -> int:
    """Width of the packed scoring vectors: 2 Dh + 1, zero-padded to a multiple of 32 (the fused top-k's plane path)."""
    return (2 * Dh + 1 + 31) // 32 * 32


def vbpr_pack(a, b, s=None, a_rows=None, b_rows=None, out=None):
    """out [R, vbpr_packed_width(Dh)] = [a[a_rows] | b[b_rows] | s | 0 ...] (rows None: row r itself; s None: 1)."""
    Lb = _l.load()
    _req(a, torch.float32, "a"); _req(b, torch.float32, "b")
    Dh = a.shape[1]
    if b.shape[1] != Dh:
        raise _l.PxrError("vbpr pack: both operands must be Dh wide")
    if (a_rows is None) != (b_rows is None):
        raise _l.PxrError("vbpr pack: give both row lists or neither")
    if a_rows is not None:
        _req(a_rows, torch.int64, "a_rows"); _req(b_rows, torch.int64, "b_rows")
        R = a_rows.numel()
        if b_rows.numel() != R:
            raise _l.PxrError("vbpr pack: row lists differ in length")
    else:
        R = a.shape[0]
        if b.shape[0] != R:
            raise _l.PxrError("vbpr pack: operands differ in row count")
    if s is not None:
        _req(s, torch.float32, "s")
        if s.numel() != R:
            raise _l.PxrError(f"vbpr pack: s must be [{R}]")
    Dp = vbpr_packed_width(Dh)
    out = out if out is not None else torch.empty(R, Dp, dtype=torch.float32, device=a.device)
    if tuple(out.shape) != (R, Dp) or not out.is_contiguous():
        raise _l.PxrError(f"vbpr pack: out must be a contiguous [{R}, {Dp}]")
    _l.check(Lb.pxr_vbpr_pack_f32(_l.ptr(a), _l.ptr(a_rows), _l.ptr(b), _l.ptr(b_rows), _l.ptr(s), R, Dh, Dp, _l.ptr(out),
                                  _l.stream_ptr()), "pxr_vbpr_pack_f32")
    return out


# ------------------------------------------------------------------------------------------------ ACF (csrc/acf.hip)
def acf_rows(profile, items, user, n_items: int, n_users: int, out=None, want_gidx: bool = True):
    """profile int64 [B, P], items int64 [B, 2] | None, user int64 [B] -> (rows, gidx) int64 [B P + 2B + B] (or [B P + B]) of
    the [1 + I + U, E] table in the order profile | items | users: rows = the row an occurrence reads, gidx = the row its gradient
    goes to (0 for item id 0, the padding row).  Bad ids flag the status word (ops.raise_on_bad_indices) and are clamped.
    out: an int64 [2, n] buffer to reuse."""
    n = profile.numel() + (items.numel() if items is not None else 0) + user.numel()
    buf = _table_rows("acf rows", [("profile", profile, n_items, 1, 1), ("items", items, n_items, 1, 1),
                                   ("user", user, n_users, 1 + n_items, 0)], out, (2, n), want_gidx)
    return buf[0], buf[1]


def acf_region_fwd(x, xt, ut, w, profile, H: int, beta=None, pooled=None):
    """Region attention forward (pxr_acf_region_fwd_f32): x, xt [B P H, E] (or [B P, H E]), ut [B, E], w [E], profile int64 [B, P]
    -> (beta [B P, H], pooled [B P, E]); a padded position gets zeros."""
    Lb = _l.load()
    for t, nm in ((x, "x"), (xt, "xt"), (ut, "ut"), (w, "w")):
        _req(t, torch.float32, nm)
    _req(profile, torch.int64, "profile")
    B, E = ut.shape
    P = profile.numel() // B
    if profile.numel() != B * P or x.numel() != B * P * H * E or xt.numel() != x.numel() or w.numel() != E:
        raise _l.PxrError("acf region attention: need x, xt [B P H, E], ut [B, E], w [E], profile [B, P]")
    beta = beta if beta is not None else torch.empty(B * P, H, dtype=torch.float32, device=x.device)
    pooled = pooled if pooled is not None else torch.empty(B * P, E, dtype=torch.float32, device=x.device)
    _l.check(Lb.pxr_acf_region_fwd_f32(_l.ptr(x), _l.ptr(xt), _l.ptr(ut), _l.ptr(w), _l.ptr(profile), B, P, H, E, _l.ptr(beta),
                                       _l.ptr(pooled), _l.stream_ptr()), "pxr_acf_region_fwd_f32")
    return beta, pooled


def acf_region_bwd(dpooled, x, xt, ut, w, profile, beta, dxt, dut, dw_part, ws):
    """Region attention backward (pxr_acf_region_bwd_f32): writes dxt [B P H, E], dut [B, E], dw_part [B P, E] (column sum = dw);
    ws [B P, E] scratch."""
    Lb = _l.load()
    for t, nm in ((dpooled, "dpooled"), (x, "x"), (xt, "xt"), (ut, "ut"), (w, "w"), (beta, "beta"), (dxt, "dxt"), (dut, "dut"),
                  (dw_part, "dw_part"), (ws, "ws")):
        _req(t, torch.float32, nm)
    _req(profile, torch.int64, "profile")
    B, E = ut.shape
    R, H = beta.shape
    P = R // B
    if (profile.numel() != R or R != B * P or x.numel() != R * H * E or xt.numel() != x.numel() or dxt.numel() != x.numel()
            or dpooled.numel() != R * E or dw_part.numel() != R * E or ws.numel() < R * E or dut.numel() != B * E or w.numel() != E):
        raise _l.PxrError("acf region attention backward: operand shapes do not match")
    _l.check(Lb.pxr_acf_region_bwd_f32(_l.ptr(dpooled), _l.ptr(x), _l.ptr(xt), _l.ptr(ut), _l.ptr(w), _l.ptr(profile), _l.ptr(beta),
                                       B, P, H, E, _l.ptr(dxt), _l.ptr(dut), _l.ptr(dw_part), _l.ptr(ws), _l.stream_ptr()),
             "pxr_acf_region_bwd_f32")


def acf_region_dx(dx, x, beta, dpooled):
    """dx [R H, E] <- (dx + beta dpooled) (x > 0), in place (pxr_acf_region_dx_f32)."""
    Lb = _l.load()
    for t, nm in ((dx, "dx"), (x, "x"), (beta, "beta"), (dpooled, "dpooled")):
        _req(t, torch.float32, nm)
    R, H = beta.shape
    E = dpooled.shape[-1]
    if dx.numel() != R * H * E or x.numel() != dx.numel() or dpooled.numel() != R * E:
        raise _l.PxrError("acf region dx: operand shapes do not match")
    _l.check(Lb.pxr_acf_region_dx_f32(_l.ptr(dx), _l.ptr(x), _l.ptr(beta), _l.ptr(dpooled), R, H, E, _l.stream_ptr()),
             "pxr_acf_region_dx_f32")
    return dx


def acf_item_fwd(uw, pq, cx, prof, w, profile, alpha=None, user=None):
    """Item attention + user vector (pxr_acf_item_fwd_f32): uw [B, E], pq / cx / prof [B P, E], w [E], profile int64 [B, P] ->
    (alpha [B, P], user [B, E])."""
    Lb = _l.load()
    for t, nm in ((uw, "uw"), (pq, "pq"), (cx, "cx"), (prof, "prof"), (w, "w")):
        _req(t, torch.float32, nm)
    _req(profile, torch.int64, "profile")
    B, E = uw.shape
    P = profile.numel() // B
    if profile.numel() != B * P or any(t.numel() != B * P * E for t in (pq, cx, prof)) or w.numel() != E:
        raise _l.PxrError("acf item attention: need uw [B, E], pq / cx / prof [B P, E], w [E], profile [B, P]")
    alpha = alpha if alpha is not None else torch.empty(B, P, dtype=torch.float32, device=uw.device)
    user = user if user is not None else torch.empty(B, E, dtype=torch.float32, device=uw.device)
    _l.check(Lb.pxr_acf_item_fwd_f32(_l.ptr(uw), _l.ptr(pq), _l.ptr(cx), _l.ptr(prof), _l.ptr(w), _l.ptr(profile), B, P, E,
                                     _l.ptr(alpha), _l.ptr(user), _l.stream_ptr()), "pxr_acf_item_fwd_f32")
    return alpha, user


def acf_item_bwd(duser, uw, pq, cx, prof, w, alpha, da, dprof, duw, dw_part):
    """Item attention backward (pxr_acf_item_bwd_f32): writes da / dprof [B P, E], duw [B, E], dw_part [B, E] (column sum = dw)."""
    Lb = _l.load()
    for t, nm in ((duser, "duser"), (uw, "uw"), (pq, "pq"), (cx, "cx"), (prof, "prof"), (w, "w"), (alpha, "alpha"), (da, "da"),
                  (dprof, "dprof"), (duw, "duw"), (dw_part, "dw_part")):
        _req(t, torch.float32, nm)
    B, E = uw.shape
    P = alpha.numel() // B
    if (alpha.numel() != B * P or any(t.numel() != B * P * E for t in (pq, cx, prof, da, dprof))
            or any(t.numel() != B * E for t in (duser, duw, dw_part)) or w.numel() != E):
        raise _l.PxrError("acf item attention backward: operand shapes do not match")
    _l.check(Lb.pxr_acf_item_bwd_f32(_l.ptr(duser), _l.ptr(uw), _l.ptr(pq), _l.ptr(cx), _l.ptr(prof), _l.ptr(w), _l.ptr(alpha), B, P,
                                     E, _l.ptr(da), _l.ptr(dprof), _l.ptr(duw), _l.ptr(dw_part), _l.stream_ptr()),
             "pxr_acf_item_bwd_f32")


# ------------------------------------------------------------------------------------------------ CuratorNet (csrc/curator.hip)
def curator_pool(h, B: int, L: int, ids=None, cat=None, argmax=None, want_argmax: bool = True):
    """Profile pooling (pxr_curator_pool_f32) -> (cat [B, 2E] = [max over L | mean over L], argmax uint8 [B, E] | None).  ids None:
    h holds the B L profile rows first ([>= B L, E], read in place); ids int64 [B, L]: h is the item matrix [I, E] and position
    (b, l) reads row ids[b, l] (a bad id flags the status word).  Padded positions are pooled like any other; the mean divides by L."""
    Lb = _l.load()
    _req(h, torch.float32, "h")
    if h.dim() != 2:
        raise _l.PxrError("curator pool: h must be 2-D ([rows, E])")
    E = h.shape[1]
    if not 1 <= L <= 255:
        raise _l.PxrError(f"curator pool: need 1 <= L <= 255 (the argmax is stored in a byte), got L={L}")
    if ids is not None:
        _req(ids, torch.int64, "ids")
        if ids.numel() != B * L:
            raise _l.PxrError(f"curator pool: ids must be [B, L] = [{B}, {L}], got {tuple(ids.shape)}")
        device_status(h.device)
    elif h.shape[0] < B * L:
        raise _l.PxrError(f"curator pool: h has {h.shape[0]} rows, the profiles need B L = {B * L}")
    cat = cat if cat is not None else torch.empty(B, 2 * E, dtype=torch.float32, device=h.device)
    if want_argmax and argmax is None:
        argmax = torch.empty(B, E, dtype=torch.uint8, device=h.device)
    if cat.numel() != 2 * B * E or cat.dtype != torch.float32 or (argmax is not None and (argmax.numel() != B * E or
                                                                                           argmax.dtype != torch.uint8)):
        raise _l.PxrError("curator pool: cat must be float32 [B, 2E] and argmax uint8 [B, E]")
    _l.check(Lb.pxr_curator_pool_f32(_l.ptr(h), _l.ptr(ids), h.shape[0] if ids is not None else 0, B, L, E, _l.ptr(cat),
                                     _l.ptr(argmax), _l.stream_ptr()), "pxr_curator_pool_f32")
    if ids is not None and _CHECK_IDX:
        raise_on_bad_indices(h.device)
    return cat, argmax


def curator_pool_bwd(dcat, argmax, di, dact, B: int, L: int, out=None):
    """Pooling backward joined with the head's item gradient and selu' of the second common Linear (pxr_curator_pool_bwd_f32):
    dcat [B, 2E], argmax uint8 [B, E], di [2B, E], dact [B (L + 2), E] -> the pre-activation gradient [B (L + 2), E]."""
    Lb = _l.load()
    for t, nm in ((dcat, "dcat"), (di, "di"), (dact, "dact")):
        _req(t, torch.float32, nm)
    _req(argmax, torch.uint8, "argmax")
    E = dact.shape[-1]
    n = B * (L + 2)
    if dcat.numel() != 2 * B * E or argmax.numel() != B * E or di.numel() != 2 * B * E or dact.numel() != n * E:
        raise _l.PxrError("curator pool backward: need dcat [B, 2E], argmax [B, E], di [2B, E], dact [B (L + 2), E]")
    out = out if out is not None else torch.empty(n, E, dtype=torch.float32, device=dact.device)
    if out.numel() != n * E or out.dtype != torch.float32 or not out.is_contiguous():
        raise _l.PxrError("curator pool backward: out must be a contiguous float32 [B (L + 2), E]")
    _l.check(Lb.pxr_curator_pool_bwd_f32(_l.ptr(dcat), _l.ptr(argmax), _l.ptr(di), _l.ptr(dact), B, L, E, _l.ptr(out),
                                         _l.stream_ptr()), "pxr_curator_pool_bwd_f32")
    return out


def curator_pair_fwd(ufeat, ifeat, B: int, out=None):
    """CuratorNet's pair loss head (pxr_curator_pair_fwd_f32): ufeat [B, H], ifeat [2B, H] -> (loss [1] = -mean log(1e-8 +
    sigmoid(x_b)), coef [B] = d loss / d x_b).  The 1e-8 is inside the log (mf_pair_fwd has it outside); mf_pair_bwd takes this
    coef.  out: a float32 [2B + 1] buffer to reuse."""
    _req(ufeat, torch.float32, "ufeat"); _req(ifeat, torch.float32, "ifeat")
    H = ufeat.shape[-1]
    if tuple(ufeat.shape) != (B, H) or tuple(ifeat.shape) != (2 * B, H):
        raise _l.PxrError(f"curator pair head: tower outputs must be [B, H] and [2B, H] for B={B}")
    f = out if out is not None else torch.empty(2 * B + 1, dtype=torch.float32, device=ufeat.device)
    if f.numel() != 2 * B + 1 or f.dtype != torch.float32:
        raise _l.PxrError("curator pair head: out must be float32 [2B + 1]")
    coef, lossrow, loss = f[:B], f[B:2 * B], f[2 * B:]
    _l.check(_l.load().pxr_curator_pair_fwd_f32(_l.ptr(ufeat), _l.ptr(ifeat), H, B, _l.ptr(coef), _l.ptr(lossrow), _l.ptr(loss),
                                                _l.stream_ptr()), "pxr_curator_pair_fwd_f32")
    return loss, coef


def mul(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """out = a * b elementwise (pxr_mul_f32): a gradient times a saved activation derivative where no GEMM epilogue can do it."""
    _req(a, torch.float32, "a"); _req(b, torch.float32, "b")
    if a.shape != b.shape:
        raise _l.PxrError(f"mul: shapes differ ({tuple(a.shape)} and {tuple(b.shape)})")
    out = out if out is not None else torch.empty_like(a)
    _req(out, torch.float32, "out")
    if out.numel() != a.numel():
        raise _l.PxrError("mul: out has the wrong size")
    _l.check(_l.load().pxr_mul_f32(_l.ptr(a), _l.ptr(b), _l.ptr(out), a.numel(), _l.stream_ptr()), "pxr_mul_f32")
    return out


# ------------------------------------------------------------------------------------------------ VISRANK (csrc/visrank.hip)
def visrank_unit_rows(feat, eps: float = 1e-8, out=None):
    """feat [N, F] -> unit [N, F] = feat / max(||feat||_2, eps) row by row (F % 4 == 0): the cosine scoring's operand, made once."""
    Lb = _l.load()
    _req(feat, torch.float32, "feat")
    if feat.dim() != 2:
        raise _l.PxrError(f"visrank unit rows: feat must be [N, F], got {tuple(feat.shape)}")
    N, F = feat.shape
    out = out if out is not None else torch.empty_like(feat)
    _req(out, torch.float32, "out")
    if tuple(out.shape) != (N, F):
        raise _l.PxrError(f"visrank unit rows: out must be [{N}, {F}]")
    _l.check(Lb.pxr_visrank_unit_rows_f32(_l.ptr(feat), N, F, float(eps), _l.ptr(out), _l.stream_ptr()), "pxr_visrank_unit_rows_f32")
    return out


def visrank_topk(unit, window, top_k: int, K: int, hist_ptr=None, hist_items=None):
    """Fused VISRANK scoring + masks + top-K (pxr_visrank_topk_f32): unit [N, F] unit rows, window int64 [B, H <= 64] left-padded
    with 0, top_k in 1..16 (the mean of the min(top_k, h) largest similarities) or 0 (the mean over the window), hist_ptr int32
    [B + 1] / hist_items int64 the CSR of the full histories.  Returns (topk_idx int64 [B, K], topk_val fp32 [B, K]).  Bad ids
    flag the status word (ops.raise_on_bad_indices) and leave both outputs untouched."""
    Lb = _l.load()
    _req(unit, torch.float32, "unit"); _req(window, torch.int64, "window")
    if unit.dim() != 2 or window.dim() != 2:
        raise _l.PxrError("visrank top-k: unit must be [N, F] and window [B, H]")
    N, F = unit.shape
    B, H = window.shape
    _topk_hist_csr("visrank top-k", hist_ptr, hist_items, B)
    ws_bytes = int(Lb.pxr_visrank_topk_ws_bytes(B, H, N, K))
    if ws_bytes < 0:
        raise _l.PxrError(f"visrank top-k: need B >= 1, 1 <= H <= 64, 1 <= K <= 32 (B={B}, H={H}, K={K})")
    idx, val = _topk_out(B, K, unit.device)
    ws = _ws.get(ws_bytes, unit.device)
    _l.check(Lb.pxr_visrank_topk_f32(_l.ptr(unit), N, F, _l.ptr(window), B, H, int(top_k), _l.ptr(hist_ptr), _l.ptr(hist_items), K,
                                     _l.ptr(idx), _l.ptr(val), _l.ptr(ws), ws_bytes, _l.stream_ptr()), "pxr_visrank_topk_f32")
    return idx, val


# ------------------------------------------------------------------------------------------------ DIN (csrc/din.hip)
def din_rows(profile, target, n_items: int, out=None):
    """profile int64 [B, L], target int64 [B, 2] -> (rows, gidx) int64 [B L + 2 B] of the [1 + I, D] table (item i at row 1 + i)
    in the occurrence order history | candidates: rows = the row an occurrence reads, gidx = the row its gradient goes to (0 for
    item id 0, the padding row).  Bad ids flag the status word (ops.raise_on_bad_indices) and are clamped.  out: int64 [2, n]."""
    buf = _table_rows("din rows", [("profile", profile, n_items, 1, 1), ("target", target, n_items, 1, 1)], out,
                      (2, profile.numel() + target.numel()), True)
    return buf[0], buf[1]


def din_positions(profile, target, n_rows: int, out=None):
    """din_rows over a batch-local [n_rows, D] row matrix (MODIN: the encoder's output, row 0 the zero image = "no item"): profile
    int64 [S, L] and target int64 [S, 2] hold positions in [0, n_rows) -> (rows, gidx) int64 [S L + 2 S]: rows = the position
    itself, gidx = the same (0 takes no gradient).  A position outside [0, n_rows) flags the status word
    (ops.raise_on_bad_indices) and is clamped: nothing downstream reads out of range.  out: int64 [2, n]."""
    buf = _table_rows("din positions", [("profile", profile, n_rows, 0, 1), ("target", target, n_rows, 0, 1)], out,
                      (2, profile.numel() + target.numel()), True)
    return buf[0], buf[1]


def _din_shapes(B, L, D, emb=None, profile=None):
    if emb is not None and (tuple(emb.shape) != (B * (L + 2), D) or not emb.is_contiguous()):
        raise _l.PxrError(f"din: emb must be a contiguous [B (L + 2), D] = [{B * (L + 2)}, {D}], got {tuple(emb.shape)}")
    if profile is not None and tuple(profile.shape) != (B, L):
        raise _l.PxrError(f"din: profile must be [B, L] = [{B}, {L}], got {tuple(profile.shape)}")


def din_att_input(table, rows, B: int, L: int, emb=None, x=None):
    """Attention input (pxr_din_att_input_f32): table [T, D], rows int64 [B L + 2 B] (din_rows) -> (emb [B (L + 2), D] the gathered
    rows, x [2 B L, 4 D] = [q | k | q - k | q * k], pair row r = (c B + b) L + l)."""
    _req(table, torch.float32, "table"); _req(rows, torch.int64, "rows")
    D = table.shape[1]
    if rows.numel() != B * (L + 2):
        raise _l.PxrError(f"din attention input: rows must hold B (L + 2) = {B * (L + 2)} entries, got {rows.numel()}")
    emb = emb if emb is not None else torch.empty(B * (L + 2), D, dtype=torch.float32, device=table.device)
    x = x if x is not None else torch.empty(2 * B * L, 4 * D, dtype=torch.float32, device=table.device)
    _req(emb, torch.float32, "emb"); _req(x, torch.float32, "x")
    _din_shapes(B, L, D, emb)
    if tuple(x.shape) != (2 * B * L, 4 * D):
        raise _l.PxrError(f"din attention input: x must be [2 B L, 4 D] = [{2 * B * L}, {4 * D}]")
    _l.check(_l.load().pxr_din_att_input_f32(_l.ptr(table), _l.ptr(rows), B, L, D, _l.ptr(emb), _l.ptr(x), _l.stream_ptr()),
             "pxr_din_att_input_f32")
    return emb, x


def din_head_fwd(alast, wd, bd, emb, profile, s=None, kq=None, head=None, reg: float = 0.01):
    """Head forward (pxr_din_head_fwd_reg_f32): alast [2 B L, hl], wd [hl], bd [1], emb [B (L + 2), D], profile int64 [B, L] ->
    (loss [1], s [2 B L], kq [2 B L], head [2 + 3 B] = loss | regulariser coefficient | coef | score differences | squares).
    reg: the weight of ||emb||_2 / B in the loss -- DIN's 0.01 (the default: pxr_din_head_fwd_f32's bits), MODIN's 0."""
    for t, n in ((alast, "alast"), (wd, "wd"), (bd, "bd"), (emb, "emb")):
        _req(t, torch.float32, n)
    _req(profile, torch.int64, "profile")
    B, L = profile.shape
    D, hl = emb.shape[1], alast.shape[-1]
    _din_shapes(B, L, D, emb, profile)
    if alast.numel() != 2 * B * L * hl or wd.numel() != hl or bd.numel() != 1:
        raise _l.PxrError(f"din head: alast must be [2 B L, hl], wd [hl], bd [1] (B={B}, L={L}, hl={hl})")
    dev = emb.device
    s = s if s is not None else torch.empty(2 * B * L, dtype=torch.float32, device=dev)
    kq = kq if kq is not None else torch.empty(2 * B * L, dtype=torch.float32, device=dev)
    head = head if head is not None else torch.empty(2 + 3 * B, dtype=torch.float32, device=dev)
    if s.numel() != 2 * B * L or kq.numel() != 2 * B * L or head.numel() != 2 + 3 * B:
        raise _l.PxrError("din head: s / kq must hold 2 B L floats and head 2 + 3 B")
    _l.check(_l.load().pxr_din_head_fwd_reg_f32(_l.ptr(alast), _l.ptr(wd), _l.ptr(bd), _l.ptr(emb), _l.ptr(profile), B, L, D, hl,
                                                _l.ptr(s), _l.ptr(kq), _l.ptr(head), float(reg), _l.stream_ptr()),
             "pxr_din_head_fwd_reg_f32")
    return head[:1], s, kq, head


def din_head_bwd(alast, dact, wd, profile, kq, head, D: int, dwd, dbd, grad_scale=1.0, grad_scale_dev=None, dz=None, dsraw=None):
    """Head backward down to the last hidden layer (pxr_din_head_bwd_f32) -> (dz [2 B L, hl], dsraw [2 B L]); dwd [hl] / dbd [1]
    are written in place (the gradients of attention.dense)."""
    for t, n in ((alast, "alast"), (dact, "dact"), (wd, "wd"), (kq, "kq"), (head, "head"), (dwd, "dwd"), (dbd, "dbd")):
        _req(t, torch.float32, n)
    _req(profile, torch.int64, "profile")
    B, L = profile.shape
    hl = alast.shape[-1]
    if alast.numel() != 2 * B * L * hl or dact.shape != alast.shape or dwd.numel() != hl or dbd.numel() != 1:
        raise _l.PxrError("din head backward: alast / dact must be [2 B L, hl], dwd [hl], dbd [1]")
    if kq.numel() != 2 * B * L or head.numel() != 2 + 3 * B:
        raise _l.PxrError("din head backward: kq must hold 2 B L floats and head 2 + 3 B")
    gsd = grad_scale_dev if grad_scale_dev is not None else torch.ones(1, dtype=torch.float32, device=alast.device)
    dz = dz if dz is not None else torch.empty_like(alast)
    dsraw = dsraw if dsraw is not None else torch.empty(2 * B * L, dtype=torch.float32, device=alast.device)
    if dz.numel() != alast.numel() or dsraw.numel() != 2 * B * L:
        raise _l.PxrError("din head backward: dz / dsraw have the wrong size")
    _l.check(_l.load().pxr_din_head_bwd_f32(_l.ptr(alast), _l.ptr(dact), _l.ptr(wd), _l.ptr(profile), _l.ptr(kq), _l.ptr(head), B, L,
                                            int(D), hl, float(grad_scale), _l.ptr(gsd), _l.ptr(dz), _l.ptr(dsraw), _l.ptr(dwd),
                                            _l.ptr(dbd), _l.stream_ptr()), "pxr_din_head_bwd_f32")
    return dz, dsraw


def din_fold_bwd(dx, emb, profile, s, head, grad_scale=1.0, grad_scale_dev=None, occ=None):
    """One gradient row per occurrence (pxr_din_fold_bwd_f32): dx [2 B L, 4 D] the MLP's input gradient -> occ [B (L + 2), D]."""
    for t, n in ((dx, "dx"), (emb, "emb"), (s, "s"), (head, "head")):
        _req(t, torch.float32, n)
    _req(profile, torch.int64, "profile")
    B, L = profile.shape
    D = emb.shape[1]
    _din_shapes(B, L, D, emb, profile)
    if dx.numel() != 2 * B * L * 4 * D or s.numel() != 2 * B * L or head.numel() != 2 + 3 * B:
        raise _l.PxrError("din fold backward: dx must be [2 B L, 4 D], s [2 B L], head [2 + 3 B]")
    gsd = grad_scale_dev if grad_scale_dev is not None else torch.ones(1, dtype=torch.float32, device=emb.device)
    occ = occ if occ is not None else torch.empty_like(emb)
    _req(occ, torch.float32, "occ")
    _din_shapes(B, L, D, occ)
    _l.check(_l.load().pxr_din_fold_bwd_f32(_l.ptr(dx), _l.ptr(emb), _l.ptr(profile), _l.ptr(s), _l.ptr(head), B, L, D,
                                            float(grad_scale), _l.ptr(gsd), _l.ptr(occ), _l.stream_ptr()), "pxr_din_fold_bwd_f32")
    return occ


def din_fold_w1(w1, D: int):
    """W1 [h1, 4 D] -> (A, Bm, C) [h1, D] each: the first attention Linear factorised over cat[q, k, q - k, q * k]."""
    _req(w1, torch.float32, "w1")
    if w1.dim() != 2 or w1.shape[1] != 4 * D:
        raise _l.PxrError(f"din fold: W1 must be [h1, 4 D] with D = {D}, got {tuple(w1.shape)}")
    h1 = w1.shape[0]
    out = torch.empty(3, h1, D, dtype=torch.float32, device=w1.device)
    _l.check(_l.load().pxr_din_fold_w1_f32(_l.ptr(w1), h1, D, _l.ptr(out[0]), _l.ptr(out[1]), _l.ptr(out[2]), _l.stream_ptr()),
             "pxr_din_fold_w1_f32")
    return out[0], out[1], out[2]


DIN_MAX_D, DIN_MAX_HIDDEN, DIN_MAX_L, DIN_WS_CAP = 128, 128, 64, 1 << 28


def din_topk_supported(D: int, hidden, L: int, K: int = 10) -> bool:
    """Whether pxr_din_topk_f32 takes this shape: D % 4 == 0 up to 128, one or two hidden layers of at most 128 units, L <= 64,
    K <= 32."""
    hidden = list(hidden)
    if len(hidden) not in (1, 2):
        return False
    h1, h2 = hidden[0], (hidden[1] if len(hidden) == 2 else 0)
    return int(_l.load().pxr_din_topk_ws_bytes(1, int(L), 1, int(D), int(h1), int(h2), int(K))) >= 0 and h1 >= 1 and (len(hidden) == 1 or h2 >= 1)


def din_topk(table, window, aq, bm, cm, w2, b2, wd, bd, K: int, hist_ptr=None, hist_items=None):
    """Fused DIN scoring + masks + top-K (pxr_din_topk_f32): table [N, D], window int64 [B, L] left-padded with 0, aq [N, h1] =
    A q + b1, bm / cm [h1, D] (din_fold_w1), w2 [h2, h1] / b2 [h2] or None (one hidden layer), wd [h_last], bd [1], hist_ptr int32
    [B + 1] / hist_items int64 the CSR of the full histories.  Returns (topk_idx int64 [B, K], topk_val fp32 [B, K]).  Users are
    taken in chunks that keep the workspace (a scaled copy of C per window position) below DIN_WS_CAP bytes.  Bad ids flag the
    status word (ops.raise_on_bad_indices) and leave both outputs untouched."""
    Lb = _l.load()
    for t, n in ((table, "table"), (aq, "aq"), (bm, "bm"), (cm, "cm"), (wd, "wd"), (bd, "bd")):
        _req(t, torch.float32, n)
    _req(window, torch.int64, "window")
    if table.dim() != 2 or window.dim() != 2:
        raise _l.PxrError("din top-k: table must be [N, D] and window [B, L]")
    N, D = table.shape
    B, L = window.shape
    h1 = bm.shape[0]
    h2 = 0
    if w2 is not None:
        _req(w2, torch.float32, "w2"); _req(b2, torch.float32, "b2")
        h2 = w2.shape[0]
        if tuple(w2.shape) != (h2, h1) or b2.numel() != h2:
            raise _l.PxrError(f"din top-k: w2 must be [h2, h1] = [{h2}, {h1}] and b2 [h2]")
    if tuple(aq.shape) != (N, h1) or tuple(bm.shape) != (h1, D) or tuple(cm.shape) != (h1, D):
        raise _l.PxrError(f"din top-k: aq must be [N, h1] and bm / cm [h1, D] (N={N}, D={D}, h1={h1})")
    if wd.numel() != (h2 or h1) or bd.numel() != 1:
        raise _l.PxrError("din top-k: wd must hold h_last floats and bd one")
    _topk_hist_csr("din top-k", hist_ptr, hist_items, B)
    if int(Lb.pxr_din_topk_ws_bytes(1, L, N, D, h1, h2, K)) < 0:
        raise _l.PxrError(f"din top-k: outside the fused limits (D % 4 == 0 up to 128, hidden widths up to 128, L <= 64, K <= 32): "
                          f"D={D}, hidden=({h1}, {h2}), L={L}, K={K}")
    idx, val = _topk_out(B, K, table.device)
    chunk = max(1, min(B, DIN_WS_CAP // max(1, L * (h1 * D + 128) * 4)))
    for lo in range(0, B, chunk):
        hi = min(B, lo + chunk)
        ws_bytes = int(Lb.pxr_din_topk_ws_bytes(hi - lo, L, N, D, h1, h2, K))
        ws = _ws.get(ws_bytes, table.device)
        # (the CSR offsets are absolute: a chunk's slice of hist_ptr still indexes the whole hist_items)
        hp = hist_ptr[lo:hi + 1] if hist_ptr is not None else None
        _l.check(Lb.pxr_din_topk_f32(_l.ptr(table), N, D, _l.ptr(window[lo:hi]), hi - lo, L, _l.ptr(aq), _l.ptr(bm), _l.ptr(cm), h1,
                                     _l.ptr(w2), _l.ptr(b2), h2, _l.ptr(wd), _l.ptr(bd), _l.ptr(hp), _l.ptr(hist_items), K,
                                     _l.ptr(idx[lo:hi]), _l.ptr(val[lo:hi]), _l.ptr(ws), ws_bytes, _l.stream_ptr()),
                 "pxr_din_topk_f32")
    return idx, val


# ------------------------------------------------------------------------------------------------ DSSM / FM (csrc/pool.hip)
def _pool_shapes(table, rows, B: int, L: int, n_rows: int, who: str):
    _req(table, torch.float32, "table"); _req(rows, torch.int64, "rows")
    if table.dim() != 2:
        raise _l.PxrError(f"{who}: table must be [rows, D], got {tuple(table.shape)}")
    D = table.shape[1]
    if D <= 0 or D % 4 or D > 4096:
        raise _l.PxrError(f"{who}: need D % 4 == 0 and 0 < D <= 4096, got D={D}")
    if B < 1 or L < 1 or rows.numel() != n_rows:
        raise _l.PxrError(f"{who}: rows must hold {n_rows} entries for B={B}, L={L} (L >= 1), got {rows.numel()}")
    return D


def _out_f32(t, shape, device, who: str, name: str):
    """the caller's float32 output buffer `t`, checked against `shape`, or a new one"""
    if t is None:
        return torch.empty(*shape, dtype=torch.float32, device=device)
    _req(t, torch.float32, name)
    if tuple(t.shape) != tuple(shape):
        raise _l.PxrError(f"{who}: {name} must be float32 {list(shape)}, got {tuple(t.shape)}")
    return t


def pool_rows(table, rows, B: int, L: int, mean: bool, pad_row: int = 1, U=None, w=None):
    """Masked pooling (pxr_pool_rows_f32): table [T, D], rows int64 [B, L] (a longer list's first B L entries) whose entries equal
    to pad_row are "no item" -> (U [B, D] = the sum over the real positions, divided by (cnt + 1e-8) when mean; w [B] = the
    backward's factor: 1 / (cnt + 1e-8) or 1, and 0 for an empty profile).  din_rows' rows over the [1 + I, D] table: pad_row 1;
    evaluation windows over an item matrix: pad_row 0.  A bad id flags the status word (ops.raise_on_bad_indices) and is clamped."""
    if rows.numel() < B * L:
        raise _l.PxrError(f"pool rows: rows must hold at least B L = {B * L} entries, got {rows.numel()}")
    D = _pool_shapes(table, rows, B, L, rows.numel(), "pool rows")
    U = _out_f32(U, (B, D), table.device, "pool", "U")
    w = _out_f32(w, (B,), table.device, "pool", "w")
    device_status(table.device)
    _l.check(_l.load().pxr_pool_rows_f32(_l.ptr(table), table.shape[0], D, _l.ptr(rows), int(pad_row), B, L, int(bool(mean)),
                                         _l.ptr(U), _l.ptr(w), _l.stream_ptr()), "pxr_pool_rows_f32")
    if _CHECK_IDX:
        raise_on_bad_indices(table.device)
    return U, w


def pool_pair_fwd(table, rows, B: int, L: int, mean: bool, pad_row: int = 1, U=None, w=None, out=None):
    """The pooled pair step without an MLP in one launch (pxr_pool_pair_fwd_f32): rows int64 [B L + 2 B] (din_rows) ->
    (loss [1] = -mean log(1e-8 + sigmoid(x_b)), coef [B] = d loss / d x_b, U [B, D], w [B], lossrow [B]).  out: a float32
    [2B + 1] buffer (coef | lossrow | loss) to reuse."""
    D = _pool_shapes(table, rows, B, L, B * (L + 2), "pool pair forward")
    U = _out_f32(U, (B, D), table.device, "pool", "U")
    w = _out_f32(w, (B,), table.device, "pool", "w")
    f = _out_f32(out, (2 * B + 1,), table.device, "pool", "out")
    coef, lossrow, loss = f[:B], f[B:2 * B], f[2 * B:]
    device_status(table.device)
    _l.check(_l.load().pxr_pool_pair_fwd_f32(_l.ptr(table), table.shape[0], D, _l.ptr(rows), int(pad_row), B, L, int(bool(mean)),
                                             _l.ptr(U), _l.ptr(w), _l.ptr(coef), _l.ptr(lossrow), _l.ptr(loss), _l.stream_ptr()),
             "pxr_pool_pair_fwd_f32")
    return loss, coef, U, w, lossrow


def pool_pair_bwd(table, rows, B: int, L: int, U, coef, grad_scale=1.0, grad_scale_dev=None, G=None):
    """The pair head's backward as the compact block G [3B, D] (pxr_pool_pair_bwd_f32): G[b] = c_b (e[p_b] - e[n_b]),
    G[B + 2b] = c_b U_b, G[B + 2b + 1] = -c_b U_b with c_b = coef[b] grad_scale grad_scale_dev[0]; the pooling weight is applied
    by pool_table_grad."""
    D = _pool_shapes(table, rows, B, L, B * (L + 2), "pool pair backward")
    _req(U, torch.float32, "U"); _req(coef, torch.float32, "coef")
    if tuple(U.shape) != (B, D) or coef.numel() != B:
        raise _l.PxrError(f"pool pair backward: U must be [B, D] = [{B}, {D}] and coef [B]")
    if grad_scale_dev is not None:
        _req(grad_scale_dev, torch.float32, "grad_scale_dev")
    G = _out_f32(G, (3 * B, D), table.device, "pool", "G")
    device_status(table.device)
    _l.check(_l.load().pxr_pool_pair_bwd_f32(_l.ptr(table), table.shape[0], D, _l.ptr(rows), B, L, _l.ptr(U), _l.ptr(coef),
                                             float(grad_scale), _l.ptr(grad_scale_dev), _l.ptr(G), _l.stream_ptr()),
             "pxr_pool_pair_bwd_f32")
    return G


def pool_table_grad(gidx, B: int, L: int, G, w, n_table: int, out: SparseRows | None = None) -> SparseRows:
    """The table gradient from the compact block (pxr_pool_table_grad_f32): gidx int64 [B L + 2 B] (din_rows; 0 = padding, dropped),
    G [3B, D], w [B] -> SparseRows(cap >= B (L + 2)).  Occurrence o < B L adds w[o / L] G[o / L], occurrence o >= B L adds
    G[B + o - B L]: what embed_grad_rows gives on the materialised [B (L + 2), D] rows, which are never built."""
    Lb = _l.load()
    _req(gidx, torch.int64, "gidx"); _req(G, torch.float32, "G"); _req(w, torch.float32, "w")
    n = B * (L + 2)
    if B < 1 or L < 1 or gidx.numel() != n or G.dim() != 2 or G.shape[0] != 3 * B or w.numel() != B:
        raise _l.PxrError(f"pool table grad: need gidx [B (L + 2)] = [{n}], G [3B, D] and w [B] for B={B}, L={L}")
    D = G.shape[1]
    sp = out if out is not None else SparseRows(n, D, G.device)
    if sp.cap < n or sp.rows.shape[1] != D:
        raise _l.PxrError(f"pool table grad: out must hold {n} rows of width {D}")
    ws_bytes = int(Lb.pxr_embed_grad_ws_bytes(n))
    ws = _ws.get(ws_bytes, G.device)
    _l.check(Lb.pxr_pool_table_grad_f32(_l.ptr(gidx), B, L, _l.ptr(G), _l.ptr(w), D, int(n_table), _l.ptr(sp.idx), _l.ptr(sp.rows),
                                        _l.ptr(sp.n), _l.ptr(ws), ws_bytes, _l.stream_ptr()), "pxr_pool_table_grad_f32")
    return sp


def pool_dense_grad(gidx, B: int, L: int, G, w, n_rows: int, out=None):
    """The same gradient as a dense block over a batch-local row space (pxr_pool_dense_grad_f32): gidx int64 [B L + 2 B] holds rows
    of an [n_rows, D] matrix (0 = "no item", dropped; ids outside [0, n_rows) dropped) -> d_rows float32 [n_rows, D]: pool_table_grad's
    row sums, bit for bit, at their rows and exactly +0.0 everywhere else (row 0, unreferenced rows), whatever `out` held before."""
    Lb = _l.load()
    _req(gidx, torch.int64, "gidx"); _req(G, torch.float32, "G"); _req(w, torch.float32, "w")
    n = B * (L + 2)
    if B < 1 or L < 1 or gidx.numel() != n or G.dim() != 2 or G.shape[0] != 3 * B or w.numel() != B or n_rows < 1:
        raise _l.PxrError(f"pool dense grad: need gidx [B (L + 2)] = [{n}], G [3B, D], w [B] and n_rows >= 1 for B={B}, L={L}")
    D = G.shape[1]
    d_rows = _out_f32(out, (int(n_rows), D), G.device, "pool", "d_rows")
    ws_bytes = int(Lb.pxr_embed_grad_ws_bytes(n))
    ws = _ws.get(ws_bytes, G.device)
    _l.check(Lb.pxr_pool_dense_grad_f32(_l.ptr(gidx), B, L, _l.ptr(G), _l.ptr(w), D, int(n_rows), _l.ptr(d_rows), _l.ptr(ws),
                                        ws_bytes, _l.stream_ptr()), "pxr_pool_dense_grad_f32")
    return d_rows


# ------------------------------------------------------------------------------------------------ WideDeep (csrc/widedeep.hip)
def wd_join(zh, zt, b1, a1=None, der=None):
    """The split first Linear joined (pxr_wd_join_f32): zh [B, h1] the history product, zt [2 B, h1] the target product, b1 [h1] ->
    (a1 [2 B, h1] = relu(zh[r / 2] + zt[r] + b1), der = [a1 > 0])."""
    for t, n in ((zh, "zh"), (zt, "zt"), (b1, "b1")):
        _req(t, torch.float32, n)
    if zh.dim() != 2 or zt.dim() != 2 or zt.shape[0] != 2 * zh.shape[0] or zt.shape[1] != zh.shape[1] or b1.numel() != zh.shape[1]:
        raise _l.PxrError(f"widedeep join: need zh [B, h1], zt [2 B, h1], b1 [h1]; got {tuple(zh.shape)}, {tuple(zt.shape)}, "
                          f"{tuple(b1.shape)}")
    B, h1 = zh.shape
    a1 = _out_f32(a1, (2 * B, h1), zh.device, "widedeep", "a1")
    der = _out_f32(der, (2 * B, h1), zh.device, "widedeep", "der")
    _l.check(_l.load().pxr_wd_join_f32(_l.ptr(zh), _l.ptr(zt), _l.ptr(b1), B, h1, _l.ptr(a1), _l.ptr(der), _l.stream_ptr()),
             "pxr_wd_join_f32")
    return a1, der


def wd_join_bwd(dz1, dzh=None):
    """dzh[b] = dz1[2 b] + dz1[2 b + 1] (pxr_wd_join_bwd_f32): dz1 [2 B, h1] -> dzh [B, h1]."""
    _req(dz1, torch.float32, "dz1")
    if dz1.dim() != 2 or dz1.shape[0] % 2:
        raise _l.PxrError(f"widedeep join backward: dz1 must be [2 B, h1], got {tuple(dz1.shape)}")
    B, h1 = dz1.shape[0] // 2, dz1.shape[1]
    dzh = _out_f32(dzh, (B, h1), dz1.device, "widedeep", "dzh")
    _l.check(_l.load().pxr_wd_join_bwd_f32(_l.ptr(dz1), B, h1, _l.ptr(dzh), _l.stream_ptr()), "pxr_wd_join_bwd_f32")
    return dzh


def _wd_head_shapes(alast, wp, target, who: str):
    _req(alast, torch.float32, "alast"); _req(wp, torch.float32, "wp"); _req(target, torch.int64, "target")
    if target.dim() != 2 or target.shape[1] != 2 or alast.dim() != 2 or alast.shape[0] != 2 * target.shape[0] or wp.numel() != alast.shape[1]:
        raise _l.PxrError(f"{who}: need alast [2 B, hl], wp [hl], target int64 [B, 2]; got {tuple(alast.shape)}, {tuple(wp.shape)}, "
                          f"{tuple(target.shape)}")
    return target.shape[0], alast.shape[1]


def wd_head_fwd(alast, wp, wide, target, head=None):
    """Head forward in the cancelled form (pxr_wd_head_fwd_f32): alast [2 B, hl], wp [hl], wide [I], target int64 [B, 2] ->
    (loss [1], head [1 + 2 B] = loss | coef | x).  A bad target flags the status word (ops.raise_on_bad_indices) and is clamped."""
    B, hl = _wd_head_shapes(alast, wp, target, "widedeep head")
    _req(wide, torch.float32, "wide")
    head = _out_f32(head, (1 + 2 * B,), alast.device, "widedeep", "head")
    device_status(alast.device)
    _l.check(_l.load().pxr_wd_head_fwd_f32(_l.ptr(alast), _l.ptr(wp), _l.ptr(wide), wide.numel(), _l.ptr(target), B, hl,
                                           _l.ptr(head), _l.stream_ptr()), "pxr_wd_head_fwd_f32")
    return head[:1], head


def wd_head_bwd(alast, dact, wp, target, head, dwp, dbp, dwide, dwide_bias, grad_scale=1.0, grad_scale_dev=None, dz=None):
    """Head backward (pxr_wd_head_bwd_f32) -> dz [2 B, hl]; dwp [hl], dbp [1], dwide [I] (dense, zero off the targets) and
    dwide_bias [1] are written in place (the two biases exactly 0: they cancel in x_b)."""
    B, hl = _wd_head_shapes(alast, wp, target, "widedeep head backward")
    for t, n in ((dact, "dact"), (head, "head"), (dwp, "dwp"), (dbp, "dbp"), (dwide, "dwide"), (dwide_bias, "dwide_bias")):
        _req(t, torch.float32, n)
    if dact.shape != alast.shape or head.numel() != 1 + 2 * B or dwp.numel() != hl or dbp.numel() != 1 or dwide_bias.numel() != 1:
        raise _l.PxrError("widedeep head backward: dact must be [2 B, hl], head [1 + 2 B], dwp [hl], dbp / dwide_bias [1]")
    gsd = grad_scale_dev if grad_scale_dev is not None else torch.ones(1, dtype=torch.float32, device=alast.device)
    dz = _out_f32(dz, (2 * B, hl), alast.device, "widedeep", "dz")
    _l.check(_l.load().pxr_wd_head_bwd_f32(_l.ptr(alast), _l.ptr(dact), _l.ptr(wp), _l.ptr(target), dwide.numel(), _l.ptr(head), B, hl,
                                           float(grad_scale), _l.ptr(gsd), _l.ptr(dz), _l.ptr(dwp), _l.ptr(dbp), _l.ptr(dwide),
                                           _l.ptr(dwide_bias), _l.stream_ptr()), "pxr_wd_head_bwd_f32")
    return dz


WD_MAX_HIDDEN, WD_MAX_L = 128, 64


def wd_topk_supported(hidden, L: int, K: int = 10) -> bool:
    """Whether pxr_wd_topk_f32 takes this shape: one or two hidden layers of at most 128 units (the first a multiple of 4), L <= 64,
    K <= 32."""
    hidden = list(hidden)
    if len(hidden) not in (1, 2):
        return False
    h1, h2 = hidden[0], (hidden[1] if len(hidden) == 2 else 0)
    return int(_l.load().pxr_wd_topk_ws_bytes(1, int(L), 1, int(h1), int(h2), int(K))) >= 0 and (len(hidden) == 1 or h2 >= 1)


def wd_topk(T, hb, window, wide, wide_bias, w2, b2, wp, bp, K: int, hist_ptr=None, hist_items=None):
    """Fused WideDeep scoring + masks + top-K (pxr_wd_topk_f32): T [N, h1] = deep W1t^T + b1, hb [B, h1] = W1h xh_b, window int64
    [B, L] left-padded with 0, wide [N], wide_bias [1], w2 [h2, h1] / b2 [h2] or None (one hidden layer), wp [h_last], bp [1],
    hist_ptr int32 [B + 1] / hist_items int64 the CSR of the full histories.  Returns (topk_idx int64 [B, K], topk_val fp32 [B, K]).
    Bad ids flag the status word (ops.raise_on_bad_indices) and leave both outputs untouched."""
    Lb = _l.load()
    for t, n in ((T, "T"), (hb, "hb"), (wide, "wide"), (wide_bias, "wide_bias"), (wp, "wp"), (bp, "bp")):
        _req(t, torch.float32, n)
    _req(window, torch.int64, "window")
    if T.dim() != 2 or window.dim() != 2:
        raise _l.PxrError("widedeep top-k: T must be [N, h1] and window [B, L]")
    N, h1 = T.shape
    B, L = window.shape
    h2 = 0
    if w2 is not None:
        _req(w2, torch.float32, "w2"); _req(b2, torch.float32, "b2")
        h2 = w2.shape[0]
        if tuple(w2.shape) != (h2, h1) or b2.numel() != h2:
            raise _l.PxrError(f"widedeep top-k: w2 must be [h2, h1] = [{h2}, {h1}] and b2 [h2]")
    if tuple(hb.shape) != (B, h1) or wide.numel() != N or wide_bias.numel() != 1 or wp.numel() != (h2 or h1) or bp.numel() != 1:
        raise _l.PxrError(f"widedeep top-k: need hb [B, h1], wide [N], wp [h_last], wide_bias / bp [1] (B={B}, N={N}, h1={h1}, h2={h2})")
    _topk_hist_csr("widedeep top-k", hist_ptr, hist_items, B)
    ws_bytes = int(Lb.pxr_wd_topk_ws_bytes(B, L, N, h1, h2, K))
    if ws_bytes < 0:
        raise _l.PxrError(f"widedeep top-k: outside the fused limits (hidden widths up to 128, the first a multiple of 4, L <= 64, "
                          f"K <= 32): hidden=({h1}, {h2}), L={L}, K={K}")
    idx, val = _topk_out(B, K, T.device)
    ws = _ws.get(ws_bytes, T.device)
    _l.check(Lb.pxr_wd_topk_f32(_l.ptr(T), N, h1, _l.ptr(hb), _l.ptr(window), B, L, _l.ptr(wide), _l.ptr(wide_bias), _l.ptr(w2),
                                _l.ptr(b2), h2, _l.ptr(wp), _l.ptr(bp), _l.ptr(hist_ptr), _l.ptr(hist_items), K, _l.ptr(idx),
                                _l.ptr(val), _l.ptr(ws), ws_bytes, _l.stream_ptr()), "pxr_wd_topk_f32")
    return idx, val


# ------------------------------------------------------------------------------------------------ CNN-F: conv2d by im2col (csrc/conv2d.hip)
# An activation is a torch VIEW of logical shape [n, C, H, W] whose strides say where it lives: the image batch is NCHW-contiguous,
# a conv GEMM's [n Ho Wo, Cout] output is NHWC storage seen through .permute(0, 3, 1, 2).  The kernels take the four strides.
def conv2d_out_hw(H: int, W: int, kh: int, kw: int, sh: int, sw: int):
    """(Ho, Wo) of a padding-0, dilation-1 convolution (nn.Conv2d's floor rule); ValueError outside its domain."""
    if kh <= 0 or kw <= 0 or sh <= 0 or sw <= 0 or kh > H or kw > W:
        raise ValueError(f"conv2d: kernel {kh}x{kw} / stride {sh}x{sw} does not fit an input of {H}x{W}")
    return (H - kh) // sh + 1, (W - kw) // sw + 1


def conv2d_ldk(C: int, kh: int, kw: int) -> int:
    """Row length of the im2col matrix: K = C kh kw rounded up to a multiple of 4 floats (the GEMMs' leading dimensions)."""
    return (C * kh * kw + 3) // 4 * 4


def conv2d_chunk_images(n: int, rows_per_image: int, ldk: int, workspace_bytes: int) -> int:
    """Images per chunk under a byte budget for the column workspace: as many whole images as fit, at least one."""
    return max(1, min(int(n), int(workspace_bytes) // (4 * rows_per_image * ldk)))


_conv_ws: dict = {}


def _conv_workspace(numel: int, device):
    """Grow-only column workspace per (device, stream)."""
    key = (device, _l.raw_stream())
    b = _conv_ws.get(key)
    if b is None or b.numel() < numel:
        b = _conv_ws[key] = torch.empty(numel, dtype=torch.float32, device=device)
    return b


def _act(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _l.PxrError(f"{name}: expected a CUDA/HIP tensor (pixelrec_amd has no CPU fallback)")
    if t.dtype != torch.float32 or t.dim() != 4:
        raise _l.PxrError(f"{name}: expected a float32 [n, C, H, W] view, got {tuple(t.shape)} {t.dtype}")
    return t


def conv2d_im2col(x, kh: int, kw: int, sh: int, sw: int, col=None, ldk=None):
    """x [n, C, H, W] (any strides) -> col [n Ho Wo, ldk], columns in (c, kh, kw) order, pad columns +0.0 (pxr_conv2d_im2col_f32;
    dvbpr.py:113-114).  Bad geometry raises PxrError from the entry, without a launch."""
    _act(x, "conv2d im2col: x")
    n, C, H, W = x.shape
    ldk = conv2d_ldk(C, kh, kw) if ldk is None else int(ldk)
    if col is None:
        Ho, Wo = conv2d_out_hw(H, W, kh, kw, sh, sw)
        col = torch.empty(n * Ho * Wo, ldk, dtype=torch.float32, device=x.device)
    _req(col, torch.float32, "col")
    sane = kh > 0 and kw > 0 and sh > 0 and sw > 0 and kh <= H and kw <= W and ldk > 0
    if sane and col.numel() != n * ((H - kh) // sh + 1) * ((W - kw) // sw + 1) * ldk:
        raise _l.PxrError(f"conv2d im2col: col holds {col.numel()} floats, the geometry needs [n Ho Wo, ldk] with ldk={ldk}")
    _l.check(_l.load().pxr_conv2d_im2col_f32(_l.ptr(x), *x.stride(), n, C, H, W, kh, kw, sh, sw, _l.ptr(col), ldk, _l.stream_ptr()),
             "pxr_conv2d_im2col_f32")
    return col


def conv2d_col2im(dcol, dx, kh: int, kw: int, sh: int, sw: int, ldk=None):
    """dcol [n Ho Wo, ldk] -> dx [n, C, H, W] (a view; written whole through its strides): the data gradient in gather form, kh outer,
    kw inner, +0.0 where no window covers an element (pxr_conv2d_col2im_f32)."""
    _act(dx, "conv2d col2im: dx")
    _req(dcol, torch.float32, "dcol")
    n, C, H, W = dx.shape
    ldk = conv2d_ldk(C, kh, kw) if ldk is None else int(ldk)
    sane = kh > 0 and kw > 0 and sh > 0 and sw > 0 and kh <= H and kw <= W and ldk > 0
    if sane and dcol.numel() != n * ((H - kh) // sh + 1) * ((W - kw) // sw + 1) * ldk:
        raise _l.PxrError(f"conv2d col2im: dcol holds {dcol.numel()} floats, the geometry needs [n Ho Wo, ldk] with ldk={ldk}")
    _l.check(_l.load().pxr_conv2d_col2im_f32(_l.ptr(dcol), ldk, n, C, H, W, kh, kw, sh, sw, _l.ptr(dx), *dx.stride(), _l.stream_ptr()),
             "pxr_conv2d_col2im_f32")
    return dx


def maxpool2x2_fwd(y, chw: bool = False):
    """nn.MaxPool2d(2) over y [n, C, H, W] (a view) -> p [n, C, H // 2, W // 2]: NHWC storage seen as [n, C, Hp, Wp], or with chw=True
    NCHW-contiguous -- the (c, h, w) order fcs.0 reads (pxr_maxpool2x2_fwd_f32; dvbpr.py:129-132)."""
    _act(y, "maxpool: y")
    n, C, H, W = y.shape
    Hp, Wp = H // 2, W // 2
    if chw:
        p = torch.empty(n, C, max(Hp, 0), max(Wp, 0), dtype=torch.float32, device=y.device)
    else:
        p = torch.empty(n, max(Hp, 0), max(Wp, 0), C, dtype=torch.float32, device=y.device).permute(0, 3, 1, 2)
    _l.check(_l.load().pxr_maxpool2x2_fwd_f32(_l.ptr(y), *y.stride(), n, C, H, W, _l.ptr(p), *p.stride(), _l.stream_ptr()),
             "pxr_maxpool2x2_fwd_f32")
    return p


def maxpool2x2_relu_bwd(y, dp):
    """The pool's backward fused with the mask of the ReLU in front of it: y [n, C, H, W] = the ReLU'd conv output that was pooled, dp
    [n, C, H // 2, W // 2] (a view) -> dy with y's strides; first maximum wins, dropped rows / columns +0.0
    (pxr_maxpool2x2_relu_bwd_f32)."""
    _act(y, "maxpool backward: y"); _act(dp, "maxpool backward: dp")
    n, C, H, W = y.shape
    if tuple(dp.shape) != (n, C, H // 2, W // 2):
        raise _l.PxrError(f"maxpool backward: dp must be {(n, C, H // 2, W // 2)}, got {tuple(dp.shape)}")
    dy = torch.empty_strided(y.shape, y.stride(), dtype=torch.float32, device=y.device)
    _l.check(_l.load().pxr_maxpool2x2_relu_bwd_f32(_l.ptr(y), *y.stride(), _l.ptr(dp), *dp.stride(), n, C, H, W, _l.ptr(dy),
                                                   _l.stream_ptr()), "pxr_maxpool2x2_relu_bwd_f32")
    return dy


def _conv_operands(who, x, Wp, kh, kw):
    _act(x, f"{who}: x"); _req(Wp, torch.float32, "Wp")
    n, C, H, W = x.shape
    if Wp.dim() != 2 or Wp.shape[1] != conv2d_ldk(C, kh, kw) or Wp.shape[0] % 4:
        raise _l.PxrError(f"{who}: the weight operand must be [Cout, {conv2d_ldk(C, kh, kw)}] (K = C kh kw = {C * kh * kw} padded to a "
                          f"multiple of 4, pad columns zero) with Cout % 4 == 0, got {tuple(Wp.shape)}")
    return n, C, H, W, Wp.shape[0], Wp.shape[1]


def conv2d_relu_fwd(x, Wp, b, kh: int, kw: int, sh: int, sw: int, workspace_bytes: int = 1 << 30, save_der: bool = False):
    """relu(conv2d(x, W, b)) as chunks of whole images through im2col + the library GEMM with the bias + ReLU epilogue
    (dvbpr.py:127).  x [n, C, H, W] (a view); Wp [Cout, ldk] = weight.view(Cout, K) with K padded to a multiple of 4 by zero
    columns; the chunk size is the number of whole images whose columns fit workspace_bytes (at least one).  -> (y, der): y
    [n, Cout, Ho, Wo] as a view of NHWC storage, der = relu'(pre-activation) in the same layout when save_der (the activation
    epilogue's own second output), else None."""
    n, C, H, W, Cout, ldk = _conv_operands("conv2d forward", x, Wp, kh, kw)
    Ho, Wo = conv2d_out_hw(H, W, kh, kw, sh, sw)
    R = Ho * Wo
    per = conv2d_chunk_images(n, R, ldk, workspace_bytes)
    ws = _conv_workspace(per * R * ldk, x.device)
    y = der = None
    if not save_der or per < n:
        y = torch.empty(n, Ho, Wo, Cout, dtype=torch.float32, device=x.device)
        der = torch.empty_like(y) if save_der else None
    for i0 in range(0, n, per):
        m = min(per, n - i0)
        col = conv2d_im2col(x[i0:i0 + m], kh, kw, sh, sw, ws[:m * R * ldk].view(m * R, ldk), ldk)
        if save_der:
            yc, dc = linear_fwd(col, Wp, b, act="relu")
            if per >= n:
                y, der = yc.view(n, Ho, Wo, Cout), dc.view(n, Ho, Wo, Cout)
            else:
                y[i0:i0 + m].view(m * R, Cout).copy_(yc)
                der[i0:i0 + m].view(m * R, Cout).copy_(dc)
        else:
            gemm(True, True, m * R, Cout, ldk, col, ldk, Wp, ldk, y[i0:i0 + m], Cout, EPI_BIAS_RELU, bias=b, use_ws=False)
    return y.permute(0, 3, 1, 2), (der.permute(0, 3, 1, 2) if der is not None else None)


def conv2d_bwd(dz, x, Wp, kh: int, kw: int, sh: int, sw: int, dWp, db, workspace_bytes: int = 1 << 30, need_dx: bool = True):
    """Backward of conv2d_relu_fwd from dz [n, Cout, Ho, Wo] (a view of NHWC storage) = the gradient at the pre-activation.  Per chunk
    of whole images: im2col recomputed from the saved input x; dW = dz^T col and db = the column sums of dz (one grouped
    weight-gradient launch), added over the chunks IN CHUNK ORDER (pxr_add_f32); dcol = dz W into the same workspace; col2im.
    dWp [Cout, ldk] and db [Cout] are overwritten.  -> dx [n, C, H, W] as a view of NHWC storage, or None (need_dx=False: the
    first layer, whose input is the image)."""
    n, C, H, W, Cout, ldk = _conv_operands("conv2d backward", x, Wp, kh, kw)
    Ho, Wo = conv2d_out_hw(H, W, kh, kw, sh, sw)
    R = Ho * Wo
    _act(dz, "conv2d backward: dz")
    dzm = dz.permute(0, 2, 3, 1)
    if tuple(dz.shape) != (n, Cout, Ho, Wo) or not dzm.is_contiguous():
        raise _l.PxrError(f"conv2d backward: dz must be {(n, Cout, Ho, Wo)} over NHWC storage, got {tuple(dz.shape)} strides {dz.stride()}")
    dzm = dzm.reshape(n * R, Cout)
    _req(dWp, torch.float32, "dWp"); _req(db, torch.float32, "db")
    if tuple(dWp.shape) != (Cout, ldk) or db.numel() != Cout:
        raise _l.PxrError(f"conv2d backward: dWp must be [{Cout}, {ldk}] and db [{Cout}]")
    per = conv2d_chunk_images(n, R, ldk, workspace_bytes)
    ws = _conv_workspace(per * R * ldk, x.device)
    dx = torch.empty(n, H, W, C, dtype=torch.float32, device=x.device).permute(0, 3, 1, 2) if need_dx else None
    tW = tb = None
    for i0 in range(0, n, per):
        m = min(per, n - i0)
        col = conv2d_im2col(x[i0:i0 + m], kh, kw, sh, sw, ws[:m * R * ldk].view(m * R, ldk), ldk)
        dy = dzm[i0 * R:(i0 + m) * R]
        if i0 == 0:
            grouped_linear_bwd_weight([(dy, col, dWp, db)])
        else:
            if tW is None:
                tW, tb = torch.empty_like(dWp), torch.empty_like(db)
            grouped_linear_bwd_weight([(dy, col, tW, tb)])
            dWp.copy_(add(dWp, tW))
            db.copy_(add(db, tb))
        if need_dx:
            linear_bwd_input(dy, Wp, out=col)                       # dcol = dz W, over the columns it was computed from
            conv2d_col2im(col, dx[i0:i0 + m], kh, kw, sh, sw, ldk)
    return dx


# ------------------------------------------------------------------------------------------------ DVBPR (csrc/dvbpr.hip)
def dvbpr_rows(user, item_id, index, n_users: int, n_items: int, n_rows: int, out=None):
    """user int64 [B], item_id int64 [B, 2] | None, index int64 [B, 2] | None -> rows int64 [6B] = [gamma row of user | theta row of
    user | gamma rows of item_id.view(-1) | positions index.view(-1) into E [n_rows, Dh], base 0] of the [1 + 2U + I, Dh] table
    (theta_users at 1, gamma_users at 1 + U, gamma_items at 1 + 2U); the 2B user rows alone in evaluation.  Bad ids flag the status
    word and are clamped."""
    B = user.numel()
    _pair_items("dvbpr rows", item_id, B)
    _pair_items("dvbpr rows", index, B)
    return _table_rows("dvbpr rows", [("user", user, n_users, 1 + n_users, 0), ("user", user, n_users, 1, 0),
                                      ("item_id", item_id, n_items, 1 + 2 * n_users, 0), ("index", index, n_rows, 0, 0)], out,
                       (6 * B if item_id is not None else 2 * B,))


def dvbpr_pair_fwd(table, rows, E, B: int, out=None):
    """DVBPR's pair loss head (dvbpr.py:49-62; pxr_dvbpr_pair_fwd_f32) on the table rows and positions of rows [6B] and the encoder's
    output E [M, Dh] -> (loss [1], coef [B]).  out: a float32 [2B + 1] buffer to reuse."""
    _req(table, torch.float32, "table"); _req(rows, torch.int64, "rows"); _req(E, torch.float32, "E")
    Dh = table.shape[1]
    if rows.numel() != 6 * B or E.dim() != 2 or E.shape[1] != Dh:
        raise _l.PxrError(f"dvbpr pair head: need rows [6B] and E [M, Dh] for B={B}, Dh={Dh}")
    f = out if out is not None else torch.empty(2 * B + 1, dtype=torch.float32, device=table.device)
    coef, lossrow, loss = f[:B], f[B:2 * B], f[2 * B:]
    _l.check(_l.load().pxr_dvbpr_pair_fwd_f32(_l.ptr(table), _l.ptr(rows), _l.ptr(E), Dh, B, _l.ptr(coef), _l.ptr(lossrow), _l.ptr(loss),
                                              _l.stream_ptr()), "pxr_dvbpr_pair_fwd_f32")
    return loss, coef


def dvbpr_pair_bwd(table, rows, E, coef, B: int, sp: SparseRows, grad_scale=1.0, grad_scale_dev=None, dE=None):
    """Its backward (pxr_dvbpr_pair_bwd_f32): the three tables' gradient as sparse rows into sp (cap >= 4B) and d loss / d E [M, Dh]
    dense, every row written (position 0 included), in a fixed summation order.  -> dE."""
    _req(table, torch.float32, "table"); _req(rows, torch.int64, "rows"); _req(E, torch.float32, "E"); _req(coef, torch.float32, "coef")
    Dh = table.shape[1]
    if rows.numel() != 6 * B or E.dim() != 2 or E.shape[1] != Dh or coef.numel() != B or sp.rows.shape[1] != Dh or sp.cap < 4 * B:
        raise _l.PxrError(f"dvbpr pair head backward: need rows [6B], E [M, Dh], coef [B], sparse rows Dh wide with >= 4B slots "
                          f"for B={B}, Dh={Dh}")
    dE = dE if dE is not None else torch.empty_like(E)
    _req(dE, torch.float32, "dE")
    if dE.shape != E.shape:
        raise _l.PxrError(f"dvbpr pair head backward: dE must be {tuple(E.shape)}, got {tuple(dE.shape)}")
    _l.check(_l.load().pxr_dvbpr_pair_bwd_f32(_l.ptr(table), _l.ptr(rows), _l.ptr(E), E.shape[0], _l.ptr(coef), Dh, B, float(grad_scale),
                                              _l.ptr(grad_scale_dev), _l.ptr(dE), _l.ptr(sp.idx), _l.ptr(sp.rows), _l.ptr(sp.n),
                                              sp.cap, _l.stream_ptr()), "pxr_dvbpr_pair_bwd_f32")
    return dE
