"""TEST INFRASTRUCTURE ONLY -- float64 restatements of the small element-wise kernels (csrc/gru.hip, conv1d.hip, pixel.hip, the
small kernels of vit.hip) and the deterministic case builders that tests/test_small_kernels_cpu.py (no GPU) and
tests/test_gpu_small_kernels.py share.  Everything here is written from the formulas in the kernels' header comments; nothing
calls the library, and nothing imports a GPU module.

Each of those kernels is a grid-stride loop behind a clamped grid: past `cap blocks * 256` work items every thread makes a second
trip.  The caps are kept here as named constants, one per launch helper; every case called "past the cap" is checked against its
constant on the CPU (test_small_kernels_cpu.py::test_every_past_the_cap_case_exceeds_its_cap), so changing a clamp fails there
instead of silently taking the second trip out of the GPU tests."""
import numpy as np
import torch

from oracle import dropout_rng

U24 = 2.0 ** -24                    # unit roundoff of float32

# work items one launch covers in the FIRST trip of its grid-stride loop (blocks of 256 threads)
GRU_CAP = 4096 * 256                # csrc/gru.hip `gru_grid`: `b > 4096 ? 4096 : b`, one thread per [B, H] element
C1D_CAP = 8192 * 256                # csrc/conv1d.hip `c1d_grid`: `b > 8192 ? 8192 : b`, im2col: per xcol element, col2im: per dx element
EMB_GRAD_CAP = 4096 * 256           # csrc/pixel.hip pxr_mosasrec_emb_grad_f32: `if (blocks > 4096) blocks = 4096`, per float4 of d_emb
IMAGE_CAP = 8192 * 256              # csrc/pixel.hip pxr_image_u8_to_f32: `if (blocks > 8192) blocks = 8192`, per output element
VIT_CAP = 256 * 16 * 256            # csrc/vit.hip `grid_for`: `if (b > 256 * 16) b = 256 * 16`, per float4 (token_mean: per output float4)
GATHER_BLOCK = 4 * 256              # csrc/embed_gather.hip default variant: U = 4 chunks per lane, 256 lanes (no cap: one trip)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------ GRU gates
def gru_fwd(gi, gh, h_prev=None):
    """gi, gh [B, 3H] (r | z | n), h_prev [B, H] | None (= zeros) -> h [B, H], save [B, 4H] = r | z | n | gh_n, all float64:
    r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r gh_n), h = (1 - z) n + z h_prev."""
    gi, gh = gi.double(), gh.double()
    H = gi.shape[1] // 3
    hp = torch.zeros(gi.shape[0], H, dtype=torch.float64) if h_prev is None else h_prev.double()
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    ghn = gh[:, 2 * H:]
    n = torch.tanh(gi[:, 2 * H:] + r * ghn)
    return (1.0 - z) * n + z * hp, torch.cat([r, z, n, ghn], dim=1)


def gru_bwd(dh, save, h_prev=None):
    """dh [B, H], save [B, 4H], h_prev [B, H] | None -> dgi, dgh [B, 3H], dh_prev [B, H] (the direct path), float64:
    da_n = dh (1 - z)(1 - n^2), da_z = dh (h_prev - n) z (1 - z), da_r = da_n gh_n r (1 - r);
    dgi = [da_r | da_z | da_n], dgh = [da_r | da_z | da_n r], dh_prev = dh z."""
    dh, save = dh.double(), save.double()
    H = dh.shape[1]
    hp = torch.zeros_like(dh) if h_prev is None else h_prev.double()
    r, z, n, ghn = (save[:, i * H:(i + 1) * H] for i in range(4))
    dan = dh * (1.0 - z) * (1.0 - n * n)
    daz = dh * (hp - n) * z * (1.0 - z)
    dar = dan * ghn * r * (1.0 - r)
    return torch.cat([dar, daz, dan], dim=1), torch.cat([dar, daz, dan * r], dim=1), dh * z


def gru_bwd_autograd(dh, gi, gh, h_prev=None):
    """The same three gradients by differentiating gru_fwd (float64 autograd)."""
    gi = gi.double().clone().requires_grad_(True)
    gh = gh.double().clone().requires_grad_(True)
    B, H = gi.shape[0], gi.shape[1] // 3
    hp = (torch.zeros(B, H, dtype=torch.float64) if h_prev is None else h_prev.double().clone()).requires_grad_(True)
    h, _ = gru_fwd(gi, gh, hp)
    dgi, dgh, dhp = torch.autograd.grad(h, (gi, gh, hp), grad_outputs=dh.double())
    return dgi, dgh, dhp


GRU_SHAPES = ((1, 4), (3, 5), (7, 260), (1028, 1021))       # (B, H); the last is past GRU_CAP, H odd on purpose
GRU_PAST_CAP = (1028, 1021)


def gru_case(B, H, seed=11):
    """Ordinary pre-activations: float32 N(0, 1) gi, gh, h_prev, dh."""
    g = _gen(seed + 1000 * B + H)
    return {"gi": torch.randn(B, 3 * H, generator=g), "gh": torch.randn(B, 3 * H, generator=g),
            "h_prev": torch.randn(B, H, generator=g), "dh": torch.randn(B, H, generator=g)}


SATURATION_VALUES = (0.0, 20.0, -20.0, 90.0, -90.0, 200.0, -200.0)


def gru_saturation_case(H=4, seed=12):
    """One row per (gate column r | z | n, value v): that gate's pre-activation is v in every column of the row, the others are
    ordinary.  r and z: gi = gh = v / 2 (their float32 sum is exactly v); n: gi_n = v with an ordinary gh_n, and a second row
    with gi_n = 0, gh_n = v (the pre-activation is then r v).  -> the gru_case dict plus "rows": [(gate, v, which)]."""
    rows = [(gate, v, "gi") for gate in range(3) for v in SATURATION_VALUES] + [(2, v, "gh") for v in SATURATION_VALUES]
    c = gru_case(len(rows), H, seed)
    for i, (gate, v, which) in enumerate(rows):
        cols = slice(gate * H, (gate + 1) * H)
        if gate < 2:
            c["gi"][i, cols] = v / 2
            c["gh"][i, cols] = v / 2
        elif which == "gi":
            c["gi"][i, cols] = v
        else:
            c["gi"][i, cols] = 0.0
            c["gh"][i, cols] = v
    c["rows"] = rows
    return c


# ------------------------------------------------------------------------------------------- causal im2col / col2im
def causal_im2col(x, k, d):
    """x [B, L, C] -> xcol [B, L, C k] with xcol[b, t, c k + j] = x[b, t - (k-1-j) d, c] (0 left of the sequence); a pure move, in
    x's dtype."""
    B, L, C = x.shape
    out = x.new_zeros(B, L, C, k)
    for j in range(k):
        s = (k - 1 - j) * d
        if s < L:
            out[:, s:, :, j] = x[:, :L - s]
    return out.reshape(B, L, C * k)


def causal_col2im(dxcol, k, d):
    """The transpose map: dx[b, t, c] = sum_j dxcol[b, t + (k-1-j) d, c k + j] (positions beyond L contribute nothing), the taps
    summed in float64."""
    B, L, Ck = dxcol.shape
    y = dxcol.double().view(B, L, Ck // k, k)
    dx = torch.zeros(B, L, Ck // k, dtype=torch.float64)
    for j in range(k):
        s = (k - 1 - j) * d
        if s < L:
            dx[:, :L - s] += y[:, s:, :, j]
    return dx


def causal_col2im_abs(dxcol, k, d):
    """sum_j |term| of the same sum: the scale of col2im's derived rounding bound."""
    return causal_col2im(dxcol.abs(), k, d)


C1D_SMALL = ((1, 1, 4, 3, 4), (2, 5, 4, 1, 1), (2, 5, 4, 2, 8), (3, 7, 9, 4, 2))       # (B, L, C, k, d)
IM2COL_PAST_CAP = (37, 19, 1000, 3, 4)          # B L C k = 2 109 000 xcol elements
COL2IM_PAST_CAP = (111, 19, 1000, 3, 4)         # B L C   = 2 109 000 dx elements


def im2col_case(shape, seed=21):
    B, L, C, k, d = shape
    return torch.randn(B, L, C, generator=_gen(seed + B * L * C + k))


def col2im_case(shape, integers=True, seed=22):
    """dxcol [B, L, C k]: integer-valued in [-8, 8] (every partial sum is exact in float32) or Gaussian."""
    B, L, C, k, d = shape
    g = _gen(seed + B * L * C + k)
    if integers:
        return torch.randint(-8, 9, (B, L, C * k), generator=g).float()
    return torch.randn(B, L, C * k, generator=g)


# ---------------------------------------------------------------------------------------------------- image transform
def image_u8_to_f64(store, ids):
    """store uint8 [n_store, H, W, 3], ids int64 [...] -> float64 [..., 3, H, W] = (u8 / 255 - 0.5) / 0.5 in CHW order; id 0 (the
    pad image) and ids outside [0, n_store) give zeros."""
    n_store = store.shape[0]
    ok = (ids > 0) & (ids < n_store)
    img = store[torch.where(ok, ids, torch.zeros_like(ids))].double()           # [..., H, W, 3]
    out = ((img / 255.0 - 0.5) / 0.5).movedim(-1, -3)
    return torch.where(ok[..., None, None, None], out, torch.zeros((), dtype=torch.float64))


IMAGE_SHAPES = ((7, 16, 12, (2, 3)), (23, 37, 29, (652,)))      # (n_store, H, W, ids shape); the second is past IMAGE_CAP
IMAGE_PAST_CAP = IMAGE_SHAPES[1]


def image_case(n_store, H, W, ids_shape, seed=31):
    g = _gen(seed + n_store)
    store = torch.randint(0, 256, (n_store, H, W, 3), generator=g, dtype=torch.uint8)
    ids = torch.randint(1, n_store, ids_shape, generator=g)
    flat = ids.view(-1)
    flat[0], flat[1], flat[-1] = n_store - 1, 0, n_store - 1        # the last stored image (twice), the pad image
    flat[2] = flat[3]                                               # and a repeat next to itself
    return store, ids


# ------------------------------------------------------------------------------------------------ mosasrec_emb_grad
def mosasrec_emb_grad(dx0, out, coef):
    """dx0, out [B, L, D], coef [B, L] -> d_emb [B, L+1, 2, D] in float64:
    d_emb[b, t, 0] = [t < L] dx0[b, t] + [t >= 1] coef[b, t-1] out[b, t-1];   d_emb[b, t, 1] = -[t >= 1] coef[b, t-1] out[b, t-1]."""
    dx0, out, coef = dx0.double(), out.double(), coef.double()
    B, L, D = out.shape
    d = torch.zeros(B, L + 1, 2, D, dtype=torch.float64)
    for b in range(B):
        for t in range(L + 1):
            if t < L:
                d[b, t, 0] += dx0[b, t]
            if t >= 1:
                d[b, t, 0] += coef[b, t - 1] * out[b, t - 1]
                d[b, t, 1] -= coef[b, t - 1] * out[b, t - 1]
    return d


def mosasrec_emb_grad_scale(dx0, out, coef):
    """|dx0 term| + |coef out term| of every element: the scale of the kernel's derived rounding bound."""
    return mosasrec_emb_grad(dx0.abs(), out.abs(), coef.abs()).abs()


EMB_GRAD_SHAPES = ((1, 1, 4), (3, 5, 8), (64, 7, 4100))         # (B, L, D); the last is past EMB_GRAD_CAP
EMB_GRAD_PAST_CAP = (64, 7, 4100)
EMB_GRAD_SENTINEL = 1.0e30


def emb_grad_case(B, L, D, seed=41):
    """dx0 is a [B, L, D] view of a buffer ONE ROW TOO LONG whose last row holds EMB_GRAD_SENTINEL: a kernel that reads a dx0 row
    for t = L reads the next sequence's first row or, for the last sequence, the sentinel."""
    g = _gen(seed + B * L + D)
    buf = torch.randn(B * L + 1, D, generator=g)
    buf[B * L] = EMB_GRAD_SENTINEL
    return {"dx0_buf": buf, "out": torch.randn(B, L, D, generator=g), "coef": torch.randn(B, L, generator=g)}


def emb_grad_dx0(buf, B, L):
    """The [B, L, D] view of emb_grad_case's "dx0_buf" (on whatever device it lives)."""
    return buf[:B * L].view(B, L, -1)


# ------------------------------------------------------------------------------------------------- ViT small kernels
def vit_embed(patches, cls, pos):
    """patches [n, T-1, H], cls [H], pos [T, H] -> [n, T, H] = [cls | patches] + pos (one addition per element: in the inputs'
    dtype this is the kernel's own arithmetic)."""
    n = patches.shape[0]
    return torch.cat([cls.expand(n, 1, -1), patches], dim=1) + pos[None]


def token_mean(x):
    """x [n, T, D] -> float64 [n, D], the mean over the T tokens."""
    return x.double().sum(1) / x.shape[1]


def token_mean_relu_bwd(dout, act):
    """dact[n, t, :] = act[n, t, :] > 0 ? dout[n, :] * (1 / T) : 0 in the inputs' dtype (in float32: one rounded reciprocal and one
    rounded product, the kernel's own arithmetic)."""
    inv = torch.ones((), dtype=dout.dtype) / torch.tensor(float(act.shape[1]), dtype=dout.dtype)
    return torch.where(act > 0, (dout * inv)[:, None, :].expand_as(act), torch.zeros((), dtype=dout.dtype))


def add(a, b):
    return a + b


VIT_TINY = (5, 17, 64)                          # (n, T, H), the shape of tests/test_gpu_vit.py
VIT_EMBED_PAST_CAP = (41, 50, 2048)             # n T H/4 = 1 049 600 float4
TOKEN_MEAN_PAST_CAP = (2049, 3, 2052)           # n D/4   = 1 051 137 output float4
ADD_TINY = 1000
ADD_PAST_CAP = 4 * 1048577                      # n / 4   = 1 048 577 float4


def vit_case(n, T, H, seed=51):
    g = _gen(seed + n * T + H)
    return {"patches": torch.randn(n, T - 1, H, generator=g), "cls": torch.randn(H, generator=g),
            "pos": torch.randn(T, H, generator=g), "act": torch.randn(n, T, H, generator=g), "dout": torch.randn(n, H, generator=g)}


def token_mean_case(n, T, D, seed=52):
    return torch.randn(n, T, D, generator=_gen(seed + n * T + D))


def flat_case(n, seed=53):
    g = _gen(seed + n)
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


# --------------------------------------------------------------------------------------------------------------- dropout
def dropout_keep(n, p, seed, stream_id, step=None):
    """The keep mask of ops.dropout over the flat element index: oracle/dropout_rng.keep_mask with the seed advanced by the
    completed-step counter (csrc/vit.hip: `seed += step_dev[0]`, modulo 2^64)."""
    s = (int(seed) + (0 if step is None else int(step))) & 0xFFFFFFFFFFFFFFFF
    return torch.from_numpy(dropout_rng.keep_mask(s, stream_id, (n,), p))


def dropout(x, p, seed, stream_id, step=None):
    """x / (1 - p) where kept, else 0, in float64."""
    keep = dropout_keep(x.numel(), p, seed, stream_id, step).view(x.shape)
    return torch.where(keep, x.double() / (1.0 - float(np.float32(p))), torch.zeros((), dtype=torch.float64))


def dropout_inv_keep_f32(p):
    """1 / (1 - p) as the library forms it: float32 throughout."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


DROPOUT_SEED, DROPOUT_STREAM, DROPOUT_STEP = 0x1234567, 7, 5


# ------------------------------------------------------------------------------------------------------- embed_gather
GATHER_CHUNKS = (1, 255, 1023, 1024, 1025, 4 * 1024 + 3)       # n D / 4 around the 1024-chunk block of the default variant
GATHER_DIMS = (4, 12, 1028)


def gather_case(chunks, D, seed=61):
    """-> table [N, D], idx [n] with n = ceil(chunks / (D / 4)) rows (exactly `chunks` float4 for D = 4, the nearest whole row count
    at or above it otherwise); ids repeat and include 0 and N - 1."""
    dv = D // 4
    n = -(-chunks // dv)
    N = 37
    g = _gen(seed + chunks + D)
    table = torch.randn(N, D, generator=g)
    idx = torch.randint(0, N, (n,), generator=g)
    idx[0] = N - 1
    if n > 1:
        idx[-1] = 0
    if n > 3:
        idx[1], idx[2] = idx[3], N - 1
    return table, idx
