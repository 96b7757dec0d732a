"""Cases and the float64 reference of ops.score_topk's threshold schedule (csrc/score_topk.hip: sample pass, tau kernel, one of the
five main-pass kernels, candidate merge or exact re-scoring) for tests/test_score_topk_cases.py (no GPU) and
tests/test_gpu_score_topk_ref.py.  Nothing here imports the library; the launcher's rules that the CPU tests need (which tiles the
sample pass scores, the threshold margin of the reduced-product passes) are restated from the source, in float64.

Every catalogue has at least 65 409 items (512 tiles of 128: the smallest that leaves the register lists).  A random history item
is practically never a top-K item, so a kernel that dropped a mask would change no output; hence
  * rows 1..384 of the table (the "hot block") are scaled by 1.6.  They lie in the first workgroup's item range of every main-pass
    kernel ([0, 384) on 128-item tiles, [0, 768) on 256-item tiles) and in sampled tile 0, and hold a fifth to a third of all
    top-K cells;
  * every user gets 0-39 random items; users with an even index also their own float64 top-min(K, 1 + u % 5) items; users 0-63 also
    64 distinct random items of the hot block each -- 4096 pairs in one workgroup's range, more than the 2048 its LDS list holds
    (ST4_HIST_CAP), so that workgroup walks the global pairs; user 2 also item 0 and one item three times; user 3 also items on
    the tile borders.
s64 = users.double() @ table.double().T with column 0 and every history pair at -inf."""
import math
from types import SimpleNamespace

import torch

HOT = 384                                        # items 1..HOT are the hot block
HOT_SCALE = 1.6
HOT_USERS, HOT_PER_USER = 64, 64                 # users 0..63 mask 64 hot items each
HIST_CAP = 2048                                  # ST4_HIST_CAP (topk_select.cuh)
CAND_CAP = 4096                                  # ST4_CAP (score_topk.hip)
RESCORE_INREG = 2048                             # 64 * RS_CPL: more candidates leave the registers of topk_rescore_kernel
TILE = 128
MIN_N = 512 * TILE - TILE + 1                    # 65 409: exactly ST4_MIN_TILES tiles, one item in the last

# name -> (B, N, D, K, seed)
SHAPES = {
    "min_n": (257, MIN_N, 32, 10, 101),
    "ragged": (257, 65_601, 64, 10, 102),
    "k16": (130, 65_601, 64, 16, 103),
    "k32": (130, 65_601, 96, 32, 104),
    "k17_noplanes": (130, MIN_N, 36, 17, 105),
    "k1": (130, MIN_N, 32, 1, 106),
    "wide": (5, MIN_N, 1056, 10, 107),
}
CROWD = (64, 70_016, 64, 10, 108)
CROWD_DUP, CROWD_MASKED = 3000, 20
CASES = list(SHAPES) + ["strided", "crowd", "one_user"]
STRIDED_B = 130


def border_items(N):
    return [127, 128, 255, 256, min(65_535, N - 2), N - 2, N - 1]


def masked_scores(users, table, hist):
    s = users.double() @ table.double().t()
    s[:, 0] = float("-inf")
    for u, h in enumerate(hist):
        if h:
            s[u, torch.tensor(h, dtype=torch.int64)] = float("-inf")
    return s


def tol_abs(s64, D):
    """the bound tests/test_gpu_gemm.py::_check holds every GEMM to"""
    return 2e-6 * math.sqrt(D) * float(s64[torch.isfinite(s64)].abs().max()) + 1e-6


def _built(B, N, D, K, seed):
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(N, D, generator=g) * 0.02
    table[1:HOT + 1] *= HOT_SCALE
    users = torch.randn(B, D, generator=g)
    raw = users.double() @ table.double().t()
    raw[:, 0] = float("-inf")
    top = torch.topk(raw, min(K, 5), dim=-1).indices
    hist, own_top = [], []
    for u in range(B):
        n = int(torch.randint(0, 40, (1,), generator=g))
        h = torch.randint(1, N, (n,), generator=g).tolist()
        mine = top[u, :min(K, 1 + u % 5)].tolist() if u % 2 == 0 else []
        h += mine
        if u < HOT_USERS:
            h += (torch.randperm(HOT, generator=g)[:HOT_PER_USER] + 1).tolist()
        if u == 2:
            d = int(torch.randint(1, N, (1,), generator=g))
            h += [0, d, d, d]
        if u == 3:
            h += border_items(N)
        hist.append(h)
        own_top.append(mine)
    return SimpleNamespace(B=B, N=N, D=D, K=K, users=users, table=table, hist=hist, own_top=own_top, ld_users=D,
                           s64=masked_scores(users, table, hist), crowd=None)


def _crowd():
    """tests/test_gpu_stress.py's construction: CROWD_DUP catalogue rows identical to user 0's direction, every user nearly user 0.
    User 0's history is the CROWD_MASKED lowest duplicate ids."""
    B, N, D, K, seed = CROWD
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(N, D, generator=g) * 0.05
    users = torch.randn(B, D, generator=g)
    dup = torch.sort(torch.randperm(N - 1, generator=g)[:CROWD_DUP] + 1).values
    table[dup] = users[0] * 0.5
    users = users[0] + 0.01 * torch.randn(B, D, generator=g)
    hist = [dup[:CROWD_MASKED].tolist()] + [[] for _ in range(B - 1)]
    return SimpleNamespace(B=B, N=N, D=D, K=K, users=users, table=table, hist=hist, own_top=[[] for _ in range(B)], ld_users=D,
                           s64=masked_scores(users, table, hist), crowd=dup.tolist())


def _cut(c, B):
    return SimpleNamespace(B=B, N=c.N, D=c.D, K=c.K, users=c.users[:B].clone(), table=c.table, hist=[list(h) for h in c.hist[:B]],
                           own_top=[list(h) for h in c.own_top[:B]], ld_users=c.D, s64=c.s64[:B].clone(), crowd=None)


def case(name):
    """-> namespace: B, N, D, K, users [B, D] (a view of row stride ld_users for "strided"), table [N, D], hist (B lists), s64 [B, N]
    float64, own_top (the float64 top items each even user masks), crowd (the duplicate ids, or None)"""
    if name == "crowd":
        return _crowd()
    if name == "strided":
        c = _cut(_built(*SHAPES["ragged"]), STRIDED_B)
        wide = torch.full((c.B, 2 * c.D), float("nan"))             # what lies between the rows is never read
        wide[:, :c.D] = c.users
        c.users, c.ld_users = wide[:, :c.D], 2 * c.D
        return c
    if name == "one_user":
        return _cut(_built(*SHAPES["ragged"]), 1)
    return _built(*SHAPES[name])


# ---- the launcher, restated ---------------------------------------------------------------------------------------------------
def sampled_tiles(N, K):
    """the 128-item tiles that the sample pass scores (score_topk_thresh: st4_stride, sample_splits, tile_stride)"""
    kt = 10 if K <= 10 else (16 if K <= 16 else 32)
    tiles = (N + TILE - 1) // TILE
    stride = 64 if kt <= 16 else 32
    n_split = (tiles + stride - 1) // stride
    per = (tiles + n_split - 1) // n_split
    return [j * per for j in range(n_split) if j * per < tiles]


def sample_columns(N, K):
    cols = torch.cat([torch.arange(t * TILE, min(N, (t + 1) * TILE)) for t in sampled_tiles(N, K)])
    return cols


def spf_margin(products, D):
    """score_topk.hip's spf_margin; 0 for the six-product passes"""
    if products == 6:
        return 0.0
    acc = (D / 16.0) * (4.0 * 4.0 + 4.0 * 3.0) * 2.0 ** -24
    dropped = 3.03 * 2.0 ** -16 if products == 3 else 1.013 * 2.0 ** -7 + 3.03 * 2.0 ** -16
    return 1.5 * (dropped + acc)


def survivors(c, products):
    """per user, how many items the main pass appends: score >= tau - delta, tau = the K-th best unmasked score of the sampled tiles
    lowered by 2^-18 |tau| (topk_tau_kernel), delta = spf_margin * ||u|| * max ||v|| (topk_tau_fast_kernel).  The reduced-product and
    the ping-pong passes do not mask the history themselves, so only column 0 is left out of the count."""
    users, table = c.users.double(), c.table.double()
    kth = torch.topk(c.s64[:, sample_columns(c.N, c.K)], c.K, dim=-1).values[:, -1]
    tau = kth - kth.abs() * 2.0 ** -18
    delta = spf_margin(products, c.D) * users.norm(dim=1) * table.norm(dim=1).max()
    raw = users @ table.t()
    raw[:, 0] = float("-inf")
    return (raw >= (tau - delta)[:, None]).sum(1)
