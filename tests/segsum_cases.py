"""The inputs of tests/test_gpu_segsum_passes.py: id sets that drive the segment sums of the table gradient (csrc/embed_grad.hip:
segsum_body and its sinks) through chosen row-group geometries, pass counts and epochs, with source values on which every fp32
operation is exact.  Plain numpy / torch, nothing from the library: tests/test_segsum_cases.py checks every case on the CPU.

How segsum_body walks the unique rows (restated here, from the kernel, so that a case can say where its rows land): a launch has
nblk = min(n, 4096) workgroups of 512 threads; dv = D / 4 lanes hold one row.
  * dv > 512 ("wide") or G = 512 // dv > 8 ("row"): one unique row per workgroup per pass, rank u in pass u // nblk;
  * 1 <= G <= 8 ("short"): G rows per workgroup per pass, rank u in pass u // (nblk * G), group u % G; the long rows (more than 8
    occurrences) and the apply sink's row marks of 16 passes (an epoch) wait for that epoch's barrier.
Unique ranks ascend with the id, so a case places a segment in a pass by the rank it gives it.

Exact arithmetic: source rows are multiples of 1/4 in [-8, 8], coefficients are +-0.5 / +-1 / +-2, the scale is 1 or 0.5.  Every
product is a multiple of 1/8 of magnitude <= 16 and every partial sum of up to 12 000 of them stays below 2^18 < 2^24 / 8: no fp32
operation rounds, with or without FMA, in any order, and the fp64 sum cast to fp32 is THE result -- compared with torch.equal."""
import functools
import math
from dataclasses import dataclass, field

import numpy as np
import torch

SEG_THREADS, SEG_SHORT, SEG_CHUNK, SEG_EPOCH, SEG_SPLIT = 512, 8, 512, 16, 1024
MAX_GRID = 4096                     # every entry point launches min(n, 4096) workgroups
FUSED_SORT_MAX = 65536              # occurrences up to which the one-launch-per-pass sort runs (beyond: the multi-launch sort)
ENDS = (1, 2, 8, 9, 512, 513)       # segment lengths every case that has room for them holds at its lowest and at its highest ranks


def geometry(n, D):
    """-> (path, G, unique rows per pass)."""
    dv, nblk = D // 4, min(n, MAX_GRID)
    if dv > SEG_THREADS:
        return "wide", 1, nblk
    G = SEG_THREADS // dv
    return ("row", G, nblk) if G > SEG_THREADS // 64 else ("short", G, nblk * G)


def predict(n, n_uniq, D):
    """-> (path, G, passes, epochs): passes = the turns of the busiest workgroup's loop; epochs = the barriers of the short path
    (1 for the two one-row-per-pass paths, which have none)."""
    path, G, per_pass = geometry(n, D)
    passes = max(1, math.ceil(n_uniq / per_pass))
    return path, G, passes, (math.ceil(passes / SEG_EPOCH) if path == "short" else 1)


def pass_of(rank, n, D):
    return rank // geometry(n, D)[2]


@dataclass(frozen=True)
class Spec:
    mode: str                       # "rows" | "sasrec" | "pool"
    D: int
    n_uniq: int
    expect: tuple                   # (path, G, passes, epochs) the case is meant to reach
    n: int = 0                      # rows: occurrences
    B: int = 0                      # sasrec / pool
    L: int = 0
    layout: str = ""                # sasrec: "sasrec" = [B, 2, L + 1] shifted windows, "bert4rec" = [B, 3, L] planes
    n_table: int = 0
    n_zero: int = 7                 # occurrences of id 0 among the free slots
    low: tuple = ENDS               # segment lengths at ranks 0, 1, ...
    high: tuple = ENDS              # ... and at the highest ranks, in this order
    mid: dict = field(default_factory=dict)    # {pass: length}: one more segment in the middle of that pass
    seed: int = 0

    @property
    def n_occ(self):
        return self.n if self.mode == "rows" else 3 * self.B * self.L if self.mode == "sasrec" else self.B * (self.L + 2)


TOP = ENDS + (1025,)                # the split route's case: 9, 513 and 1 025 occurrences on the top ids
SPLIT_ENDS = dict(low=(1, 2, 8, 9, 512), high=(1, 2, 8, 9, 513), n_zero=3)   # n too small for both long lengths at both ends

# The shapes are the smallest that reach the stated pass count.  n_uniq is odd on purpose (the last pass ends inside a row group).
# Three MODE_ROWS shapes are too small to hold ENDS at both ends and still reach their unique-row count (2 x 1 045 occurrences of
# n = 6 000 / 10 000 / 300): D = 100 and D = 2048 put 512 at the low end and 513 at the high end, D = 4096 stops at 9; each has a
# sibling ("n=...") with just enough more occurrences for the whole of ENDS at both ends.
SPECS = {
    # ---- MODE_ROWS (ops.embed_grad_rows) ----
    "rows D=4": Spec("rows", 4, 703, ("row", 512, 1, 1), n=3000, n_table=5000),
    "rows D=100": Spec("rows", 100, 4901, ("row", 20, 2, 1), n=6000, n_table=9000, **SPLIT_ENDS),
    "rows D=100 n=8200": Spec("rows", 100, 6001, ("row", 20, 2, 1), n=8200, n_table=9000),
    "rows D=252": Spec("rows", 252, 36003, ("short", 8, 2, 1), n=40000, n_table=50000),
    "rows D=260": Spec("rows", 260, 36003, ("short", 7, 2, 1), n=40000, n_table=50000),
    "rows D=384": Spec("rows", 384, 36003, ("short", 5, 2, 1), n=40000, n_table=50000),
    "rows D=512": Spec("rows", 512, 36003, ("short", 4, 3, 1), n=40000, n_table=50000, mid={1: 9}),
    "rows D=768": Spec("rows", 768, 36003, ("short", 2, 5, 1), n=40000, n_table=50000, mid={2: 9}),
    "rows D=2048": Spec("rows", 2048, 8901, ("short", 1, 3, 1), n=10000, n_table=20000, mid={1: 9}, **SPLIT_ENDS),
    "rows D=2048 n=12000": Spec("rows", 2048, 9501, ("short", 1, 3, 1), n=12000, n_table=20000, mid={1: 9}),
    "rows D=1028": Spec("rows", 1028, 69803, ("short", 1, 18, 2), n=72000, n_table=80000, n_zero=3, mid={7: 9, 15: 9, 16: 9}),
    "rows D=2052": Spec("rows", 2052, 2503, ("wide", 1, 1, 1), n=5000, n_table=9000),
    "rows D=4096": Spec("rows", 4096, 203, ("wide", 1, 1, 1), n=300, n_table=1000, low=(1, 2, 8, 9), high=(1, 2, 8, 9)),
    "rows D=4096 n=3000": Spec("rows", 4096, 703, ("wide", 1, 1, 1), n=3000, n_table=5000),
    # ---- MODE_SASREC (ops.occ_sort + ops.sasrec_occ_segsum[_apply]) ----
    "sasrec D=512": Spec("sasrec", 512, 21965, ("short", 4, 2, 1), B=256, L=50, layout="sasrec", n_table=40000, n_zero=5, high=TOP),
    "bert4rec D=512": Spec("sasrec", 512, 33001, ("short", 4, 3, 1), B=256, L=50, layout="bert4rec", n_table=40000, n_zero=100,
                           high=TOP, mid={1: 9}),
    "sasrec D=1028": Spec("sasrec", 1028, 69947, ("short", 1, 18, 2), B=720, L=50, layout="sasrec", n_table=80000, n_zero=5,
                          mid={8: 9, 15: 9, 16: 9}),
    "bert4rec D=1028": Spec("sasrec", 1028, 70003, ("short", 1, 18, 2), B=720, L=50, layout="bert4rec", n_table=80000, n_zero=100,
                            mid={8: 9, 15: 9, 16: 9}),
    # ---- MODE_POOL (ops.pool_table_grad / ops.pool_dense_grad) ----
    "pool D=256": Spec("pool", 256, 34003, ("short", 8, 2, 1), B=2400, L=14, n_table=40000, n_zero=20),
    "pool D=64": Spec("pool", 64, 4201, ("row", 32, 2, 1), B=400, L=14, n_table=6000, n_zero=10),
    "pool D=1028": Spec("pool", 1028, 69803, ("short", 1, 18, 2), B=4500, L=14, n_table=80000, n_zero=3, mid={7: 9, 15: 9, 16: 9}),
    "pool D=512": Spec("pool", 512, 34003, ("short", 4, 3, 1), B=2400, L=14, n_table=40000, n_zero=20, mid={1: 9}),   # (Gaussian)
}
ROWS_CASES = [k for k, s in SPECS.items() if s.mode == "rows"]
SASREC_CASES = [k for k, s in SPECS.items() if s.mode == "sasrec"]
POOL_CASES = [k for k, s in SPECS.items() if s.mode == "pool" and k != "pool D=512"]
GAUSS_CASES = ["rows D=512", "sasrec D=512", "pool D=512"]
BAD_IDS = (5, -3)                   # MODE_ROWS: one id n_table + 5 and one id -3 in every case


# ---- ids ----------------------------------------------------------------------------------------------------------------------
def planted(spec):
    """{rank: occurrences} of the segments a case places on purpose."""
    R, per_pass = spec.n_uniq, geometry(spec.n_occ, spec.D)[2]
    p = {k: c for k, c in enumerate(spec.low)}
    p.update({R - len(spec.high) + k: c for k, c in enumerate(spec.high)})
    for ps, c in spec.mid.items():
        r = ps * per_pass + per_pass // 2 + 1
        assert r not in p and len(spec.low) <= r < R - len(spec.high), (ps, r)
        p[r] = c
    assert len(p) == len(spec.low) + len(spec.high) + len(spec.mid)
    return p


def _rank_counts(spec, n_free, n_single, rng):
    """Occurrences per unique rank over `n_free` slots of one occurrence each (n_zero of them hold id 0): the planted ranks get their
    length, `n_single` of the other ranks get none here (the caller puts them, once each, into slots of its own), the rest get one,
    and the occurrences then left over make short segments of 2 .. 8, dealt round-robin over the passes so that every pass has some.
    -> (counts [R], the single ranks)."""
    R = spec.n_uniq
    plant = planted(spec)
    counts = np.zeros(R, dtype=np.int64)
    for r, c in plant.items():
        counts[r] = c
    fill = rng.permutation(np.setdiff1d(np.arange(R), np.fromiter(plant, dtype=np.int64)))
    single, fill = fill[:n_single], fill[n_single:]
    counts[fill] = 1
    extras = n_free - spec.n_zero - int(counts.sum())
    assert 0 <= extras <= (SEG_SHORT - 1) * len(fill), (extras, len(fill))
    per_pass = geometry(spec.n_occ, spec.D)[2]
    by_pass = [list(fill[fill // per_pass == ps]) for ps in range(math.ceil(R / per_pass))]
    cyc, k, turn = (4, 2, 5, 3, 6, 2, 7, 3, 8, 2), 0, 0
    while extras > 0:                                  # the first turn deals 3 to every pass, the second 2, then the cycle
        assert any(by_pass)
        for rows in by_pass:
            if extras > 0 and rows:
                c = min(3 if turn == 0 else 2 if turn == 1 else cyc[k % len(cyc)], extras + 1)
                counts[rows.pop()] = c
                extras -= c - 1
                k += 1
        turn += 1
    return counts, single


def _free_slots(spec, counts, ids, rng):
    occ = np.concatenate([np.repeat(ids, counts), np.zeros(spec.n_zero, dtype=np.int64)])
    return rng.permutation(occ)


@functools.lru_cache(maxsize=None)
def case_ids(name):
    """-> the int64 id array of the case as the entry point takes it: rows [n]; pool [B L + 2 B]; sasrec [B, 2, L + 1] or [B, 3, L]."""
    spec = SPECS[name]
    rng = np.random.default_rng(spec.seed + 1000 * list(SPECS).index(name))
    ids = np.sort(rng.choice(np.arange(1, spec.n_table, dtype=np.int64), spec.n_uniq, replace=False))
    if spec.mode == "rows":
        counts, _ = _rank_counts(spec, spec.n - len(BAD_IDS), 0, rng)
        free = _free_slots(spec, counts, ids, rng)
        out = np.concatenate([free, [spec.n_table + BAD_IDS[0], BAD_IDS[1]]])
        return rng.permutation(out)
    if spec.mode == "pool" or spec.layout == "bert4rec":
        counts, _ = _rank_counts(spec, spec.n_occ, 0, rng)
        free = _free_slots(spec, counts, ids, rng)
        return free if spec.mode == "pool" else free.reshape(spec.B, 3, spec.L)
    # SASRec's shifted windows: items[b, 0, t] is the input of position t (t < L) AND the target of position t - 1 (t > 0), so a
    # slot of plane 0 is one occurrence at the ends of a sequence and two inside; items[b, 1, 1:] are the negatives, one occurrence
    # each, and items[b, 1, 0] is never read.  Plane 0 holds distinct ids behind two slots of left padding in every fifth sequence;
    # every planted segment lives in the negatives.
    B, L = spec.B, spec.L
    pad = np.zeros((B, L + 1), dtype=bool)
    pad[::5, :2] = True
    counts, single = _rank_counts(spec, B * L, int((~pad).sum()), rng)
    out = np.zeros((B, 2, L + 1), dtype=np.int64)
    plane0 = np.zeros((B, L + 1), dtype=np.int64)
    plane0[~pad] = ids[single]
    out[:, 0] = plane0
    out[:, 1, 1:] = _free_slots(spec, counts, ids, rng).reshape(B, L)
    out[:, 1, 0] = ids[-1]          # never read: were it counted, the top segment would grow
    return out


def bert4rec_layout(L):
    return (3 * L, 0, L, 2 * L)


def occurrence_ids(items, spec):
    """The flat id of every occurrence, in occurrence order (sasrec: inputs | targets | negatives).  numpy or torch."""
    if spec.mode != "sasrec":
        return items.reshape(-1)
    L = spec.L
    cat = torch.cat if torch.is_tensor(items) else np.concatenate
    if spec.layout == "sasrec":
        return cat([items[:, 0, :L].reshape(-1), items[:, 0, 1:].reshape(-1), items[:, 1, 1:].reshape(-1)])
    return cat([items[:, 0].reshape(-1), items[:, 1].reshape(-1), items[:, 2].reshape(-1)])


# ---- values -------------------------------------------------------------------------------------------------------------------
def exact_rows(shape, gen):
    """Multiples of 1/4 in [-8, 8]."""
    return torch.randint(-32, 33, shape, generator=gen, device=gen.device, dtype=torch.int32).float() / 4


def exact_coef(shape, gen):
    """+-0.5, +-1, +-2."""
    table = torch.tensor([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], device=gen.device)
    return table[torch.randint(0, 6, shape, generator=gen, device=gen.device)]


def gauss(shape, gen):
    return torch.randn(shape, generator=gen, device=gen.device)


def case_values(name, device, draw=exact_rows, draw_coef=exact_coef, cols=None):
    """The float32 sources of a case, drawn on `device`: rows -> (rows [n, D],); sasrec -> (dx0, out [B, L, D], coef [B, L]); pool ->
    (G [3 B, D], w [B]).  cols: a narrower D (the CPU check of the wide cases)."""
    spec = SPECS[name]
    D = spec.D if cols is None else cols
    gen = torch.Generator(device=device).manual_seed(spec.seed + 17)
    if spec.mode == "rows":
        return (draw((spec.n, D), gen),)
    if spec.mode == "sasrec":
        return draw((spec.B, spec.L, D), gen), draw((spec.B, spec.L, D), gen), draw_coef((spec.B, spec.L), gen)
    return draw((3 * spec.B, D), gen), draw_coef((spec.B,), gen)


def contributions(name, ids_flat, values):
    """[(ids [k], source rows [k, D], coefficient [k] or None)]: what every occurrence adds, in occurrence order."""
    spec = SPECS[name]
    if spec.mode == "rows":
        return [(ids_flat, values[0], None)]
    if spec.mode == "sasrec":
        dx0, out, coef = values
        T, D = spec.B * spec.L, dx0.shape[-1]
        return [(ids_flat[:T], dx0.reshape(T, D), None), (ids_flat[T:2 * T], out.reshape(T, D), coef.reshape(T)),
                (ids_flat[2 * T:], out.reshape(T, D), -coef.reshape(T))]
    G, w = values
    T = spec.B * spec.L
    return [(ids_flat[:T], G[:spec.B].repeat_interleave(spec.L, 0), w.repeat_interleave(spec.L)), (ids_flat[T:], G[spec.B:], None)]


def segment_reference(parts, n_table, absolute=False):
    """The segment sums in float64, compactly: -> (uniq [n_uniq] ascending valid ids, ref [n_uniq, D] float64, cnt [n_uniq]).  Ids
    outside (0, n_table) are dropped.  absolute: the sums of |coefficient * value| (the scale of the rounding-error bound)."""
    ids = torch.cat([p[0] for p in parts])
    valid = (ids > 0) & (ids < n_table)
    uniq, inv = torch.unique(ids[valid], return_inverse=True)
    where = torch.full_like(ids, -1)
    where[valid] = inv
    ref = torch.zeros(uniq.numel(), parts[0][1].shape[1], dtype=torch.float64, device=ids.device)
    k = 0
    for pid, val, cf in parts:
        w = where[k:k + pid.numel()]
        k += pid.numel()
        sel = w >= 0
        v = val[sel].double()
        if cf is not None:
            v *= cf[sel].double().unsqueeze(1)
        ref.index_add_(0, w[sel], v.abs() if absolute else v)
    return uniq, ref, torch.bincount(inv, minlength=uniq.numel())
