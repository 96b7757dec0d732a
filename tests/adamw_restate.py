"""Yardstick of tests/test_gpu_adamw_ref.py and tests/test_adamw_ref_cpu.py (CPU only): deterministic inputs, torch.optim.AdamW in
float64 as the reference, a running forward error bound derived from the roundings csrc/adamw.hip commits, a numpy-float32
emulation of adam_elem, and mutants of it.

Nothing here reads a scalar from the library: the per-step scalars are restated in Python floats
    decay = 1 - lr wd,  step_size = lr / (1 - b1^t),  inv_sqrt_bc2 = 1 / sqrt(1 - b2^t),  cumlog[t] = sum_i log(float32(decay_i)).

THE BOUND (first order, per element, beside the reference; u = 2^-24, TINY = 2^-126 = the smallest normal fp32).  Capital letters
are the float64 reference, E_x the bound on |kernel x - reference X| before the step; hats are fp32-cast scalars (each off by u):
    p1 = fmul(p, ^decay)                    E_p1 = E_p |d| + 2u (|P d| + E_p)                        scalar cast + 1 rounding
    m' = fma(g - m, ^(1-b1), m)             E_m' = E_m |b1| + 2u (1-b1)(|g - M| + E_m) + u |M'| + TINY  sub rounding, cast, fma rounding
    v' = fma(v, ^b2, fmul(fmul(^(1-b2), g), g))
                                            E_v' = E_v b2 + u b2 V + 3u (1-b2) g^2 + u V' + 2 TINY      cast; cast + 2 roundings; fma
    s  = v_sqrt_f32(v')   (1 ulp = 2u, denormal input flushed: + TINY on v')
                                            E_s  = max(sqrt(V' + e) - S, S - sqrt(max(V' - e, 0))) + 2u S,   e = E_v' + TINY
    den = fma(s, ^isb, ^eps)                E_den = E_s isb + u S isb + u eps + u DEN                   two casts, fma rounding
    r  = v_rcp_f32(den)   (1 ulp = 2u)      E_r  = 1 / (DEN - E_den) - 1 / DEN + 2u / DEN
    q  = fmul(m', r)                        E_q  = E_m' R + |M'| E_r + u |Q|
    p' = fma(-^ss, q, p1)                   E_p' = E_p1 + ss E_q + u ss |Q| + u |P'| + TINY             cast, fma rounding
The reported bounds are TWICE these (one overall factor for every second-order term).  The TINY floors cover results that are
subnormal in fp32 (rounded to 2^-149 or flushed): g^2 of a 1e-20 gradient, m and v of rows that decayed for hundreds of steps.
The zero-gradient form adam_elem0 commits a subset of these roundings.

LAZY schedule (adamw_rows_kernel): every replayed step is adam_elem0, so the same propagation holds row by row; what the closed
forms add is stated by the source and added per gap (a gap = the steps a row is brought forward by in one launch):
  * window truncation: beyond `window` replayed steps (256 exact mode, 128 fast mode) only the weight decay acts; the dropped Adam
    terms are bounded by  max_j(step_size_j) / sqrt(1 - b2) * rho^window / (1 - rho),  rho = b1 / sqrt(b2)  (the source's
    31.6 lr rho^window / (1 - rho) at the default betas, with lr / (1 - b1^t) in place of lr so that it also holds early on);
  * fast mode, series armed (rho <= 0.95) and gap >= 6: the truncated series' remainder, at most 2.2e-7 of the gap's summed Adam
    terms (tests/test_lazy_series_algebra.py), taken here on the sum of their magnitudes.
Exact mode gets nothing for gaps <= 256: there the replay is the sweep's own arithmetic."""
import math
from dataclasses import dataclass

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
SERIES_REL = 2.2e-7
SERIES_MIN = 6
WINDOW = {"exact": 256, "fast": 128}
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ per-step scalars
def step_scalars(lr, wd, b1, b2, t):
    """(decay, step_size, inv_sqrt_bc2) of optimizer step t (1-based) in Python floats."""
    return 1.0 - lr * wd, lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t)


def hyper_restate(lrs, wds, b1, b2, mutant=None):
    """Rows 0..T of the hyper table and cumlog for steps 1..T (lrs[t-1], wds[t-1] belong to step t): float64 [T+1, 3], [T+1].
    mutant "h": cumlog summed from the PREVIOUS step's lr."""
    T = len(lrs)
    hyper = np.zeros((T + 1, 3))
    hyper[0] = (1.0, 0.0, 1.0)
    cumlog = np.zeros(T + 1)
    for t in range(1, T + 1):
        hyper[t] = step_scalars(lrs[t - 1], wds[t - 1], b1, b2, t)
        dec = hyper[t, 0]
        if mutant == "h" and t > 1:
            dec = 1.0 - lrs[t - 2] * wds[t - 1]
        cumlog[t] = cumlog[t - 1] + math.log(float(F32(dec)))
    return hyper, cumlog


def cumlog_tolerance(cumlog, hyper):
    """What "equal to rounding" means for cumlog[t]: one float64 rounding per partial sum and a 2-ulp device log per term."""
    per = 2.0 ** -53 * np.abs(cumlog) + 2.0 ** -51 * np.abs(np.log(hyper[:, 0].astype(F32).astype(F64)))
    return np.cumsum(per)


def ulp_distance(a, b):
    """Distance in fp32 units in the last place between two float32 arrays of equal sign pattern (or zeros)."""
    ia = np.ascontiguousarray(a, dtype=F32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, dtype=F32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


# ------------------------------------------------------------------------------------------------ inputs
def make_params(rng, shape):
    """|p| log-uniform in [1e-4, 1], random sign."""
    mag = 10.0 ** rng.uniform(-4.0, 0.0, size=shape)
    return (mag * rng.choice([-1.0, 1.0], size=shape)).astype(F32)


def make_grads(rng, rows, D):
    """[rows, D]: standard normal times a per-column log-spaced scale from 1e-12 to 1e2 (eps-dominated, mixed and sqrt(v)-dominated
    columns), with exact zeros and components whose square is subnormal in fp32 (|g| ~ 1e-20 .. 1e-21) sprinkled in."""
    scale = np.logspace(-12.0, 2.0, D)[rng.permutation(D)] if D > 1 else np.ones(1)
    g = rng.standard_normal((rows, D)) * scale
    kind = rng.integers(0, 16, size=(rows, D))
    g[kind == 0] = 0.0
    sub = kind == 1
    g[sub] = rng.standard_normal(int(sub.sum())) * 10.0 ** rng.uniform(-21.0, -20.0, size=int(sub.sum()))
    return g.astype(F32)


def make_moments(rng, rows, D):
    """A plausible (m, v) of a run in progress, for single steps at a large step number: m of the gradients' size, v of their squares."""
    g = make_grads(rng, rows, D).astype(F64)
    m = (g * rng.uniform(0.05, 1.0, size=g.shape)).astype(F32)
    v = (g * g * rng.uniform(0.05, 2.0, size=g.shape)).astype(F32)
    return m, v


def sparse_list(rng, N, n_valid, cap):
    """A sparse-gradient row list of `cap` entries as the table forms take it: unique valid ids (1 .. N-1), id 0 and out-of-range ids
    mixed in, no duplicates among the valid ones.  -> int64 [cap], number of entries that count (the rest of the list is padding that
    the device count excludes)."""
    n_valid = min(n_valid, N - 1, cap - 6)
    valid = rng.choice(np.arange(1, N), size=n_valid, replace=False)
    junk = np.array([0, N, N + 5, 2 ** 40, -3, 0], dtype=np.int64)
    lst = np.concatenate([valid, junk])
    lst = lst[rng.permutation(lst.size)]
    out = np.full(cap, N + 11, dtype=np.int64)           # padding past the count: never read
    out[:lst.size] = lst
    return out, int(lst.size)


def raw_ids(rng, N, n, hi=None):
    """A raw id list for the claim-mode catch-up, drawn from rows 1 .. hi-1: duplicates, 0, negative and huge ids included."""
    ids = rng.integers(1, hi if hi is not None else N, size=n)
    ids[rng.integers(0, n, size=max(1, n // 3))] = ids[0]                      # duplicates
    junk = np.array([0, 0, -3, -2 ** 40, N, N + 17, 2 ** 40, 2 ** 62], dtype=np.int64)
    ids[rng.choice(n, size=min(n, junk.size), replace=False)] = junk[:min(n, junk.size)]
    return ids.astype(np.int64)


def densify(N, D, ids, n, rows):
    """Dense float32 [N, D] gradient of a sparse list: ids outside 1 .. N-1 are dropped, untouched rows stay zero."""
    g = np.zeros((N, D), dtype=F32)
    lst = np.asarray(ids[:n], dtype=np.int64)
    keep = (lst > 0) & (lst < N)
    g[lst[keep]] = np.asarray(rows)[:n][keep]
    return g


# ------------------------------------------------------------------------------------------------ reference + bound
def bound_step(P, M, V, Ep, Em, Ev, g, scal, b1, b2, eps):
    """One step of the restated recurrence in float64 with the error bound pushed through it (module docstring).
    -> (P', M', V', E_p', E_m', E_v', |Adam term|, the Adam term's size before m + (g - m)(1 - b1) cancels)."""
    d, ss, isb = scal
    u = U
    c1, c2 = 1.0 - b1, 1.0 - b2
    P1 = P * d
    Ep1 = Ep * abs(d) + 2 * u * (np.abs(P1) + Ep)
    Gm = g - M
    M1 = M + Gm * c1
    Em1 = Em * abs(1.0 - c1) + 2 * u * c1 * (np.abs(Gm) + Em) + u * np.abs(M1) + TINY
    G2 = c2 * g * g
    V1 = V * b2 + G2
    Ev1 = Ev * b2 + u * b2 * V + 3 * u * G2 + u * V1 + 2 * TINY
    S = np.sqrt(V1)
    e = Ev1 + TINY
    Es = np.maximum(np.sqrt(V1 + e) - S, S - np.sqrt(np.maximum(V1 - e, 0.0))) + 2 * u * S
    DEN = S * isb + eps
    Eden = Es * isb + u * S * isb + u * eps + u * DEN
    assert (Eden < 0.5 * DEN).all(), "the bound's linearisation of 1/denominator needs E_den << denominator"
    R = 1.0 / DEN
    Er = 1.0 / (DEN - Eden) - R + 2 * u * R
    Q = M1 * R
    Eq = Em1 * R + np.abs(M1) * Er + u * np.abs(Q)
    P2 = P1 - ss * Q
    Ep2 = Ep1 + ss * Eq + u * ss * np.abs(Q) + u * np.abs(P2) + TINY
    return P2, M1, V1, Ep2, Em1, Ev1, ss * np.abs(Q), ss * R * (np.abs(M) + c1 * np.abs(g))


class Reference:
    """torch.optim.AdamW (foreach=False, amsgrad=False) on float64 CPU tensors, with the bound propagated beside it.  t0 = number of
    steps already taken (m0 / v0: the moments they left)."""

    def __init__(self, p0, b1, b2, eps, t0=0, m0=None, v0=None):
        self.b1, self.b2, self.eps, self.t = b1, b2, eps, t0
        self.p = torch.from_numpy(np.array(p0, dtype=F64)).requires_grad_(True)
        self.opt = torch.optim.AdamW([self.p], lr=1e-3, betas=(b1, b2), eps=eps, weight_decay=0.0, foreach=False, amsgrad=False)
        m = torch.zeros_like(self.p) if m0 is None else torch.from_numpy(np.array(m0, dtype=F64))
        v = torch.zeros_like(self.p) if v0 is None else torch.from_numpy(np.array(v0, dtype=F64))
        self.opt.state[self.p] = {"step": torch.tensor(float(t0)), "exp_avg": m, "exp_avg_sq": v}
        z = np.zeros(self.p.shape)
        self.Ep, self.Em, self.Ev = z.copy(), z.copy(), z.copy()
        self.cum_upd = z.copy()          # running sum of |Adam term| per element (series remainder of the lazy fast mode)
        self.restate_gap = 0.0           # worst relative distance restated recurrence <-> torch, over all steps

    @property
    def P(self):
        return self.p.detach().numpy()

    @property
    def M(self):
        return self.opt.state[self.p]["exp_avg"].numpy()

    @property
    def V(self):
        return self.opt.state[self.p]["exp_avg_sq"].numpy()

    def step(self, g, lr, wd):
        """g: dense float32 gradient (the very values the kernel gets)."""
        self.t += 1
        g64 = np.asarray(g, dtype=F64)
        scal = step_scalars(lr, wd, self.b1, self.b2, self.t)
        P0, M0, V0 = self.P.copy(), self.M.copy(), self.V.copy()
        P2, M1, V1, self.Ep, self.Em, self.Ev, upd, upd_ops = bound_step(P0, M0, V0, self.Ep, self.Em, self.Ev, g64, scal, self.b1, self.b2, self.eps)
        self.cum_upd += upd
        grp = self.opt.param_groups[0]
        grp["lr"], grp["weight_decay"] = lr, wd
        self.p.grad = torch.from_numpy(g64.copy())
        self.opt.step()
        # relative to the size of the operands each update adds up (p may cross zero within a step at lr 1e-2, and the new m may be a
        # small difference of m and g, whose float64 rounding the Adam term then carries)
        for a, b, scale in ((P2, self.P, np.abs(P0) + upd_ops), (M1, self.M, np.abs(M0) + np.abs(g64)), (V1, self.V, V0 + g64 * g64)):
            self.restate_gap = max(self.restate_gap, float((np.abs(a - b) / np.maximum(scale, 1e-300)).max()))
        return scal

    def add_p(self, rows, extra):
        """Widen E_p of `rows` by `extra` (a truncation term of the lazy schedule)."""
        self.Ep[rows] += extra

    def bounds(self):
        return 2.0 * self.Ep, 2.0 * self.Em, 2.0 * self.Ev

    def ratios(self, p, m, v):
        """Worst |x - X| / bound per tensor, over EVERY element (no masking; a non-finite value gives inf)."""
        out = []
        for got, ref, bnd in zip((p, m, v), (self.P, self.M, self.V), self.bounds()):
            err = np.abs(np.asarray(got, dtype=F64).reshape(ref.shape) - ref)
            err = np.where(np.isfinite(err), err, np.inf)
            out.append(float((err / bnd).max()))
        return tuple(out)


class LazyBook:
    """Host book-keeping of the lazy schedule for the truncation terms: which step each row is current through, and the gap every
    launch closes.  mode "exact" | "fast"."""

    def __init__(self, ref: Reference, N, mode, b1, b2):
        self.ref, self.mode, self.window = ref, mode, WINDOW[mode]
        self.rho = b1 / math.sqrt(b2)
        self.b2 = b2
        self.series = mode == "fast" and self.rho <= 0.95
        self.last = np.zeros(N, dtype=np.int64)
        self.cum_at_last = np.zeros_like(ref.cum_upd)
        self.ss = [0.0]                       # step_size per step (index = step)
        self.ever_applied = np.zeros(N, dtype=bool)
        self.tail_gaps = []                   # every gap > window closed on a row that has been applied before

    def note_step(self, scal):
        self.ss.append(scal[1])

    def bring_forward(self, rows, t_prev):
        """`rows` are replayed through t_prev by one launch (cum_upd must already include step t_prev)."""
        rows = np.unique(np.asarray(rows, dtype=np.int64))
        gap = t_prev - self.last[rows]
        rows, gap = rows[gap > 0], gap[gap > 0]
        far = gap > self.window
        for k0 in np.unique(self.last[rows[far]]):
            ss_max = max(self.ss[k0 + self.window + 1:t_prev + 1])
            self.ref.Ep[rows[far & (self.last[rows] == k0)]] += ss_max / math.sqrt(1.0 - self.b2) * self.rho ** self.window / (1.0 - self.rho)
        # the gaps beyond the window that rows WITH moments (applied before) see: what the closed-form tail is tested on
        self.tail_gaps += [int(x) for x in gap[far & self.ever_applied[rows]]]
        if self.series:
            sr = rows[gap >= SERIES_MIN]
            self.ref.Ep[sr] += SERIES_REL * (self.ref.cum_upd[sr] - self.cum_at_last[sr])
        self.last[rows] = t_prev
        self.cum_at_last[rows] = self.ref.cum_upd[rows]

    def applied(self, rows, t):
        rows = np.unique(np.asarray(rows, dtype=np.int64))
        self.last[rows] = t
        self.ever_applied[rows] = True
        self.cum_at_last[rows] = self.ref.cum_upd[rows]


# ------------------------------------------------------------------------------------------------ fp32 emulation + mutants
MUTANTS = ("a", "b", "c", "d", "e", "f", "g")       # adam_elem mutants; "h" is a mutant of the hyper table (hyper_restate)


def _fma(a, b, c):
    return (np.asarray(a, dtype=F64) * np.asarray(b, dtype=F64) + np.asarray(c, dtype=F64)).astype(F32)


def _nudge(x, rng):
    """x moved by -1, 0 or +1 fp32 ulp at random: a 1-ulp hardware sqrt / reciprocal instead of the correctly rounded one."""
    if rng is None:
        return x
    k = rng.integers(-1, 2, size=x.shape)
    lo, hi = np.nextafter(x, F32(-np.inf)), np.nextafter(x, F32(np.inf))
    return np.where(k < 0, lo, np.where(k > 0, hi, x)).astype(F32)


def emu_scalars(lr, wd, b1, b2, eps, t, mutant=None):
    """The fp32 scalars adam_elem reads, cast from the float64 formulas as make_hyper / hyper_append_body cast them."""
    tb = t - 1 if mutant == "e" else t
    with np.errstate(divide="ignore", invalid="ignore"):
        bc1, bc2 = F64(1.0) - F64(b1) ** tb, F64(1.0) - F64(b2) ** tb
        h = {"decay": F32(1.0 - lr * wd), "one_m_b1": F32(1.0 - b1), "b2": F32(b2), "one_m_b2": F32(1.0 - b2),
             "step_size": F32(F64(lr) / bc1), "inv_sqrt_bc2": F32(F64(1.0) / np.sqrt(bc2)), "eps": F32(eps), "l2": F32(0.0)}
    if mutant == "a":
        h["decay"], h["l2"] = F32(1.0), F32(wd)
    if mutant == "c":
        h["decay"] = F32(1.0)
    if mutant == "f":
        h["inv_sqrt_bc2"] = F32(1.0)
    if mutant == "g":
        h["one_m_b1"] = F32(b1)
    return h


def emu_adam_elem(p, m, v, g, h, mutant=None, rng=None):
    """adam_elem of csrc/adamw.hip in numpy float32 (fma = one rounding of the float64 a b + c), on arrays.  -> (p, m, v)."""
    with np.errstate(all="ignore"):
        if mutant == "a":
            g = _fma(h["l2"], p, g)
        if mutant != "b":
            p = (p * h["decay"]).astype(F32)
        m = _fma((g - m).astype(F32), h["one_m_b1"], m)
        v = _fma(v, h["b2"], ((h["one_m_b2"] * g).astype(F32) * g).astype(F32))
        if mutant == "d":
            denom = (_nudge(np.sqrt((v + h["eps"]).astype(F32)), rng) * h["inv_sqrt_bc2"]).astype(F32)
        else:
            denom = _fma(_nudge(np.sqrt(v), rng), h["inv_sqrt_bc2"], h["eps"])
        r = _nudge((F32(1.0) / denom).astype(F32), rng)
        p = _fma(-h["step_size"], (m * r).astype(F32), p)
        if mutant == "b":
            p = (p * h["decay"]).astype(F32)
    return p, m, v


class EmuLazy:
    """The lazy schedule on top of emu_adam_elem: rows replay their missed zero-gradient steps one by one up to `window`, then the
    closed-form tail (p by exp of the cumlog difference, m and v by powers of float(b1), float(b2)).  This IS the exact mode's
    arithmetic.  For the fast mode (window 128) it is NOT the kernel's arithmetic: the carried sqrt product, the Newton reciprocals,
    m *= float(b1) and the fp32-evaluated series are not emulated, and the bound has no term of its own for the carried-product loop
    (gaps under 6, rho > 0.95, the first ~200 steps).  So the CPU check shows the fast-mode bound fair for the window truncation
    and the tail only; that the fast arithmetic itself stays inside it is shown by the GPU measurement alone."""

    def __init__(self, p, m, v, b1, b2, eps, window, rng=None, tail_mutant=None):
        self.p, self.m, self.v = p.copy(), m.copy(), v.copy()
        self.b1, self.b2, self.eps, self.window, self.rng = b1, b2, eps, window, rng
        self.tail_mutant = tail_mutant      # "rem": one step too many in the tail's powers; "cumlog": its decay product starts one entry late
        self.last = np.zeros(p.shape[0], dtype=np.int64)
        self.h = [None]
        self.cumlog = [0.0]

    def append(self, lr, wd, t):
        assert t == len(self.h)
        self.h.append(emu_scalars(lr, wd, self.b1, self.b2, self.eps, t))
        self.cumlog.append(self.cumlog[-1] + math.log(float(self.h[-1]["decay"])))

    def catch_up(self, rows, t_prev):
        rows = np.unique(np.asarray(rows, dtype=np.int64))
        rows = rows[self.last[rows] < t_prev]
        for k0 in np.unique(self.last[rows]):                  # rows with the same gap replay together
            k0 = int(k0)
            r = rows[self.last[rows] == k0]
            p, m, v = self.p[r], self.m[r], self.v[r]
            end = min(t_prev, k0 + self.window)
            z = np.zeros_like(p)
            for s in range(k0 + 1, end + 1):
                p, m, v = emu_adam_elem(p, m, v, z, self.h[s], rng=self.rng)
            if end < t_prev:
                rem = t_prev - end + (1 if self.tail_mutant == "rem" else 0)
                first = end + (1 if self.tail_mutant == "cumlog" else 0)
                p = (p * F32(math.exp(self.cumlog[t_prev] - self.cumlog[first]))).astype(F32)
                m = (m * F32(float(F32(self.b1)) ** rem)).astype(F32)
                v = (v * F32(float(F32(self.b2)) ** rem)).astype(F32)
            self.p[r], self.m[r], self.v[r] = p, m, v
        self.last[rows] = t_prev

    def apply(self, ids, n, grows, t):
        lst = np.asarray(ids[:n], dtype=np.int64)
        keep = lst > 0
        r = lst[keep]
        assert np.unique(r).size == r.size
        self.catch_up(r, t - 1)
        self.p[r], self.m[r], self.v[r] = emu_adam_elem(self.p[r], self.m[r], self.v[r], np.asarray(grows)[:n][keep], self.h[t], rng=self.rng)
        self.last[r] = t


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class FlatCase:
    name: str
    n: int
    t0: int            # steps already taken (single steps at step t0 + 1 start from make_moments)
    T: int             # consecutive steps
    lr: float
    wd: float
    betas: tuple = (0.9, 0.999)
    vary_lr: bool = False
    seed: int = 0

    def lrs(self):
        if not self.vary_lr:
            return [self.lr] * self.T
        return [self.lr * (0.25 + 0.75 * min(1.0, (k + 1) / 8.0)) * (0.5 + 0.5 * math.cos(math.pi * k / (2.0 * self.T))) for k in range(self.T)]


FLAT_BIG = 4 * (4096 * 256 + 300)       # float4 count just past the 4096-block x 256-thread launch cap


SEGMENT_CASE = FlatCase("segment-problem", 64 * 400, 11, 1, 1e-2, 0.1, seed=109)      # the buffer of the plane-segment tests
CLOSE_CASE = FlatCase("close-problem", 64 * 300, 8, 1, 1e-2, 0.1, seed=110)            # and of the close= test


def flat_cases():
    out, k = [], 0
    for t in (1, 2, 10, 1000, 100000):
        for lr in (1e-4, 1e-3, 1e-2):
            for wd in (0.0, 0.1):
                k += 1
                out.append(FlatCase(f"single-t{t}-lr{lr:g}-wd{wd:g}", 4096 + 4 * (k % 5), t - 1, 1, lr, wd, seed=k))
    out.append(FlatCase("single-n4", 4, 9, 1, 1e-3, 0.1, seed=101))
    out.append(FlatCase("single-n260", 260, 1, 1, 1e-2, 0.1, seed=102))
    out.append(FlatCase("single-betas", 8192, 9, 1, 1e-3, 0.1, betas=(0.8, 0.98), seed=103))
    out.append(FlatCase("single-past-the-launch-cap", FLAT_BIG, 999, 1, 1e-3, 0.1, seed=104))
    out.append(FlatCase("run40-lr1e-3-wd0.1", 16384, 0, 40, 1e-3, 0.1, vary_lr=True, seed=105))
    out.append(FlatCase("run40-lr1e-2-wd0", 4100, 0, 40, 1e-2, 0.0, vary_lr=True, seed=106))
    out.append(FlatCase("run30-betas", 4096, 0, 30, 1e-2, 0.1, betas=(0.8, 0.98), vary_lr=True, seed=107))
    out.append(FlatCase("run24-from-t1000", 2048, 1000, 24, 1e-4, 0.1, seed=108))
    out += [SEGMENT_CASE, CLOSE_CASE]
    return out


def flat_inputs(c: FlatCase):
    """-> p0, m0, v0 (float32 [n]) and the T gradients (float32 [T, n])."""
    rng = np.random.default_rng(1000 + c.seed)
    cols = 64 if c.n % 64 == 0 else 4
    rows = c.n // cols
    p0 = make_params(rng, c.n)
    if c.t0:
        m0, v0 = (x.reshape(-1) for x in make_moments(rng, rows, cols))
    else:
        m0, v0 = np.zeros(c.n, dtype=F32), np.zeros(c.n, dtype=F32)
    gs = np.stack([make_grads(rng, rows, cols).reshape(-1) for _ in range(c.T)])
    return p0, m0, v0, gs


TABLE_D = (4, 36, 64, 260, 512, 1028, 2048, 4096)


@dataclass(frozen=True)
class TableCase:
    name: str
    N: int
    D: int
    T: int
    lr: float
    wd: float
    betas: tuple = (0.9, 0.999)
    seed: int = 0
    cap: int = 32

    def lrs(self):
        return [self.lr * (1.0 if k % 2 == 0 else 0.3) for k in range(self.T)]


def table_cases():
    out = []
    for i, D in enumerate(TABLE_D):
        N = 16384 + 150 if D == 4 else max(40, 32768 // D + 3)
        out.append(TableCase(f"D{D}", N, D, 6, (1e-3, 1e-2)[i % 2], (0.1, 0.0)[(i // 2) % 2], seed=200 + i))
    out.append(TableCase("D36-many-rows", 16384 + 70, 36, 3, 1e-2, 0.1, seed=220))
    out.append(TableCase("D64-betas", 300, 64, 12, 1e-2, 0.1, betas=(0.8, 0.98), seed=221))
    return out


def table_inputs(c: TableCase):
    """-> p0 [N, D] and per step (ids [cap] | None, count, gradient rows [cap, D]); one step of every case has no gradient at all."""
    rng = np.random.default_rng(2000 + c.seed)
    p0 = make_params(rng, (c.N, c.D))
    steps = []
    for k in range(c.T):
        if k == 2:
            steps.append((None, 0, None))
            continue
        ids, n = sparse_list(rng, c.N, 20, c.cap)
        steps.append((ids, n, make_grads(rng, c.cap, c.D)))
    return p0, steps


LAZY_D = TABLE_D + (192, 768)      # + the widths that select adamw_rows_kernel<128, 2>, <512, 2> and <256, 4>
HOT, WARM = 8, 32                  # rows 1..7 hot, 8..31 warm, 32.. cold


@dataclass(frozen=True)
class LazyCase:
    name: str
    N: int
    D: int
    T: int
    lr: float
    wd: float
    betas: tuple = (0.9, 0.999)
    seed: int = 0
    cap: int = 24
    big: bool = False      # more rows than one trip of the grid-stride loop covers (16384 blocks of 4 rows at D = 4)

    def lrs(self):
        return [self.lr * min(1.0, (k + 1) / 20.0) * (1.0 - 0.5 * k / self.T) for k in range(self.T)]


LAZY_BIG_N = 4 * 16384 + 470


def lazy_cases():
    out = []
    for i, D in enumerate(LAZY_D):
        N = 160 if D <= 64 else (96 if D <= 512 else 64)
        out.append(LazyCase(f"D{D}", N, D, 330, (1e-3, 1e-2)[i % 2], (0.1, 0.0)[(i // 2) % 2], seed=300 + i))
    out.append(LazyCase("D64-rho-above-0.95", 160, 64, 330, 1e-3, 0.1, betas=(0.95, 0.98), seed=320))
    out.append(LazyCase("D512-rho-above-0.95", 64, 512, 300, 1e-2, 0.0, betas=(0.95, 0.98), seed=321))
    out.append(LazyCase("D768-rho-above-0.95", 64, 768, 300, 1e-3, 0.1, betas=(0.95, 0.98), seed=323))
    out.append(LazyCase("D260-other-betas", 96, 260, 330, 1e-3, 0.1, betas=(0.8, 0.98), seed=322))
    out.append(LazyCase("D4-past-the-launch-cap", LAZY_BIG_N, 4, 12, 1e-2, 0.1, seed=330, cap=LAZY_BIG_N + 2, big=True))
    out.append(LazyCase("D4-past-the-launch-cap-rho-above-0.95", LAZY_BIG_N, 4, 12, 1e-3, 0.1, betas=(0.95, 0.98), seed=331,
                        cap=LAZY_BIG_N + 2, big=True))
    return out


def _apply_list(rng, valid, cap):
    lst = np.concatenate([np.asarray(valid, dtype=np.int64), np.zeros(2, dtype=np.int64)])
    lst = lst[rng.permutation(lst.size)]
    ids = np.zeros(cap, dtype=np.int64)
    ids[:lst.size] = lst
    return ids, int(lst.size)


def lazy_inputs(c: LazyCase):
    """-> p0 and per step (apply ids [cap], count, gradient rows, raw catch-up ids | None).  Rows 1..7 are hot (every step or two),
    8..31 warm (gaps of tens to ~200 steps).  The cold rows 32.. get a gradient in the first steps, so that they carry moments, and
    are then left alone for hundreds of steps (a few return once, late in the run; the last four never get a gradient): the gaps
    beyond the replay window.  The raw catch-up lists name hot and warm rows only, so they do not shorten those gaps.
    big: every row gets a gradient in step 1 through ONE list longer than a trip of the grid-stride loop, two raw lists are as long,
    and so is the flush."""
    rng = np.random.default_rng(3000 + c.seed)
    p0 = make_params(rng, (c.N, c.D))
    steps = []
    if c.big:
        for k in range(c.T):
            if k == 0:
                valid = np.arange(1, c.N)
            else:
                valid = rng.choice(np.arange(1, c.N), size=40, replace=False)
            ids, n = _apply_list(rng, valid, c.cap)
            rows = make_grads(rng, n, c.D)
            raw = raw_ids(rng, c.N, 4 * 17500) if k in (3, 6) else None
            steps.append((ids, n, rows, raw))
        return p0, steps
    cold = np.arange(WARM, c.N - 4)
    for k in range(c.T):
        hot = rng.choice(np.arange(1, HOT), size=3, replace=False)
        warm = rng.choice(np.arange(HOT, WARM), size=1) if rng.random() < 0.4 else np.zeros(0, dtype=np.int64)
        if 16 * k < cold.size:
            late = cold[16 * k:16 * k + 16]                                   # the early gradient of the cold rows
        else:
            late = rng.choice(cold, size=1) if (k > 270 and rng.random() < 0.25) else np.zeros(0, dtype=np.int64)
        ids, n = _apply_list(rng, np.unique(np.concatenate([hot, warm, late])), c.cap)
        # (one late list names rows of the whole table: the claim form meets the tail too)
        raw = raw_ids(rng, c.N, 24, hi=None if k == 299 else WARM) if k % 5 == 4 else None
        steps.append((ids, n, make_grads(rng, c.cap, c.D), raw))
    return p0, steps


# ------------------------------------------------------------------------------------------------ drivers
# One driver per kernel family, shared by the emulation (CPU) and the library (GPU): the backend gets the very arrays the reference
# gets.  A backend has step / append / catch_up_raw / apply / flush as its family needs and result() -> (p, m, v) numpy arrays.
EPS = 1e-8


def run_flat(c: FlatCase, make_backend):
    p0, m0, v0, gs = flat_inputs(c)
    ref = Reference(p0, c.betas[0], c.betas[1], EPS, t0=c.t0, m0=m0, v0=v0)
    be = make_backend(p0, m0, v0)
    for k, lr in enumerate(c.lrs()):
        ref.step(gs[k], lr, c.wd)
        be.step(gs[k], lr, c.wd, c.t0 + k + 1)
    return ref, be


def run_table(c: TableCase, make_backend):
    p0, steps = table_inputs(c)
    ref = Reference(p0, c.betas[0], c.betas[1], EPS)
    be = make_backend(p0)
    for k, lr in enumerate(c.lrs()):
        ids, n, rows = steps[k]
        g = densify(c.N, c.D, ids, n, rows) if ids is not None else np.zeros((c.N, c.D), dtype=F32)
        ref.step(g, lr, c.wd)
        be.step(ids, n, rows, g, lr, c.wd, k + 1)
    return ref, be


def valid_rows(ids, N):
    ids = np.asarray(ids, dtype=np.int64)
    return np.unique(ids[(ids > 0) & (ids < N)])


def run_lazy(c: LazyCase, mode, make_backend):
    p0, steps = lazy_inputs(c)
    ref = Reference(p0, c.betas[0], c.betas[1], EPS)
    book = LazyBook(ref, c.N, mode, c.betas[0], c.betas[1])
    be = make_backend(p0)
    for k, lr in enumerate(c.lrs()):
        t = k + 1
        ids, n, rows, raw = steps[k]
        be.append(lr, c.wd, t)
        if raw is not None:
            book.bring_forward(valid_rows(raw, c.N), t - 1)
            be.catch_up_raw(raw, t - 1, k)
        touched = valid_rows(ids[:n], c.N)
        book.bring_forward(touched, t - 1)
        book.note_step(ref.step(densify(c.N, c.D, ids, n, rows), lr, c.wd))
        book.applied(touched, t)
        be.apply(ids, n, rows, t)
    book.bring_forward(np.arange(c.N), c.T)
    be.flush(c.T)
    if not c.big:          # the closed-form tail really is reached, in-run and at the flush, on rows that carry moments
        assert len(book.tail_gaps) >= 8 and max(book.tail_gaps) > WINDOW["exact"], (c.name, mode, book.tail_gaps)
    return ref, be


class EmuDense:
    """emu_adam_elem over whole arrays, every step: the flat kernels and the dense table sweep."""

    def __init__(self, p, m, v, betas, mutant=None, rng=None):
        self.p, self.m, self.v, self.betas, self.mutant, self.rng = p.copy(), m.copy(), v.copy(), betas, mutant, rng

    def step(self, g, lr, wd, t):
        h = emu_scalars(lr, wd, self.betas[0], self.betas[1], EPS, t, self.mutant)
        self.p, self.m, self.v = emu_adam_elem(self.p, self.m, self.v, np.asarray(g, dtype=F32).reshape(self.p.shape), h, self.mutant, self.rng)

    def result(self):
        return self.p, self.m, self.v


class EmuTable(EmuDense):
    def step(self, ids, n, rows, g, lr, wd, t):
        EmuDense.step(self, g, lr, wd, t)


class EmuLazyBackend:
    def __init__(self, p0, betas, window, rng=None, tail_mutant=None):
        z = np.zeros_like(p0)
        self.N = p0.shape[0]
        self.e = EmuLazy(p0, z, z, betas[0], betas[1], EPS, window, rng, tail_mutant)

    def append(self, lr, wd, t):
        self.e.append(lr, wd, t)

    def catch_up_raw(self, raw, t_prev, k):
        self.e.catch_up(valid_rows(raw, self.N), t_prev)

    def apply(self, ids, n, rows, t):
        self.e.apply(ids, n, rows, t)

    def flush(self, T):
        self.e.catch_up(np.arange(self.N), T)

    def result(self):
        return self.e.p, self.e.m, self.e.v
