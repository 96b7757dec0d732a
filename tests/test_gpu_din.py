"""DIN on the gfx950 kernels (csrc/din.hip): the training kernels against float64, the model against the golden fixture of the
reference's own DIN (loss, all seven gradients, predict, a 4-step AdamW trajectory), one step at the shipped widths, run-to-run and
hipGraph bit identity, the fused top-k against float64 and against the chunked predict, bad ids, checkpoints in the reference
layout, and main.py end to end.  Every test here needs the model or its kernels, so each fails without the feature."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pixelrec_amd import ops
from tests import din_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "din_tiny.npz")
U32 = 2.0 ** -24
# Fused scores: the largest error of the REFERENCE's own float32 predict ([B, N, L + 1] form, CPU) against the float64 restatement
# over the inputs of test_fused_topk_matches_float64 (R.topk_case, all 54 shapes), relative to the largest score magnitude of the
# case, measured as 2.28e-6 (hidden [12, 4], item_num 131, B 1, L 4: scores of magnitude 1.5e-3 that are sums of cancelling
# terms).  The kernel is allowed four times that: it sums in another order and the factorised first layer adds two roundings per
# term.  With this bound float64 alone excuses 0 of the 765 (user, rank) cells of those inputs.
FUSED_MEASURED = 2.284e-6
FUSED_TOL = 4 * FUSED_MEASURED


class _Data:
    def __init__(self, I):
        self.item_num = I


def _model(I, D, hidden, L=4, sd=None):
    from pixelrec_amd.model import DIN

    m = DIN({"embedding_size": D, "mlp_hidden_size": list(hidden), "dropout_prob": 0, "MAX_ITEM_LIST_LENGTH": L}, _Data(I))
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.cuda().train()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _gold_sd(g):
    return {str(k): torch.from_numpy(np.asarray(g["sd." + str(k)])) for k in g["sd.keys"]}


def _gold_model(g):
    I, D, L = (int(x) for x in g["meta"][:3])
    return _model(I, D, [int(x) for x in g["meta"][6:]], L=L, sd=_gold_sd(g))


def _opt(m, how="lazy", lr=1e-4, wd=0.1):
    from pixelrec_amd.optim import PxrAdamW

    return PxrAdamW(m, lr=lr, weight_decay=wd, table_update=how)


def _grad_of(m, name):
    """The dense gradient of a reference parameter: the Linears from the flat buffer, the table from the sparse rows."""
    if name == R.TABLE:
        return m.sparse_table_grad.to_dense(m.lazy_table().shape[0])[1:].cpu().numpy()
    return dict(m.named_parameters())[name].grad.cpu().numpy()


def _steps(m, opt, batches, which):
    losses = []
    for s in which:
        opt.zero_grad()
        loss = m(batches[s])
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    return losses


# ------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("B,L,D", [(1, 1, 4), (3, 4, 8), (5, 10, 64)])
def test_training_kernels_match_float64(B, L, D):
    """Attention input, head forward, head backward and the fold against float64 torch on the same float32 operands, hl = 12.
    Bounds (u = 2^-24; a float32 sum of n rounded products in any order is off by at most (n + 1) u sum|terms|):
      x = [q | k | q - k | q * k]: one IEEE operation per element -- bit-equal to torch's float32.
      s = (sum_j a_j w_j + bd) / sqrt(D): (hl + 4) u (sum|a w| + |bd|) / sqrt(D);   kq = <k, q>: (D + 1) u sum|k q|.
      loss: the scores sum L terms s kq, each off by (err_s |kq| + |s| err_kq + 2 u |s kq|); x_b = pos - neg; -log(sigmoid + 1e-8)
        is 1-Lipschitz in x, the mean and the norm add (B (L + 2) D + B + 8) u of their magnitude.
      dsraw = g coef kq / sqrt(D): coef is sigmoid' / (sigmoid + 1e-8) / B of a score off by err_x (|d coef / dx| <= 1 / B) plus 8 u.
      dz = dsraw w act': 3 u more.  dwd_j = sum_r dsraw a: (R + 1) u sum|terms| + sum|a| err_ds.
      occ: sums of 2 (history) or L (candidate) groups of four products, plus the regulariser: (4 L + 8) u sum|terms| on float32
        inputs s, head, dx taken from the kernels themselves (the fold's own arithmetic is what is bounded).
    Padding: s exactly 0, the slot's gidx 0 and its row zero.  The regulariser moves positive, negative and history rows alike."""
    rng = np.random.default_rng(100 * B + L)
    I, hl = 23, 12
    g = torch.Generator().manual_seed(B + L + D)
    table = torch.zeros(1 + I, D)
    table[1:] = torch.randn(I, D, generator=g) * 0.5
    prof = torch.from_numpy(rng.integers(1, I, size=(B, L)))
    if B >= 3:
        prof[1, :] = 0                                       # an all-padding row
        prof[2, :max(1, L // 2)] = 0                         # padded positions
        prof[0, -1] = prof[0, 0]                             # a repeated id within a row ...
        prof[2, -1] = prof[0, 0]                             # ... and across rows
    tgt = torch.from_numpy(rng.integers(1, I, size=(B, 2)))
    tgt[:, 1] = (tgt[:, 0] % (I - 1)) + 1                    # the negative differs from the positive
    if B >= 3:
        tgt[1, 0] = tgt[0, 1]                                # one sample's positive is another's negative
    table, prof, tgt = table.cuda(), prof.cuda(), tgt.cuda()
    rows, gidx = ops.din_rows(prof, tgt, I)
    ops.raise_on_bad_indices()
    assert torch.equal(rows, torch.cat((prof.view(-1), tgt.view(-1))) + 1)
    assert torch.equal(gidx, torch.where(torch.cat((prof.view(-1), tgt.view(-1))) == 0, 0, rows))
    emb, x = ops.din_att_input(table, rows, B, L)
    assert torch.equal(emb, table[rows])
    k32 = table[rows[:B * L]].view(B, L, D)
    q32 = table[rows[B * L:]].view(B, 2, D).transpose(0, 1)                        # [2, B, D]
    qq = q32[:, :, None, :].expand(2, B, L, D)
    kk = k32[None].expand(2, B, L, D)
    assert torch.equal(x.view(2, B, L, 4 * D), torch.cat((qq, kk, qq - kk, qq * kk), dim=-1))
    # ---- head forward
    alast = torch.rand(2 * B * L, hl, generator=g).cuda()
    dact = (alast * (1 - alast)).contiguous()
    wd, bd = (torch.randn(hl, generator=g) * 0.5).cuda(), torch.randn(1, generator=g).cuda()
    loss, s, kq, head = ops.din_head_fwd(alast, wd, bd, emb, prof)
    loss2, s2, kq2, head2 = ops.din_head_fwd(alast, wd, bd, emb, prof)
    assert torch.equal(head, head2) and torch.equal(s, s2) and torch.equal(kq, kq2)
    d = lambda t: t.double()
    mask = (prof == 0)[None].expand(2, B, L)
    sraw64 = (d(alast) @ d(wd) + d(bd)).view(2, B, L)
    s64 = sraw64.masked_fill(mask, 0.0) / D ** 0.5
    kq64 = (d(kk) * d(qq)).sum(-1)
    err_s = (hl + 4) * U32 * float(((d(alast).abs() @ d(wd).abs()) + d(bd).abs()).max()) / D ** 0.5
    err_kq = (D + 1) * U32 * float((d(kk) * d(qq)).abs().sum(-1).max())
    assert float((d(s).view(2, B, L) - s64).abs().max()) <= err_s
    assert float((d(kq).view(2, B, L) - kq64).abs().max()) <= err_kq
    assert float(s.view(2, B, L)[mask].abs().max() if mask.any() else 0.0) == 0                 # padding: exactly 0
    sc64 = (s64 * kq64).sum(-1)
    x64 = sc64[0] - sc64[1]
    nrm64 = d(emb).norm()
    loss64 = -(torch.log(torch.sigmoid(x64) + 1e-8)).mean() + 0.01 * nrm64 / B
    err_x = 2 * L * (err_s * float(kq64.abs().max()) + float(s64.abs().max()) * err_kq + (L + 2) * U32 * float((s64 * kq64).abs().max()))
    err_loss = err_x + (B * (L + 2) * D + B + 8) * U32 * (float(loss64.abs()) + 1.0)
    print("loss", float(loss), float(loss64), "bound", err_loss)
    assert abs(float(loss) - float(loss64)) <= err_loss
    assert float((d(head[2 + B:2 + 2 * B]) - x64).abs().max()) <= err_x
    sg = torch.sigmoid(x64)
    coef64 = -(1.0 / B) * sg * (1 - sg) / (sg + 1e-8)
    err_coef = err_x / B + 8 * U32 / B
    assert float((d(head[2:2 + B]) - coef64).abs().max()) <= err_coef
    assert abs(float(head[1]) - 0.01 / (B * float(nrm64))) <= (B * (L + 2) * D + 8) * U32 * 0.01 / (B * float(nrm64))
    # ---- head backward
    gsd = torch.full((1,), 0.75, device="cuda")
    gscale = 2.0
    gg = gscale * 0.75
    dwd, dbd = torch.empty(hl, device="cuda"), torch.empty(1, device="cuda")
    dz, dsraw = ops.din_head_bwd(alast, dact, wd, prof, kq, head, D, dwd, dbd, gscale, gsd)
    sign = torch.tensor([1.0, -1.0], device="cuda", dtype=torch.float64).view(2, 1, 1)
    ds64 = (gg * sign * coef64.view(1, B, 1) * kq64 / D ** 0.5).masked_fill(mask, 0.0)
    err_ds = gg * (err_coef * float(kq64.abs().max()) + float(coef64.abs().max()) * err_kq) / D ** 0.5 + 6 * U32 * float(ds64.abs().max())
    assert float((d(dsraw).view(2, B, L) - ds64).abs().max()) <= err_ds
    assert float(dsraw.view(2, B, L)[mask].abs().max() if mask.any() else 0.0) == 0
    dz64 = ds64.reshape(-1, 1) * d(wd) * d(dact)
    assert float((d(dz) - dz64).abs().max()) <= (err_ds + 4 * U32 * float(ds64.abs().max())) * float(wd.abs().max()) * 0.25
    Rr = 2 * B * L
    dwd64 = (ds64.reshape(-1, 1) * d(alast)).sum(0)
    tol_dwd = (Rr + 1) * U32 * float((ds64.reshape(-1, 1) * d(alast)).abs().sum(0).max()) + Rr * err_ds
    assert float((d(dwd) - dwd64).abs().max()) <= tol_dwd
    assert abs(float(dbd) - float(ds64.sum())) <= (Rr + 1) * U32 * float(ds64.abs().sum()) + Rr * err_ds
    # ---- fold: the kernel's own float32 s / head, a random dx
    dx = (torch.randn(2 * B * L, 4 * D, generator=g) * 0.1).cuda()
    occ = ops.din_fold_bwd(dx, emb, prof, s, head, gscale, gsd)
    assert torch.equal(occ, ops.din_fold_bwd(dx, emb, prof, s, head, gscale, gsd))
    dx4 = d(dx).view(2, B, L, 4, D)
    coefk, regk = d(head[2:2 + B]).view(1, B, 1, 1), float(head[1]) * gg
    gs = gg * sign.view(2, 1, 1, 1) * coefk * d(s).view(2, B, L, 1)
    hist_terms = [gs * d(qq), dx4[:, :, :, 1], -dx4[:, :, :, 2], dx4[:, :, :, 3] * d(qq)]
    cand_terms = [gs * d(kk), dx4[:, :, :, 0], dx4[:, :, :, 2], dx4[:, :, :, 3] * d(kk)]
    hist64 = sum(hist_terms).sum(0) + regk * d(k32)                                  # [B, L, D]
    cand64 = sum(cand_terms).sum(2) + regk * d(q32)                                  # [2, B, D]
    habs = sum(t.abs() for t in hist_terms).sum(0) + abs(regk) * d(k32).abs()
    cabs = sum(t.abs() for t in cand_terms).sum(2) + abs(regk) * d(q32).abs()
    pad = (prof == 0)
    hist64 = hist64.masked_fill(pad[:, :, None], 0.0)
    got_h, got_c = d(occ[:B * L]).view(B, L, D), d(occ[B * L:]).view(B, 2, D).transpose(0, 1)
    assert float((got_h - hist64).abs().max()) <= (4 * L + 8) * U32 * float(habs.max())
    assert float((got_c - cand64).abs().max()) <= (4 * L + 8) * U32 * float(cabs.max())
    assert float(occ[:B * L][pad.view(-1)].abs().max() if pad.any() else 0.0) == 0
    assert bool((gidx[:B * L][pad.view(-1)] == 0).all())
    # the regulariser is part of every kind of row: without it the float64 value is ten bounds away
    real = ~pad
    reg_h, reg_c = (regk * d(k32)).abs(), (regk * d(q32)).abs()
    if real.any():
        assert float(reg_h[real].max()) > 10 * (4 * L + 8) * U32 * float(habs.max())
    assert float(reg_c[0].max()) > 10 * (4 * L + 8) * U32 * float(cabs.max()) and float(reg_c[1].max()) > 10 * (4 * L + 8) * U32 * float(cabs.max())
    # the sparse rows: one slot per occurrence, reduced by id; id 0 never appears
    sp = ops.embed_grad_rows(gidx, occ, 1 + I)
    n = sp.count()
    ids = torch.cat((prof.view(-1), tgt.view(-1)))
    assert sorted(sp.idx[:n].tolist()) == sorted(set((ids[ids != 0] + 1).tolist()))
    dense64 = torch.zeros(1 + I, D, dtype=torch.float64, device="cuda").index_add_(0, gidx, d(occ))
    dense64[0] = 0
    assert float((d(sp.to_dense(1 + I)) - dense64).abs().max()) <= (B * (L + 2) + 1) * U32 * float(occ.abs().max()) * B * (L + 2)


# ------------------------------------------------------------------------------------------------------------ the fixture
def _dist32(gold):
    """Distances of the float32 restatement (the reference's arithmetic) from the float64 restatement on the fixture's inputs."""
    rows = gold["rows"]
    lr, wd = (float(x) for x in gold["optim"])
    res = {}
    for dt in (torch.float64, torch.float32):
        P = R.state_from(gold, "sd.", dt)
        L, g = R.loss_and_grads(P, rows[0])
        sc = R.predict_literal(P, gold["eval.windows"])
        losses = R.adamw(P, list(rows), lr, wd)
        res[dt] = (L, g, sc, losses, P)
    a, b = res[torch.float64], res[torch.float32]
    out = {"loss": abs(a[0] - b[0]), "scores": float((a[2] - b[2].double()).abs().max())}
    for k in R.names(2):
        out["grad." + k] = float((a[1][k] - b[1][k].double()).abs().max())
        out["final." + k] = float((a[4][k] - b[4][k].double()).abs().max())
    for s in range(len(rows)):
        out[f"loss{s}"] = abs(a[3][s] - b[3][s])
    return out, a


def test_model_matches_the_reference_fixture(gold):
    """Tolerances: the ones tests/test_gpu_acf.py::test_model_matches_the_reference_fixture uses for the same quantities (loss 2e-6,
    gradients 1e-5 of the largest entry, scores 2e-5, trajectory losses 5e-6, final weights 5e-6 of the largest entry), each
    alternatively twice the distance of the float32 restatement from the float64 restatement measured on the same inputs (a factor
    2 for a different summation order), with the native result then compared against float64 -- ACF's rule, unchanged.  The
    fused top-k on the fixture's windows: values within FUSED_TOL of the float64 scores, ids equal (the generator kept adjacent
    float64 scores down to rank K + 1 more than 1e-5 apart); the all-padding window is compared on values only."""
    d32, ref64 = _dist32(gold)
    print(d32)
    m = _gold_model(gold)
    rows = torch.from_numpy(gold["rows"]).cuda()
    loss = m(rows[0])
    loss.backward()
    loss = loss.detach()
    ops.raise_on_bad_indices()
    print("loss", float(loss), float(gold["loss"]))
    assert (abs(float(loss) - float(gold["loss"])) <= 2e-6 * max(1.0, float(gold["loss"]))
            or abs(float(loss) - ref64[0]) <= 2 * d32["loss"])
    for k in R.names(2):
        ref = gold["grad." + k]
        got = _grad_of(m, k).reshape(ref.shape)
        err, err64 = np.abs(got - ref).max(), np.abs(got - ref64[1][k].numpy()).max()
        print("grad", k, err, err64, np.abs(ref).max())
        assert err <= 1e-5 * max(1.0, np.abs(ref).max()) or err64 <= 2 * d32["grad." + k], k
    assert np.abs(_grad_of(m, R.TABLE)[0]).max() == 0                              # the padding row never receives a gradient
    m.eval()
    feat = m.compute_item_all()
    win = torch.from_numpy(gold["eval.windows"]).cuda()
    I, L, K = int(gold["meta"][0]), int(gold["meta"][2]), int(gold["meta"][4])
    form = torch.zeros(len(win), I, L + 1, dtype=torch.int64, device="cuda")
    form[:, :, :L] = win[:, None, :]
    form[:, :, L] = torch.arange(I, device="cuda")[None]
    for scores in (m.predict(form, feat), m.predict(win, feat)):                   # the reference's form, and the window form
        err = np.abs(scores.cpu().numpy() - gold["eval.scores"]).max()
        print("scores", err)
        assert err <= 2e-5
        assert float(scores[(win != 0).sum(1) == 0].abs().max()) == 0             # all padding: exactly 0
    idx, val = m.fused_topk(win, None, None, K)
    ops.raise_on_bad_indices()
    s64 = ref64[2].clone()
    s64[:, 0] = float("-inf")
    top = torch.topk(s64, K, dim=-1)
    tol = FUSED_TOL * float(ref64[2].abs().max())
    assert float((val.cpu().double() - top.values).abs().max()) <= tol
    real = (win != 0).any(1).cpu()
    assert torch.equal(idx.cpu()[real], top.indices[real])
    lr, wd = (float(x) for x in gold["optim"])
    for how in ("lazy", "dense"):
        m2 = _gold_model(gold)
        opt = _opt(m2, how, lr, wd)
        for s, loss in enumerate(_steps(m2, opt, rows, range(len(rows)))):
            print(how, "trajectory loss", s, float(loss), float(gold[f"adamw.loss{s}"]))
            assert (abs(float(loss) - float(gold[f"adamw.loss{s}"])) <= 5e-6 * max(1.0, float(loss))
                    or abs(float(loss) - ref64[3][s]) <= 2 * d32[f"loss{s}"]), (how, s)
        sd = m2.state_dict()
        assert list(sd) == R.names(2)
        for k, v in sd.items():
            ref = gold["adamw.final." + k]
            err = np.abs(v.cpu().numpy() - ref).max()
            err64 = np.abs(v.cpu().numpy() - ref64[4][k].numpy()).max()
            print(how, "final", k, err, err64, d32["final." + k])
            assert err <= 5e-6 * max(1.0, np.abs(ref).max()) or err64 <= 2 * d32["final." + k], (how, k)
        # row 0 (decayed, never given a gradient) and the rows no batch touched follow the reference
        touched = set(gold["rows"].reshape(-1).tolist())
        for i in [0] + [i for i in range(I) if i not in touched]:
            assert np.abs(sd[R.TABLE][i].cpu().numpy() - gold["adamw.final." + R.TABLE][i]).max() <= 5e-6, (how, i)
        assert not np.array_equal(sd[R.TABLE][0].cpu().numpy(), gold["sd." + R.TABLE][0])


def _wide_batch(rng, I, L, B):
    prof = rng.integers(1, I, size=(B, L))
    n_real = rng.integers(0, L + 1, size=B)
    n_real[:2] = 0
    n_real[2:4] = L
    prof[np.arange(L)[None, :] < (L - n_real)[:, None]] = 0
    pos = rng.integers(1, I, size=B)
    neg = (pos + rng.integers(1, I - 1, size=B) - 1) % (I - 1) + 1
    return torch.from_numpy(np.concatenate((prof, pos[:, None], neg[:, None]), axis=1))


def test_a_step_at_the_shipped_widths_matches_float64():
    """One training step at D = 64, hidden [80, 40], L = 10, B = 64, item_num = 257 against the float64 restatement on the same
    device.  tests/test_gpu_acf.py::test_a_step_at_the_shipped_width_matches_float64_and_touches_only_its_rows's rule: each quantity
    is allowed twice the float32 restatement's distance from float64 on the same inputs plus, for the loss, 2e-6 relative and, for
    the gradients, 1e-6 of the largest entry."""
    rng = np.random.default_rng(31)
    I, D, L, B = 257, 64, 10, 64
    torch.manual_seed(5)
    m = _model(I, D, [80, 40], L=L)
    rows = _wide_batch(rng, I, L, B).cuda()
    loss = m(rows)
    loss.backward()
    ops.raise_on_bad_indices()
    sp = m.sparse_table_grad
    ids = rows.view(-1)
    assert sorted(sp.idx[:sp.count()].tolist()) == sorted(set((ids[ids != 0] + 1).tolist()))
    res = {}
    for dt in (torch.float64, torch.float32):
        P = {k: v.detach().to(dt) for k, v in m.state_dict().items()}
        res[dt] = R.loss_and_grads(P, rows)
    (L64, g64), (L32, g32) = res[torch.float64], res[torch.float32]
    print("loss", float(loss), L64, "float32 restatement", L32)
    assert abs(float(loss) - L64) <= 2 * abs(L32 - L64) + 2e-6 * max(1.0, abs(L64))
    for k in R.names(2):
        got = torch.from_numpy(_grad_of(m, k)).cuda().double().view(g64[k].shape)
        err, d32 = float((got - g64[k]).abs().max()), float((g32[k].double() - g64[k]).abs().max())
        big = float(g64[k].abs().max())
        print("grad", k, "err", err, "float32 restatement", d32, "largest entry", big)
        assert err <= 2 * d32 + 1e-6 * big, k


def test_two_runs_and_graph_replay_are_bit_identical_to_eager_steps():
    from pixelrec_amd.graph import GraphedTrainStep

    rng = np.random.default_rng(8)
    I, D, L, B, hidden = 60, 16, 5, 16, [12, 4]
    torch.manual_seed(1)
    sd = {k: v.cpu() for k, v in _model(I, D, hidden, L).state_dict().items()}
    batches = [_wide_batch(rng, 30 if s % 3 else I, L, B).cuda() for s in range(6)]
    out = {}
    for how in ("eager", "eager again", "graph"):
        m = _model(I, D, hidden, L, sd={k: v.clone() for k, v in sd.items()})
        opt = _opt(m, lr=1e-3, wd=0.01)
        losses = []
        split = lambda r: (r[:, :L].contiguous(), r[:, L:].contiguous())       # the batcher's two tensors
        gs = GraphedTrainStep(m, opt, *split(batches[0]), warmup=0) if how == "graph" else None
        for r in batches:
            if gs is not None:
                loss = gs(*split(r))
            else:
                opt.zero_grad()
                loss = m(r)
                loss.backward()
                opt.step()
            losses.append(loss.detach().clone())
        opt.flush()
        torch.cuda.synchronize()
        assert opt.step_count == len(batches)
        out[how] = [torch.stack(losses).view(-1)] + [v.clone() for v in m.state_dict().values()] + \
                   [opt._m.clone(), opt._v.clone(), opt._tm.clone(), opt._tv.clone()]
    assert len(set(out["eager"][0].tolist())) == len(batches)             # different batches, different losses
    for how in ("eager again", "graph"):
        for a, b in zip(out["eager"], out[how]):
            assert torch.equal(a, b), how


# ------------------------------------------------------------------------------------------------------------ evaluation
def _compare_topk(idx, val, s64_masked, K, tol_abs, real=None):
    """ids equal wherever the float64 gaps around that rank exceed tol_abs; values within tol_abs.  -> (cells, excused).  real
    [B] bool: False marks an all-padding window, which scores exactly 0 for every item -- compared on values only, never on
    ids, and not counted."""
    N = s64_masked.shape[1]
    top = torch.topk(s64_masked, min(K + 1, N), dim=-1)
    v, ix = top.values, top.indices
    cells = excused = 0
    for b in range(idx.shape[0]):
        for r in range(K):
            if r >= v.shape[1] or v[b, r] == float("-inf"):
                assert int(idx[b, r]) == -1 and float(val[b, r]) == float("-inf"), (b, r)      # fewer than K unmasked items
                continue
            assert abs(float(val[b, r]) - float(v[b, r])) <= tol_abs, (b, r, float(val[b, r]), float(v[b, r]))
            if real is not None and not bool(real[b]):
                assert float(val[b, r]) == 0.0, (b, r)
                continue
            cells += 1
            gaps = []
            if r > 0:
                gaps.append(float(v[b, r - 1] - v[b, r]))
            if r + 1 < v.shape[1] and v[b, r + 1] > float("-inf"):
                gaps.append(float(v[b, r] - v[b, r + 1]))
            if gaps and min(gaps) <= tol_abs:
                excused += 1
            else:
                assert int(idx[b, r]) == int(ix[b, r]), (b, r)
    return cells, excused


def _csr(hist, B):
    hu = torch.tensor([b for b in range(B) for _ in hist[b]], dtype=torch.int64)
    hi = torch.tensor([i for b in range(B) for i in hist[b]], dtype=torch.int64)
    return ops.history_csr(hu, hi, B, "cuda")


@pytest.mark.parametrize("hidden", list(R.TOPK_HIDDEN))
@pytest.mark.parametrize("item_num", R.TOPK_ITEM_NUMS)
def test_fused_topk_matches_float64(item_num, hidden):
    """pxr_din_topk_f32 against float64 scores (the factorised restatement, itself checked against the literal one on the CPU)
    with column 0 and the full histories masked and a float64 top-K: B in {1, 3}, L in {1, 4, 10}, K = 10; item_num 131 and 257
    end in a partial item tile.  Histories are longer than the window (masked, no part in the attention), user 0's masks its float64
    top-3, the last user of a B = 3 batch keeps fewer than K items.  Ids must be equal wherever the float64 gap at that rank
    exceeds FUSED_TOL x the largest score magnitude, values within it (measured 2.28e-6 x 4 = 9.14e-6, see FUSED_MEASURED); at
    most 2 % of the (user, rank) cells may be excused by the gap rule (float64 alone: 0 of 765)."""
    K = R.TOPK_K
    cells = excused = 0
    for B in R.TOPK_BS:
        for L in R.TOPK_LS:
            P, win, hist = R.topk_case(item_num, B, L, hidden)
            s64 = R.predict_factorised({k: v.double() for k, v in P.items()}, win)
            hist = R.topk_histories(s64, hist)
            _, masked = R.masked_topk(s64, hist, 1)
            # longer than the window: items outside it are masked too (unless the window's own items already cover the catalogue)
            assert all(set(w[w != 0].tolist()) < set(h) or len(h) == item_num - 1 for h, w in zip(hist, win))
            m = _model(item_num, R.TOPK_HIDDEN[tuple(hidden)], hidden, L=L, sd=P).eval()
            assert m.fused_topk_supported
            ptr, items = _csr(hist, B)
            idx, val = m.fused_topk(win.cuda(), ptr, items, K)
            ops.raise_on_bad_indices()
            tol_abs = FUSED_TOL * float(s64.abs().max())
            c, e = _compare_topk(idx.cpu(), val.cpu().double(), masked, K, tol_abs)
            live = val.cpu() > float("-inf")                                        # (a user may have no unmasked item at all)
            diff = (val.cpu().double() - torch.topk(masked, min(K, item_num), -1).values[:, :K])[live].abs()
            err = float(diff.max()) if diff.numel() else 0.0
            print(f"N={item_num} hidden={hidden} B={B} L={L}: value error {err:.3e} (bound {tol_abs:.3e}), excused {e}/{c}")
            if B == 3:
                assert int((idx[2] >= 0).sum()) < K                                 # fewer than K unmasked items: padded with -1
            cells, excused = cells + c, excused + e
    assert excused <= 0.02 * cells, (excused, cells)


def test_fused_topk_equals_chunked_predict_and_the_cache_follows_training():
    """The fused path against predict([B, L]) -> masks -> torch.topk to the same rule.  The chunked path's float32 scores stand in
    for float64; it is the reference's arithmetic in float32, whose distance from float64 is what FUSED_MEASURED measures, so the
    bound is FUSED_TOL + FUSED_MEASURED = five times the measured figure, relative to the largest score magnitude (the scores of a
    freshly initialised model are of magnitude 1e-2: an absolute bound would excuse every rank).  A q + b1 is cached, dropped by
    train(), and a
    training step changes the fused result's values; hidden width 132 reports fused_topk_supported == False."""
    rng = np.random.default_rng(3)
    I, D, L, B, K, hidden = 300, 64, 10, 24, 10, [80, 40]
    torch.manual_seed(11)
    m = _model(I, D, hidden, L=L).eval()
    win = _wide_batch(rng, I, L, B)[:, :L].contiguous()
    hist = [sorted(set(w[w != 0].tolist()) | set(rng.integers(1, I, size=7).tolist())) for w in win]
    ptr, items = _csr(hist, B)
    idx, val = m.fused_topk(win.cuda(), ptr, items, K)
    assert m._eval_cache is not None
    cache = m._eval_cache[0]
    scores = m.predict(win.cuda(), m.compute_item_all())
    assert scores.shape == (B, I)
    _, masked = R.masked_topk(scores.double().cpu(), hist, 1)
    tol_abs = (FUSED_TOL + FUSED_MEASURED) * float(scores.abs().max())
    ref_top = torch.topk(masked, K, -1).values
    print("largest score", float(scores.abs().max()), "largest value difference", float((val.cpu().double() - ref_top).abs().max()),
          "bound", tol_abs)
    real = (win != 0).any(1)
    assert int((~real).sum()) >= 2                                                  # _wide_batch: all-padding windows
    cells, excused = _compare_topk(idx.cpu(), val.cpu().double(), masked, K, tol_abs, real)
    print("excused", excused, "of", cells)
    assert excused <= 0.02 * cells
    m.train()
    assert m._eval_cache is None
    opt = _opt(m, lr=1e-2, wd=0.01)
    _steps(m, opt, [_wide_batch(rng, I, L, 16).cuda()], [0])
    m.eval()
    idx2, val2 = m.fused_topk(win.cuda(), ptr, items, K)
    assert m._eval_cache[0] is not cache and not torch.equal(val, val2)
    scores2 = m.predict(win.cuda(), m.compute_item_all())
    _, masked2 = R.masked_topk(scores2.double().cpu(), hist, 1)
    _compare_topk(idx2.cpu(), val2.cpu().double(), masked2, K, (FUSED_TOL + FUSED_MEASURED) * float(scores2.abs().max()), real)
    wide = _model(I, D, [132], L=L)
    assert wide.fused_topk_supported is False and m.fused_topk_supported is True


def test_bad_ids_raise_index_error(gold):
    m = _gold_model(gold)
    I, L = int(gold["meta"][0]), int(gold["meta"][2])
    good = torch.from_numpy(gold["rows"][0]).cuda()
    ops.raise_on_bad_indices()
    for col, val in ((0, I), (L, I), (L + 1, -2), (1, -1)):
        bad = good.clone()
        bad[0, col] = val
        m(bad).backward()
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices()
    m(good).backward()
    ops.raise_on_bad_indices()                             # a clean batch leaves the word clear
    m.eval()
    win = torch.from_numpy(gold["eval.windows"]).cuda()
    ptr, items = _csr([[1, 2]] * len(win), len(win))
    for where in ("window", "history"):
        w, it = win.clone(), items.clone()
        if where == "window":
            w[0, -1] = I
        else:
            it[3] = I + 5
        idx = m.fused_topk_batch(w, ptr, it, 5)
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices()
    with pytest.raises(IndexError):
        w = win.clone()
        w[0, -1] = I
        m.predict(w, m.compute_item_all())
    m.fused_topk_batch(win, ptr, items, 5)
    ops.raise_on_bad_indices()


def test_checkpoint_loads_into_the_reference_layout_and_resumes_the_trajectory(gold, tmp_path, monkeypatch):
    monkeypatch.setenv("PXR_LAZY_REPLAY", "exact")     # flushed and lagging rows then replay the dense sweep's own arithmetic
    rows = torch.from_numpy(gold["rows"]).cuda()
    names = R.names(2)
    ref = _gold_model(gold)
    _steps(ref, _opt(ref), rows, range(4))
    a = _gold_model(gold)
    opt = _opt(a)
    _steps(a, opt, rows, range(2))
    ck = {"state_dict": {k: v.detach().cpu() for k, v in a.state_dict().items()}, "optimizer": opt.state_dict(layout="torch")}
    path = tmp_path / "din.pth"
    torch.save(ck, path)
    ck = torch.load(path, weights_only=False)
    assert list(ck["state_dict"].keys()) == names
    assert ck["optimizer"]["param_groups"][0]["params"] == list(range(len(names)))  # the reference's seven parameters
    for j, n in enumerate(names):
        assert tuple(ck["optimizer"]["state"][j]["exp_avg"].shape) == tuple(ck["state_dict"][n].shape), n
    tor = [torch.nn.Parameter(ck["state_dict"][n].clone()) for n in names]
    topt = torch.optim.AdamW(tor, lr=1.0, weight_decay=0.5)
    topt.load_state_dict(ck["optimizer"])                  # strict layout: torch's own loader
    assert (topt.param_groups[0]["lr"], topt.param_groups[0]["weight_decay"]) == (1e-4, 0.1)
    b = _gold_model(gold)
    b.load_state_dict(ck["state_dict"], strict=True)
    opt_b = _opt(b)
    opt_b.load_state_dict(ck["optimizer"])
    _steps(b, opt_b, rows, range(2, 4))
    sr, sb = ref.state_dict(), b.state_dict()
    for k in sr:
        assert torch.equal(sr[k], sb[k]), k


def test_main_py_trains_two_epochs_and_reports_recall_and_ndcg(tmp_path):
    from pixelrec_amd.config import Config
    from pixelrec_amd.data import bulid_dataloader, load_data
    from pixelrec_amd.utils.utils import get_model

    os.makedirs(tmp_path / "data")
    with open(os.path.join(ROOT, "tests", "golden", "TinyInter.csv")) as f:
        (tmp_path / "data" / "TinyInter.csv").write_text(f.read())
    shipped = [os.path.join(ROOT, "configs", "IDNet", "din.yaml"), os.path.join(ROOT, "configs", "overall", "ID.yaml")]
    (tmp_path / "o.yaml").write_text(f"state: INFO\nreproducibility: True\ncheckpoint_dir: '{tmp_path}/saved'\nlog_path: '{tmp_path}/log'\n"
                                     f"data_path: {tmp_path}/data/\ndataset: TinyInter\nepochs: 2\ntrain_batch_size: 64\n"
                                     "eval_batch_size: 64\noptim_args: {learning_rate: 0.001, weight_decay: 0.01}\n")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "OMP_NUM_THREADS")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--device", "0", "--config_file", *shipped,
                        str(tmp_path / "o.yaml")], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    epochs = re.findall(r"epoch \d+ training \[time: [0-9.]+s, train loss: ([0-9.]+)\]", out)
    assert len(epochs) == 2, out[-3000:]
    assert "training step captured as a hipGraph (batch size 64)" in out, out[-3000:]
    assert "Loading model structure and parameters from" in out, out[-3000:]     # the test result comes from the checkpoint
    for metric in ("recall@5", "ndcg@5", "recall@10", "ndcg@10"):
        mm = re.search(r"test result: .*?'%s', ([0-9.]+)\)" % metric, out)
        assert mm is not None and 0.0 <= float(mm.group(1)) <= 1.0 and np.isfinite(float(mm.group(1))), out[-2000:]
    # the mean step loss of the second epoch against the loss of the first step of a freshly initialised model on this data
    config = Config(shipped + [str(tmp_path / "o.yaml")])
    data = load_data(config)
    train_loader = bulid_dataloader(config, data)[0]
    torch.manual_seed(int(config["seed"]))
    fresh = get_model("DIN")(config, data).cuda().train()
    first = float(fresh(tuple(t.cuda() for t in next(iter(train_loader)))))
    mean_last = float(epochs[1]) / len(train_loader)
    print("first step loss", first, "mean step loss of epoch 2", mean_last)
    assert np.isfinite(first) and mean_last < first
