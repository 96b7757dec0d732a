"""DSSM and FM on the gfx950 kernels (csrc/pool.hip, MODE_POOL of csrc/embed_grad.hip): the kernels against float64, the MODE_POOL
segment sum against the materialised rows, the models against the golden fixtures of the reference's own DSSM and FM (loss, every
gradient, predict, a 4-step AdamW trajectory, a one-row batch), dropout under the library's keep masks, run-to-run and hipGraph bit
identity, the fused top-k, bad ids, checkpoints in the reference layout, and main.py end to end.  Every test here needs the models
or their kernels, so each fails without the feature.

Bounds are analytic in u = 2^-24 (tests/pool_restate.py `analytic` carries them next to the float64 values): a float32 sum of n
rounded products in any order is off by at most (n + 1) u sum|terms|; the library GEMMs by (K + 4) u sum|terms|."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pixelrec_amd import lib, ops
from tests import pool_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
U32 = 2.0 ** -24
CASES = {"dssm_tiny": ("DSSM", []), "dssm_mlp_tiny": ("DSSM", [8, 12, 8]), "fm_tiny": ("FM", [])}


class _Data:
    def __init__(self, I):
        self.item_num = I


def _model(kind, I, D, hidden=(), L=4, sd=None, p=0.0):
    from pixelrec_amd import model

    m = getattr(model, kind)({"embedding_size": D, "mlp_hidden_size": list(hidden), "dropout_prob": p, "MAX_ITEM_LIST_LENGTH": L},
                             _Data(I))
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.cuda().train()


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    kind, hidden = CASES[request.param]
    return kind, hidden, np.load(os.path.join(GOLD, request.param + ".npz"))


def _gold_sd(g):
    return {str(k): torch.from_numpy(np.asarray(g["sd." + str(k)])) for k in g["sd.keys"]}


def _gold_model(kind, hidden, g, p=0.0):
    I, D, L = (int(x) for x in g["meta"][:3])
    return _model(kind, I, D, hidden, L=L, sd=_gold_sd(g), p=p)


def _opt(m, how="lazy", lr=1e-4, wd=0.1):
    from pixelrec_amd.optim import PxrAdamW

    return PxrAdamW(m, lr=lr, weight_decay=wd, table_update=how)


def _inp(kind, rows):
    """The reference's input form of [B, L + 2] rows: DSSM takes them as they are, FM as [B, 2, L + 1]."""
    return R.fm_form(rows).cuda() if kind == "FM" else torch.as_tensor(rows).cuda()


def _grad_of(m, name):
    """The dense gradient of a reference parameter: the Linears from the flat buffer, the table from the sparse rows."""
    if name == R.TABLE:
        return m.sparse_table_grad.to_dense(m.lazy_table().shape[0])[1:].cpu().double()
    return dict(m.named_parameters())[name].grad.cpu().double()


def _within(got, want, bound, what):
    """got within `bound` of want, elementwise (a bound of exactly 0 demands equality)."""
    got, want, bound = (torch.as_tensor(t).double().cpu() for t in (got, want, bound))
    over = (got - want).abs() - bound
    assert float(over.max()) <= 0, (what, float((got - want).abs().max()), float(bound.max()))


# ------------------------------------------------------------------------------------------------------------ kernels
def _edge_batch(B, L, I, seed):
    """test_gpu_din.py's edge rows: all padding, partial padding, a repeated id within and across rows, a positive that is another
    row's negative -- and a positive inside its own profile."""
    rng = np.random.default_rng(seed)
    prof = torch.from_numpy(rng.integers(1, I, size=(B, L)))
    tgt = torch.from_numpy(rng.integers(1, I, size=(B, 2)))
    if B >= 3:
        prof[1, :] = 0                                       # an all-padding row
        prof[2, :max(1, L // 2)] = 0                         # padded positions
        prof[0, -1] = prof[0, 0]                             # a repeated id within a row ...
        prof[2, -1] = prof[0, 0]                             # ... and across rows
        tgt[0, 0] = prof[0, 0]                               # a positive inside its own profile
    elif B == 2:
        prof[1, 0] = 0
    tgt[:, 1] = (tgt[:, 0] % (I - 1)) + 1                    # the negative differs from the positive
    if B >= 3:
        tgt[1, 0] = tgt[0, 1]                                # one sample's positive is another's negative
        tgt[1, 1] = (tgt[1, 0] % (I - 1)) + 1
    return prof, tgt


@pytest.mark.parametrize("mean", [False, True], ids=["sum", "mean"])
@pytest.mark.parametrize("B,L,D", [(1, 1, 4), (3, 4, 8), (5, 10, 64), (3, 4, 260), (2, 3, 4096), (3, 4, 2052)])
def test_kernels_match_float64(B, L, D, mean):
    """pool_rows, pool_pair_fwd, pool_pair_bwd and pool_table_grad against float64 torch on the same float32 operands, both
    pooling modes.  D = 260: a row ends inside a 64-lane chunk; 4096: the widest instantiation and the segment sum's
    one-row-per-workgroup path; 2052: just past that path's threshold.  Bounds (u = 2^-24):
      U = the sum of <= L rows [then the division]: (L + 2) u sum|terms| (the float32 cnt + 1e-8 is cnt itself: 1e-8 / cnt, below u);
      x = <U, p> - <U, n>: (D + 1) u sum|U p| + sum|U n| plus U's error carried through (|p| + |n|); lossrow and loss are
        1-Lipschitz in x (+ 8 u for expf / logf, (B + 2) u for the mean); coef: |d coef / d x| <= 1 / B;
      G from the kernel's own float32 coef and U: c = coef (grad_scale grad_scale_dev) is two roundings, the product a third
        (3 u |value|); the history row's p - n is rounded too (4 u |value|);
      table gradient from the kernel's own G and w: (count + 1) u sum|terms| per row.
    Then the whole chain against the float64 chain with the errors carried (pool_restate.analytic).  Exact: U of an empty profile is
    0, w is bit-equal to torch's float32 1 / (cnt + 1e-8) (0 for an empty profile; 1 in sum mode), padding never appears in
    uniq_idx, pool_rows / pool_pair_fwd / the evaluation form (item matrix + window ids) give the same bits, two runs too."""
    I, kind = 23, ("DSSM" if mean else "FM")
    g = torch.Generator().manual_seed(B + L + D)
    table = torch.zeros(1 + I, D)
    table[1:] = torch.randn(I, D, generator=g) * 0.5         # row 1 = item 0, the padding item: a row like any other, never pooled
    prof, tgt = _edge_batch(B, L, I, 100 * B + L)
    rows_np = torch.cat((prof, tgt), 1)
    table, prof, tgt = table.cuda(), prof.cuda(), tgt.cuda()
    rows, gidx = ops.din_rows(prof, tgt, I)
    ops.raise_on_bad_indices()
    d = lambda t: t.double()
    gscale, gsd = 2.0, torch.full((1,), 0.75, device="cuda")
    gg = gscale * 0.75
    a = R.analytic(kind, {R.TABLE: table[1:]}, rows_np.cuda(), gscale=gg)
    # ---- pooling
    U, w = ops.pool_rows(table, rows, B, L, mean)
    loss, coef, U2, w2, lossrow = ops.pool_pair_fwd(table, rows, B, L, mean)
    Ue, we = ops.pool_rows(table[1:], prof, B, L, mean, pad_row=0)               # the evaluation form
    assert torch.equal(U, U2) and torch.equal(w, w2) and torch.equal(U, Ue) and torch.equal(w, we)
    _within(U, *a["U"], "U")
    cnt = (prof != 0).sum(1).cpu().float()
    w_torch = torch.where(cnt > 0, 1.0 / (cnt + 1e-8), torch.zeros(())) if mean else (cnt > 0).float()
    assert torch.equal(w.cpu(), w_torch)
    empty = (cnt == 0)
    if empty.any():
        assert float(U[empty.cuda()].abs().max()) == 0 and float(w[empty.cuda()].abs().max()) == 0
    # ---- head forward
    x64, ex = a["x"]
    lossrow64 = -torch.log(1e-8 + torch.sigmoid(x64))
    _within(lossrow, lossrow64, ex + 8 * U32 * (1 + lossrow64.abs()), "lossrow")
    _within(loss.view(()), *a["loss"], "loss")
    _within(coef, *a["coef"], "coef")
    loss_b, coef_b, _, _, _ = ops.pool_pair_fwd(table, rows, B, L, mean)
    assert torch.equal(loss, loss_b) and torch.equal(coef, coef_b)
    # ---- head backward: from the kernel's own coef and U, then the whole chain
    G = ops.pool_pair_bwd(table, rows, B, L, U, coef, gscale, gsd)
    assert torch.equal(G, ops.pool_pair_bwd(table, rows, B, L, U, coef, gscale, gsd))
    c64 = d(coef) * gg
    p64, n64 = d(table[rows[B * L::2]]), d(table[rows[B * L + 1::2]])
    Gh, Gt = c64[:, None] * (p64 - n64), c64[:, None] * d(U)
    _within(G[:B], Gh, 4 * U32 * Gh.abs(), "G history")
    _within(G[B::2], Gt, 3 * U32 * Gt.abs(), "G positive")
    _within(G[B + 1::2], -Gt, 3 * U32 * Gt.abs(), "G negative")
    _within(G, *a["G"], "G chain")
    # ---- table gradient: from the kernel's own G and w, then the whole chain
    sp = ops.pool_table_grad(gidx, B, L, G, w, 1 + I)
    n = sp.count()
    ids = torch.cat((prof.view(-1), tgt.view(-1)))
    assert sp.idx[:n].tolist() == sorted(set((ids[ids != 0] + 1).tolist()))       # ascending; neither row 0 nor the padding item
    terms = torch.cat(((d(w)[:, None] * d(G[:B])).repeat_interleave(L, 0), d(G[B:])))
    z = lambda: torch.zeros(1 + I, D, dtype=torch.float64, device="cuda")
    dense64, dabs = z().index_add_(0, gidx, terms), z().index_add_(0, gidx, terms.abs())
    count = torch.zeros(1 + I, dtype=torch.float64, device="cuda").index_add_(0, gidx, torch.ones_like(gidx, dtype=torch.float64))
    dense64[0], dabs[0] = 0, 0
    got = sp.to_dense(1 + I)
    _within(got, dense64, (count[:, None] + 1) * U32 * dabs, "table gradient")
    _within(got[1:], *a["grad"][R.TABLE], "table gradient chain")
    assert float(got[:2].abs().max()) == 0
    sp2 = ops.pool_table_grad(gidx, B, L, G, w, 1 + I)
    assert torch.equal(sp.rows[:n], sp2.rows[:n]) and torch.equal(sp.idx[:n], sp2.idx[:n])


def _seg_constants():
    src = open(os.path.join(ROOT, "pixelrec_amd", "csrc", "embed_grad.hip")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("SEG_SHORT", "SEG_CHUNK"))


@pytest.mark.parametrize("mean", [False, True], ids=["sum", "mean"])
@pytest.mark.parametrize("B", [48, "chunk"])
def test_pool_segment_sum_equals_the_materialised_rows(B, mean):
    """MODE_POOL against ops.embed_grad_rows fed the materialised B (L + 2) rows (G expanded and weighted in torch), L = 4, D = 64.
    One item sits in every profile and is every sample's negative, so its segment holds 2 B occurrences: at B = 48 it is longer than
    SEG_SHORT (the whole-workgroup path, one chunk); B = SEG_CHUNK / 2 + 8 sizes it past one SEG_CHUNK as well (two chunks), which 48
    samples cannot reach.  Same uniq_idx; rows within (count + 1) u sum|terms|; bit-equal where every w is 1 (sum pooling)."""
    seg_short, seg_chunk = _seg_constants()
    B = seg_chunk // 2 + 8 if B == "chunk" else B
    L, D, I = 4, 64, 40
    rng = np.random.default_rng(B)
    prof = torch.from_numpy(rng.integers(1, I, size=(B, L)))
    prof[np.arange(B) % 3 == 1, 0] = 0                        # some padded positions
    prof[:, -1] = 7                                           # one item in every profile ...
    tgt = torch.from_numpy(rng.integers(1, I, size=(B, 2)))
    tgt[:, 1] = 7                                             # ... and every sample's negative
    assert 2 * B > seg_short and (B == 48 or 2 * B > seg_chunk)
    prof, tgt = prof.cuda(), tgt.cuda()
    rows, gidx = ops.din_rows(prof, tgt, I)
    g = torch.Generator().manual_seed(B)
    G = torch.randn(3 * B, D, generator=g).cuda()
    cnt = (prof != 0).sum(1).float()
    w = (1.0 / (cnt + 1e-8)) if mean else torch.ones(B, device="cuda")
    sp = ops.pool_table_grad(gidx, B, L, G, w, 1 + I)
    mat = torch.cat(((w[:, None] * G[:B]).repeat_interleave(L, 0), G[B:])).contiguous()
    ref = ops.embed_grad_rows(gidx, mat, 1 + I)
    n = sp.count()
    assert n == ref.count() and torch.equal(sp.idx[:n], ref.idx[:n]) and 8 in sp.idx[:n].tolist() and 0 not in sp.idx[:n].tolist()
    if not mean:
        assert torch.equal(sp.rows[:n], ref.rows[:n])
    dabs = torch.zeros(1 + I, D, dtype=torch.float64, device="cuda").index_add_(0, gidx, mat.double().abs())
    count = torch.zeros(1 + I, dtype=torch.float64, device="cuda").index_add_(0, gidx, torch.ones_like(gidx, dtype=torch.float64))
    assert int(count[8]) >= 2 * B
    dabs[0] = 0
    _within(sp.to_dense(1 + I), ref.to_dense(1 + I), (count[:, None] + 1) * U32 * dabs, "segment sums")


# ------------------------------------------------------------------------------------------------------------ the fixtures
def _trajectory_tolerances(kind, gold):
    """Per step the loss tolerance and, at the end, a per-entry tolerance of every state_dict tensor, from the float64 trajectory
    (the factored form) and pool_restate.analytic's bounds at its states.  AdamW's step of an entry is lr r with r = m^ / (sqrt(v^) +
    eps), |r| <= sqrt(t) <= 2 over four steps; r is homogeneous of degree 0 in that entry's gradients, so gradients off by a
    relative rho (the analytic bound over |g|) move it by (1 + rho) / (1 - rho) - 1 <= 4 rho for rho <= 1 / 2 (taken as 8 rho
    against the second-order effect of the drifting weights on the gradient) and never by more than 2 |r| <= 4.  An entry without a
    gradient (an untouched row, row 0) only decays: a few roundings of the weight per step (8 u |w|), which the touched entries get
    too.  The loss of a step sees the weights' drift so far through its gradient: sum |g| drift."""
    lr, wd = (float(x) for x in gold["optim"])
    T = R.state_from(gold, "sd.", torch.float64)
    names = [str(k) for k in gold["param.keys"]]
    drift = {k: torch.zeros_like(T[k]) for k in names}
    loss_tol = []
    for s, rows in enumerate(gold["rows"]):
        a = R.analytic(kind, T, rows)
        loss_tol.append(float(gold[f"ref_err.loss{s}"]) + float(a["loss"][1]) + sum(float((a["grad"][k][0].abs() * drift[k]).sum()) for k in names))
        for k in names:
            gv, gb = a["grad"][k]
            rho = torch.where(gv != 0, gb / gv.abs().clamp_min(1e-300), torch.where(gb > 0, torch.full_like(gb, 1.0), torch.zeros_like(gb)))
            drift[k] = drift[k] + lr * torch.clamp(8 * rho, max=4.0) + 8 * U32 * T[k].abs()
        R.adamw(kind, T, [rows], lr, wd)
    final_tol = {k: float(gold["ref_err.final." + k]) + drift[R.TABLE if k == R.ALIAS else k] for k in (str(x) for x in gold["sd.keys"])}
    return loss_tol, final_tol


def test_model_matches_the_reference_fixture(case):
    """Loss, every gradient (the table's through sparse_table_grad.to_dense), predict and the 4-step trajectory under the lazy
    PxrAdamW against the stored results of the reference (the per-row losses and gradients averaged over the batch, torch.optim.AdamW
    on them).  The tolerance of each quantity is its stored ref_err -- the reference's own float32 distance from float64 -- plus the
    analytic bound of the native arithmetic (pool_restate.analytic / predict_bounds; the trajectory: _trajectory_tolerances).  Row 0
    and the rows no batch touched only decay and stay inside that tolerance, which has no gradient part for them."""
    kind, hidden, gold = case
    names = [str(k) for k in gold["param.keys"]]
    P = R.state_from(gold, "sd.", torch.float64)
    a = R.analytic(kind, P, gold["rows"][0])
    m = _gold_model(kind, hidden, gold)
    assert list(m.state_dict()) == [str(k) for k in gold["sd.keys"]]
    loss = m(_inp(kind, gold["rows"][0]))
    loss.backward()
    ops.raise_on_bad_indices()
    loss = loss.detach()
    print("loss", float(loss), float(gold["loss"]), "ref_err", float(gold["ref_err.loss"]), "native bound", float(a["loss"][1]))
    assert abs(float(loss) - float(gold["loss"])) <= float(gold["ref_err.loss"]) + float(a["loss"][1])
    for k in names:
        got, ref = _grad_of(m, k), torch.from_numpy(gold["grad." + k]).double()
        print("grad", k, float((got - ref).abs().max()), "ref_err", float(gold["ref_err.grad." + k]), "native bound", float(a["grad"][k][1].max()))
        _within(got, ref, float(gold["ref_err.grad." + k]) + a["grad"][k][1], k)
    assert float(_grad_of(m, R.TABLE)[0].abs().max()) == 0                         # the padding row never receives a gradient
    m.eval()
    win = torch.from_numpy(gold["eval.windows"]).cuda()
    s64, sb = R.predict_bounds(kind, P, gold["eval.windows"])
    scores = m.predict(win, m.compute_item_all())
    print("scores", float((scores.cpu().double() - torch.from_numpy(gold["eval.scores"]).double()).abs().max()), "ref_err",
          float(gold["ref_err.scores"]), "native bound", float(sb.max()))
    _within(scores, torch.from_numpy(gold["eval.scores"]), float(gold["ref_err.scores"]) + sb, "scores")
    pad = (win != 0).sum(1) == 0
    if kind == "FM" or not hidden:
        assert float(scores[pad].abs().max()) == 0                                 # all padding: exactly 0 for every item
    q_eval = m.encode_last(win)[1]
    assert torch.equal(m.predict(win, None), scores) and q_eval.shape == (len(win), int(gold["meta"][1]))
    # ---- the trajectory
    lr, wd = (float(x) for x in gold["optim"])
    loss_tol, final_tol = _trajectory_tolerances(kind, gold)
    m2 = _gold_model(kind, hidden, gold)
    opt = _opt(m2, "lazy", lr, wd)
    for s, rows in enumerate(gold["rows"]):
        opt.zero_grad()
        l = m2(_inp(kind, rows))
        l.backward()
        opt.step()
        l = l.detach()
        print("trajectory loss", s, float(l), float(gold[f"adamw.loss{s}"]), "tolerance", loss_tol[s])
        assert abs(float(l) - float(gold[f"adamw.loss{s}"])) <= loss_tol[s], s
    sd = m2.state_dict()
    assert list(sd) == [str(k) for k in gold["sd.keys"]]
    for k, v in sd.items():
        ref = torch.from_numpy(gold["adamw.final." + k])
        print("final", k, float((v.cpu() - ref).abs().max()), "tolerance up to", float(torch.as_tensor(final_tol[k]).max()))
        _within(v, ref, final_tol[k], "final " + k)
    I = int(gold["meta"][0])
    touched = set(gold["rows"].reshape(-1).tolist())
    quiet = [0] + [i for i in range(I) if i not in touched]
    assert float(torch.as_tensor(final_tol[R.TABLE])[quiet].max()) <= float(gold["ref_err.final." + R.TABLE]) + 4 * 8 * U32 * 2.0
    assert not np.array_equal(sd[R.TABLE][0].cpu().numpy(), gold["sd." + R.TABLE][0])       # row 0 is decayed all the same


def test_one_row_batch_equals_the_reference_on_that_row(case):
    """On a one-row batch the native models compute exactly what the reference's forward (which keeps row 0 of any batch) computes:
    the stored one.* results, within their ref_err plus the native bound."""
    kind, hidden, gold = case
    one = gold["rows"][0][:1]
    a = R.analytic(kind, R.state_from(gold, "sd.", torch.float64), one)
    m = _gold_model(kind, hidden, gold)
    loss = m(_inp(kind, one))
    loss.backward()
    loss = loss.detach().clone()                          # the returned loss is a view of a buffer the next step may rewrite
    ops.raise_on_bad_indices()
    assert abs(float(loss) - float(gold["one.loss"])) <= float(gold["ref_err.one.loss"]) + float(a["loss"][1])
    for k in (str(x) for x in gold["param.keys"]):
        _within(_grad_of(m, k), torch.from_numpy(gold["one.grad." + k]), float(gold["ref_err.one.grad." + k]) + a["grad"][k][1], k)
    # a batch of that row repeated: the same loss (the mean of equal terms, one rounding away), where the reference would still see one row
    twice = m(_inp(kind, np.repeat(one, 2, axis=0)))
    assert abs(float(twice) - float(loss)) <= 4 * U32 * abs(float(loss))


def _keep_masks(seed, step, widths, B, p):
    """The library's keep masks of ops.dropout(x [B, width], p, seed, stream_id = layer, step_dev = step) (pxr_dropout_keep_host)."""
    L = lib.load()
    out = []
    for k, width in enumerate(widths):
        buf = (ctypes.c_uint8 * (B * width))()
        assert L.pxr_dropout_keep_host((seed + step) & 0xFFFFFFFFFFFFFFFF, k, 0, B * width, p, ctypes.cast(buf, ctypes.c_void_p)) == 0
        out.append((torch.tensor(list(buf), dtype=torch.float64).view(B, width), p))
    return out


def test_dssm_dropout_matches_the_restatement_under_the_librarys_keep_masks():
    """DSSM with dropout_prob 0.25 and the [8, 12, 8] MLP: one step against pool_restate.analytic with the keep masks of
    pxr_dropout_keep_host (layer k is stream k; the seed is config seed + completed steps), within its bounds.  The init seed is the
    first whose float64 pre-activations under those masks stay 1e-4 away from 0 (rows whose layer input is exactly zero apart:
    their pre-activation is the zero bias itself), so no rounding can flip a ReLU.  A second step draws other masks."""
    gold = np.load(os.path.join(GOLD, "dssm_mlp_tiny.npz"))
    hidden, p = [8, 12, 8], 0.25
    I, D, L, B = (int(x) for x in gold["meta"][:4])
    rows = gold["rows"][0]
    keeps = _keep_masks(2020, 0, hidden[:-1], B, p)
    assert 0 < float(keeps[0][0].mean()) < 1
    for seed in range(20):
        torch.manual_seed(seed)
        m = _model("DSSM", I, D, hidden, L=L, p=p)
        P = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
        saved = R._pool_mlp("DSSM", P, torch.as_tensor(rows[:, :-2]), [(k.clone(), q) for k, q in keeps])[5]
        if all(float(z[~(x == 0).all(1)].abs().min()) > 1e-4 for x, _, _, _, z in saved):
            break
    else:
        raise AssertionError("no init seed keeps the pre-activations away from 0")
    a = R.analytic("DSSM", P, rows, keeps=keeps)
    loss = m(torch.as_tensor(rows).cuda())
    loss.backward()
    loss = loss.detach().clone()                          # the returned loss is a view of a buffer the next step rewrites
    _within(loss.view(()), *a["loss"], "loss")
    for k in (str(x) for x in gold["param.keys"]):
        _within(_grad_of(m, k), *a["grad"][k], k)
    a0 = R.analytic("DSSM", P, rows)
    assert abs(float(a0["loss"][0]) - float(a["loss"][0])) > 100 * float(a["loss"][1])      # the masks matter
    loss2 = m(torch.as_tensor(rows).cuda())
    loss2.backward()
    assert float(loss2) != float(loss)                                                       # step 1 draws other masks


# ------------------------------------------------------------------------------------------------------------ determinism
def _wide_batch(rng, I, L, B):
    prof = rng.integers(1, I, size=(B, L))
    n_real = rng.integers(0, L + 1, size=B)
    n_real[:2] = 0
    n_real[2:4] = L
    prof[np.arange(L)[None, :] < (L - n_real)[:, None]] = 0
    pos = rng.integers(1, I, size=B)
    neg = (pos + rng.integers(1, I - 1, size=B) - 1) % (I - 1) + 1
    return torch.from_numpy(np.concatenate((prof, pos[:, None], neg[:, None]), axis=1))


@pytest.mark.parametrize("kind,hidden,p", [("DSSM", [], 0.0), ("DSSM", [16, 12, 16], 0.25), ("FM", [], 0.0)])
def test_two_runs_and_graph_replay_are_bit_identical_to_eager_steps(kind, hidden, p):
    """Three steps, eager twice and replayed from a hipGraph: the losses, the state_dict (flat buffer and table) and the optimizer's
    moments are bit-identical."""
    from pixelrec_amd.graph import GraphedTrainStep

    rng = np.random.default_rng(8)
    I, D, L, B = 60, 16, 5, 16
    torch.manual_seed(1)
    sd = {k: v.cpu() for k, v in _model(kind, I, D, hidden, L).state_dict().items()}
    batches = [_wide_batch(rng, 30 if s % 2 else I, L, B).cuda() for s in range(3)]
    split = lambda r: (r[:, :L].contiguous(), r[:, L:].contiguous())           # the batcher's two tensors
    out = {}
    for how in ("eager", "eager again", "graph"):
        m = _model(kind, I, D, hidden, L, sd={k: v.clone() for k, v in sd.items()}, p=p)
        opt = _opt(m, lr=1e-3, wd=0.01)
        losses = []
        gs = GraphedTrainStep(m, opt, *split(batches[0]), warmup=0) if how == "graph" else None
        for r in batches:
            if gs is not None:
                loss = gs(*split(r))
            else:
                opt.zero_grad()
                loss = m(split(r))
                loss.backward()
                opt.step()
            losses.append(loss.detach().clone())
        opt.flush()
        torch.cuda.synchronize()
        assert opt.step_count == len(batches)
        out[how] = [torch.stack(losses).view(-1)] + [v.clone() for v in m.state_dict().values()] + \
                   [opt._m.clone(), opt._v.clone(), opt._tm.clone(), opt._tv.clone()]
    ops.raise_on_bad_indices()
    assert len(set(out["eager"][0].tolist())) == len(batches)             # different batches, different losses
    for how in ("eager again", "graph"):
        for x, y in zip(out["eager"], out[how]):
            assert torch.equal(x, y), how


# ------------------------------------------------------------------------------------------------------------ evaluation
def _csr(hist, B):
    hu = torch.tensor([b for b in range(B) for _ in hist[b]], dtype=torch.int64)
    hi = torch.tensor([i for b in range(B) for i in hist[b]], dtype=torch.int64)
    return ops.history_csr(hu, hi, B, "cuda")


@pytest.mark.parametrize("kind,hidden", [("DSSM", []), ("DSSM", [8, 12, 8]), ("FM", [])])
def test_fused_topk_through_encode_last_equals_predict_mask_topk(kind, hidden):
    """The Trainer's generic path -- encode_last, then ops.score_topk with the history CSR -- at item_num 131, D 8, K 10: the ids
    equal predict -> column 0 and the histories masked -> torch.topk, and the float64 top-K, on inputs whose float64 adjacent-score
    margin down to rank K + 1 exceeds 1e-5 (the first init seed that has it; float32 scores of this size are good to 1e-6).  An
    all-padding window does not crash and returns K valid ids."""
    I, D, L, K, B = 131, 8, 4, 10, 5
    rng = np.random.default_rng(5)
    win = torch.from_numpy(rng.integers(1, I, size=(B, L)))
    win[1, :2] = 0
    win[3, :] = 0                                                                  # an all-padding window
    hist = [sorted(set(w[w != 0].tolist()) | set(rng.integers(1, I, size=6).tolist())) for w in win]
    for seed in range(20):
        torch.manual_seed(seed)
        m = _model(kind, I, D, hidden, L=L).eval()
        P = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
        s64 = R.predict(kind, P, win)
        s64[:, 0] = float("-inf")
        for b, h in enumerate(hist):
            s64[b, h] = float("-inf")
        top = torch.sort(s64, dim=-1, descending=True)
        real = (win != 0).any(1)
        if float((top.values[real, :K] - top.values[real, 1:K + 1]).min()) > 1e-5:
            break
    else:
        raise AssertionError("no init seed separates the float64 scores by 1e-5")
    ptr, items = _csr(hist, B)
    out, last = m.encode_last(win.cuda(), m.compute_item_all())
    assert out.shape == (B, 1, D) and last.shape == (B, D)
    idx, val = ops.score_topk(last, last.stride(0), B, m.compute_item_all().data, K, ptr, items)
    ops.raise_on_bad_indices()
    scores = m.predict(win.cuda(), m.compute_item_all()).cpu()
    scores[:, 0] = float("-inf")
    for b, h in enumerate(hist):
        scores[b, h] = float("-inf")
    assert torch.equal(idx.cpu()[real], torch.topk(scores, K, -1).indices[real])
    assert torch.equal(idx.cpu()[real], top.indices[real, :K])
    lone = idx.cpu()[3].tolist()
    assert len(set(lone)) == K and all(0 < i < I and i not in hist[3] for i in lone) and bool(torch.isfinite(val[3]).all())


def test_bad_ids_raise_index_error(case):
    kind, hidden, gold = case
    m = _gold_model(kind, hidden, gold)
    I, L = int(gold["meta"][0]), int(gold["meta"][2])
    good = torch.from_numpy(gold["rows"][0])
    ops.raise_on_bad_indices()
    for col, val in ((0, I), (L, I), (L + 1, -2), (1, -1)):
        bad = good.clone()
        bad[0, col] = val
        m(_inp(kind, bad)).backward()
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices()
    m(_inp(kind, good)).backward()
    ops.raise_on_bad_indices()                             # a clean batch leaves the word clear
    m.eval()
    win = torch.from_numpy(gold["eval.windows"]).cuda()
    with pytest.raises(IndexError):
        w = win.clone()
        w[0, -1] = I
        m.predict(w, m.compute_item_all())
    m.predict(win, m.compute_item_all())
    ops.raise_on_bad_indices()


def test_checkpoint_loads_into_the_reference_layout_and_resumes_the_trajectory(case, tmp_path, monkeypatch):
    """strict=True load of the fixture's state_dict, a save / load round trip of model and optimizer in the reference layout
    (torch.optim.AdamW's own loader takes the optimizer state over the reference's parameters), and the resumed trajectory equals
    the uninterrupted one bit for bit."""
    monkeypatch.setenv("PXR_LAZY_REPLAY", "exact")     # flushed and lagging rows then replay the dense sweep's own arithmetic
    kind, hidden, gold = case
    rows = [_inp(kind, r) for r in gold["rows"]]
    keys, names = [str(k) for k in gold["sd.keys"]], [str(k) for k in gold["param.keys"]]

    def steps(m, opt, which):
        for s in which:
            opt.zero_grad()
            m(rows[s]).backward()
            opt.step()

    ref = _gold_model(kind, hidden, gold)
    steps(ref, _opt(ref), range(4))
    a = _gold_model(kind, hidden, gold)
    opt = _opt(a)
    steps(a, opt, range(2))
    ck = {"state_dict": {k: v.detach().cpu() for k, v in a.state_dict().items()}, "optimizer": opt.state_dict(layout="torch")}
    path = tmp_path / "pool.pth"
    torch.save(ck, path)
    ck = torch.load(path, weights_only=False)
    assert list(ck["state_dict"].keys()) == keys
    assert ck["optimizer"]["param_groups"][0]["params"] == list(range(len(names)))   # the reference's parameters: no alias
    for j, n in enumerate(names):
        assert tuple(ck["optimizer"]["state"][j]["exp_avg"].shape) == tuple(ck["state_dict"][n].shape), n
    tor = [torch.nn.Parameter(ck["state_dict"][n].clone()) for n in names]
    topt = torch.optim.AdamW(tor, lr=1.0, weight_decay=0.5)
    topt.load_state_dict(ck["optimizer"])                  # strict layout: torch's own loader
    assert (topt.param_groups[0]["lr"], topt.param_groups[0]["weight_decay"]) == (1e-4, 0.1)
    b = _gold_model(kind, hidden, gold)
    b.load_state_dict(ck["state_dict"], strict=True)
    opt_b = _opt(b)
    opt_b.load_state_dict(ck["optimizer"])
    steps(b, opt_b, range(2, 4))
    sr, sb = ref.state_dict(), b.state_dict()
    assert list(sr) == keys
    for k in sr:
        assert torch.equal(sr[k], sb[k]), k


@pytest.mark.parametrize("name", ["dssm", "fm"])
def test_main_py_trains_two_epochs_and_reports_recall_and_ndcg(name, tmp_path):
    from pixelrec_amd.config import Config
    from pixelrec_amd.data import bulid_dataloader, load_data
    from pixelrec_amd.utils.utils import get_model

    os.makedirs(tmp_path / "data")
    with open(os.path.join(ROOT, "tests", "golden", "TinyInter.csv")) as f:
        (tmp_path / "data" / "TinyInter.csv").write_text(f.read())
    shipped = [os.path.join(ROOT, "configs", "IDNet", name + ".yaml"), os.path.join(ROOT, "configs", "overall", "ID.yaml")]
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
    fresh = get_model(name.upper())(config, data).cuda().train()
    first = float(fresh(tuple(t.cuda() for t in next(iter(train_loader)))))
    mean_last = float(epochs[1]) / len(train_loader)
    print("first step loss", first, "mean step loss of epoch 2", mean_last)
    assert np.isfinite(first) and mean_last < first
