"""CuratorNet on the gfx950 kernels (csrc/curator.hip, the SELU epilogue of the GEMMs): the epilogue and the two pooling kernels
against float64 torch, the model against the golden fixture of the reference's own CuratorNet (loss, the ten gradients,
compute_item_all, predict, a 4-step AdamW trajectory), one step at the shipped widths against the float64 restatement, run-to-run
and hipGraph-replay bit identity, the fused top-k against the literal predict, checkpoints in the reference layout, and main.py
end to end.  Every test here needs the model, its ops or the `selu` code, so each fails without the feature."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pixelrec_amd import ops
from tests import curatornet_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "curatornet_tiny.npz")
U32 = 2.0 ** -24
SA = R.SCALE * R.ALPHA


class _Data:
    def __init__(self, I):
        self.item_num = I


def _model(tmp, v_feat, E, hidden, L, sd=None):
    from pixelrec_amd.model import CuratorNet

    path = os.path.join(str(tmp), "v_feat_%d_%d.npy" % v_feat.shape)
    np.save(path, v_feat)
    m = CuratorNet({"embedding_size": E, "hidden_size": hidden, "v_feat_path": path, "MAX_ITEM_LIST_LENGTH": L}, _Data(len(v_feat)))
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.cuda().train()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _gold_model(g, tmp):
    _, _, E, hidden, L, _ = (int(x) for x in g["meta"][:6])
    sd = {k[len("sd."):]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith("sd.")}
    return _model(tmp, g["v_feat"], E, hidden, L, sd)


def _opt(m, lr=1e-4, wd=0.01):
    from pixelrec_amd.optim import PxrAdamW

    return PxrAdamW(m, lr=lr, weight_decay=wd)


def _steps(m, opt, rows, which):
    losses = []
    for s in which:
        opt.zero_grad()
        loss = m(rows[s])
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    return losses


# ------------------------------------------------------------------------------------------------------------ SELU epilogue
@pytest.mark.parametrize("M,N,K", [(5, 12, 20), (37, 24, 12)])
def test_selu_epilogue_matches_float64_and_is_s_a_at_exact_zero(M, N, K):
    """Pre-activations spread over [-30, 30], two bias-driven columns at -120 / +120 (exp underflows; exp of the positive one would
    be inf), and exact zeros (a zero input row under zero biases).  Output: 1e-4 absolute, the tolerance of the existing GPU test
    of linear_fwd(act=...)'s outputs (test_gpu_sasrec.py::test_hidden_act_variants_match_reference_golden, its scores).  Saved
    derivative: selu' is Lipschitz with constant s a < 2, so it may move by s a times the pre-activation's rounding error --
    (K + 2) u on the magnitude sum of its terms, whatever the summation order -- plus 8 u s a for the exponential."""
    rng = np.random.default_rng(M)
    x = rng.standard_normal((M, K))
    W = rng.standard_normal((N, K))
    b = rng.standard_normal(N)
    x[0] = 0.0
    b[:4] = 0.0
    W[N - 2:] = 0.0                                                        # the last two columns are their bias alone
    x *= 30.0 / np.abs(x @ W.T + b)[:, :N - 2].max()
    b[N - 2], b[N - 1] = -120.0, 120.0
    x, W, b = (torch.from_numpy(a.astype(np.float32)) for a in (x, W, b))
    pre = x.double() @ W.double().T + b.double()
    assert float(pre[:, :N - 2].abs().max()) > 25 and (pre[0, :4] == 0).all() and float(pre[:, N - 2].max()) < -100
    y, d = ops.linear_fwd(x.cuda(), W.cuda(), b.cuda(), act="selu")
    y, d = y.cpu().double(), d.cpu().double()
    assert torch.isfinite(y).all() and torch.isfinite(d).all()
    tol_pre = (K + 2) * U32 * float((x.double().abs() @ W.double().abs().T + b.double().abs()).max())
    err_y, err_d = float((y - F.selu(pre)).abs().max()), float((d - R.selu_grad(pre)).abs().max())
    print("selu output error", err_y, "derivative error", err_d, "bound", SA * tol_pre + 8 * U32 * SA)
    assert err_y <= 1e-4
    assert err_d <= SA * tol_pre + 8 * U32 * SA
    assert (y[0, :4] == 0).all() and float((d[0, :4] - SA).abs().max()) <= 4 * U32 * SA         # x == 0: the negative branch
    assert (d[:, N - 2] == 0).all() and float((y[:, N - 2] + SA).abs().max()) <= 4 * U32 * SA    # exp underflows: -s a, slope 0
    assert float((d[:, N - 1] - R.SCALE).abs().max()) <= U32 * R.SCALE
    # the neighbouring branch of the same epilogue is undisturbed
    yt, dt = ops.linear_fwd(x.cuda(), W.cuda(), b.cuda(), act="tanh")
    th = torch.tanh(pre)
    assert float((yt.cpu().double() - th).abs().max()) <= 1e-4
    assert float((dt.cpu().double() - (1 - th * th)).abs().max()) <= 2 * tol_pre + 8 * U32


# ------------------------------------------------------------------------------------------------------------ pooling kernels
@pytest.mark.parametrize("B,L,E", [(3, 5, 12), (2, 1, 4), (4, 10, 512)])
def test_pool_kernels_match_float64_torch(B, L, E):
    rng = np.random.default_rng(B * 100 + L)
    n = B * (L + 2)
    pre = rng.standard_normal((n, E)).astype(np.float32)
    if L >= 3:
        v = pre[:B * L].reshape(B, L, E)
        v[:, 2] = v[:, 0]                                                  # duplicated rows: maxima tie exactly
        v[-1, :] = v[-1, 1]                                                # ... and a profile whose rows are all one row (padding)
    pre = torch.from_numpy(pre)
    h = R.selu(pre.double()).float()                                       # what the common tower hands the pooling
    dact = R.selu_grad(pre.double()).float()
    dcat = torch.from_numpy(rng.standard_normal((B, 2 * E)).astype(np.float32))
    di = torch.from_numpy(rng.standard_normal((2 * B, E)).astype(np.float32))
    cat, arg = ops.curator_pool(h.cuda(), B, L)
    prof = h[:B * L].view(B, L, E).double()
    mx, idx = F.adaptive_max_pool2d(prof, (1, E), return_indices=True)
    av = F.adaptive_avg_pool2d(prof, (1, E))
    cat_c = cat.cpu()
    assert torch.equal(cat_c[:, :E].double(), mx.squeeze(1))               # the max is a selection: exact
    assert float((cat_c[:, E:].double() - av.squeeze(1)).abs().max()) <= L * U32 * float(prof.abs().max())
    assert torch.equal(arg.cpu().long(), idx.squeeze(1) // E)              # torch's first-of-equals, entry for entry
    if L >= 3:
        assert (arg.cpu() != 2).all() and (arg.cpu()[-1] == 0).all()
    # backward: autograd through selu and the two pools, tail rows included
    p = pre.double().requires_grad_(True)
    hh = F.selu(p)
    pr = hh[:B * L].view(B, L, E)
    c64 = torch.cat((F.adaptive_max_pool2d(pr, (1, E)), F.adaptive_avg_pool2d(pr, (1, E))), -1).squeeze(1)
    ((c64 * dcat.double()).sum() + (hh[B * L:] * di.double()).sum()).backward()
    out = torch.full((n, E), float("nan"), device="cuda")
    ops.curator_pool_bwd(dcat.cuda(), arg, di.cuda(), dact.cuda(), B, L, out=out)
    err = float((out.cpu().double() - p.grad).abs().max())
    print("pool backward error", err, "largest entry", float(p.grad.abs().max()))
    assert err <= 1e-6 * max(1.0, float(p.grad.abs().max()))
    # the ids form over an item matrix: the same bits as the dense form on the gathered rows
    I = 7
    items = torch.from_numpy(rng.standard_normal((I, E)).astype(np.float32)).cuda()
    ids = torch.from_numpy(rng.integers(0, I, size=(B, L))).cuda()
    ids[0, :] = 0
    ops.raise_on_bad_indices()
    c_ids, a_ids = ops.curator_pool(items, B, L, ids=ids)
    c_den, a_den = ops.curator_pool(items[ids.view(-1)].contiguous(), B, L)
    ops.raise_on_bad_indices()
    assert torch.equal(c_ids, c_den) and torch.equal(a_ids, a_den)
    c_no, none = ops.curator_pool(items, B, L, ids=ids, want_argmax=False)
    assert none is None and torch.equal(c_no, c_ids)
    for bad in (I, -1):
        ids2 = ids.clone()
        ids2[B - 1, L - 1] = bad
        ops.curator_pool(items, B, L, ids=ids2)
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices()
    ops.raise_on_bad_indices()


# ------------------------------------------------------------------------------------------------------------ pair head
def test_pair_head_keeps_the_epsilon_inside_the_log():
    """-log(1e-8 + sigmoid(x)) as the reference writes it, against float64, with pairs ranked so badly that the loss saturates at
    -log(1e-8) and the gradient fades (MF's head, with the 1e-8 outside the log, grows without bound there).  x_b is a dot product
    of H = 8 terms: its float32 error is at most (H + 2) u on the magnitude sum; |d loss_b / d x| <= 1 and |d coef B / d x| <= 1/4."""
    H, xs = 8, [-60.0, -18.4, -3.0, 0.0, 0.5, 7.0, 30.0, 90.0]
    B = len(xs)
    rng = np.random.default_rng(2)
    u = rng.standard_normal((B, H)).astype(np.float32)
    it = rng.standard_normal((B, 2, H)).astype(np.float32)
    for b, x in enumerate(xs):                             # scale the positive so that <u, p> - <u, n> is about x
        it[b, 0] = u[b] * ((x + float(u[b] @ it[b, 1])) / float(u[b] @ u[b]))
    u_t, it_t = torch.from_numpy(u), torch.from_numpy(it)
    u64 = u_t.double().requires_grad_(True)
    x64 = (u64.unsqueeze(1) * it_t.double()).sum(-1)
    x64 = x64[:, 0] - x64[:, 1]
    assert float((x64.detach() - torch.tensor(xs)).abs().max()) < 1e-3
    row64 = -torch.log(1e-8 + torch.sigmoid(x64))
    c64 = torch.autograd.grad(row64.mean(), x64)[0]
    loss, coef = ops.curator_pair_fwd(u_t.cuda(), it_t.view(2 * B, H).cuda(), B)
    dx = (H + 2) * U32 * float((u_t.double().abs().unsqueeze(1) * it_t.double().abs()).sum(-1).sum(-1).max())
    print("head loss", float(loss), float(row64.mean()), "coef error", float((coef.cpu().double() - c64).abs().max()), "dx", dx)
    assert abs(float(loss) - float(row64.mean())) <= dx + 8 * U32 * float(row64.mean())
    assert float((coef.cpu().double() - c64).abs().max()) <= (dx / 4 + 8 * U32) / B
    assert float(row64[0]) > 18.0 and abs(float(c64[0])) < 1e-9 / B          # saturated: the loss is capped, the gradient gone


# ------------------------------------------------------------------------------------------------------------ the model
def test_model_matches_the_reference_fixture(gold, tmp_path):
    """Tolerances: the ones test_gpu_vbpr.py::test_model_matches_the_reference_fixture uses for the same quantities.  The fixture's
    generator asserts that no maximum and no pre-activation sits within 1e-4 of a tie / of zero and that every gradient entry is
    non-zero, so the final weights are compared, not bounded."""
    m = _gold_model(gold, tmp_path)
    rows = torch.from_numpy(gold["rows"]).cuda()
    L = int(gold["meta"][4])
    frozen = m.embedding.weight.detach().clone()
    loss = m(rows[0])
    loss.backward()
    print("loss", float(loss), float(gold["loss"]))
    assert abs(float(loss) - float(gold["loss"])) <= 2e-6 * max(1.0, float(gold["loss"]))
    named = dict(m.named_parameters())
    for k in R.NAMES:
        ref = gold["grad." + k]
        got = named[k].grad.cpu().numpy()
        print("grad", k, np.abs(got - ref).max(), np.abs(ref).max())
        assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), k
    assert m.embedding.weight.grad is None
    # the two-tensor form the training loop stages gives the same bits
    loss2 = m((rows[0][:, :L].contiguous(), rows[0][:, L:].contiguous()))
    assert torch.equal(loss2.detach(), loss.detach())
    m.eval()
    feat = m.compute_item_all()
    print("item_all", np.abs(feat.cpu().numpy() - gold["eval.item_all"]).max())
    assert feat.shape == gold["eval.item_all"].shape and np.abs(feat.cpu().numpy() - gold["eval.item_all"]).max() <= 2e-5
    win = torch.from_numpy(gold["eval.windows"]).cuda()
    scores = m.predict(win, feat).cpu().numpy()
    print("scores", np.abs(scores - gold["eval.scores"]).max())
    assert (gold["eval.windows"] == 0).all(1).any()                        # the all-padding window is among them
    assert np.abs(scores - gold["eval.scores"]).max() <= 2e-5
    m2 = _gold_model(gold, tmp_path)
    lr, wd = (float(x) for x in gold["optim"])
    opt = _opt(m2, lr, wd)
    for s, loss in enumerate(_steps(m2, opt, rows, range(4))):
        print("trajectory loss", s, float(loss), float(gold[f"adamw.loss{s}"]))
        assert abs(float(loss) - float(gold[f"adamw.loss{s}"])) <= 5e-6 * max(1.0, float(loss)), s
    for k, v in m2.state_dict().items():
        ref = gold["adamw.final." + k]
        print("final", k, np.abs(v.cpu().numpy() - ref).max())
        assert np.abs(v.cpu().numpy() - ref).max() <= 5e-6 * max(1.0, np.abs(ref).max()), k
    assert torch.equal(m2.embedding.weight.detach(), frozen) and m2.embedding.weight.grad is None      # frozen, bit for bit
    assert len(opt.state_dict(layout="torch")["param_groups"][0]["params"]) == 10


def test_one_step_at_the_shipped_widths_matches_float64(tmp_path):
    """E = 512, hidden 1024, F = 2048, B = 8, L = 10 over a 64-item catalogue, against the float64 restatement.  Bounds, written
    down before any run, from the operands' magnitudes: a reduction of length k in float32 moves its result by at most k u times
    the magnitude sum of its terms, whatever the order (the split-operand GEMMs are no worse than the f32-input MFMA, README), and
    SELU and the pooling are 2-Lipschitz / 1-Lipschitz, so first-order errors add along a path.
      * forward path to x_b: F + E (common tower) + L (mean) + 2E + Hd + Hd (profile tower) + E (the head's dot) = kf terms:
        |d x_b| <= kf u S with S = max_b sum_e |u_be| (|p_be| + |n_be|), and |d loss| <= max_b |d x_b| (|d loss / d x_b| <= 1/B
        each, B of them).
      * a gradient tensor adds the backward path (Hd + Hd + E + E) and its own reduction over the B (L + 2) rows: kg = kf + 2 Hd
        + 2 E + B (L + 2) terms, taken on the largest entry of the float64 gradient: |d G| <= kg u max |G|."""
    rng = np.random.default_rng(23)
    I, E, hidden, Fw, B, L = 64, 512, 2, 2048, 8, 10
    Hd = hidden * E
    v_feat = rng.standard_normal((I, Fw)).astype(np.float32)
    torch.manual_seed(3)
    m = _model(tmp_path, v_feat, E, hidden, L)
    prof = rng.integers(1, I, size=(B, L))                                 # ids spread over the catalogue
    prof[0, :] = 0
    prof[1, :7] = 0
    prof[2, :3] = 0
    tgt = np.stack((rng.permutation(np.arange(1, I))[:B], rng.permutation(np.arange(1, I))[:B]), 1)
    tgt[:, 1] = np.where(tgt[:, 1] == tgt[:, 0], tgt[:, 0] % (I - 1) + 1, tgt[:, 1])
    rows = torch.from_numpy(np.concatenate((prof, tgt), 1)).cuda()
    P = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    loss = m(rows)
    loss.backward()
    L64, g64 = R.loss_and_grads(P, prof, tgt)
    feat = P["embedding.weight"]
    u = R.profile_tower(P, R.pool(R.common(P, feat[torch.from_numpy(prof)]))[0])
    it = R.common(P, feat[torch.from_numpy(tgt)])
    S = float((u.abs().unsqueeze(1) * it.abs()).sum(-1).sum(-1).max())
    kf = Fw + E + L + 2 * E + Hd + Hd + E
    kg = kf + 2 * Hd + 2 * E + B * (L + 2)
    print("loss", float(loss), L64, "error", abs(float(loss) - L64), "bound", kf * U32 * S)
    assert abs(float(loss) - L64) <= kf * U32 * S
    named = dict(m.named_parameters())
    for k in R.NAMES:
        ref = g64[k].numpy()
        err = np.abs(named[k].grad.cpu().double().numpy() - ref).max()
        print("grad", k, "max error", err, "bound", kg * U32 * np.abs(ref).max(), "largest entry", np.abs(ref).max())
        assert np.isfinite(err) and err <= kg * U32 * np.abs(ref).max(), k


def _random_rows(rng, I, B, L, n):
    out = []
    for _ in range(n):
        prof = rng.integers(1, I, size=(B, L))
        prof[0, :] = 0
        prof[1, :L // 2] = 0
        tgt = rng.integers(1, I, size=(B, 2))
        tgt[:, 1][tgt[:, 1] == tgt[:, 0]] = 0
        out.append((torch.from_numpy(prof).cuda(), torch.from_numpy(tgt).cuda()))
    return out


def test_two_runs_and_graph_replay_are_bit_identical_to_eager_steps(tmp_path):
    from pixelrec_amd.graph import GraphedTrainStep

    rng = np.random.default_rng(8)
    I, E, Fw, B, L = 60, 64, 24, 16, 5
    v_feat = rng.standard_normal((I, Fw)).astype(np.float32)
    sd = _model(tmp_path, v_feat, E, 2, L).state_dict()
    batches = _random_rows(rng, I, B, L, 8)                                # eight different batches
    out = {}
    for how in ("eager", "eager again", "graph"):
        m = _model(tmp_path, v_feat, E, 2, L, sd={k: v.clone() for k, v in sd.items()})
        opt = _opt(m, lr=1e-3)
        losses = []
        gs = GraphedTrainStep(m, opt, batches[0][0], batches[0][1], warmup=0) if how == "graph" else None
        for prof, tgt in batches:
            if gs is not None:
                loss = gs(prof, tgt)
            else:
                opt.zero_grad()
                loss = m((prof, tgt))
                loss.backward()
                opt.step()
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        assert opt.step_count == len(batches)
        out[how] = [torch.stack(losses).view(-1)] + [v.clone() for v in m.state_dict().values()] + [opt._m.clone(), opt._v.clone()]
    assert len(set(out["eager"][0].tolist())) == len(batches)             # different batches, different losses
    for how in ("eager again", "graph"):
        for a, b in zip(out["eager"], out[how]):
            assert torch.equal(a, b), how
    assert not torch.equal(out["eager"][2], sd["selu_common1.weight"].cuda())       # ... and the steps moved the weights


def test_fused_topk_equals_predict_mask_topk_and_the_cache_follows_the_weights(tmp_path):
    """Top-10 ids of the fused path (pool by id -> profile tower -> fused scoring against compute_item_all) against predict ->
    column 0 and history masked -> torch.topk: 16 users, 300 items.  The near-tie rule of
    test_gpu_vbpr.py::test_fused_topk_equals_predict_mask_topk: a user whose literal scores around the cut are closer than the
    score tolerance (2e-5) may be compared on scores instead of ids, at most one user in sixteen; with this seed (chosen on the
    float64 restatement alone: its smallest gap among the first K + 1 scores is 4.5e-3) the restatement has no near-tie, asserted."""
    rng = np.random.default_rng(5)
    In, E, Fw, K, H, L, Un = 300, 64, 40, 10, 5, 6, 16
    v_feat = (0.25 * rng.standard_normal((In, Fw))).astype(np.float32)
    win = rng.integers(1, In, size=(Un, L))
    win[0, :] = 0
    win[1, :3] = 0
    win[2, :5] = 0
    hi = torch.from_numpy(rng.integers(1, In, size=Un * H))
    hu = torch.from_numpy(np.repeat(np.arange(Un), H))
    torch.manual_seed(25)
    m = _model(tmp_path, v_feat, E, 2, L)
    m.eval()
    feat = m.compute_item_all()
    assert m.compute_item_all() is feat and feat.shape == (In, E)          # cached while evaluating
    win_d = torch.from_numpy(win).cuda()
    ptr, hitems = ops.history_csr(hu, hi, Un, "cuda")
    out, last = m.encode_last(win_d, feat)
    assert out.shape == (Un, 1, E)
    idx, val = ops.score_topk(last, last.stride(0), Un, feat, K, ptr, hitems)
    if ops.score_planes_supported(feat):                                   # the Trainer's route: pre-split item planes
        idx_p, _ = ops.score_topk(last, last.stride(0), Un, feat, K, ptr, hitems, table_planes=ops.split_planes(feat),
                                  table_norm_max=ops.row_norm_max(feat))
        assert torch.equal(idx_p, idx)
    scores = m.predict(win_d, feat)
    first = scores.clone()
    scores[:, 0] = -np.inf
    scores[(hu.cuda(), hi.cuda())] = -np.inf
    ref = torch.topk(scores, K + 1, dim=-1)
    P = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    s64 = R.predict(P, win)
    assert float((first.cpu().double() - s64).abs().max()) <= 2e-5
    s64[:, 0] = -np.inf
    s64[(hu, hi)] = -np.inf
    top64 = torch.topk(s64, K + 1, dim=-1).values
    assert float((top64[:, :-1] - top64[:, 1:]).min()) > 2 * 2e-5
    same = (idx == ref.indices[:, :K]).all(-1)
    on_scores = int((~same).sum())
    print("users compared on scores:", on_scores, "of", Un)
    assert on_scores <= Un // 16
    assert float((val - ref.values[:, :K]).abs().max()) <= 2e-5
    # the cache goes with train() and is rebuilt from the updated weights
    m.train()
    assert m.store_ifeatures is None
    opt = _opt(m, lr=1e-2)
    prof, tgt = _random_rows(rng, In, 8, L, 1)[0]
    m((prof, tgt)).backward()
    opt.step()
    m.eval()
    feat2 = m.compute_item_all()
    assert feat2 is not feat and not torch.equal(feat2, feat)
    assert not torch.equal(m.predict(win_d, feat2), first)


def test_bad_ids_raise_index_error(gold, tmp_path):
    m = _gold_model(gold, tmp_path)
    I = int(gold["meta"][0])
    good = torch.from_numpy(gold["rows"][0]).cuda()
    ops.raise_on_bad_indices()
    for col, bad in ((0, I), (0, -1), (-1, I), (-2, -2)):
        rows = good.clone()
        rows[3, col] = bad
        m(rows).backward()
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices()
    m(good).backward()
    ops.raise_on_bad_indices()                             # a clean batch leaves the word clear
    m.eval()
    feat = m.compute_item_all()
    win = torch.from_numpy(gold["eval.windows"]).cuda()
    with pytest.raises(IndexError):
        m.predict(win.clone().fill_(I), feat)
    m.predict(win, feat)


class _RefLayout(torch.nn.Module):
    """A module laid out like the reference's CuratorNet (curatornet.py:22-37): what its checkpoints load into."""

    def __init__(self, v, E, Hd):
        super().__init__()
        self.embedding = torch.nn.Embedding.from_pretrained(v, freeze=True)
        self.selu_common1 = torch.nn.Linear(v.shape[1], E)
        self.selu_common2 = torch.nn.Linear(E, E)
        self.maxpool = torch.nn.AdaptiveMaxPool2d((1, E))
        self.avgpool = torch.nn.AdaptiveAvgPool2d((1, E))
        self.selu_pu1 = torch.nn.Linear(2 * E, Hd)
        self.selu_pu2 = torch.nn.Linear(Hd, Hd)
        self.selu_pu3 = torch.nn.Linear(Hd, E)


def test_checkpoint_loads_into_the_reference_layout_and_resumes_the_trajectory(gold, tmp_path):
    rows = torch.from_numpy(gold["rows"]).cuda()
    _, _, E, hidden, _, _ = (int(x) for x in gold["meta"][:6])
    ref = _gold_model(gold, tmp_path)
    _steps(ref, _opt(ref), rows, range(4))
    a = _gold_model(gold, tmp_path)
    opt = _opt(a)
    _steps(a, opt, rows, range(2))
    ck = {"state_dict": {k: v.detach().cpu() for k, v in a.state_dict().items()}, "optimizer": opt.state_dict(layout="torch")}
    path = tmp_path / "curatornet.pth"
    torch.save(ck, path)
    ck = torch.load(path, weights_only=False)
    names = list(ck["state_dict"].keys())
    assert names == list(R.KEYS) and len(names) == 11
    tor = _RefLayout(torch.zeros_like(ck["state_dict"]["embedding.weight"]), E, hidden * E)
    res = tor.load_state_dict(ck["state_dict"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    trainable = [p for p in tor.parameters() if p.requires_grad]           # what the reference trainer hands its optimizer
    assert len(trainable) == 10 and [g["params"] for g in ck["optimizer"]["param_groups"]] == [list(range(10))]
    for j, p in enumerate(trainable):
        assert tuple(ck["optimizer"]["state"][j]["exp_avg"].shape) == tuple(p.shape), j
    topt = torch.optim.AdamW(trainable, lr=1.0, weight_decay=0.5)
    topt.load_state_dict(ck["optimizer"])                  # strict layout: torch's own loader
    assert (topt.param_groups[0]["lr"], topt.param_groups[0]["weight_decay"]) == (1e-4, 0.01)
    b = _gold_model(gold, tmp_path)
    res = b.load_state_dict(tor.state_dict(), strict=True)                 # ... and back
    assert not res.missing_keys and not res.unexpected_keys
    opt_b = _opt(b)
    opt_b.load_state_dict(ck["optimizer"])
    _steps(b, opt_b, rows, range(2, 4))
    sr, sb = ref.state_dict(), b.state_dict()
    for k in sr:
        assert torch.equal(sr[k], sb[k]), k


def test_main_py_trains_two_epochs_and_reports_recall_and_ndcg(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth_dataset

    from pixelrec_amd.config import Config
    from pixelrec_amd.data import load_data

    synth_dataset.main(str(tmp_path / "data"), 3000, 800)
    shipped = os.path.join(ROOT, "configs", "ViNet", "curatornet.yaml")
    (tmp_path / "o.yaml").write_text(f"embedding_size: 64\nstate: INFO\nreproducibility: True\ncheckpoint_dir: '{tmp_path}/saved'\n"
                                     f"log_path: '{tmp_path}/log'\ndata_path: {tmp_path}/data/\nv_feat_path: {tmp_path}/feat.npy\n"
                                     "epochs: 2\ntrain_batch_size: 64\noptim_args: {learning_rate: 0.001, weight_decay: 0.01}\n")
    cfg = Config([shipped, str(tmp_path / "o.yaml")])
    assert cfg["model"] == "CuratorNet" and cfg["hidden_size"] == 2
    item_num = load_data(cfg).item_num
    np.save(str(tmp_path / "feat.npy"), np.random.default_rng(0).standard_normal((item_num, 40)).astype(np.float32))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "OMP_NUM_THREADS")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--device", "0", "--config_file", shipped,
                        str(tmp_path / "o.yaml")], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    losses = [float(x) for x in re.findall(r"epoch \d+ training \[time: [0-9.]+s, train loss: ([0-9.]+)\]", out)]
    assert len(losses) == 2 and losses[1] < losses[0], out[-3000:]
    assert "training step captured as a hipGraph (batch size 64)" in out, out[-3000:]
    assert "Loading model structure and parameters from" in out, out[-3000:]     # the test result comes from the checkpoint
    for metric in ("recall@10", "ndcg@10"):
        mm = re.search(r"test result: .*?'%s', ([0-9.]+)\)" % metric, out)
        assert mm is not None and 0.0 <= float(mm.group(1)) <= 1.0, out[-2000:]
