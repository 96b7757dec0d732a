"""VBPR on the gfx950 kernels (csrc/vbpr.hip): the model against the golden fixture of the reference's own VBPR (loss, all five
gradients with user 0 and item 0, predict, a 4-step trajectory under the shipped two parameter groups), the kernels at the shipped
width against float64 with run-to-run bit identity, lazy against dense table updates, hipGraph replay against eager steps, the
fused top-k on the packed matrices against the literal predict, bad ids and feature files, checkpoints in the reference layout,
and main.py end to end.  Every test here needs the model or its kernels, so each fails without the feature."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pixelrec_amd import ops
from tests import vbpr_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "vbpr_tiny.npz")
U32 = 2.0 ** -24
ARGS4 = {"modal_lr": 1e-4, "rec_lr": 1e-3, "modal_decay": 0.1, "rec_decay": 0}
TABLES = ("user_id_embedding.weight", "item_id_embedding.weight", "user_modal_embedding.weight")


class _Data:
    def __init__(self, U, I):
        self.user_num, self.item_num = U, I


def _model(tmp, U, I, D, v_feat, sd=None):
    from pixelrec_amd.model import VBPR

    path = os.path.join(str(tmp), "v_feat_%d_%d.npy" % v_feat.shape)
    np.save(path, v_feat)
    m = VBPR({"embedding_size": D, "mlp_hidden_size": [], "dropout_prob": 0.0, "v_feat_path": path}, _Data(U, I))
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.cuda().train()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _gold_model(g, tmp):
    U, I, D = (int(x) for x in g["meta"][:3])
    sd = {k[len("sd."):]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith("sd.")}
    return _model(tmp, U, I, D, g["v_feat"], sd)


def _opt(m, how="lazy"):
    from pixelrec_amd.optim import flat_table_adamw

    return flat_table_adamw(m, ARGS4, "projection", table_update=how)


def _grad_of(m, name):
    """The dense gradient of a reference parameter: the projections from the flat buffer, the tables from the sparse rows."""
    if name in TABLES:
        dense = m.sparse_table_grad.to_dense(m.lazy_table().shape[0])
        lo, hi = m.table_parameter_spans()[name]
        return dense[lo:hi].cpu().numpy()
    return dict(m.named_parameters())[name].grad.cpu().numpy()


def _steps(m, opt, users, items, which):
    losses = []
    for s in which:
        opt.zero_grad()
        loss = m((users[s], items[s]))
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    return losses


def test_model_matches_the_reference_fixture(gold, tmp_path):
    """Tolerances: the ones test_gpu_mf.py::test_model_matches_the_reference_fixture uses for the same quantities.  No parameter's
    trajectory is driven by rounding noise here: in the float64 restatement every gradient entry of a touched row and of both
    projections is non-zero (asserted below), so the final weights are compared, not bounded."""
    m = _gold_model(gold, tmp_path)
    users = torch.from_numpy(gold["users"]).cuda()
    items = torch.from_numpy(gold["items"]).cuda()
    loss = m((users[0], items[0]))
    loss.backward()
    print("loss", float(loss), float(gold["loss"]))
    assert abs(float(loss) - float(gold["loss"])) <= 2e-6 * max(1.0, float(gold["loss"]))
    for k in R.NAMES:
        ref = gold["grad." + k]
        got = _grad_of(m, k)
        print("grad", k, np.abs(got - ref).max(), np.abs(ref).max())
        assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), k
    for k in TABLES:
        assert np.abs(_grad_of(m, k)[0]).max() > 0                 # row 0 of every table is an ordinary, trained row
    m.eval()
    feat = m.compute_item_all()
    scores = m.predict(torch.from_numpy(gold["eval.users"]).cuda(), feat).cpu().numpy()
    print("scores", np.abs(scores - gold["eval.scores"]).max())
    assert np.abs(scores - gold["eval.scores"]).max() <= 2e-5
    m2 = _gold_model(gold, tmp_path)
    opt = _opt(m2)
    for s, loss in enumerate(_steps(m2, opt, users, items, range(4))):
        print("trajectory loss", s, float(loss), float(gold[f"adamw.loss{s}"]))
        assert abs(float(loss) - float(gold[f"adamw.loss{s}"])) <= 5e-6 * max(1.0, float(loss)), s
    for k, v in m2.state_dict().items():
        ref = gold["adamw.final." + k]
        print("final", k, np.abs(v.cpu().numpy() - ref).max())
        assert np.abs(v.cpu().numpy() - ref).max() <= 5e-6 * max(1.0, np.abs(ref).max()), k
    _, g64 = R.loss_and_grads(R.state_from(gold, "sd."), gold["v_feat"], gold["users"][0], gold["items"][0])
    assert all(float(g64[k].abs().min()) > 0 for k in ("feature_projection.weight", "bias_projection.weight"))


def test_kernels_at_the_shipped_width_match_float64_and_touch_only_their_rows():
    """Dh = 2048, F = 2048, B = 512 on the ops themselves, against the float64 restatement.  Bounds, derived before any run:

    * e and dW are GEMMs of the library: the error of its f32-input MFMA GEMM on the SAME operands against float64 is measured
      here, and the default operand split may have 2 x that (different summation order, nothing more).
    * x_b sums 4 Dh products in fp32: a lane adds 2 Dh / 64 products to each of two chains, six wave-reduction adds and the
      biases follow: n_x = 2 Dh / 64 + 16 roundings on S_b = sum |terms|, plus the projection's error through <um_b, e>:
      dx = n_x u S + max_b |um_b|_1 err_e.   |d coef / d x| <= 1 / (4 B) (the slope of the sigmoid), so
      dc = dx / (4 B) + 16 u max|c| (the float32 evaluation of the sigmoid quotient).
    * a sparse row sums `mult` occurrences of c_b times a difference of two rows (or one row): mult (dc + 8 u cmax) times the
      largest such operand, for the modal rows plus mult cmax 2 err_e.
    * d w_b sums R = 2B rows: 32 row lanes of R / 32 adds, then 32 partials: R (dc + (R / 32 + 40) u cmax) max|x|.
    * dW against the restatement: the measured GEMM allowance on its own operands, plus the operand's error through the sum:
      R (dc + 4 u cmax) max|um| max|x|."""
    rng = np.random.default_rng(17)
    U, I, Dh, F, B = 40, 60, 2048, 2048, 512
    user = rng.integers(0, 6, size=B)                                      # heavy repetition
    item = rng.integers(0, 9, size=(B, 2))
    item[:, 1][item[:, 1] == item[:, 0]] = 11
    v_feat = rng.standard_normal((I, F)).astype(np.float32)
    table = (rng.standard_normal((1 + 2 * U + I, Dh)) * 0.02).astype(np.float32)
    W = (rng.standard_normal((Dh, F)) * np.sqrt(2.0 / (Dh + F))).astype(np.float32)
    wb = (rng.standard_normal(F) * np.sqrt(2.0 / (1 + F))).astype(np.float32)
    t = lambda a: torch.from_numpy(a).cuda()
    user_d, item_d, feat_d, table_d, W_d, wb_d = t(user), t(item), t(v_feat), t(table), t(W), t(wb)
    gs = torch.tensor([0.75], device="cuda")
    outs = []
    for _ in range(2):
        rows = ops.vbpr_rows(user_d, item_d, U, I)
        x, beta = ops.vbpr_gather(feat_d, item_d.view(-1), wb_d)
        e = ops.linear_fwd(x, W_d, None)
        loss, coef = ops.vbpr_pair_fwd(table_d, rows, e, beta, B)
        sp = ops.SparseRows(4 * B, Dh, "cuda")
        sp.rows.fill_(float("nan"))
        de = torch.full((2 * B, Dh), float("nan"), device="cuda")
        cs = torch.full((2 * B,), float("nan"), device="cuda")
        ops.vbpr_pair_bwd(table_d, rows, e, coef, B, de, cs, sp, grad_scale=2.0, grad_scale_dev=gs)
        dwb = ops.vbpr_bias_grad(x, cs, torch.full((F,), float("nan"), device="cuda"))
        dW = torch.full((Dh, F), float("nan"), device="cuda")
        ops.grouped_linear_bwd_weight([(de, x, dW, None)])
        torch.cuda.synchronize()
        outs.append([a.clone() for a in (rows, x, beta, e, loss, coef, de, cs, sp.idx, sp.rows, dwb, dW)] + [sp.count()])
    for a, b in zip(outs[0][:-1], outs[1][:-1]):
        assert torch.equal(a, b)                                           # bit-identical from run to run
    rows, x, beta, e, loss, coef, de, cs, idx, srows, dwb, dW, n = outs[0]
    assert n == 4 * B and all(torch.isfinite(a).all() for a in (e, loss, coef, de, cs, srows, dwb, dW))
    ops.raise_on_bad_indices()
    assert torch.equal(x, feat_d[item_d.view(-1)])                         # the gather is a copy
    touched = set(rows.cpu().tolist())
    live = idx[idx > 0].cpu().tolist()
    assert len(live) == len(set(live)) and set(live) == touched           # one slot per touched row, nothing else
    # the f32-input MFMA GEMM on the same operands, against float64
    prev = ops.set_gemm_mode("f32")
    try:
        e32 = ops.linear_fwd(x, W_d, None)
        dW32 = torch.empty_like(dW)
        ops.grouped_linear_bwd_weight([(de, x, dW32, None)])
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_mode(prev)
    x64 = x.double().cpu()
    e64 = x64 @ torch.from_numpy(W).double().T
    dW64_same = de.double().cpu().T @ x64
    err_e32 = float((e32.double().cpu() - e64).abs().max())
    err_dW32 = float((dW32.double().cpu() - dW64_same).abs().max())
    err_e = float((e.double().cpu() - e64).abs().max())
    err_dW = float((dW.double().cpu() - dW64_same).abs().max())
    print("GEMM errors: e", err_e, "f32-input", err_e32, "| dW", err_dW, "f32-input", err_dW32)
    assert err_e <= 2 * err_e32 and err_dW <= 2 * err_dW32
    # the float64 restatement (the loss scaled by grad_scale * grad_scale_dev = 1.5)
    sp_ = {"user_id_embedding.weight": (1, 1 + U), "item_id_embedding.weight": (1 + U, 1 + U + I),
           "user_modal_embedding.weight": (1 + U + I, 1 + 2 * U + I)}
    P = {k: torch.from_numpy(table[lo:hi]).double() for k, (lo, hi) in sp_.items()}
    P["feature_projection.weight"] = torch.from_numpy(W).double()
    P["bias_projection.weight"] = torch.from_numpy(wb).double()[None]
    L64, g64 = R.loss_and_grads(P, v_feat, user, item)
    assert abs(float(loss) - L64) <= 2e-6 * max(1.0, L64)
    g64 = {k: (1.5 * v).numpy() for k, v in g64.items()}
    um = np.abs(table[1 + U + I + user])
    s64 = R.scores(P, v_feat, user, item)
    xb = (s64[:, 0] - s64[:, 1]).numpy()
    cmax = 1.5 / B                                                         # |coef| <= 1 / B, times the scale
    ev = np.abs(e64.numpy()).reshape(B, 2, Dh)
    S = (np.abs(table[1 + user])[:, None] * np.abs(table[1 + U + item])).sum(-1).sum(-1) + (um[:, None] * ev).sum(-1).sum(-1) \
        + np.abs(beta.cpu().numpy()).reshape(B, 2).sum(-1)
    dx = (2 * Dh / 64 + 16) * U32 * S.max() + um.sum(-1).max() * 2 * err_e32
    dc = 1.5 * dx / (4 * B) + 16 * U32 * cmax
    print("|x| max", np.abs(xb).max(), "dx", dx, "dc", dc, "cmax", cmax)
    dense = torch.zeros(1 + 2 * U + I, Dh, dtype=torch.float64)
    keep = idx > 0
    dense[idx[keep].cpu()] = srows[keep].double().cpu()
    dense = dense.numpy()
    mult = np.bincount(rows.cpu().numpy(), minlength=1 + 2 * U + I)[:, None]
    tmax, emax, xmax = np.abs(table).max(), float(e64.abs().max()), np.abs(v_feat).max()
    for k, (lo, hi) in sp_.items():
        op = 2 * emax if k == "user_modal_embedding.weight" else 2 * tmax
        tol = mult[lo:hi] * ((dc + 8 * U32 * cmax) * op + (cmax * 2 * 2 * err_e32 if k == "user_modal_embedding.weight" else 0.0)) + 1e-12
        err = np.abs(dense[lo:hi] - g64[k])
        print(k, "max error", err.max(), "largest bound", tol.max(), "largest entry", np.abs(g64[k]).max())
        assert (err <= tol).all(), k
    assert float(np.abs(dense[[i for i in range(1 + 2 * U + I) if i not in touched]]).max(initial=0.0)) == 0.0
    Rn = 2 * B
    tol_wb = Rn * (dc + (Rn / 32 + 40) * U32 * cmax) * xmax
    err_wb = np.abs(dwb.double().cpu().numpy() - g64["bias_projection.weight"][0]).max()
    print("d w_b max error", err_wb, "bound", tol_wb, "largest entry", np.abs(g64["bias_projection.weight"]).max())
    assert err_wb <= tol_wb
    tol_W = 2 * err_dW32 + Rn * (dc + 4 * U32 * cmax) * um.max() * xmax
    err_W = np.abs(dW.double().cpu().numpy() - g64["feature_projection.weight"]).max()
    print("dW max error", err_W, "bound", tol_W, "largest entry", np.abs(g64["feature_projection.weight"]).max())
    assert err_W <= tol_W


def _random_batches(rng, U, I, B, n):
    out = []
    for s in range(n):
        lo = 0 if s % 3 else 20                            # some rows sit out several steps, then come back
        item = rng.integers(lo, lo + 25, size=(B, 2))
        item[:, 1][item[:, 1] == item[:, 0]] = lo + 26
        out.append((torch.from_numpy(rng.integers(lo, lo + 10, size=B)).cuda(), torch.from_numpy(item).cuda()))
    return out


def test_lazy_and_dense_table_updates_are_bit_identical(tmp_path, monkeypatch):
    monkeypatch.setenv("PXR_LAZY_REPLAY", "exact")
    rng = np.random.default_rng(4)
    U, I, D, F, B = 40, 60, 128, 24, 16
    v_feat = rng.standard_normal((I, F)).astype(np.float32)
    sd = _model(tmp_path, U, I, D, v_feat).state_dict()
    batches = _random_batches(rng, U, I, B, 12)
    res = {}
    for how in ("lazy", "dense"):
        m = _model(tmp_path, U, I, D, v_feat, sd={k: v.clone() for k, v in sd.items()})
        opt = _opt(m, how)
        for u, it in batches:
            opt.zero_grad()
            m((u, it)).backward()
            opt.step()
        opt.flush()
        torch.cuda.synchronize()
        res[how] = (m.lazy_table().clone(), opt._tm.clone(), opt._tv.clone(), m.flat_parameters()[0].clone(), opt._m.clone())
    for a, b in zip(res["lazy"], res["dense"]):
        assert torch.equal(a, b)
    assert not torch.equal(res["lazy"][0][1:], torch.cat([sd[k] for k in TABLES]))         # ... and the steps moved the tables


def test_two_runs_and_graph_replay_are_bit_identical_to_eager_steps(tmp_path):
    from pixelrec_amd.graph import GraphedTrainStep

    rng = np.random.default_rng(8)
    U, I, D, F, B = 40, 60, 128, 24, 16
    v_feat = rng.standard_normal((I, F)).astype(np.float32)
    sd = _model(tmp_path, U, I, D, v_feat).state_dict()
    batches = _random_batches(rng, U, I, B, 6)                             # six different batches
    out = {}
    for how in ("eager", "eager again", "graph"):
        m = _model(tmp_path, U, I, D, v_feat, sd={k: v.clone() for k, v in sd.items()})
        opt = _opt(m)
        losses = []
        gs = GraphedTrainStep(m, opt, batches[0][0], batches[0][1], warmup=0) if how == "graph" else None
        for u, it in batches:
            if gs is not None:
                loss = gs(u, it)
            else:
                opt.zero_grad()
                loss = m((u, it))
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


def test_fused_topk_equals_predict_mask_topk(tmp_path):
    """Top-10 ids of the fused path on the packed matrices against predict -> column 0 and history masked -> torch.topk.  A user
    whose literal scores around the cut are closer than the fixture's score tolerance (2e-5) may be compared on scores instead of
    ids; at most 1 % of the users may need that (a cap, not a measurement), and with these seeds the float64 restatement has no
    such near-tie at all (asserted), so a difference in ids is a difference in arithmetic."""
    rng = np.random.default_rng(5)
    Un, In, D, F, K, H = 200, 3000, 64, 40, 10, 5
    v_feat = rng.standard_normal((In, F)).astype(np.float32)
    torch.manual_seed(7)                                   # (chosen on the float64 restatement alone: seeds 1-6 leave gaps below 5e-5)
    m = _model(tmp_path, Un, In, D, v_feat)
    m.eval()
    feat = m.compute_item_all()
    packed = m.scoring_item_matrix()
    assert packed.shape == (In, ops.vbpr_packed_width(D // 2)) and packed.shape[1] % 32 == 0
    user = torch.arange(0, Un, dtype=torch.int64)
    hu = torch.from_numpy(np.repeat(np.arange(Un), H))
    hi = torch.from_numpy(rng.integers(1, In, size=Un * H))
    ptr, hitems = ops.history_csr(hu, hi, Un, "cuda")
    out, last = m.encode_last(user.cuda(), feat)
    assert out.shape == (Un, 1, packed.shape[1])
    idx, val = ops.score_topk(last, last.stride(0), Un, packed, K, ptr, hitems)
    planes = ops.split_planes(packed.contiguous()) if ops.score_planes_supported(packed) else None
    if planes is not None:                                                # the Trainer's route: pre-split item planes
        idx_p, _ = ops.score_topk(last, last.stride(0), Un, packed, K, ptr, hitems, table_planes=planes,
                                  table_norm_max=ops.row_norm_max(packed))
        assert torch.equal(idx_p, idx)
    scores = m.predict(user.cuda(), feat)
    scores[:, 0] = -np.inf
    scores[(hu.cuda(), hi.cuda())] = -np.inf
    ref = torch.topk(scores, K + 1, dim=-1)
    # float64: no near-tie among the first K + 1 scores of any user
    P = {k: v.double().cpu() for k, v in m.state_dict().items()}
    s64 = R.predict(P, v_feat, user.numpy())
    s64[:, 0] = -np.inf
    s64[(hu, hi)] = -np.inf
    top64 = torch.topk(s64, K + 1, dim=-1).values
    assert float((top64[:, :-1] - top64[:, 1:]).min()) > 2 * 2e-5
    same = (idx == ref.indices[:, :K]).all(-1)
    on_scores = int((~same).sum())
    print("users compared on scores:", on_scores, "of", Un)
    assert on_scores <= Un // 100
    assert (val[~same] - ref.values[~same][:, :K]).abs().max(initial=0.0) <= 2e-5 if on_scores else True
    assert float((val - ref.values[:, :K]).abs().max()) <= 2e-5


def test_bad_ids_raise_index_error_and_bad_feature_files_raise_value_error(gold, tmp_path):
    from pixelrec_amd.model import VBPR

    m = _gold_model(gold, tmp_path)
    U, I = (int(x) for x in gold["meta"][:2])
    good_u, good_i = torch.from_numpy(gold["users"][0]).cuda(), torch.from_numpy(gold["items"][0]).cuda()
    ops.raise_on_bad_indices()
    for u, it in ((good_u.clone().fill_(U), good_i), (good_u, good_i.clone().fill_(I)), (good_u.clone().fill_(-1), good_i),
                  (good_u, good_i.clone().fill_(-3))):
        m((u, it)).backward()
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices()
    m((good_u, good_i)).backward()
    ops.raise_on_bad_indices()                             # a clean batch leaves the word clear
    m.eval()
    feat = m.compute_item_all()
    with pytest.raises(IndexError):
        m.predict(good_u.clone().fill_(U), feat)
    m.predict(good_u, feat)
    for shape, what in (((I + 1, 12), "item_num"), ((I, 10), "multiple of 4")):
        path = str(tmp_path / ("bad_%d_%d.npy" % shape))
        np.save(path, np.zeros(shape, dtype=np.float32))
        with pytest.raises(ValueError, match=what):
            VBPR({"embedding_size": 16, "mlp_hidden_size": [], "dropout_prob": 0.0, "v_feat_path": path}, _Data(U, I))


def test_checkpoint_loads_into_the_reference_layout_and_resumes_the_trajectory(gold, tmp_path, monkeypatch):
    monkeypatch.setenv("PXR_LAZY_REPLAY", "exact")     # flushed and lagging rows then replay the dense sweep's own arithmetic
    users = torch.from_numpy(gold["users"]).cuda()
    items = torch.from_numpy(gold["items"]).cuda()
    ref = _gold_model(gold, tmp_path)
    _steps(ref, _opt(ref), users, items, range(4))
    a = _gold_model(gold, tmp_path)
    opt = _opt(a)
    _steps(a, opt, users, items, range(2))
    ck = {"state_dict": {k: v.detach().cpu() for k, v in a.state_dict().items()}, "optimizer": opt.state_dict(layout="torch")}
    path = tmp_path / "vbpr.pth"
    torch.save(ck, path)
    ck = torch.load(path, weights_only=False)
    # the Trainer's checkpoint content (trainer._checkpoint_tensors): the reference's names, shapes and optimizer layout
    names = list(ck["state_dict"].keys())
    assert names == list(R.NAMES)
    assert [g["params"] for g in ck["optimizer"]["param_groups"]] == [[0, 1], [2, 3, 4]]
    for j, n in enumerate(names):
        assert tuple(ck["optimizer"]["state"][j]["exp_avg"].shape) == tuple(ck["state_dict"][n].shape), n
    tor = [torch.nn.Parameter(ck["state_dict"][n].clone()) for n in names]
    topt = torch.optim.AdamW([{"params": [p for n, p in zip(names, tor) if "projection" in n], "lr": 1.0, "weight_decay": 0.5},
                              {"params": [p for n, p in zip(names, tor) if "projection" not in n], "lr": 1.0, "weight_decay": 0.5}])
    topt.load_state_dict(ck["optimizer"])                  # strict layout: torch's own loader
    assert (topt.param_groups[0]["lr"], topt.param_groups[0]["weight_decay"]) == (1e-4, 0.1)
    assert (topt.param_groups[1]["lr"], topt.param_groups[1]["weight_decay"]) == (1e-3, 0)
    b = _gold_model(gold, tmp_path)
    b.load_state_dict(ck["state_dict"], strict=True)
    opt_b = _opt(b)
    opt_b.load_state_dict(ck["optimizer"])
    _steps(b, opt_b, users, items, range(2, 4))
    sr, sb = ref.state_dict(), b.state_dict()
    for k in sr:
        assert torch.equal(sr[k], sb[k]), k


def test_main_py_trains_two_epochs_and_reports_recall_and_ndcg(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth_dataset

    from pixelrec_amd.config import Config
    from pixelrec_amd.data import load_data

    synth_dataset.main(str(tmp_path / "data"), 3000, 800)
    shipped = os.path.join(ROOT, "configs", "ViNet", "vbpr.yaml")
    (tmp_path / "o.yaml").write_text(f"embedding_size: 128\nstate: INFO\nreproducibility: True\ncheckpoint_dir: '{tmp_path}/saved'\n"
                                     f"log_path: '{tmp_path}/log'\ndata_path: {tmp_path}/data/\nv_feat_path: {tmp_path}/feat.npy\n"
                                     "epochs: 2\ntrain_batch_size: 64\n")
    item_num = load_data(Config([shipped, str(tmp_path / "o.yaml")])).item_num
    np.save(str(tmp_path / "feat.npy"), np.random.default_rng(0).standard_normal((item_num, 40)).astype(np.float32))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "OMP_NUM_THREADS")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--device", "0", "--config_file", shipped,
                        str(tmp_path / "o.yaml")], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert len(re.findall(r"epoch \d+ training \[time", out)) == 2, out[-3000:]
    assert "training step captured as a hipGraph (batch size 64)" in out, out[-3000:]
    assert "Loading model structure and parameters from" in out, out[-3000:]     # the test result comes from the checkpoint
    for metric in ("recall@5", "ndcg@5", "recall@10", "ndcg@10"):
        mm = re.search(r"test result: .*?'%s', ([0-9.]+)\)" % metric, out)
        assert mm is not None and 0.0 <= float(mm.group(1)) <= 1.0, out[-2000:]
