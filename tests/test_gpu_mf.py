"""MF on the gfx950 kernels (csrc/mf.hip): the model against the golden fixture of the reference's own MF (loss, every gradient
with user 0 and item 0, predict, a 4-step PxrAdamW trajectory with the BatchNorm running statistics; identity towers and
[8, 4]), the BatchNorm + tanh kernels and the sparse pair backward against float64 with run-to-run bit identity, lazy against
dense table updates, hipGraph replay against eager steps, the fused top-k, bad ids, checkpoints in the reference layout, and
main.py end to end."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pixelrec_amd import ops
from tests import mf_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "mf_tiny.npz")
U32 = 2.0 ** -24


class _Data:
    def __init__(self, U, I):
        self.user_num, self.item_num = U, I


def _model(U, I, D, hidden, sd=None, dropout=0.0):
    from pixelrec_amd.model import MF

    m = MF({"embedding_size": D, "mlp_hidden_size": list(hidden), "dropout_prob": dropout}, _Data(U, I))
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.cuda().train()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _gold_model(g, cfg):
    U, I, D = (int(x) for x in g["meta"][:3])
    pre = cfg + ".sd."
    sd = {k[len(pre):]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith(pre)}
    return _model(U, I, D, [int(h) for h in g[cfg + ".hidden"]], sd)


def _grad_of(m, name):
    """The dense gradient of a reference parameter: tower parameters from the flat buffer, the tables from the sparse rows."""
    if name.endswith("_embedding.weight"):
        sp = m.sparse_table_grad
        dense = sp.to_dense(m.lazy_table().shape[0])
        lo, hi = m.table_parameter_spans()[name]
        return dense[lo:hi].cpu().numpy()
    return dict(m.named_parameters())[name].grad.cpu().numpy()


@pytest.mark.parametrize("cfg", ["c0", "c1"])
def test_model_matches_the_reference_fixture(gold, cfg):
    from pixelrec_amd.optim import PxrAdamW

    m = _gold_model(gold, cfg)
    users = torch.from_numpy(gold["users"]).cuda()
    items = torch.from_numpy(gold["items"]).cuda()
    loss = m((users[0], items[0]))
    loss.backward()
    assert abs(float(loss) - float(gold[cfg + ".loss"])) <= 2e-6 * max(1.0, float(gold[cfg + ".loss"]))
    for k in [k[len(cfg + ".grad."):] for k in gold.files if k.startswith(cfg + ".grad.")]:
        ref = gold[cfg + ".grad." + k]
        got = _grad_of(m, k)
        assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), k
    for k in ("user_embedding.weight", "item_embedding.weight"):
        assert np.abs(_grad_of(m, k)[0]).max() > 0                 # row 0 of either table is an ordinary, trained row
    m.eval()
    feat = m.compute_item_all()
    scores = m.predict(torch.from_numpy(gold["eval.users"]).cuda(), feat).cpu().numpy()
    assert np.abs(scores - gold[cfg + ".eval.scores"]).max() <= 2e-5
    m2 = _gold_model(gold, cfg)
    lr, wd = (float(x) for x in gold["lr_wd"])
    opt = PxrAdamW(m2, lr=lr, weight_decay=wd)
    for s in range(4):
        opt.zero_grad()
        loss = m2((users[s], items[s]))
        loss.backward()
        opt.step()
        assert abs(float(loss) - float(gold[cfg + f".adamw.loss{s}"])) <= 5e-6 * max(1.0, float(loss)), s
    sd = m2.state_dict()
    for k, v in sd.items():
        ref = gold[cfg + ".adamw.final." + k]
        got = v.cpu().numpy()
        if v.dtype == torch.int64:
            assert int(v) == int(ref), k
        elif R.noise_driven(k):
            assert np.abs(got - ref).max() <= 4 * 4 * lr, k
        else:
            assert np.abs(got - ref).max() <= 5e-6 * max(1.0, np.abs(ref).max()), k


@pytest.mark.parametrize("rows", [2, 3, 128, 2049])
@pytest.mark.parametrize("H", [4, 260, 4096])
def test_bn_tanh_kernels_match_float64_and_are_deterministic(rows, H):
    rng = np.random.default_rng(rows * 7 + H)
    x = (rng.standard_normal((rows, H)) * 2 + rng.standard_normal(H)).astype(np.float32)
    gam = (1 + 0.3 * rng.standard_normal(H)).astype(np.float32)
    bet = (0.2 * rng.standard_normal(H)).astype(np.float32)
    dy = rng.standard_normal((rows, H)).astype(np.float32)
    rm0 = (0.1 * rng.standard_normal(H)).astype(np.float32)
    rv0 = (0.5 + rng.random(H)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).cuda()
    outs = []
    for _ in range(2):
        rm, rv, nbt = t(rm0.copy()), t(rv0.copy()), torch.zeros((), dtype=torch.int64, device="cuda")
        y, mean, rstd = ops.mf_bn_tanh_fwd(t(x), t(gam), t(bet), rm, rv, nbt)
        dg, db = torch.empty(H, device="cuda"), torch.empty(H, device="cuda")
        dx = ops.mf_bn_tanh_bwd(t(dy), t(x), y, mean, rstd, t(gam), dg, db)
        ye = ops.mf_bn_tanh_eval(t(x), t(gam), t(bet), rm, rv)
        torch.cuda.synchronize()
        outs.append([a.clone() for a in (y, dx, dg, db, rm, rv, ye)] + [int(nbt)])
    for a, b in zip(outs[0][:-1], outs[1][:-1]):
        assert torch.equal(a, b)                                   # bit-identical from run to run
    assert outs[0][-1] == 1
    # float64 through torch autograd
    X = torch.from_numpy(x).double().requires_grad_(True)
    G = torch.from_numpy(gam).double().requires_grad_(True)
    Bt = torch.from_numpy(bet).double().requires_grad_(True)
    mu = X.mean(0)
    var = ((X - mu) ** 2).mean(0)
    Y = torch.tanh(G * (X - mu) / torch.sqrt(var + 1e-5) + Bt)
    dX, dG, dB = torch.autograd.grad(Y, (X, G, Bt), torch.from_numpy(dy).double())
    y, dx, dg, db, rm, rv, ye = (a.cpu().double().numpy() for a in outs[0][:-1])
    # error bounds from fp32 rounding: a column statistic is a sum of rows / 32 terms per lane plus 32 lane partials
    n_add = rows / 32 + 40
    rstd = 1 / np.sqrt(var.detach().numpy() + 1e-5)
    xh = np.abs((x - mu.detach().numpy()) * rstd)
    Yd = Y.detach().numpy()
    # error scale of dz = dy (1 - y^2): y carries the forward's rounding (bounded below), which dz inherits
    dz = np.abs(dy) * (1 + xh) * (1 + np.abs(gam))
    assert (np.abs(y - Yd) <= 8 * n_add * U32 * (1 + xh) * (1 + np.abs(gam)) + 1e-6).all()
    assert (np.abs(db - dB.numpy()) <= 8 * n_add * U32 * dz.sum(0) + 1e-6).all()
    s_dzx = (dz * (1 + xh)).sum(0)
    assert (np.abs(dg - dG.numpy()) <= 16 * n_add * U32 * s_dzx + 1e-6).all()
    tol_dx = 32 * n_add * U32 * np.abs(gam) * rstd * (dz + (dz.sum(0) + (1 + xh) * s_dzx) / rows) * (1 + xh)
    assert (np.abs(dx - dX.numpy()) <= tol_dx + 1e-6).all()
    uvar = var.detach().numpy() * rows / (rows - 1)
    assert np.allclose(rm, 0.9 * rm0 + 0.1 * mu.detach().numpy(), rtol=1e-5, atol=1e-6)
    assert np.allclose(rv, 0.9 * rv0 + 0.1 * uvar, rtol=1e-5, atol=1e-6)
    ref_e = np.tanh(gam * (x - rm) / np.sqrt(rv + 1e-5) + bet)
    assert np.abs(ye - ref_e).max() <= 1e-5


def test_sparse_pair_backward_at_d4096_matches_float64_and_touches_only_its_rows():
    rng = np.random.default_rng(11)
    U, I, D, B = 50, 80, 4096, 300
    user = torch.from_numpy(rng.integers(0, 5, size=B)).cuda()             # heavy repetition
    item = torch.from_numpy(rng.integers(0, 7, size=(B, 2))).cuda()
    item[:, 1][item[:, 1] == item[:, 0]] = 9
    table = torch.from_numpy(rng.standard_normal((1 + U + I, D)).astype(np.float32) * 0.05).cuda()
    rows = ops.mf_pair_rows(user, item, U, I)
    loss, coef = ops.mf_pair_fwd(table, table, B, rows=rows)
    gs = torch.tensor([0.75], device="cuda")
    outs = []
    for _ in range(2):
        sp = ops.SparseRows(3 * B, D, "cuda")
        sp.rows.fill_(float("nan"))
        ops.mf_table_grad(rows, B, sp, table=table, coef=coef, grad_scale=2.0, grad_scale_dev=gs)
        torch.cuda.synchronize()
        outs.append((sp.idx.clone(), sp.rows.clone(), sp.count()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    idx, srows, n = outs[0]
    assert n == 3 * B and torch.isfinite(srows).all()
    touched = set(rows.cpu().tolist())
    live = idx[idx > 0].cpu().tolist()
    assert len(live) == len(set(live)) and set(live) == touched           # one slot per touched row, nothing else
    # float64
    T = table.double().cpu().requires_grad_(True)
    r = rows.cpu()
    u, p, q = T[r[:B]], T[r[B::2]], T[r[B + 1::2]]
    x = (u * p).sum(-1) - (u * q).sum(-1)
    L = -torch.mean(1e-8 + torch.nn.functional.logsigmoid(x))
    (dT,) = torch.autograd.grad(L * 1.5, T)
    dense = torch.zeros(1 + U + I, D, dtype=torch.float64)
    keep = idx > 0
    dense[idx[keep].cpu()] = srows[keep].double().cpu()
    mult = np.bincount(r.numpy(), minlength=1 + U + I)[:, None]
    tol = 64 * U32 * mult * (np.abs(T.detach().numpy()).max() * 1.5 / B * 4) + 1e-9
    assert (np.abs(dense.numpy() - dT.numpy()) <= tol).all()
    assert float(np.abs(dense.numpy()[[i for i in range(1 + U + I) if i not in touched]]).max(initial=0.0)) == 0.0


@pytest.mark.parametrize("hidden", [[], [8, 4]])
def test_lazy_and_dense_table_updates_are_bit_identical(hidden, monkeypatch):
    from pixelrec_amd.optim import PxrAdamW

    monkeypatch.setenv("PXR_LAZY_REPLAY", "exact")
    rng = np.random.default_rng(4)
    U, I, D, B = 40, 60, 64, 16
    sd = _model(U, I, D, hidden).state_dict()
    batches = []
    for s in range(12):
        lo = 0 if s % 3 else 20                            # some rows sit out several steps, then come back
        batches.append((torch.from_numpy(rng.integers(lo, lo + 10, size=B)).cuda(),
                        torch.from_numpy(rng.integers(lo, lo + 25, size=(B, 2))).cuda()))
    res = {}
    for how in ("lazy", "dense"):
        m = _model(U, I, D, hidden, sd={k: v.clone() for k, v in sd.items()})
        opt = PxrAdamW(m, lr=1e-2, weight_decay=0.1, table_update=how)
        for u, it in batches:
            opt.zero_grad()
            m((u, it)).backward()
            opt.step()
        opt.flush()
        torch.cuda.synchronize()
        res[how] = (m.lazy_table().clone(), opt._tm.clone(), opt._tv.clone(), m.flat_parameters()[0].clone())
    for a, b in zip(res["lazy"], res["dense"]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("cfg", ["c0", "c1"])
def test_graph_replay_is_bit_identical_to_eager_steps(gold, cfg):
    from pixelrec_amd.graph import GraphedTrainStep
    from pixelrec_amd.optim import PxrAdamW

    users = torch.from_numpy(gold["users"]).cuda()
    items = torch.from_numpy(gold["items"]).cuda()
    out = {}
    for how in ("eager", "graph"):
        m = _gold_model(gold, cfg)
        opt = PxrAdamW(m, lr=1e-3, weight_decay=0.1)
        losses = []
        gs = GraphedTrainStep(m, opt, users[0], items[0], warmup=0) if how == "graph" else None
        for s in range(4):
            if gs is not None:
                loss = gs(users[s], items[s])
            else:
                opt.zero_grad()
                loss = m((users[s], items[s]))
                loss.backward()
                opt.step()
            losses.append(loss.detach().clone())
        opt.flush()
        torch.cuda.synchronize()
        bufs = [b.clone() for b in m.buffers()]
        out[how] = [torch.stack(losses), m.lazy_table().clone(), m.flat_parameters()[0].clone(), opt._m.clone(), opt._tm.clone(),
                    opt._tv.clone()] + bufs
    for a, b in zip(out["eager"], out["graph"]):
        assert torch.equal(a, b)


def test_fused_topk_equals_predict_mask_topk():
    rng = np.random.default_rng(5)
    Un, In, D = 60, 400, 64
    m = _model(Un, In, D, [32])
    m.eval()
    feat = m.compute_item_all()
    user = torch.arange(0, Un, dtype=torch.int64)
    hu = torch.from_numpy(np.repeat(np.arange(Un), 5))
    hi = torch.from_numpy(rng.integers(1, In, size=Un * 5))
    ptr, hitems = ops.history_csr(hu, hi, Un, "cuda")
    _, last = m.encode_last(user.cuda(), feat)
    idx, _ = ops.score_topk(last, last.stride(0), Un, feat, 10, ptr, hitems)
    scores = m.predict(user.cuda(), feat)
    scores[:, 0] = -np.inf
    scores[(hu.cuda(), hi.cuda())] = -np.inf
    ref = torch.topk(scores, 10, dim=-1).indices
    assert torch.equal(idx, ref)


def test_bad_ids_raise_index_error_and_single_row_towers_raise_value_error(gold):
    m = _gold_model(gold, "c0")
    U, I = (int(x) for x in gold["meta"][:2])
    good_u, good_i = torch.from_numpy(gold["users"][0]).cuda(), torch.from_numpy(gold["items"][0]).cuda()
    ops.raise_on_bad_indices()
    for u, it in ((good_u.clone().fill_(U), good_i), (good_u, good_i.clone().fill_(I)), (good_u.clone().fill_(-1), good_i)):
        m((u, it)).backward()
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices()
    m((good_u, good_i)).backward()
    ops.raise_on_bad_indices()                             # a clean batch leaves the word clear
    mt = _gold_model(gold, "c1")
    with pytest.raises(ValueError):
        mt((good_u[:1], good_i[:1]))


def test_checkpoint_loads_into_the_reference_layout_and_resumes_the_trajectory(gold, tmp_path, monkeypatch):
    from pixelrec_amd.optim import PxrAdamW

    monkeypatch.setenv("PXR_LAZY_REPLAY", "exact")     # flushed and lagging rows then replay the dense sweep's own arithmetic

    users = torch.from_numpy(gold["users"]).cuda()
    items = torch.from_numpy(gold["items"]).cuda()

    def steps(m, opt, rng_):
        for s in rng_:
            opt.zero_grad()
            m((users[s], items[s])).backward()
            opt.step()

    ref = _gold_model(gold, "c1")
    ref_opt = PxrAdamW(ref, lr=1e-3, weight_decay=0.1)
    steps(ref, ref_opt, range(4))
    a = _gold_model(gold, "c1")
    opt = PxrAdamW(a, lr=1e-3, weight_decay=0.1)
    steps(a, opt, range(2))
    ck = {"state_dict": {k: v.detach().cpu() for k, v in a.state_dict().items()}, "optimizer": opt.state_dict(layout="torch")}
    path = tmp_path / "mf.pth"
    torch.save(ck, path)
    ck = torch.load(path, weights_only=False)
    # the Trainer's checkpoint content (trainer._checkpoint_tensors): the reference's names, shapes and optimizer layout
    names = list(ck["state_dict"].keys())
    assert names[-2:] == ["user_embedding.weight", "item_embedding.weight"]
    assert tuple(ck["state_dict"]["user_embedding.weight"].shape) == (7, 8)
    params = [n for n in names if not (n.endswith("running_mean") or n.endswith("running_var") or n.endswith("num_batches_tracked"))]
    assert len(ck["optimizer"]["state"]) == len(params)
    for j, n in enumerate(params):
        assert tuple(ck["optimizer"]["state"][j]["exp_avg"].shape) == tuple(ck["state_dict"][n].shape), n
    tor = torch.nn.ParameterList([torch.nn.Parameter(ck["state_dict"][n].clone()) for n in params])
    topt = torch.optim.AdamW(tor.parameters(), lr=1e-3, weight_decay=0.1)
    topt.load_state_dict(ck["optimizer"])                  # strict layout: torch's own loader
    b = _gold_model(gold, "c1")
    b.load_state_dict(ck["state_dict"], strict=True)
    opt_b = PxrAdamW(b, lr=1e-3, weight_decay=0.1)
    opt_b.load_state_dict(ck["optimizer"])
    steps(b, opt_b, range(2, 4))
    sr, sb = ref.state_dict(), b.state_dict()
    for k in sr:
        assert torch.equal(sr[k], sb[k]), k


def test_main_py_trains_two_epochs_and_reports_recall_and_ndcg(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth_dataset

    synth_dataset.main(str(tmp_path / "data"), 3000, 800)
    (tmp_path / "m.yaml").write_text("model: MF\nembedding_size: 64\ndropout_prob: 0\nmlp_hidden_size: [32]\n")
    (tmp_path / "o.yaml").write_text(f"seed: 2020\nstate: INFO\nuse_modality: False\nreproducibility: True\n"
                                     f"checkpoint_dir: '{tmp_path}/saved'\nlog_path: '{tmp_path}/log'\nshow_progress: False\n"
                                     f"MAX_ITEM_LIST_LENGTH: 10\ndata_path: {tmp_path}/data/\ndataset: Pixel200K\nepochs: 2\n"
                                     "train_batch_size: 64\noptim_args: {learning_rate: 0.001, weight_decay: 0.1}\n"
                                     "eval_batch_size: 512\ntopk: [5,10]\nmetrics: ['Recall', 'NDCG']\nvalid_metric: NDCG@10\n"
                                     "metric_decimal_place: 7\neval_step: 1\nstopping_step: 30\n")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "OMP_NUM_THREADS")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--device", "0", "--config_file", str(tmp_path / "m.yaml"),
                        str(tmp_path / "o.yaml")], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert len(re.findall(r"epoch \d+ training \[time", out)) == 2, out[-3000:]
    for metric in ("recall@10", "ndcg@10"):
        mm = re.search(r"test result: .*?'%s', ([0-9.]+)\)" % metric, out)
        assert mm is not None and 0.0 <= float(mm.group(1)) <= 1.0, out[-2000:]
