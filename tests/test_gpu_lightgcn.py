"""LightGCN on the gfx950 kernels (csrc/lightgcn.hip): the CSR SpMM with its layer-mean epilogue against float64 with a tolerance
derived from fp32 rounding, run-to-run bit identity, the model against the golden fixture of the reference's own LightGCN (loss,
both table gradients, 4 AdamW steps, K = 1 and 3), the pair head through sigmoid saturation, hipGraph replay against eager steps,
the fused top-k against the literal predict -> mask -> topk path, bad ids, and main.py end to end."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pixelrec_amd import ops
from pixelrec_amd.data.dataload import norm_adj_csr
from tests import lightgcn_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lightgcn_tiny.npz")
U32 = 2.0 ** -24                                           # unit roundoff of fp32


class _Data:
    """What LightGCN reads from a Data object: the table sizes and the CSR."""

    def __init__(self, U, I, csr):
        self.user_num, self.item_num, self._csr = U, I, csr

    def get_norm_adj_csr(self):
        return self._csr


def _model(U, I, csr, D, K, sd=None):
    from pixelrec_amd.model import LightGCN

    m = LightGCN({"embedding_size": D, "n_layers": K}, _Data(U, I, csr))
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.cuda().train()


def _skewed_csr(n, rng, long_row=None, long_deg=0):
    """A CSR over n nodes (not bipartite: the kernel does not care) with rows of degree 0, 1, a Zipf-ish spread and one row of
    long_deg edges; weights in (0, 1]."""
    deg = np.minimum(rng.zipf(1.6, size=n), 300).astype(np.int64)
    deg[0] = 0; deg[1] = 1; deg[n // 2] = 0; deg[-1] = 1
    if long_row is not None:
        deg[long_row] = long_deg
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=row_ptr[1:])
    col = rng.integers(0, n, size=int(row_ptr[-1])).astype(np.int32)
    w = rng.uniform(0.01, 1.0, size=len(col)).astype(np.float32)
    return row_ptr, col, w


def _bound(A, e0, K, deg):
    """Entrywise bound on |fp32 propagation - exact| (the fp32 inputs are exact): each layer's row sums carry at most
    gamma_{deg+2} |A| |E| of fresh error (deg products and additions in some order, plus the epilogue add), the propagated error
    of the previous layer |A| err, and the mean's K+1 additions and scaling gamma_{K+3} sum |E_k|."""
    absA = abs(A)
    gam = lambda n: n * U32 / (1 - n * U32)
    g_row = gam(deg + 2.0)[:, None]
    e_abs, err, tot_abs, tot_err = np.abs(e0), np.zeros_like(e0), np.abs(e0), np.zeros_like(e0)
    for _ in range(K):
        nxt = absA @ e_abs
        err = absA @ err + g_row * nxt
        e_abs = nxt + err
        tot_abs = tot_abs + e_abs
        tot_err = tot_err + err
    return (tot_err + gam(K + 3.0) * tot_abs) / (K + 1)


@pytest.mark.parametrize("D", [4, 64, 256, 1024])
def test_spmm_propagation_matches_float64_and_is_deterministic(D):
    rng = np.random.default_rng(D)
    n = 1001                                               # not a multiple of the 4 rows of a block
    long_deg = 120_000 if D in (4, 256) else 3_000         # > 100 K edges: the split path (part_len 512 either way)
    csr = _skewed_csr(n, rng, long_row=7, long_deg=long_deg)
    A = R.csr_matrix(*csr)
    deg = np.diff(csr[0]).astype(np.float64)
    e0 = rng.standard_normal((n, D)).astype(np.float32)
    for K in (1, 2, 3):
        m = _model(500, n - 500, csr, D, K, {"user_embedding.weight": torch.from_numpy(e0[:500]),
                                             "item_embedding.weight": torch.from_numpy(e0[500:])})
        m.flat_parameters()                                # packs the tables, puts the graph on the device
        assert m._graph.n_split >= 1
        u, i = m.computer()
        got = torch.cat([u, i]).cpu().numpy().astype(np.float64)
        ref = R.propagate(A, e0.astype(np.float64), K)
        tol = _bound(A, e0.astype(np.float64), K, deg)
        bad = np.abs(got - ref) > tol
        assert not bad.any(), (K, np.argwhere(bad)[:5], np.abs(got - ref)[bad][:5], tol[bad][:5])
        u2, i2 = m.computer()
        assert torch.equal(u, u2) and torch.equal(i, i2)   # bit-identical from run to run
        # the backward's Horner chain on the same graph
        g = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).cuda()
        out = torch.empty_like(g)
        m.propagate_grad(g, out)
        ref_g = R.propagate(A, g.cpu().numpy().astype(np.float64), K)
        tol_g = _bound(A, g.cpu().numpy().astype(np.float64), K, deg)
        assert (np.abs(out.cpu().numpy() - ref_g) <= tol_g).all(), K
    torch.cuda.synchronize()
    ops.raise_on_bad_indices()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _gold_model(g, K):
    U, I, D = int(g["meta"][0]), int(g["meta"][1]), int(g["meta"][2])
    csr = norm_adj_csr(g["train_u"], g["train_i"], U, I)
    sd = {k: torch.from_numpy(g["sd." + k]) for k in ("user_embedding.weight", "item_embedding.weight")}
    return _model(U, I, csr, D, K, sd), U


@pytest.mark.parametrize("K", [1, 3])
def test_model_matches_the_reference_fixture(gold, K):
    from pixelrec_amd.optim import PxrAdamW

    p = f"k{K}."
    m, U = _gold_model(gold, K)
    lr, wd = (float(x) for x in gold["lr_wd"])
    users = torch.from_numpy(gold["users"]).cuda()
    items = torch.from_numpy(gold["items"]).cuda()
    loss = m((users[0], items[0]))
    loss.backward()
    assert abs(float(loss) - float(gold[p + "loss"])) <= 2e-6 * max(1.0, float(gold[p + "loss"]))
    for name in ("user_embedding.weight", "item_embedding.weight"):
        got = getattr(m, name.split(".")[0]).weight.grad.cpu().numpy()
        ref = gold[p + "grad." + name]
        assert np.abs(got - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()), name
    m.eval()
    m.compute_item_all()
    scores = m.predict(torch.from_numpy(gold["eval.users"]).cuda()).cpu().numpy()
    assert np.abs(scores - gold[p + "eval.scores"]).max() <= 1e-5
    m2, _ = _gold_model(gold, K)
    opt = PxrAdamW(m2, lr=lr, weight_decay=wd)
    for s in range(4):
        opt.zero_grad()
        loss = m2((users[s], items[s]))
        loss.backward()
        opt.step()
        assert abs(float(loss) - float(gold[p + f"adamw.loss{s}"])) <= 2e-6 * max(1.0, float(loss)), s
    sd = m2.state_dict()
    for name in ("user_embedding.weight", "item_embedding.weight"):
        assert np.abs(sd[name].cpu().numpy() - gold[p + "adamw.final." + name]).max() <= 2e-6, name


def test_pair_head_saturation_stays_finite_and_close_to_float64():
    xs = np.array([-100.0, -60.0, -20.0, -3.0, -1e-3, 0.0, 1e-3, 3.0, 20.0, 60.0, 100.0])
    B, U, D = len(xs), len(xs), 4
    I = len(xs) + 1
    emb = np.zeros((U + I, D), dtype=np.float32)
    emb[:U, 0] = 1.0                                       # u_b = e_0
    emb[U + np.arange(B), 0] = xs                          # i+_b = x_b e_0, i-_b = item B = 0  =>  x_b exactly
    user = torch.arange(B, dtype=torch.int64).cuda()
    item = torch.from_numpy(np.stack([np.arange(B), np.full(B, B)], 1).astype(np.int64)).cuda()
    e = torch.from_numpy(emb).cuda()
    loss, diff, coef, nodes = ops.lgcn_pair_fwd(e, U, I, user, item)
    grad = ops.lgcn_pair_bwd(e, nodes, coef, torch.empty_like(e))
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(coef).all() and torch.isfinite(grad).all()
    assert np.array_equal(diff.cpu().numpy(), xs.astype(np.float32))
    terms = -(1e-8 + R.log_sigmoid(xs))
    ref_loss = float(np.mean(terms))
    # each term: a few ulp (exp, log1p, two adds); the mean: B additions and a division
    assert abs(float(loss) - ref_loss) <= (8 + B + 1) * U32 * float(np.mean(np.abs(terms)))
    ref_coef = -R.sigmoid_neg(xs) / B
    got = coef.cpu().numpy().astype(np.float64)
    # exp, division, 1/B: a few ulp; below fp32's normal range (e^-100 / B ~ 3e-45) only an absolute bound of that range holds
    tiny = np.finfo(np.float32).tiny
    assert (np.abs(got - ref_coef) <= 16 * U32 * np.abs(ref_coef) + tiny).all(), (got, ref_coef)
    g = grad.cpu().numpy().astype(np.float64)
    assert (np.abs(g[:U, 0] - ref_coef * xs) <= 16 * U32 * np.abs(ref_coef * xs) + 100 * tiny).all()   # d u_b = c_b (i+ - i-)
    assert (np.abs(g[U:U + B, 0] - ref_coef) <= 16 * U32 * np.abs(ref_coef) + tiny).all()             # d i+_b = c_b u_b


def test_graph_replay_is_bit_identical_to_eager_steps(gold):
    from pixelrec_amd.graph import GraphedTrainStep
    from pixelrec_amd.optim import PxrAdamW

    users = torch.from_numpy(gold["users"]).cuda()
    items = torch.from_numpy(gold["items"]).cuda()
    out = {}
    for how in ("eager", "graph"):
        m, _ = _gold_model(gold, 3)
        opt = PxrAdamW(m, lr=1e-3, weight_decay=0.1)
        losses = []
        gs = GraphedTrainStep(m, opt, users[0], items[0], warmup=0) if how == "graph" else None
        for s in range(3):
            if gs is not None:
                loss = gs(users[s], items[s])
            else:
                opt.zero_grad()
                loss = m((users[s], items[s]))
                loss.backward()
                opt.step()
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        out[how] = (torch.stack(losses), m.flat_parameters()[0].clone(), opt._m.clone(), opt._v.clone())
    for a, b in zip(out["eager"], out["graph"]):
        assert torch.equal(a, b)


def test_fused_topk_equals_predict_mask_topk():
    rng = np.random.default_rng(5)
    # a larger catalogue so that top-10 is a real selection: a random bipartite graph
    Un, In, D = 60, 400, 64
    tu = rng.integers(1, Un, size=3000)
    ti = rng.integers(1, In, size=3000)
    m = _model(Un, In, norm_adj_csr(tu, ti, Un, In), D, 2)
    m.eval()
    feat = m.compute_item_all()
    user = torch.arange(1, Un, dtype=torch.int64)
    hu = torch.from_numpy(np.repeat(np.arange(Un - 1), 5))
    hi = torch.from_numpy(rng.integers(1, In, size=(Un - 1) * 5))
    ptr, hitems = ops.history_csr(hu, hi, Un - 1, "cuda")
    _, last = m.encode_last(user.cuda(), feat)
    idx, _ = ops.score_topk(last, last.stride(0), Un - 1, feat, 10, ptr, hitems)
    scores = m.predict(user.cuda(), feat)
    scores[:, 0] = -np.inf
    scores[(hu.cuda(), hi.cuda())] = -np.inf
    ref = torch.topk(scores, 10, dim=-1).indices
    assert torch.equal(idx, ref)


def test_bad_user_or_item_id_raises_index_error(gold):
    m, U = _gold_model(gold, 1)
    I = int(gold["meta"][1])
    good_u, good_i = torch.from_numpy(gold["users"][0]).cuda(), torch.from_numpy(gold["items"][0]).cuda()
    ops.raise_on_bad_indices()
    for u, it in ((good_u.clone().fill_(U), good_i), (good_u, good_i.clone().fill_(I)), (good_u, good_i.clone().fill_(-1))):
        m((u, it)).backward()
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices()
    m((good_u, good_i)).backward()
    ops.raise_on_bad_indices()                             # a clean batch leaves the word clear


def test_main_py_trains_two_epochs_and_reports_recall_and_ndcg(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth_dataset

    synth_dataset.main(str(tmp_path / "data"), 3000, 800)
    (tmp_path / "m.yaml").write_text("model: LightGCN\nembedding_size: 64\nn_layers: 2\n")
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
