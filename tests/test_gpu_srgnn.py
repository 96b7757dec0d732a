"""SRGNN on the gfx950 kernels (csrc/srgnn.hip): the device graph build against the reference collate and the float64
restatement (exactly), propagation and readout forward / backward against float64 and run to run, the model against the golden
fixture of the reference's own SRGNN (state_dict, loss, every gradient, predict, 4 AdamW steps with the lazy and the dense table
schedule), hipGraph replay against eager steps, the fused top-k, bad ids, and main.py end to end."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pixelrec_amd import ops
from pixelrec_amd.lib import PxrError
from tests import srgnn_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "srgnn_tiny.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _cfg(D, step, L):
    return {"embedding_size": D, "step": step, "MAX_ITEM_LIST_LENGTH": L}


def _model(gold, step, sd=True):
    from pixelrec_amd.model import SRGNN

    item_num, D, L = (int(x) for x in gold["meta"][:3])
    m = SRGNN(_cfg(D, step, L), type("D", (), {"item_num": item_num})())
    if sd:
        res = m.load_state_dict({k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd.")}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    return m.cuda().train()


def _batch(gold, j):
    return tuple(torch.from_numpy(gold[f"b{j}.{k}"]).cuda() for k in ("item_seq", "mask", "target"))


# ------------------------------------------------------------------------------------------------ graph build
def test_graph_build_equals_the_reference_collate(gold):
    seq = torch.from_numpy(gold["b0.item_seq"]).cuda()
    B, L = seq.shape
    g = ops.srgnn_graph(seq, int(gold["meta"][0]))
    torch.cuda.synchronize()
    items, alias, A = gold["collate.items"], gold["collate.alias"], gold["collate.A"]
    n = items.shape[1]
    nodes, A_d = g["nodes"].cpu().numpy(), g["A"].cpu().numpy()
    assert np.array_equal(nodes[:, :n], items) and not nodes[:, n:].any()
    assert np.array_equal(g["alias"].cpu().numpy(), alias)
    assert np.array_equal(A_d[:, :n, :n], A[:, :, :n]) and np.array_equal(A_d[:, :n, L:L + n], A[:, :, n:])
    A_d[:, :n, :n] = 0
    A_d[:, :n, L:L + n] = 0
    assert not A_d.any()                                   # padding nodes: zero rows and columns


@pytest.mark.parametrize("L", [1, 7, 33, 64])
def test_graph_build_matches_the_restatement_on_random_sessions(L):
    rng = np.random.default_rng(L)
    B, N = 300, 40
    seq = rng.integers(1, 6 if L > 8 else N, size=(B, L))              # heavy repeats: ids from a handful
    lens = rng.integers(0, L + 1, size=B)
    lens[:3] = (L, 1, 0)
    seq[np.arange(L)[None, :] >= lens[:, None]] = 0
    seq[5, :] = 3                                                      # one id all along: a self-loop
    tgt = rng.integers(1, N, size=(B, 2))
    g = ops.srgnn_graph(torch.from_numpy(seq).cuda(), N, torch.from_numpy(tgt).cuda(), want_occ=True, want_mask=True)
    nodes, alias, A = R.session_graph(seq)
    assert np.array_equal(g["nodes"].cpu().numpy(), nodes)
    assert np.array_equal(g["alias"].cpu().numpy(), alias)
    assert np.array_equal(g["A"].cpu().numpy(), A.astype(np.float32))
    assert np.array_equal(g["mask"].cpu().numpy(), (seq != 0).astype(np.int64))
    occ = g["occ"].cpu().numpy()
    assert np.array_equal(occ[:, :L], nodes) and np.array_equal(occ[:, L], tgt[:, 0]) and np.array_equal(occ[:, 2 * L], tgt[:, 1])
    assert not occ[:, L + 1:2 * L].any() and not occ[:, 2 * L + 1:].any()


def test_graph_build_refuses_more_than_64_positions():
    seq = torch.ones(2, 65, dtype=torch.int64, device="cuda")
    with pytest.raises(PxrError):
        ops.srgnn_graph(seq, 10)
    from pixelrec_amd.model import SRGNN

    with pytest.raises(ValueError):
        SRGNN(_cfg(8, 1, 65), type("D", (), {"item_num": 10})())


# ------------------------------------------------------------------------------------------------ propagation and readout
def _sessions(rng, B, L, pool):
    seq = rng.integers(1, pool, size=(B, L))
    lens = rng.integers(0, L + 1, size=B)
    lens[0] = L
    seq[np.arange(L)[None, :] >= lens[:, None]] = 0
    return seq


@pytest.mark.parametrize("L,D", [(10, 8), (10, 512), (64, 256), (5, 2048)])
def test_propagation_forward_and_backward_match_float64(L, D):
    rng = np.random.default_rng(D + L)
    B = 24
    _, _, A = R.session_graph(_sessions(rng, B, L, 7))
    x = rng.standard_normal((B, L, 2 * D)).astype(np.float32)
    bias = rng.standard_normal(2 * D).astype(np.float32)
    Ad, xd, bd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (A.astype(np.float32), x, bias))
    xd = xd.view(B * L, 2 * D)
    y = ops.srgnn_prop(Ad, xd, bias=bd)
    yt = ops.srgnn_prop(Ad, xd, transpose=True)
    x64 = x.astype(np.float64)
    ref = np.concatenate([A[:, :, :L] @ x64[..., :D], A[:, :, L:] @ x64[..., D:]], axis=2) + bias
    reft = np.concatenate([np.transpose(A[:, :, :L], (0, 2, 1)) @ x64[..., :D],
                           np.transpose(A[:, :, L:], (0, 2, 1)) @ x64[..., D:]], axis=2)
    for got, r in ((y, ref), (yt, reft)):
        got = got.view(B, L, 2 * D).cpu().numpy()
        assert np.abs(got - r).max() <= 4e-6 * (np.abs(r).max() + 1.0)
    assert torch.equal(y, ops.srgnn_prop(Ad, xd, bias=bd)) and torch.equal(yt, ops.srgnn_prop(Ad, xd, transpose=True))


def _readout64(Hn, P, alias, mask, w3, dcat):
    B, L = alias.shape
    D = Hn.shape[-1]
    Hn, P = Hn.reshape(B, L, D), P.reshape(B, L, 2 * D)
    bi = np.arange(B)
    last = R.last_index(mask)
    sh = Hn[bi[:, None], alias]
    ht = sh[bi, last]
    q1 = P[bi, alias[bi, last], :D]
    s = 1.0 / (1.0 + np.exp(-(q1[:, None, :] + P[bi[:, None], alias, D:])))
    alpha = s @ w3
    mf = mask.astype(np.float64)
    cat = np.concatenate([(alpha[..., None] * sh * mf[..., None]).sum(1), ht], axis=1)
    da, dht = dcat[:, :D], dcat[:, D:]
    dalpha = mf * (da[:, None, :] * sh).sum(-1)
    dsh = (alpha * mf)[..., None] * da[:, None, :]
    dpre = dalpha[..., None] * w3 * s * (1 - s)
    dP = np.zeros((B, L, 2 * D))
    dH = np.zeros((B, L, D))
    for b in range(B):
        np.add.at(dP[b, :, D:], alias[b], dpre[b])
        dP[b, alias[b, last[b]], :D] += dpre[b].sum(0)
        np.add.at(dH[b], alias[b], dsh[b])
        dH[b, alias[b, last[b]]] += dht[b]
    dw3 = (dalpha[..., None] * s).sum((0, 1))
    return cat, alpha, dP.reshape(B * L, 2 * D), dH.reshape(B * L, D), dw3


@pytest.mark.parametrize("L,D", [(10, 8), (10, 512), (64, 128), (7, 2048)])
def test_readout_forward_and_backward_match_float64(L, D):
    rng = np.random.default_rng(3 * D + L)
    B = 20
    seq = _sessions(rng, B, L, 6)
    seq[1] = 0                                                          # an empty history: ht from the last slot
    _, alias, _ = R.session_graph(seq)
    mask = (seq != 0).astype(np.int64)
    Hn = rng.standard_normal((B * L, D)).astype(np.float32)
    P = rng.standard_normal((B * L, 2 * D)).astype(np.float32)
    w3 = (rng.standard_normal(D) / np.sqrt(D)).astype(np.float32)
    dcat = rng.standard_normal((B, 2 * D)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    sig = torch.empty(B, L, D, device="cuda")
    alpha = torch.empty(B, L, device="cuda")
    al32, md = t(alias.astype(np.int32)), t(mask)
    cat = ops.srgnn_readout_fwd(t(Hn), t(P), al32, md, t(w3), sig=sig, alpha=alpha)
    dP, dH, dw3p = ops.srgnn_readout_bwd(t(dcat), t(Hn), al32, md, t(w3), sig, alpha)
    dw3 = ops.colsum(dw3p)
    rc, ra, rdP, rdH, rdw3 = _readout64(*(a.astype(np.float64) for a in (Hn, P)), alias, mask, w3.astype(np.float64),
                                        dcat.astype(np.float64))
    for got, r in ((cat, rc), (alpha, ra), (dP, rdP), (dH, rdH), (dw3, rdw3)):
        got = got.cpu().numpy().reshape(r.shape)
        assert np.abs(got - r).max() <= 2e-5 * (np.abs(r).max() + 1.0)
    again = ops.srgnn_readout_bwd(t(dcat), t(Hn), al32, md, t(w3), sig, alpha)
    assert all(torch.equal(a, b) for a, b in zip((dP, dH, dw3p), again))


# ------------------------------------------------------------------------------------------------ the model vs the reference
def _grads(m):
    g = {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters() if p.grad is not None and n != "embedding.weight"}
    g["embedding.weight"] = m.sparse_table_grad.to_dense(m.item_num).cpu().numpy()
    return g


@pytest.mark.parametrize("step", [1, 2])
def test_fixture_loss_gradients_and_predict(gold, step):
    p = f"s{step}."
    m = _model(gold, step)
    names = [k[3:] for k in gold.files if k.startswith("sd.")]
    assert list(m.state_dict().keys()) == names                     # the reference's names and order
    loss = m(_batch(gold, 0))
    loss.backward()
    assert abs(float(loss) - float(gold[p + "loss"])) <= 5e-6
    G = _grads(m)
    ref_names = {k[len(p + "grad."):] for k in gold.files if k.startswith(p + "grad.")}
    assert ref_names == set(G) and m.gnn.linear_edge_f.weight.grad is None
    for n in ref_names:
        ref = gold[p + "grad." + n]
        assert np.abs(G[n] - ref).max() <= 2e-6 + 2e-5 * np.abs(ref).max(), n
    m.eval()
    feat = m.compute_item_all()
    scores = m.predict(torch.from_numpy(gold["eval.item_seq"]).cuda(), feat).cpu().numpy()
    assert np.abs(scores - gold[p + "eval.scores"]).max() <= 2e-6 + 2e-5 * np.abs(gold[p + "eval.scores"]).max()


@pytest.mark.parametrize("table_update", ["lazy", "dense"])
@pytest.mark.parametrize("step", [1, 2])
def test_fixture_adamw_trajectory(gold, step, table_update):
    from pixelrec_amd.optim import PxrAdamW

    p = f"s{step}."
    m = _model(gold, step)
    ef0 = m.gnn.linear_edge_f.weight.detach().clone(), m.gnn.linear_edge_f.bias.detach().clone()
    lr, wd = (float(x) for x in gold["lr_wd"])
    opt = PxrAdamW(m, lr=lr, weight_decay=wd, table_update=table_update)
    for s in range(4):
        opt.zero_grad()
        loss = m(_batch(gold, s))
        loss.backward()
        opt.step()
        assert abs(float(loss) - float(gold[p + f"adamw.loss{s}"])) <= 2e-5, s
    sd = m.state_dict()
    for k in sd:
        ref = gold[p + "adamw.final." + k]
        assert np.abs(sd[k].cpu().numpy() - ref).max() <= 5e-5 * max(1.0, np.abs(ref).max()), k
    assert torch.equal(m.gnn.linear_edge_f.weight, ef0[0]) and torch.equal(m.gnn.linear_edge_f.bias, ef0[1])
    tsd = opt.state_dict(layout="torch")                           # no optimizer state for the parameter nothing reads
    assert len(tsd["param_groups"][0]["params"]) == len(list(m.parameters())) and len(tsd["state"]) == len(sd) - 2


def test_graph_replay_is_bit_identical_to_eager_steps(gold):
    from pixelrec_amd.graph import GraphedTrainStep
    from pixelrec_amd.optim import PxrAdamW

    L = int(gold["meta"][2])
    packed = []
    for j in range(4):
        seq, mask, tgt = _batch(gold, j)
        packed.append((seq, torch.cat((mask, tgt), 1)))
    out = {}
    for how in ("eager", "graph"):
        m = _model(gold, 2)
        opt = PxrAdamW(m, lr=1e-2, weight_decay=0.1)
        gs = GraphedTrainStep(m, opt, *packed[0], warmup=0) if how == "graph" else None
        losses = []
        for s in range(4):
            if gs is not None:
                loss = gs(*packed[s])
            else:
                opt.zero_grad()
                loss = m(packed[s])
                loss.backward()
                opt.step()
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        opt.flush()
        out[how] = (torch.stack(losses), m.flat_parameters()[0].clone(), m.embedding.weight.detach().clone(), opt._m.clone(),
                    opt._tm.clone())
        assert m.max_seq_length == L
    for a, b in zip(out["eager"], out["graph"]):
        assert torch.equal(a, b)


def test_fused_topk_equals_predict_mask_topk():
    from pixelrec_amd.model import SRGNN

    rng = np.random.default_rng(11)
    N, D, L, B = 700, 64, 10, 50
    m = SRGNN(_cfg(D, 2, L), type("D", (), {"item_num": N})()).cuda().eval()
    seq = _sessions(rng, B, L, N)
    feat = m.compute_item_all()
    hu = torch.from_numpy(np.repeat(np.arange(B), 4))
    hi = torch.from_numpy(rng.integers(1, N, size=B * 4))
    ptr, hitems = ops.history_csr(hu, hi, B, "cuda")
    sd = torch.from_numpy(seq).cuda()
    _, last = m.encode_last(sd)
    idx, _ = ops.score_topk(last, last.stride(0), B, feat, 10, ptr, hitems)
    scores = m.predict(sd, feat)
    scores[:, 0] = -np.inf
    scores[(hu.cuda(), hi.cuda())] = -np.inf
    assert torch.equal(idx, torch.topk(scores, 10, dim=-1).indices)


def test_bad_ids_raise_index_error(gold):
    m = _model(gold, 1)
    N = m.item_num
    seq, mask, tgt = _batch(gold, 0)
    ops.raise_on_bad_indices()
    bad_seq = seq.clone()
    bad_seq[0, 0] = N
    bad_tgt = tgt.clone()
    bad_tgt[1, 1] = -1
    for batch in ((bad_seq, mask, tgt), (seq, mask, bad_tgt)):
        m(batch).backward()                                        # a training step: the trainer's sync raises
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices()
    m.eval()
    with pytest.raises(IndexError):
        m.predict(bad_seq, m.compute_item_all())
    m.train()
    m((seq, mask, tgt)).backward()
    ops.raise_on_bad_indices()                                     # a clean batch leaves the word clear


def test_main_py_trains_validates_checkpoints_and_tests(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth_dataset

    synth_dataset.main(str(tmp_path / "data"), 2000, 600)
    (tmp_path / "m.yaml").write_text("model: SRGNN\nembedding_size: 64\nstep: 2\n")
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
    assert len(list((tmp_path / "saved").rglob("*.pth"))) >= 1, out[-2000:]
    for metric in ("recall@10", "ndcg@10"):
        mm = re.search(r"test result: .*?'%s', ([0-9.]+)\)" % metric, out)
        assert mm is not None and 0.0 <= float(mm.group(1)) <= 1.0, out[-2000:]
