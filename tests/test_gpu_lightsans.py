"""LightSANs on the gfx950 kernels (csrc/lightsans.hip): the low-rank attention core and the position probabilities, forward and
backward, against float64 and run to run (dropout on and off); the model against the golden fixture of the reference's own
LightSANs (state_dict, loss, every gradient, predict, 4 AdamW steps with the lazy and the dense table schedule) and against the
float64 restatement with dropout on; hipGraph replay against eager steps; the fused top-k; bad ids; main.py end to end."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.dropout_rng import keep_mask
from pixelrec_amd import ops
from tests import lightsans_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lightsans_tiny.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _cfg(D, H, K, L, n_layers, inner=2, p_hidden=0.0, p_attn=0.0, seed=2020):
    return {"n_layers": n_layers, "n_heads": H, "embedding_size": D, "inner_size": inner, "k_interests": K,
            "hidden_dropout_prob": p_hidden, "attn_dropout_prob": p_attn, "hidden_act": "gelu", "layer_norm_eps": 1e-12,
            "initializer_range": 0.02, "MAX_ITEM_LIST_LENGTH": L, "seed": seed}


def _model(gold, n_layers, **kw):
    from pixelrec_amd.model import LightSANs

    item_num, D, H, K, L, _, inner = (int(x) for x in gold["meta"][:7])
    m = LightSANs(_cfg(D, H, K, L, n_layers, inner, **kw), type("D", (), {"item_num": item_num})())
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in R.unpack(gold, "sd", n_layers).items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m.cuda().train()


def _items(gold, j):
    return torch.from_numpy(gold[f"b{j}.items"]).cuda()


def _close(got, ref, rel=2e-5, what=""):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref).max()
    assert err <= rel * (np.abs(ref).max() + 1.0), f"{what}: max error {err:.3e} vs max |ref| {np.abs(ref).max():.3e}"


# ------------------------------------------------------------------------------------------------ kernels vs float64
SHAPES = [(1, 64, 1, 1), (10, 512, 4, 3), (50, 512, 8, 3), (64, 1024, 4, 16)]     # (L, D, H, K)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("L,D,H,K", SHAPES)
def test_core_forward_and_backward_match_float64(L, D, H, K, p):
    rng = np.random.default_rng(L * 1000 + D + K)
    B = 3
    qkv = rng.standard_normal((B, L, 3 * D))
    theta = rng.standard_normal((2, D, K)) * 0.1
    A = torch.softmax(torch.from_numpy(rng.standard_normal((H, L, L))), dim=-2).numpy()
    dctx = rng.standard_normal((B, L, D))
    seed, stream, step = 987654321, 4, 7
    sdv = torch.full((1,), step, dtype=torch.int64, device="cuda")
    keep = torch.from_numpy(keep_mask(seed + step, stream, (B, H, L, K), p)) if p > 0 else None
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    q32, th32, A32 = t(qkv), t(theta), t(A)
    ctx, saved = ops.lightsans_fwd(q32, th32, A32, B, L, H, K, p, seed, stream, step_dev=sdv)
    dqkv, dKVp, dth, dA = ops.lightsans_bwd(t(dctx), q32, th32, A32, saved, B, L, H, K, p, seed, stream, step_dev=sdv)
    X = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (qkv, theta, A)]
    # the float64 reference sees the fp32-rounded operands
    with torch.no_grad():
        for x, a in zip(X, (q32, th32, A32)):
            x.copy_(a.cpu().double())
    ref = R.core(X[0], X[1], X[2], H, K, keep, p)
    ref.backward(torch.from_numpy(np.asarray(dctx, dtype=np.float32)).double())
    _close(ctx.view(B, L, D).cpu().numpy(), ref.detach().numpy(), what="ctx")
    _close(dqkv.view(B, L, 3 * D).cpu().numpy(), X[0].grad.numpy(), what="dqkv")
    _close(ops.colsum(dth).view(2, D, K).cpu().numpy(), X[1].grad.numpy(), what="dtheta")
    _close(ops.colsum(dA).view(H, L, L).cpu().numpy(), X[2].grad.numpy(), what="dA")
    again = ops.lightsans_fwd(q32, th32, A32, B, L, H, K, p, seed, stream, step_dev=sdv)
    assert torch.equal(again[0], ctx) and all(torch.equal(again[1][k], saved[k]) for k in saved)
    again = ops.lightsans_bwd(t(dctx), q32, th32, A32, saved, B, L, H, K, p, seed, stream, step_dev=sdv)
    assert all(torch.equal(a, b) for a, b in zip((dqkv, dKVp, dth, dA), again))


@pytest.mark.parametrize("L,D,H,K", SHAPES)
def test_position_probabilities_match_float64(L, D, H, K):
    rng = np.random.default_rng(L + D)
    pqk = torch.from_numpy(rng.standard_normal((L, 2 * D)).astype(np.float32))
    dA = torch.from_numpy(rng.standard_normal((H, L, L)).astype(np.float32))
    A = ops.lightsans_pos_fwd(pqk.cuda(), H)
    dpqk = ops.lightsans_pos_bwd(pqk.cuda(), A, dA.cuda())
    x = pqk.double().requires_grad_(True)
    ref = R.pos_probs(x, H)
    ref.backward(dA.double())
    _close(A.cpu().numpy(), ref.detach().numpy(), what="A")
    _close(dpqk.cpu().numpy(), x.grad.numpy(), what="dpqk")
    assert torch.equal(ops.lightsans_pos_fwd(pqk.cuda(), H), A)
    assert torch.equal(ops.lightsans_pos_bwd(pqk.cuda(), A, dA.cuda()), dpqk)


def test_kernels_refuse_shapes_beyond_their_limits():
    qkv = torch.zeros(65, 3 * 64, device="cuda")
    for L, D, H, K in ((65, 64, 1, 1), (1, 2048, 4, 3), (1, 96, 16, 3), (1, 64, 1, 17)):
        with pytest.raises(ops._l.PxrError):
            ops.lightsans_fwd(torch.zeros(L, 3 * D, device="cuda"), torch.zeros(2, D, K, device="cuda"),
                              torch.zeros(H, L, L, device="cuda"), 1, L, H, K)
    with pytest.raises(ops._l.PxrError):
        ops.lightsans_pos_fwd(qkv[:, :128].contiguous(), 1)                     # L = 65



def test_backward_entries_refuse_shapes_and_mismatched_buffers():
    from pixelrec_amd import lib

    Lb = lib.load()
    z = torch.zeros(1 << 16, device="cuda")
    p = lambda: lib.ptr(z)
    for L, D, H, K in ((65, 64, 1, 1), (1, 2048, 4, 3), (1, 96, 16, 3), (1, 64, 1, 17), (1, 64, 1, 0)):
        rc = Lb.pxr_lightsans_bwd_f32(p(), p(), p(), p(), p(), p(), p(), 1, L, D, H, K, 0.0, 0, 0, None, p(), p(), p(), p(), None)
        assert rc == -1 and b"pxr_lightsans_bwd_f32" in Lb.pxr_last_error()
    for L, D, H in ((65, 64, 1), (1, 2048, 4), (1, 96, 16)):
        rc = Lb.pxr_lightsans_pos_bwd_f32(p(), p(), p(), L, D, H, p(), None)
        assert rc == -1 and b"pxr_lightsans_pos_bwd_f32" in Lb.pxr_last_error()
    rc = Lb.pxr_lightsans_bwd_f32(p(), p(), p(), p(), None, p(), p(), 1, 10, 64, 1, 3, 0.0, 0, 0, None, p(), p(), p(), p(), None)
    assert rc == -1 and b"null pointer" in Lb.pxr_last_error()
    # the wrapper checks every operand against (B, L, H, K) before the launch
    B, L, D, H, K = 2, 10, 64, 2, 3
    qkv, th, A = torch.zeros(B * L, 3 * D, device="cuda"), torch.zeros(2, D, K, device="cuda"), torch.zeros(H, L, L, device="cuda")
    _, saved = ops.lightsans_fwd(qkv, th, A, B, L, H, K)
    dctx = torch.zeros(B * L, D, device="cuda")
    ops.lightsans_bwd(dctx, qkv, th, A, saved, B, L, H, K)
    for name, bad in (("dctx", dict(dctx=dctx[:-1])), ("theta", dict(theta=th[:1])), ("A", dict(A=A[:1])),
                      ("KVp", dict(saved=dict(saved, KVp=saved["KVp"][:1]))), ("pi", dict(saved=dict(saved, pi=saved["pi"][:1])))):
        args = dict(dctx=dctx, qkv=qkv, theta=th, A=A, saved=saved)
        args.update(bad)
        with pytest.raises(ops._l.PxrError, match=name):
            ops.lightsans_bwd(args["dctx"], args["qkv"], args["theta"], args["A"], args["saved"], B, L, H, K)
    with pytest.raises(ops._l.PxrError, match="pos bwd"):
        ops.lightsans_pos_bwd(torch.zeros(L, 2 * D, device="cuda"), A, A[:1].contiguous())

# ------------------------------------------------------------------------------------------------ the model vs the reference
def _grads(m):
    g = {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters() if n != "item_embedding.weight"}
    g["item_embedding.weight"] = m.sparse_table_grad.to_dense(m.item_num).cpu().numpy()
    return g


@pytest.mark.parametrize("n_layers", [1, 2])
def test_fixture_loss_gradients_and_predict(gold, n_layers):
    p = f"n{n_layers}."
    m = _model(gold, n_layers)
    assert list(m.state_dict().keys()) == [str(k) for k in gold[p + "sd_keys"]]      # the reference's names and order
    loss = m(_items(gold, 0))
    loss.backward()
    assert abs(float(loss.detach()) - float(gold[p + "loss"])) <= 5e-6
    G = _grads(m)
    ref = R.unpack(gold, p + "grad", n_layers)
    assert set(ref) == set(G)
    for n, r in ref.items():
        assert np.abs(G[n] - r).max() <= 2e-6 + 2e-5 * np.abs(r).max(), n
    m.eval()
    scores = m.predict(torch.from_numpy(gold["eval.item_seq"]).cuda(), m.compute_item_all()).cpu().numpy()
    r = gold[p + "eval.scores"]
    assert np.abs(scores - r).max() <= 2e-6 + 2e-5 * np.abs(r).max()


def test_loader_pair_and_bare_rows_give_the_same_loss(gold):
    m = _model(gold, 1)
    items = _items(gold, 0)
    L = m.max_seq_length
    with torch.no_grad():
        a = m(items)
        b = m((items[:, :L].contiguous(), items[:, L:].contiguous()))
    assert torch.equal(a, b)


@pytest.mark.parametrize("table_update", ["lazy", "dense"])
def test_fixture_adamw_trajectory(gold, table_update):
    from pixelrec_amd.optim import PxrAdamW

    m = _model(gold, 2)
    lr, wd = (float(x) for x in gold["lr_wd"])
    opt = PxrAdamW(m, lr=lr, weight_decay=wd, table_update=table_update)
    for s in range(4):
        opt.zero_grad()
        loss = m(_items(gold, s))
        loss.backward()
        opt.step()
        assert abs(float(loss.detach()) - float(gold[f"n2.adamw.loss{s}"])) <= 2e-5, s
    sd = m.state_dict()
    ref = R.unpack(gold, "n2.adamw.final", 2)
    for k in sd:
        assert np.abs(sd[k].cpu().numpy() - ref[k]).max() <= 5e-5 * max(1.0, np.abs(ref[k]).max()), k


def test_training_step_with_dropout_matches_float64(gold):
    """Both dropout sites' masks, fed to the float64 restatement by their stream ids and the completed-step counter."""
    ph, pa = 0.1, 0.2
    m = _model(gold, 2, p_hidden=ph, p_attn=pa, seed=77)
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    item_num, D, H, K, L, B = (int(x) for x in gold["meta"][:6])
    base = (77 * 1000003) & 0xFFFFFFFFFFFFFFFF
    m.set_dropout_step(3)
    loss = m(_items(gold, 1))
    loss.backward()
    drop = R.masks(base + 3, B, L, D, H, K, 2, ph, pa)
    rl, rg = R.forward_backward(sd, gold["b1.items"], 2, H, K, drop=drop, p_hidden=ph, p_attn=pa)
    assert abs(float(loss.detach()) - rl) <= 5e-6
    G = _grads(m)
    for n, r in rg.items():
        assert np.abs(G[n] - r).max() <= 2e-6 + 2e-5 * np.abs(r).max(), n
    assert m.dropout_step() == 4


def test_graph_replay_is_bit_identical_to_eager_steps(gold):
    from pixelrec_amd.graph import GraphedTrainStep
    from pixelrec_amd.optim import PxrAdamW

    L = int(gold["meta"][4])
    pairs = [(_items(gold, j)[:, :L].contiguous(), _items(gold, j)[:, L:].contiguous()) for j in range(4)]
    out = {}
    for how in ("eager", "graph"):
        m = _model(gold, 2, p_hidden=0.1, p_attn=0.1)
        opt = PxrAdamW(m, lr=1e-2, weight_decay=0.1)
        gs = GraphedTrainStep(m, opt, *pairs[0], warmup=0) if how == "graph" else None
        losses = []
        for s in range(4):
            if gs is not None:
                loss = gs(*pairs[s])
            else:
                opt.zero_grad()
                loss = m(pairs[s])
                loss.backward()
                opt.step()
            losses.append(loss.detach().clone().reshape(()))
        torch.cuda.synchronize()
        opt.flush()
        out[how] = (torch.stack(losses), m.flat_parameters()[0].clone(), m.item_embedding.weight.detach().clone(), opt._m.clone(),
                    opt._tm.clone())
    assert len(set(float(x) for x in out["eager"][0])) == 4
    for a, b in zip(out["eager"], out["graph"]):
        assert torch.equal(a, b)


def test_fused_topk_equals_predict_mask_topk():
    from pixelrec_amd.model import LightSANs

    rng = np.random.default_rng(11)
    N, D, H, K, L, B = 700, 64, 2, 3, 10, 50
    m = LightSANs(_cfg(D, H, K, L, 2), type("D", (), {"item_num": N})()).cuda().eval()
    seq = rng.integers(1, N, size=(B, L))
    seq[:, :3] = np.where(rng.random((B, 3)) < 0.5, 0, seq[:, :3])        # some left padding
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
    items = _items(gold, 0)
    ops.raise_on_bad_indices()
    for col, val in ((0, N), (-2, -1), (-1, N + 5)):
        bad = items.clone()
        bad[1, col] = val
        m(bad).backward()                                          # a training step: the trainer's sync raises
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices()
    m.eval()
    bad = items[:, :-2].clone()
    bad[0, 3] = N
    with pytest.raises(IndexError):
        m.predict(bad, m.compute_item_all())
    m.train()
    m(items).backward()
    ops.raise_on_bad_indices()                                     # a clean batch leaves the word clear


def test_main_py_trains_validates_checkpoints_and_tests(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth_dataset

    synth_dataset.main(str(tmp_path / "data"), 2000, 600)
    (tmp_path / "m.yaml").write_text("model: LightSANs\nn_layers: 1\nn_heads: 4\nembedding_size: 64\ninner_size: 2\nk_interests: 3\n"
                                     "hidden_dropout_prob: 0.1\nattn_dropout_prob: 0.1\nhidden_act: 'gelu'\nlayer_norm_eps: 1e-12\n"
                                     "initializer_range: 0.02\n")
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
