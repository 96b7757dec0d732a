"""BERT4Rec on the GPU (pixelrec_amd/model/bert4rec.py): loss, gradients, the sparse table gradient, a 4-step AdamW trajectory and
predict against the golden vectors of the reference's own BERT4Rec (tests/golden/bert4rec_tiny.npz) and the test-side restatement
(tests/bert4rec_restate.py), in each GEMM mode (h2 default, PXR_SEQ_H2=0, PXR_GEMM_MODE f32) with the fused and the unfused loss
head; the fused evaluation against the literal GEMM -> mask -> top-k path; a captured step against eager steps; main.py end to end.
Tolerances are test_gpu_sasrec.py's."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import sasrec_oracle as O
from tests import bert4rec_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bert4rec_tiny.npz")
MODES = [(m, f) for m in ("h2", "planes", "f32") for f in (True, False)]


@pytest.fixture
def mode(request):
    """(GEMM mode, fused head): set like tests/conftest.py's pxr_mode, plus PXR_FUSED_HEAD."""
    from pixelrec_amd import ops

    gemm, fused = request.param
    keys = ("PXR_PLANES", "PXR_SEQ_H2", "PXR_FUSED_HEAD")
    prev_env = {k: os.environ.get(k) for k in keys}
    prev = ops.set_gemm_mode("f32" if gemm == "f32" else "bf16x3")
    os.environ["PXR_PLANES"] = "1"
    os.environ["PXR_SEQ_H2"] = "1" if gemm == "h2" else "0"
    os.environ["PXR_FUSED_HEAD"] = "1" if fused else "0"
    try:
        yield request.param
    finally:
        ops.set_gemm_mode(prev)
        for k, v in prev_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _golden():
    z = np.load(GOLDEN, allow_pickle=False)
    meta = dict(zip(("item_num", "D", "L", "H", "inner", "n_layers", "B", "seed"), [int(x) for x in z["meta"]]))
    return meta, z


def _model(meta, z, p_drop=0.0):
    from pixelrec_amd.model import BERT4Rec

    cfg = {"n_layers": meta["n_layers"], "n_heads": meta["H"], "embedding_size": meta["D"], "inner_size": meta["inner"],
           "hidden_dropout_prob": p_drop, "attn_dropout_prob": p_drop, "hidden_act": "gelu", "layer_norm_eps": 1e-12,
           "initializer_range": 0.02, "MAX_ITEM_LIST_LENGTH": meta["L"], "mask_ratio": 0.4, "seed": 2020}

    class DL:
        item_num = meta["item_num"]

    m = BERT4Rec(cfg, DL())
    p = R.golden_params(z)
    m.load_state_dict(p, strict=True)
    return m.cuda(), p


def _cfg(meta):
    return {"n_layers": meta["n_layers"], "n_heads": meta["H"], "layer_norm_eps": 1e-12}


@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_loss_gradients_and_sparse_table_gradient(mode):
    meta, z = _golden()
    m, p = _model(meta, z)
    m.train()
    items, mask = torch.from_numpy(z["items"]), torch.from_numpy(z["masked_index"])
    loss = m((items.cuda(), mask.cuda()))
    loss.backward()
    loss = loss.detach()
    ref_loss, g = R.loss_and_grads(p, items, mask, _cfg(meta))
    assert abs(float(loss) - float(z["loss"])) <= 2e-5 * max(1.0, abs(float(z["loss"])))
    assert abs(float(loss) - float(ref_loss)) <= 2e-5 * max(1.0, abs(float(ref_loss)))
    n_table = meta["item_num"] + 1
    for k, v in m.named_parameters():
        ref = torch.from_numpy(z["grad." + k])
        if k == "item_embedding.weight":
            sp = m.sparse_table_grad
            dense = sp.to_dense(n_table).cpu()
            n = sp.count()
            idx = sp.idx[:n].cpu().numpy()
            assert np.all(np.diff(idx) > 0) and (idx != 0).all() and meta["item_num"] in idx   # the mask token is an ordinary row
            assert dense[0].abs().max().item() == 0.0
            for r in (ref, g[k]):
                err = (dense - r).abs().max().item()
                assert err <= 3e-6 + 1e-4 * r.abs().max().item(), f"table grad err {err}"
        else:
            got = v.grad.detach().cpu()
            for r in (ref, g[k]):
                err = (got - r).abs().max().item()
                assert err <= 5e-6 + 2e-4 * r.abs().max().item(), f"{k}: err {err}"


@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_adamw_four_steps(mode):
    from pixelrec_amd.optim import PxrAdamW

    meta, z = _golden()
    m, p = _model(meta, z)
    m.train()
    opt = PxrAdamW(m, lr=1e-4, weight_decay=0.1)
    batches = [(torch.from_numpy(i), torch.from_numpy(k)) for i, k in zip(z["adamw.items"], z["adamw.masks"])]
    losses_r, final_r = R.adamw_trajectory(p, batches, _cfg(meta))
    for s, (it, mk) in enumerate(batches):
        loss = m((it.cuda(), mk.cuda()))
        loss.backward()
        opt.step()
        loss = loss.detach()
        assert abs(float(loss) - float(z[f"adamw.loss{s}"])) <= 3e-5 * max(1.0, abs(float(loss)))
        assert abs(float(loss) - losses_r[s]) <= 3e-5 * max(1.0, abs(float(loss)))
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    for k, v in sd.items():
        assert (v - torch.from_numpy(z["adamw.final." + k])).abs().max().item() <= 1e-5, k
        assert (v - final_r[k]).abs().max().item() <= 1e-5, k


@pytest.mark.parametrize("mode", MODES[::2], indirect=True)
def test_predict_scores_and_top10(mode):
    meta, z = _golden()
    m, p = _model(meta, z)
    m.eval()
    seq = torch.from_numpy(z["eval.item_seq"])
    feat = m.compute_item_all()
    assert feat.shape[0] == meta["item_num"]
    scores = m.predict(seq.cuda(), feat).cpu()
    ref = R.predict(p, seq, p["item_embedding.weight"][:meta["item_num"]], _cfg(meta), meta["item_num"])
    for r in (torch.from_numpy(z["eval.scores"]), ref):
        assert (scores - r).abs().max().item() <= 1e-4
    masked = O.full_sort_scores(scores)
    _, idx = torch.topk(masked, 10, dim=-1)
    _, idx_ref = torch.topk(O.full_sort_scores(torch.from_numpy(z["eval.scores"])), 10, dim=-1)
    assert torch.equal(idx, idx_ref)


@pytest.mark.parametrize("mode", MODES[::2], indirect=True)
def test_fused_evaluation_equals_the_literal_path(mode):
    """Recall@10 / NDCG@10 from the fused scoring (ops.score_topk on the encoder's last position, row stride (L+1) D -- what
    Trainer._full_sort_batch_topk runs) equal the literal predict -> history mask -> top-k path."""
    from pixelrec_amd import ops, synth

    meta, z = _golden()
    m, p = _model(meta, z)
    m.eval()
    N, L, B = meta["item_num"], meta["L"], 24
    rng = np.random.default_rng(5)
    item_seq, hu, hi, pos_i = synth.eval_batch(N, B, L, rng, synth.ZipfItems(N, seed=3), hist_lo=2, hist_hi=2 * L)
    seq = torch.from_numpy(item_seq).cuda()
    feat = m.compute_item_all()
    out, last = m.encode_last(seq)
    assert out.shape == (B, L + 1, meta["D"]) and last.stride(0) == (L + 1) * meta["D"]
    ptr, hist = ops.history_csr(torch.from_numpy(hu), torch.from_numpy(hi), B, "cuda")
    idx, _ = ops.score_topk(last, last.stride(0), B, feat.detach(), 10, ptr, hist)
    scores = m.predict(seq, feat).cpu()
    masked = O.full_sort_scores(scores, torch.from_numpy(hu), torch.from_numpy(hi))
    rec_lit, idx_lit = O.topk_hits(masked, torch.arange(B), torch.from_numpy(pos_i), 10)
    assert torch.equal(idx.cpu(), idx_lit)
    pos_matrix = torch.zeros(B, N, dtype=torch.int)
    pos_matrix[torch.arange(B), torch.from_numpy(pos_i)] = 1
    rec_fused = torch.cat((torch.gather(pos_matrix, 1, idx.cpu()), pos_matrix.sum(1, keepdim=True)), dim=1)
    a, b = O.recall_ndcg(rec_fused.numpy(), [10]), O.recall_ndcg(rec_lit.numpy(), [10])
    assert a == b


def test_captured_step_replays_the_eager_loss():
    from pixelrec_amd.graph import GraphedTrainStep
    from pixelrec_amd.optim import PxrAdamW
    from pixelrec_amd.parallel import DataParallel

    meta, z = _golden()
    batches = [(torch.from_numpy(i).cuda(), torch.from_numpy(k).cuda()) for i, k in zip(z["adamw.items"], z["adamw.masks"])] * 3
    out = {}
    for how in ("graph", "eager"):
        m, _ = _model(meta, z)
        m.train()
        opt = PxrAdamW(m, lr=1e-4, weight_decay=0.1)
        if how == "graph":
            g = GraphedTrainStep(DataParallel(m), opt, *batches[0], warmup=0)   # sizes its buffers on a snapshot: no step consumed
            losses = [float(g(*b)) for b in batches]
        else:
            losses = []
            for b in batches:
                loss = m(b)
                loss.backward()
                opt.step()
                losses.append(float(loss.detach()))
        opt.flush()
        out[how] = losses
    for a, b in zip(out["graph"], out["eager"]):
        assert abs(a - b) <= 2e-5 * max(1.0, abs(b)), (out["graph"], out["eager"])


def test_main_py_trains_validates_checkpoints_and_tests(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth_dataset

    synth_dataset.main(str(tmp_path / "data"), 3000, 800)
    (tmp_path / "m.yaml").write_text("model: BERT4Rec\nn_layers: 2\nn_heads: 2\nembedding_size: 64\ninner_size: 1\n"
                                     "hidden_dropout_prob: 0.1\nattn_dropout_prob: 0.1\nhidden_act: 'gelu'\nlayer_norm_eps: 1e-12\n"
                                     "initializer_range: 0.02\nmask_ratio: 0.6\n")
    (tmp_path / "o.yaml").write_text(f"seed: 2020\nstate: INFO\nuse_modality: False\nreproducibility: True\n"
                                     f"checkpoint_dir: '{tmp_path}/saved'\nlog_path: '{tmp_path}/log'\nshow_progress: False\n"
                                     f"MAX_ITEM_LIST_LENGTH: 10\ndata_path: {tmp_path}/data/\ndataset: Pixel200K\nepochs: 3\n"
                                     "train_batch_size: 64\noptim_args: {learning_rate: 0.001, weight_decay: 0.1}\n"
                                     "eval_batch_size: 512\ntopk: [5,10]\nmetrics: ['Recall', 'NDCG']\nvalid_metric: NDCG@10\n"
                                     "metric_decimal_place: 7\neval_step: 1\nstopping_step: 30\n")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "OMP_NUM_THREADS")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--device", "0", "--config_file", str(tmp_path / "m.yaml"),
                        str(tmp_path / "o.yaml")], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert len(re.findall(r"epoch \d+ training \[time", out)) == 3 and len(re.findall(r"epoch \d+ evaluating \[time", out)) == 3, out[-3000:]
    m = re.search(r"test result: .*?'ndcg@10', ([0-9.]+)\)", out)
    assert m is not None and 0.0 <= float(m.group(1)) <= 1.0, out[-2000:]
    assert len([f for f in os.listdir(tmp_path / "saved") if f.endswith(".pth")]) == 1
