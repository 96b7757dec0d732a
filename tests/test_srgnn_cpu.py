"""SRGNN host side (no GPU): the AUGSEQ build against the reference's _build_aug_seq, GraphTrainBatcher / GraphEvalBatcher, and a
float64 restatement (tests/srgnn_restate.py) against the golden fixture made by the reference's SRGNN and collates
(tools/make_golden_srgnn.py), against finite differences, and at a padded node count."""
import os

import numpy as np
import pytest

from pixelrec_amd.data.dataload import Data
from pixelrec_amd.data.dataset import GraphEvalBatcher, GraphTrainBatcher
from pixelrec_amd.data.utils import SUPPORTED
from pixelrec_amd.model import SRGNN
from pixelrec_amd.utils.enum_type import InputType
from tests import srgnn_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "srgnn_tiny.npz")
GDIR = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _data(L, batch=16, eval_batch=7):
    cfg = {"data_path": GDIR, "dataset": "TinyInter", "MAX_ITEM_LIST_LENGTH": L, "MODEL_INPUT_TYPE": InputType.AUGSEQ,
           "train_batch_size": batch, "eval_batch_size": eval_batch, "seed": 5}
    d = Data(cfg)
    d.build()
    return cfg, d


def _params(g, prefix="sd."):
    return {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}


def test_registered_as_augseq():
    assert SUPPORTED["SRGNN"] == "AUGSEQ" and SRGNN.input_type == InputType.AUGSEQ


def test_augseq_samples_equal_the_reference(gold):
    L = int(gold["aug.L"])
    _, d = _data(L)
    seqs = d.aug_item_seqs()
    lens = np.array([len(s) for s in seqs])
    assert np.array_equal(lens, gold["aug.lens"])
    assert np.array_equal(np.concatenate(seqs), gold["aug.flat"])
    assert np.array_equal(d.train_feat["user_id"], gold["aug.user_id"])
    assert lens.min() >= 2 and lens.max() <= L + 1


def test_train_batcher_padding_mask_and_negatives(gold):
    L = int(gold["aug.L"])
    cfg, d = _data(L)
    bt = GraphTrainBatcher(cfg, d)
    seqs = d.aug_item_seqs()
    idx = bt._indices()
    assert sorted(idx.tolist()) == list(range(len(seqs)))
    n_seen = 0
    for b, (item_seq, mask, target) in enumerate(bt):
        item_seq, mask, target = item_seq.numpy(), mask.numpy(), target.numpy()
        assert item_seq.dtype == mask.dtype == target.dtype == np.int64
        assert item_seq.shape[1] == L and mask.shape == item_seq.shape and target.shape == (len(item_seq), 2)
        for r in range(len(item_seq)):
            s = seqs[idx[n_seen + r]]
            k = len(s) - 1
            assert np.array_equal(item_seq[r, :k], s[:-1]) and not item_seq[r, k:].any()     # right-padded
            assert mask[r, :k].all() and not mask[r, k:].any()
            assert target[r, 0] == s[-1]
            assert 1 <= target[r, 1] < d.item_num and target[r, 1] not in s                  # never in its prefix
        n_seen += len(item_seq)
    assert n_seen == len(seqs)


def test_train_batcher_order_is_the_distributed_samplers(gold):
    cfg, d = _data(int(gold["aug.L"]))
    a = GraphTrainBatcher(cfg, d, rank=0, world=2)
    b = GraphTrainBatcher(cfg, d, rank=1, world=2)
    ia, ib = a._indices(), b._indices()
    assert len(ia) == len(ib) == -(-len(d.aug_item_seqs()) // 2)
    assert set(ia.tolist()) | set(ib.tolist()) == set(range(len(d.aug_item_seqs())))


@pytest.mark.parametrize("phase", ["valid", "test"])
def test_eval_batches_are_right_padded_with_full_history(phase):
    L = 4
    cfg, d = _data(L)
    ev = GraphEvalBatcher(cfg, d, phase=phase)
    seqs = list(d.user_seq.values())
    cut = 2 if phase == "valid" else 1
    u0 = 0
    for item_seq, (hu, hi), pos_u, target in ev:
        item_seq, hu, hi, target = item_seq.numpy(), hu.numpy(), hi.numpy(), target.numpy()
        for r in range(len(item_seq)):
            s = seqs[u0 + r]
            hist = s[:-cut]
            tail = hist[-L:]
            assert np.array_equal(item_seq[r, :len(tail)], tail) and not item_seq[r, len(tail):].any()
            assert np.array_equal(hi[hu == r], hist)                                         # the whole history is masked
            assert target[r] == s[-cut]
        assert np.array_equal(pos_u.numpy(), np.arange(len(item_seq)))
        u0 += len(item_seq)
    assert u0 == len(seqs)


def test_graph_restatement_equals_the_collate(gold):
    seq = gold["b0.item_seq"]
    n = gold["collate.items"].shape[1]
    nodes, alias, A = R.session_graph(seq, n)
    assert np.array_equal(nodes, gold["collate.items"])
    assert np.array_equal(alias, gold["collate.alias"])
    assert np.array_equal(A.astype(np.float32), gold["collate.A"])
    # 1/k in float64 then fp32 is the fp32 quotient: the device's fp32 division lands on the same bits
    k = np.arange(1, 65)
    assert np.array_equal((1.0 / k).astype(np.float32), np.float32(1.0) / k.astype(np.float32))


@pytest.mark.parametrize("step", [1, 2])
def test_restatement_matches_the_golden_fixture(gold, step):
    p = f"s{step}."
    P = _params(gold)
    loss, G, _ = R.forward_backward(P, gold["b0.item_seq"], gold["b0.mask"], gold["b0.target"], step)
    assert abs(loss - float(gold[p + "loss"])) <= 2e-6 * max(1.0, abs(loss))
    names = [k[len(p + "grad."):] for k in gold.files if k.startswith(p + "grad.")]
    assert set(names) == set(G) and not any(n.startswith("gnn.linear_edge_f") for n in names)
    for n in names:
        ref = gold[p + "grad." + n]
        assert np.abs(G[n] - ref).max() <= 1e-6 + 1e-5 * np.abs(ref).max(), n
    scores = R.predict(P, gold["eval.item_seq"], step)
    assert np.abs(scores - gold[p + "eval.scores"]).max() <= 1e-5


def test_padding_the_graph_to_L_nodes_changes_nothing(gold):
    P = _params(gold)
    seq, mask, target = gold["b0.item_seq"], gold["b0.mask"], gold["b0.target"]
    n_min = max(len(np.unique(s)) for s in seq)
    l0, g0, e0 = R.forward_backward(P, seq, mask, target, 2, n_nodes=n_min)
    l1, g1, e1 = R.forward_backward(P, seq, mask, target, 2, n_nodes=seq.shape[1])
    l2, g2, _ = R.forward_backward(P, seq, mask, target, 2, n_nodes=seq.shape[1] + 3)
    assert abs(l0 - l1) <= 1e-14 and abs(l0 - l2) <= 1e-14
    for n in g0:
        assert np.abs(g0[n] - g1[n]).max() <= 1e-13 and np.abs(g0[n] - g2[n]).max() <= 1e-13, n
    assert np.abs(e0["out"] - e1["out"]).max() <= 1e-14


def test_restatement_gradients_match_finite_differences():
    rng = np.random.default_rng(3)
    D, N, L = 4, 9, 4
    shapes = {"embedding.weight": (N, D), "gnn.w_ih": (3 * D, 2 * D), "gnn.w_hh": (3 * D, D), "gnn.b_ih": (3 * D,),
              "gnn.b_hh": (3 * D,), "gnn.b_iah": (D,), "gnn.b_oah": (D,), "gnn.linear_edge_in.weight": (D, D),
              "gnn.linear_edge_in.bias": (D,), "gnn.linear_edge_out.weight": (D, D), "gnn.linear_edge_out.bias": (D,),
              "gnn.linear_edge_f.weight": (D, D), "gnn.linear_edge_f.bias": (D,), "linear_one.weight": (D, D),
              "linear_one.bias": (D,), "linear_two.weight": (D, D), "linear_two.bias": (D,), "linear_three.weight": (1, D),
              "linear_transform.weight": (D, 2 * D), "linear_transform.bias": (D,)}
    P = {k: rng.uniform(-0.8, 0.8, size=s) for k, s in shapes.items()}
    seq = np.array([[1, 2, 1, 3], [4, 4, 5, 0], [6, 0, 0, 0]])
    mask = (seq != 0).astype(np.int64)
    target = np.array([[7, 8], [2, 1], [8, 3]])
    _, G, _ = R.forward_backward(P, seq, mask, target, 2)
    h = 1e-6
    for name, g in G.items():
        flat = P[name].reshape(-1)
        for i in rng.choice(flat.size, size=min(6, flat.size), replace=False):
            keep = flat[i]
            flat[i] = keep + h
            lp = R.forward_backward(P, seq, mask, target, 2, want_grad=False)[0]
            flat[i] = keep - h
            lm = R.forward_backward(P, seq, mask, target, 2, want_grad=False)[0]
            flat[i] = keep
            fd = (lp - lm) / (2 * h)
            assert abs(fd - g.reshape(-1)[i]) <= 1e-7 + 1e-5 * abs(fd), (name, i, fd, g.reshape(-1)[i])


def test_empty_history_reads_the_last_slot():
    assert R.last_index(np.array([[0, 0, 0], [1, 1, 0], [1, 1, 1]])).tolist() == [2, 1, 2]
