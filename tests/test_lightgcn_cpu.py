"""LightGCN host side (no GPU): the CSR of the normalised graph against the reference's own edge_index / edge_weight, the pair
data path (PAIR build, PairTrainBatcher, PairEvalBatcher), and a float64 restatement against the golden fixture made by the
reference's LightGCN (tools/make_golden_lightgcn.py)."""
import os

import numpy as np
import pytest

from pixelrec_amd.data.dataload import Data, norm_adj_csr
from pixelrec_amd.data.dataset import PairEvalBatcher, PairTrainBatcher
from pixelrec_amd.utils.enum_type import InputType
from tests import lightgcn_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lightgcn_tiny.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _fixture_csr(g):
    U, I = int(g["meta"][0]), int(g["meta"][1])
    return U, I, norm_adj_csr(g["train_u"], g["train_i"], U, I)


def test_csr_equals_reference_edges_as_a_multiset(gold):
    U, I, (row_ptr, col, w) = _fixture_csr(gold)
    assert row_ptr.dtype == np.int64 and col.dtype == np.int32 and w.dtype == np.float32
    src = np.repeat(np.arange(U + I), np.diff(row_ptr))
    ours = sorted(zip(src.tolist(), col.tolist(), w.view(np.int32).tolist()))
    ei, ew = gold["edge_index"], gold["edge_weight"].astype(np.float32)
    ref = sorted(zip(ei[0].tolist(), ei[1].tolist(), ew.view(np.int32).tolist()))
    assert ours == ref                                     # same edges, same fp32 weights bit for bit
    deg = np.diff(row_ptr)
    assert deg[0] == 0 and deg[U] == 0                     # the [PAD] user and item have no edge (weight of degree 0 = 1)
    assert len(col) == 2 * len(gold["train_u"])            # both directions, duplicates kept


def _restate_case(g, K):
    U, I, csr = _fixture_csr(g)
    A = R.csr_matrix(*csr)
    e0 = np.concatenate([g["sd.user_embedding.weight"], g["sd.item_embedding.weight"]]).astype(np.float64)
    return U, A, e0


@pytest.mark.parametrize("K", [1, 3])
def test_float64_restatement_matches_the_golden_fixture(gold, K):
    p = f"k{K}."
    U, A, e0 = _restate_case(gold, K)
    users, items = gold["users"], gold["items"]
    loss, g0 = R.loss_and_grad(A, e0, K, U, users[0], items[0])
    assert abs(loss - float(gold[p + "loss"])) <= 2e-6 * max(1.0, abs(loss))
    ref_g = np.concatenate([gold[p + "grad.user_embedding.weight"], gold[p + "grad.item_embedding.weight"]])
    assert np.abs(g0 - ref_g).max() <= 1e-6 * max(1.0, np.abs(ref_g).max())
    # predict scores (the fixture's eval users include user 0 and the edge-less user 6)
    ef = R.propagate(A, e0, K)
    scores = ef[:U][gold["eval.users"]] @ ef[U:].T
    assert np.abs(scores - gold[p + "eval.scores"]).max() <= 1e-5
    # 4 AdamW steps
    lr, wd = (float(x) for x in gold["lr_wd"])
    opt, e = R.AdamW(lr, wd), e0
    for s in range(4):
        l, g_ = R.loss_and_grad(A, e, K, U, users[s], items[s])
        assert abs(l - float(gold[p + f"adamw.loss{s}"])) <= 2e-6 * max(1.0, abs(l)), s
        e = opt.step(e, g_)
    ref_e = np.concatenate([gold[p + "adamw.final.user_embedding.weight"], gold[p + "adamw.final.item_embedding.weight"]])
    assert np.abs(e - ref_e).max() <= 2e-6


# ---- data path -------------------------------------------------------------------------------------------------------------------
def _tiny_data(tmp_path, n_users=40, n_items=30, seed=3):
    rng = np.random.default_rng(seed)
    rows = []
    t = 0
    for u in range(n_users):
        for _ in range(int(rng.integers(3, 12))):   # the PixelRec data keeps users of >= 5 interactions
            rows.append((f"i{int(rng.integers(0, n_items))}", f"u{u}", t))    # repeats of an item happen
            t += int(rng.integers(1, 4))
    order = rng.permutation(len(rows))
    path = tmp_path / "tiny.csv"
    with open(path, "w") as f:
        f.write("item_id,user_id,timestamp\n")
        for k in order:
            f.write("%s,%s,%d\n" % rows[k])
    cfg = {"data_path": str(tmp_path), "dataset": "tiny", "MODEL_INPUT_TYPE": InputType.PAIR, "train_batch_size": 16, "seed": 7,
           "eval_batch_size": 9, "MAX_ITEM_LIST_LENGTH": 10}
    d = Data(cfg)
    d.build()
    return cfg, d


def test_pair_build_keeps_all_but_the_last_two_of_each_user(tmp_path):
    _, d = _tiny_data(tmp_path)
    want = [(u, int(i)) for u, s in d.user_seq.items() for i in s[:-2]]
    got = list(zip(d.train_feat["user_id"].tolist(), d.train_feat["item_id"].tolist()))
    assert got == want                                     # reference order: users by first appearance, time order inside


def test_pair_batcher_negatives_epoch_coverage_and_rank_split(tmp_path):
    cfg, d = _tiny_data(tmp_path)
    hist = {u: set(int(i) for i in s[:-2]) for u, s in d.user_seq.items()}
    b = PairTrainBatcher(cfg, d)
    for epoch in (0, 1):
        b.set_epoch(epoch)
        seen = []
        for user, item in b:
            assert user.dtype.is_floating_point is False and item.shape == (user.shape[0], 2)
            for u, (pos, neg) in zip(user.tolist(), item.tolist()):
                assert 1 <= neg < d.item_num and neg not in hist[u]
                assert pos in hist[u]
                seen.append((u, pos))
        want = list(zip(d.train_feat["user_id"].tolist(), d.train_feat["item_id"].tolist()))
        assert sorted(seen) == sorted(want)                # every interaction exactly once per epoch
    n = len(d.train_feat["user_id"])
    for world in (2, 3, 4):
        parts = [PairTrainBatcher(cfg, d, rank=r, world=world)._indices() for r in range(world)]
        allidx = np.concatenate(parts)
        assert set(allidx.tolist()) == set(range(n))       # covering
        assert len(allidx) - n < world                     # disjoint up to DistributedSampler's wrap-around padding
        if n % world == 0:
            assert len(allidx) == n


def test_pair_eval_batcher_hands_over_user_ids(tmp_path):
    cfg, d = _tiny_data(tmp_path)
    uids = list(d.user_seq.keys())
    for phase, cut in (("valid", 2), ("test", 1)):
        ev = PairEvalBatcher(cfg, d, phase=phase)
        k = 0
        for user, (hu, hi), pos_u, target in ev:
            for j, u in enumerate(user.tolist()):
                assert u == uids[k]
                s = d.user_seq[u]
                assert int(target[j]) == int(s[-cut])
                assert sorted(hi[hu == j].tolist()) == sorted(int(x) for x in s[:-cut])
                k += 1
        assert k == len(uids)


def test_lightgcn_is_registered_for_the_pair_path():
    from pixelrec_amd.data.utils import SUPPORTED
    from pixelrec_amd.utils import get_model

    assert SUPPORTED["LightGCN"] == "PAIR"
    assert get_model("LightGCN").input_type == InputType.PAIR
