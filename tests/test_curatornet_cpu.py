"""CuratorNet without a GPU: the float64 restatement against the reference's golden fixture (and its two tie rules against
torch.nn.functional), the training batcher, the SEQ registration, the shipped YAML, the state_dict layout, the constructor's
errors, and the two pooling entry points in the built library."""
import os

import numpy as np
import pytest
import torch

from tests import curatornet_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "curatornet_tiny.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_has_the_cases_it_is_meant_to_have(gold):
    item_num, F, E, hidden, L, B = (int(x) for x in gold["meta"][:6])
    assert (item_num, F, E, hidden, L, B) == (9, 12, 8, 2, 4, 6) and gold["rows"].shape == (4, B, L + 2)
    assert list(gold["optim"]) == [1e-4, 0.01]
    for rows in gold["rows"]:
        prof, pos, neg = rows[:, :L], rows[:, L], rows[:, L + 1]
        assert (pos != neg).all() and pos.min() >= 1 and neg.min() >= 1
        pads = sorted(int((p == 0).sum()) for p in prof)
        assert set(pads) == {0, 1, 2, 3, 4}                                       # full ... all padding
        for p in prof:                                                            # left-padded
            real = p != 0
            assert not (real[:-1] & ~real[1:]).any()
        assert any(len(set(p[p != 0].tolist())) < int((p != 0).sum()) for p in prof)     # a repeated item inside a profile
        assert set(pos.tolist()) & set(neg.tolist())                              # one sample's positive is another's negative
    assert (gold["eval.windows"] == 0).all(1).any() and gold["eval.windows"].shape == (8, L)
    assert np.abs(gold["sd.selu_common1.bias"]).max() == 0                         # a padded position's first pre-activation is 0
    assert np.abs(gold["sd.embedding.weight"][0]).max() == 0                       # the reference zero-fills row 0
    assert np.array_equal(gold["sd.embedding.weight"][1:], gold["v_feat"][1:])
    for k in R.NAMES:
        assert (gold["grad." + k] != 0).all(), k


def test_float64_restatement_matches_the_golden_fixture(gold):
    """Tolerances: those of tests/test_vbpr_cpu.py for its restatement against its fixture."""
    P = R.state_from(gold, "sd.")
    L = int(gold["meta"][4])
    rows = gold["rows"]
    loss, grads = R.loss_and_grads(P, rows[0][:, :L], rows[0][:, L:])
    assert abs(loss - float(gold["loss"])) <= 1e-6
    assert set(grads) == set(R.NAMES)
    for k, g in grads.items():
        ref = gold["grad." + k]
        assert np.abs(g.numpy() - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()), k
    feat = R.compute_item_all(P)
    assert np.abs(feat.numpy() - gold["eval.item_all"]).max() <= 1e-5
    scores = R.predict(P, gold["eval.windows"], feat).numpy()
    assert np.abs(scores - gold["eval.scores"]).max() <= 1e-5
    lr, wd = (float(x) for x in gold["optim"])
    losses = R.adamw(P, [(r[:, :L], r[:, L:]) for r in rows], lr, wd)
    for s, val in enumerate(losses):
        assert abs(val - float(gold[f"adamw.loss{s}"])) <= 2e-6, s
    for k, val in P.items():
        ref = gold["adamw.final." + k]
        assert np.abs(val.numpy() - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max()), k
    assert np.array_equal(gold["adamw.final.embedding.weight"], gold["sd.embedding.weight"])       # frozen


def test_restated_tie_rules_are_torchs():
    """Max-pool gradient to the FIRST of equal positions; SELU derivative s * a at exactly 0 -- against torch.nn.functional."""
    g = torch.Generator().manual_seed(0)
    h = torch.randn(3, 5, 8, dtype=torch.float64, generator=g)
    h[:, 3] = h[:, 1]                                                             # duplicated rows: every maximum there ties
    h[1, 0] = h[1, 4] = h[1].max(0).values + 1.0                                  # the maximum of sample 1 at positions 0 and 4
    w = torch.randn(3, 16, dtype=torch.float64, generator=g)
    a = h.clone().requires_grad_(True)
    cat, idx = R.pool(a)
    (cat * w).sum().backward()
    b = h.clone().requires_grad_(True)
    mx, ti = torch.nn.functional.adaptive_max_pool2d(b, (1, 8), return_indices=True)
    av = torch.nn.functional.adaptive_avg_pool2d(b, (1, 8))
    (torch.cat((mx, av), -1).squeeze(1) * w).sum().backward()
    assert torch.equal(idx, ti.squeeze(1) // 8) and (idx[1] == 0).all() and (idx != 3).all()
    assert torch.equal(cat[:, :8], mx.squeeze(1)) and torch.allclose(cat[:, 8:], av.squeeze(1), rtol=0, atol=1e-15)
    assert torch.allclose(a.grad, b.grad, rtol=0, atol=1e-15)
    x = torch.tensor([-30.0, -1.0, -1e-9, 0.0, 1e-9, 2.0, 30.0, -800.0, 800.0], dtype=torch.float64)
    y = x.clone().requires_grad_(True)
    torch.nn.functional.selu(y).sum().backward()
    # (a few float64 roundings: the two sides may order the products differently)
    assert torch.allclose(R.selu(x), torch.nn.functional.selu(x), rtol=1e-14, atol=0)
    assert torch.allclose(R.selu_grad(x), y.grad, rtol=1e-14, atol=0)
    assert float(R.selu_grad(x)[3]) == R.SCALE * R.ALPHA == float(y.grad[3])


# ------------------------------------------------------------------------------------------------------------ batcher
class _Synth:
    """A Data stand-in with SEQ chunks: user_seq (leave-last-two-out applied by the batchers) and train_feat."""

    def __init__(self, L=4, n_users=23, item_num=40, seed=3):
        rng = np.random.default_rng(seed)
        self.item_num, self.user_num = item_num, n_users + 1
        self.user_seq, uid_list, seqs = {}, [], []
        W = L + 1
        for u in range(1, n_users + 1):
            n = int(rng.integers(3, 15))
            s = rng.permutation(np.arange(1, item_num))[:n]
            self.user_seq[u] = s
            hist = s[:-2]
            if len(hist) > W:
                off = len(hist) % W
                for c in range((len(hist) - off) // W):
                    uid_list.append(u); seqs.append(hist[off + c * W: off + (c + 1) * W])
            else:
                uid_list.append(u); seqs.append(hist)
        self.train_feat = {"user_id": np.array(uid_list), "item_seq": seqs}

    def build(self):
        return None


CFG = {"MAX_ITEM_LIST_LENGTH": 4, "train_batch_size": 7, "eval_batch_size": 5, "seed": 11, "device_sampler": None,
       "eval_vectorized": None, "eval_num_workers": 0}


def test_train_batcher_is_one_two_tower_row_per_chunk():
    from pixelrec_amd.data.dataset import CuratorTrainBatcher, SeqTrainBatcher

    data, L = _Synth(), CFG["MAX_ITEM_LIST_LENGTH"]
    seqs = [[int(i) for i in s] for s in data.train_feat["item_seq"]]
    assert any(len(s) == 1 for s in seqs) and any(len(s) == L + 1 for s in seqs)
    lit = sorted((tuple([0] * (L + 1 - len(s)) + s)) for s in seqs)               # the chunk, left-padded: profile | positive
    by_row = {}
    for s in seqs:
        by_row.setdefault(tuple([0] * (L + 1 - len(s)) + s), set()).update(s)
    for epoch in (0, 1):
        b = CuratorTrainBatcher(CFG, data)
        b.set_epoch(epoch)
        assert b.n == len(seqs) and len(b) == -(-len(seqs) // CFG["train_batch_size"])
        got = []
        for prof, target in b:
            assert prof.dtype == target.dtype == torch.int64 and prof.shape[1] == L and target.shape[1] == 2
            for p, (pos, neg) in zip(prof.tolist(), target.tolist()):
                row = tuple(p) + (pos,)
                got.append(row)
                assert 1 <= neg < data.item_num and neg not in by_row[row]
                real = [x != 0 for x in p]
                assert real == sorted(real) and pos != 0                          # left padding; the positive is a real item
        assert sorted(got) == lit                                                 # one sample per chunk, nothing else
        assert any(all(x == 0 for x in r[:L]) for r in got)                       # a one-item chunk: an all-padding profile
        # the order and the rank split are SeqTrainBatcher's for equal seeds
        s = SeqTrainBatcher(CFG, data)
        s.set_epoch(epoch)
        assert np.array_equal(b._indices(), s._indices()) and len(b) == len(s)
        first = b.windows[b._indices()[:CFG["train_batch_size"]]]
        assert np.array_equal(np.asarray(got[:len(first)]), first)
    for r in range(3):
        b, s = CuratorTrainBatcher(CFG, data, rank=r, world=3), SeqTrainBatcher(CFG, data, rank=r, world=3)
        assert np.array_equal(b._indices(), s._indices()) and b.num_samples == s.num_samples
    tiny = _Synth(item_num=40)
    tiny.item_num = 2
    with pytest.raises(ValueError, match="negative"):
        CuratorTrainBatcher(CFG, tiny)


def test_curatornet_is_registered_and_the_yaml_parses():
    from pixelrec_amd.config.configurator import Config
    from pixelrec_amd.data.dataset import CuratorTrainBatcher, SeqEvalBatcher
    from pixelrec_amd.data.utils import SUPPORTED, bulid_dataloader
    from pixelrec_amd.model import CuratorNet
    from pixelrec_amd.utils.enum_type import InputType
    from pixelrec_amd.utils.utils import get_model

    assert SUPPORTED["CuratorNet"] == "SEQ" and CuratorNet.input_type == InputType.SEQ and get_model("CuratorNet") is CuratorNet
    train, valid, test = bulid_dataloader(dict(CFG, model="CuratorNet"), _Synth())
    assert type(train.batcher) is CuratorTrainBatcher and type(valid) is SeqEvalBatcher and type(test) is SeqEvalBatcher
    c = Config([os.path.join(ROOT, "configs/ViNet/curatornet.yaml")])
    assert c["model"] == "CuratorNet" and c["embedding_size"] == 512 and c["hidden_size"] == 2 and c["seed"] == 2020
    assert c["MAX_ITEM_LIST_LENGTH"] == 10 and c["train_batch_size"] == 512 and c["eval_batch_size"] == 512 and c["epochs"] == 200
    assert dict(c["optim_args"]) == {"learning_rate": 1e-4, "weight_decay": 0.01}
    assert c["v_feat_path"] == "../dataset/visual_features/RN50.npy" and c["dataset"] == "Pixel200K"
    assert list(c["topk"]) == [5, 10] and c["valid_metric"] == "NDCG@10" and c["stopping_step"] == 30
    assert c["MODEL_INPUT_TYPE"] == InputType.SEQ
    head = open(os.path.join(ROOT, "configs/ViNet/curatornet.yaml")).read().split("\nmodel:")[0]
    assert "NO yaml" in head and "does not exist" in head


# ------------------------------------------------------------------------------------------------------------ the model
class _Data:
    item_num = 9


def _feat(tmp_path, shape=(9, 12), name="v.npy"):
    path = str(tmp_path / name)
    np.save(path, np.random.default_rng(1).standard_normal(shape).astype(np.float32))
    return path


def _model(path, E=8, hidden=2, L=4):
    from pixelrec_amd.model import CuratorNet

    return CuratorNet({"embedding_size": E, "hidden_size": hidden, "v_feat_path": path, "MAX_ITEM_LIST_LENGTH": L}, _Data())


def test_state_dict_has_the_reference_keys_in_order_and_loads_the_fixture(gold, tmp_path):
    m = _model(_feat(tmp_path))
    ref = [k[len("sd."):] for k in gold.files if k.startswith("sd.")]
    assert ref == list(R.KEYS) and len(ref) == 11
    assert list(m.state_dict().keys()) == ref and not list(m.named_buffers())
    assert [n for n, p in m.named_parameters() if p.requires_grad] == list(R.NAMES) == list(m.rec_parameter_names())
    assert not m.embedding.weight.requires_grad and m.embedding.weight.data[0].abs().max() == 0       # frozen; row 0 zero-filled
    assert m.hidden_size == 16 and tuple(m.selu_pu1.weight.shape) == (16, 16) and tuple(m.selu_pu3.weight.shape) == (8, 16)
    sd = {k: torch.from_numpy(np.asarray(gold["sd." + k])) for k in ref}
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.embedding.weight.data, sd["embedding.weight"])


def test_init_is_xavier_uniform_with_linear_default_biases(tmp_path):
    torch.manual_seed(0)
    m = _model(_feat(tmp_path, shape=(9, 400)), E=64)
    for lin in R.LINEARS:
        w, b = getattr(m, lin).weight.data, getattr(m, lin).bias.data
        bound = (6.0 / (w.shape[0] + w.shape[1])) ** 0.5
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound, lin
        assert 0 < float(b.abs().max()) <= w.shape[1] ** -0.5, lin


def test_bad_settings_raise_value_errors_that_say_which(tmp_path):
    with pytest.raises(ValueError, match="v2.npy"):
        _model(_feat(tmp_path, shape=(9, 2, 2, 12), name="v2.npy"))               # region features are ACF's
    with pytest.raises(ValueError, match="item_num"):
        _model(_feat(tmp_path, shape=(8, 12)))
    with pytest.raises(ValueError, match="multiple of 4.*10"):
        _model(_feat(tmp_path, shape=(9, 10)))
    with pytest.raises(ValueError, match="embedding_size.*6"):
        _model(_feat(tmp_path), E=6)
    with pytest.raises(ValueError, match="hidden_size.*0"):
        _model(_feat(tmp_path), hidden=0)
    with pytest.raises(ValueError, match="hidden_size.*1.5"):
        _model(_feat(tmp_path), hidden=1.5)
    with pytest.raises(ValueError, match="MAX_ITEM_LIST_LENGTH.*256"):
        _model(_feat(tmp_path), L=256)


def test_forward_on_the_cpu_raises_instead_of_falling_back(gold, tmp_path):
    from pixelrec_amd import ops
    from pixelrec_amd.lib import PxrError

    m = _model(_feat(tmp_path)).train()
    with pytest.raises(PxrError):
        m(torch.from_numpy(gold["rows"][0]))
    with pytest.raises(PxrError):
        m.eval().predict(torch.from_numpy(gold["eval.windows"]), None)
    with pytest.raises(PxrError):
        ops.curator_pool(torch.zeros(6, 8), 2, 3)
    with pytest.raises(PxrError):
        ops.curator_pool_bwd(torch.zeros(2, 16), torch.zeros(2, 8, dtype=torch.uint8), torch.zeros(4, 8), torch.zeros(10, 8), 2, 3)
    assert ops.ACT_CODES["selu"] == 7


def test_the_built_library_exports_the_pooling_entries_and_checks_their_shapes():
    import __graft_entry__ as entry
    from pixelrec_amd import lib

    entry.build()
    L = lib.load()
    assert hasattr(L, "pxr_curator_pool_f32") and hasattr(L, "pxr_curator_pool_bwd_f32") and hasattr(L, "pxr_curator_pair_fwd_f32")
    one = 16                                  # (a non-null, 16-byte aligned address: the checks run before any launch)
    assert L.pxr_curator_pool_f32(one, None, 0, 2, 3, 6, one, one, None) == -1
    assert b"E % 4" in L.pxr_last_error()
    assert L.pxr_curator_pool_f32(one, None, 0, 2, 256, 8, one, one, None) == -1
    assert b"L <= 255" in L.pxr_last_error()
    assert L.pxr_curator_pool_bwd_f32(one, one, one, one, 2, 0, 8, one, None) == -1
    assert L.pxr_linear_fwd_f32(one, one, one, one, one, 2, 4, 4, 8, None) == -1       # act 7 (selu) is the last code
    assert b"bad act" in L.pxr_last_error()
