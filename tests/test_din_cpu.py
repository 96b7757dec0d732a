"""DIN without a GPU: the float64 restatement against the golden fixture of the reference's own DIN, the factorised first Linear
against the literal scoring, the training batcher against SampleTwoTowerTrainDataset's row format and negative-sampling rule, the
state_dict layout, registration and the shipped yaml.  Every test needs pixelrec_amd.model.DIN or its data path."""
import os

import numpy as np
import pytest
import torch

from tests import din_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "din_tiny.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_has_the_cases_it_is_meant_to_have(gold):
    from pixelrec_amd.model import DIN  # noqa: F401  (the fixture belongs to this model)

    I, D, L, B, K = (int(x) for x in gold["meta"][:5])
    assert (I, D, L, B, K) == (13, 8, 4, 6, 10) and [int(x) for x in gold["meta"][6:]] == [12, 4]
    assert gold["rows"].shape == (4, B, L + 2)
    for rows in gold["rows"]:
        prof, pos, neg = rows[:, :L], rows[:, L], rows[:, L + 1]
        assert sorted((prof != 0).sum(1).tolist()) == [0, 1, 2, 3, 4, 4]          # full, 1 / 2 / 3 padded, all padding
        assert all((p[np.argmax(p != 0):] != 0).all() for p in prof if p.any())    # left padding only
        assert any(len(set(p[p != 0])) < (p != 0).sum() for p in prof)              # a repeated item
        assert (pos != neg).all() and (pos > 0).all() and (neg > 0).all()
        assert set(pos.tolist()) & set(neg.tolist())                               # a positive that is another sample's negative
    assert (gold["grad." + R.TABLE][0] == 0).all()
    w = gold["eval.windows"]
    assert w.shape == (8, L) and ((w != 0).sum(1) == 0).sum() == 1
    assert (gold["eval.scores"][(w != 0).sum(1) == 0] == 0).all()                  # all padding: exactly 0 for every item
    assert [str(k) for k in gold["sd.keys"]] == R.names(2)


def test_float64_restatement_matches_the_golden_fixture(gold):
    """The reference ran in float32: its distance from the float64 restatement is float32 rounding (a few 1e-8 on these sizes);
    1e-6 relative is far below any mistake in the arithmetic."""
    from pixelrec_amd.model import DIN  # noqa: F401

    P = R.state_from(gold, "sd.", torch.float64)
    loss, g = R.loss_and_grads(P, gold["rows"][0])
    assert abs(loss - float(gold["loss"])) <= 1e-6
    for k in R.names(2):
        ref = gold["grad." + k]
        assert np.abs(g[k].numpy() - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()), k
    assert float(g[R.TABLE][0].abs().max()) == 0
    s = R.predict_literal(P, gold["eval.windows"])
    assert float((s - torch.from_numpy(gold["eval.scores"]).double()).abs().max()) <= 1e-6
    lr, wd = (float(x) for x in gold["optim"])
    losses = R.adamw(P, list(gold["rows"]), lr, wd)
    for i, v in enumerate(losses):
        assert abs(v - float(gold[f"adamw.loss{i}"])) <= 1e-6
    for k in R.names(2):
        ref = gold["adamw.final." + k]
        assert np.abs(P[k].numpy() - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()), k
    # row 0 is decayed though it never gets a gradient: 4 steps of p <- p (1 - lr wd)
    r0 = torch.from_numpy(gold["sd." + R.TABLE][0]).double() * (1 - lr * wd) ** 4
    assert float((P[R.TABLE][0] - r0).abs().max()) <= 1e-12


@pytest.mark.parametrize("hidden", [[16], [12, 4], [80, 40]])
def test_factorised_scoring_equals_literal_scoring_in_float64(hidden):
    from pixelrec_amd.model import DIN  # noqa: F401

    rng = np.random.default_rng(5)
    N, D, L = 37, 8, 5
    g = torch.Generator().manual_seed(3)
    P = {}
    sizes = [4 * D] + hidden
    for i, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        P[f"attention.att_mlp_layers.mlp_layers.{3 * i + 1}.weight"] = torch.randn(b, a, generator=g, dtype=torch.float64) * 0.3
        P[f"attention.att_mlp_layers.mlp_layers.{3 * i + 1}.bias"] = torch.randn(b, generator=g, dtype=torch.float64) * 0.1
    P["attention.dense.weight"] = torch.randn(1, sizes[-1], generator=g, dtype=torch.float64)
    P["attention.dense.bias"] = torch.randn(1, generator=g, dtype=torch.float64)
    P[R.TABLE] = torch.randn(N, D, generator=g, dtype=torch.float64)
    win = rng.integers(1, N, size=(6, L))
    win[0, :] = 0
    win[1, :3] = 0
    lit, fac = R.predict_literal(P, win), R.predict_factorised(P, win)
    assert float((lit - fac).abs().max()) <= 1e-13 * max(1.0, float(lit.abs().max()))
    assert float(lit[0].abs().max()) == 0 == float(fac[0].abs().max())


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


def test_train_batcher_yields_sample_two_tower_rows():
    """SampleTwoTowerTrainDataset.__getitem__ (trainset.py:324-332): for every position idx of a chunk, the chunk without that item,
    then the item, then a negative outside the chunk, left-padded to L + 2."""
    from pixelrec_amd.data.dataset import DinTrainBatcher, SampleAcfTrainBatcher

    data, L = _Synth(), CFG["MAX_ITEM_LIST_LENGTH"]
    seqs = [[int(i) for i in s] for s in data.train_feat["item_seq"]]
    lit, chunk_of = [], {}
    for s in seqs:
        for idx, item in enumerate(s):
            row = s[:idx] + s[idx + 1:] + [item]
            row = tuple([0] * (L + 1 - len(row)) + row)
            lit.append(row)
            chunk_of.setdefault(row, set()).update(s)
    b = DinTrainBatcher(CFG, data)
    assert b.n == len(lit) and len(b) == -(-len(lit) // CFG["train_batch_size"])
    got = []
    for prof, target in b:
        assert prof.dtype == target.dtype == torch.int64 and prof.shape[1] == L and target.shape[1] == 2
        assert prof.shape[0] <= CFG["train_batch_size"]
        for p, (pos, neg) in zip(prof.tolist(), target.tolist()):
            row = tuple(p) + (pos,)
            got.append(row)
            assert 1 <= neg < data.item_num and neg not in chunk_of[row] and pos != 0
    assert sorted(got) == sorted(lit)
    # ACF's machinery: the same sample order for equal seeds
    a = SampleAcfTrainBatcher(CFG, data)
    assert np.array_equal(a._indices(), b._indices())


def test_din_is_registered_and_the_yaml_parses():
    from pixelrec_amd.config.configurator import Config
    from pixelrec_amd.data.dataset import DinTrainBatcher, SeqEvalBatcher
    from pixelrec_amd.data.utils import SUPPORTED, bulid_dataloader
    from pixelrec_amd.model import DIN
    from pixelrec_amd.utils.enum_type import InputType
    from pixelrec_amd.utils.utils import get_model

    assert SUPPORTED["DIN"] == "SEQ" and DIN.input_type == InputType.SEQ and get_model("DIN") is DIN
    train, valid, test = bulid_dataloader(dict(CFG, model="DIN"), _Synth())
    assert type(train.batcher) is DinTrainBatcher and type(valid) is SeqEvalBatcher and type(test) is SeqEvalBatcher
    c = Config([os.path.join(ROOT, "configs/IDNet/din.yaml"), os.path.join(ROOT, "configs/overall/ID.yaml")])
    assert c["model"] == "DIN" and c["embedding_size"] == 64 and list(c["mlp_hidden_size"]) == [80, 40] and c["dropout_prob"] == 0
    assert c["MAX_ITEM_LIST_LENGTH"] == 10 and dict(c["optim_args"]) == {"learning_rate": 1e-4, "weight_decay": 0.1}
    assert c["MODEL_INPUT_TYPE"] == InputType.SEQ


# ------------------------------------------------------------------------------------------------------------ the model
class _Data:
    item_num = 13


def _model(D=8, hidden=(12, 4), L=4):
    from pixelrec_amd.model import DIN

    return DIN({"embedding_size": D, "mlp_hidden_size": list(hidden), "dropout_prob": 0.3, "MAX_ITEM_LIST_LENGTH": L}, _Data())


def test_state_dict_has_the_reference_keys_in_order_and_loads_the_fixture(gold):
    m = _model()
    ref = [str(k) for k in gold["sd.keys"]]
    assert list(m.state_dict().keys()) == ref == R.names(2) and not list(m.named_buffers())
    assert [n for n, _ in m.named_parameters()] == ref == list(m.rec_parameter_names())
    sd = {k: torch.from_numpy(np.asarray(gold["sd." + k])) for k in ref}
    for k in ref:
        assert tuple(m.state_dict()[k].shape) == tuple(sd[k].shape), k
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.item_embedding.weight.data, sd[R.TABLE])
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "attention.dense.bias"}, strict=True)
    one = _model(hidden=(16,))
    assert list(one.state_dict().keys()) == R.names(1)
    three = _model(hidden=(16, 8, 4))
    assert list(three.state_dict().keys()) == R.names(3)


def test_init_is_xavier_normal_with_zero_biases_and_a_nonzero_padding_row():
    torch.manual_seed(0)
    m = _model(D=64, hidden=(80, 40))
    for n, p in m.named_parameters():
        if n.endswith("bias"):
            assert float(p.abs().max()) == 0, n
        else:
            fan_out, fan_in = p.shape
            std = (2.0 / (fan_in + fan_out)) ** 0.5
            assert abs(float(p.std()) - std) <= 0.25 * std, n
    assert float(m.item_embedding.weight[0].abs().max()) > 0                       # xavier_normal_ on the whole table (din.py:40)


def test_bad_settings_raise_and_the_cpu_is_not_a_fallback(gold):
    from pixelrec_amd.lib import PxrError

    with pytest.raises(ValueError, match="embedding_size"):
        _model(D=6)
    with pytest.raises(ValueError, match="mlp_hidden_size"):
        _model(hidden=(10,))
    with pytest.raises(ValueError, match="mlp_hidden_size"):
        _model(hidden=())
    m = _model().train()
    with pytest.raises(PxrError):
        m(torch.from_numpy(gold["rows"][0]))
    assert _model().fused_topk_supported and not _model(hidden=(132,)).fused_topk_supported
    assert not _model(hidden=(16, 8, 4)).fused_topk_supported and not _model(D=132, hidden=(16,)).fused_topk_supported
