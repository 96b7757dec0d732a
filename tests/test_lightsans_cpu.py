"""LightSANs host side (no GPU): the float64 restatement (tests/lightsans_restate.py) against the golden fixture made by the
reference's own LightSANs (tools/make_golden_lightsans.py) and against finite differences; the model's state_dict names and order,
its init and its shape limits; TwoTowerTrainBatcher against the reference's AUGSEQ prefixes; the YAML and the data dispatch."""
import os

import numpy as np
import pytest
import torch

from pixelrec_amd.config import Config
from pixelrec_amd.data.dataload import Data
from pixelrec_amd.data.dataset import TwoTowerTrainBatcher
from pixelrec_amd.data.utils import SUPPORTED
from pixelrec_amd.model import LightSANs
from pixelrec_amd.utils.enum_type import InputType
from tests import lightsans_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lightsans_tiny.npz")
GDIR = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _cfg(D=16, H=2, K=3, L=6, n_layers=2, inner=1):
    return {"n_layers": n_layers, "n_heads": H, "embedding_size": D, "inner_size": inner, "k_interests": K,
            "hidden_dropout_prob": 0.1, "attn_dropout_prob": 0.1, "hidden_act": "gelu", "layer_norm_eps": 1e-12,
            "initializer_range": 0.02, "MAX_ITEM_LIST_LENGTH": L, "seed": 2020}


def _meta(gold):
    item_num, D, H, K, L, B, inner = (int(x) for x in gold["meta"][:7])
    return item_num, D, H, K, L, B, inner


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n_layers", [1, 2])
def test_restatement_matches_the_golden_fixture(gold, n_layers):
    _, D, H, K, L, B, _ = _meta(gold)
    p = f"n{n_layers}."
    sd = R.unpack(gold, "sd", n_layers)
    assert list(sd) == [str(k) for k in gold[p + "sd_keys"]]
    loss, G = R.forward_backward(sd, gold["b0.items"], n_layers, H, K)
    assert abs(loss - float(gold[p + "loss"])) <= 2e-6
    ref = R.unpack(gold, p + "grad", n_layers)
    assert set(ref) == set(G)
    for n, r in ref.items():
        assert np.abs(G[n] - r).max() <= 1e-6 + 1e-5 * np.abs(r).max(), n
    assert not ref["item_embedding.weight"][0].any()                       # padding_idx: no gradient into row 0
    scores = R.predict(sd, gold["eval.item_seq"], n_layers, H, K)
    assert np.abs(scores - gold[p + "eval.scores"]).max() <= 1e-5


def test_restatement_matches_the_fixture_trajectory(gold):
    _, D, H, K, L, B, _ = _meta(gold)
    lr, wd = (float(x) for x in gold["lr_wd"])
    losses, final = R.adamw_trajectory(R.unpack(gold, "sd", 2), [gold[f"b{j}.items"] for j in range(4)], 2, H, K, lr, wd)
    for s, l in enumerate(losses):
        assert abs(l - float(gold[f"n2.adamw.loss{s}"])) <= 2e-6, s
    ref = R.unpack(gold, "n2.adamw.final", 2)
    for k, r in ref.items():
        assert np.abs(final[k] - r).max() <= 2e-5 * max(1.0, np.abs(r).max()), k


def test_fixture_rows_cover_heavy_padding_and_a_full_row(gold):
    _, _, _, _, L, B, _ = _meta(gold)
    items = gold["b0.items"]
    assert items.shape == (B, L + 2)
    n_real = (items[:, :L] != 0).sum(1)
    assert n_real.min() == 0 and n_real.max() == L                          # a history of padding only, and a full one
    for r in items:                                                         # the negative lies outside the sequence
        assert r[-1] not in set(r[:-1][r[:-1] != 0].tolist())


def test_restatement_gradients_match_finite_differences():
    """Every parameter, theta and the position branch included, with dropout masks injected."""
    rng = np.random.default_rng(5)
    N, D, H, K, L, B, n_layers = 9, 8, 2, 2, 4, 3, 2
    torch.manual_seed(0)
    m = LightSANs(_cfg(D, H, K, L, n_layers, inner=1), type("D", (), {"item_num": N})())
    sd = {k: v.double().numpy() + rng.normal(0, 0.3, v.shape) for k, v in m.state_dict().items()}
    items = np.array([[0, 0, 3, 4, 5, 6], [1, 2, 3, 4, 7, 8], [0, 0, 0, 0, 2, 1]])
    drop = R.masks(1234, B, L, D, H, K, n_layers, 0.2, 0.3)
    kw = dict(drop=drop, p_hidden=0.2, p_attn=0.3)
    _, G = R.forward_backward(sd, items, n_layers, H, K, **kw)
    h = 1e-6
    for name, g in G.items():
        flat = sd[name].reshape(-1)
        picks = rng.choice(flat.size, size=min(4, flat.size), replace=False)
        if name == "item_embedding.weight":
            picks = [i for i in picks if i >= D] or [D]                     # row 0 is the padding row: no gradient
        for i in picks:
            keep = flat[i]
            flat[i] = keep + h
            lp = R.forward_backward(sd, items, n_layers, H, K, **kw)[0]
            flat[i] = keep - h
            lm = R.forward_backward(sd, items, n_layers, H, K, **kw)[0]
            flat[i] = keep
            fd = (lp - lm) / (2 * h)
            assert abs(fd - g.reshape(-1)[i]) <= 1e-7 + 1e-5 * abs(fd), (name, i, fd, g.reshape(-1)[i])


def test_position_probabilities_normalise_over_queries():
    rng = np.random.default_rng(1)
    A = R.pos_probs(torch.from_numpy(rng.standard_normal((5, 16))), 2)
    assert torch.allclose(A.sum(-2), torch.ones(2, 5, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------ the model (construction only)
def test_state_dict_names_and_order_equal_the_fixture(gold):
    item_num, D, H, K, L, _, inner = _meta(gold)
    for n_layers in (1, 2):
        m = LightSANs(_cfg(D, H, K, L, n_layers, inner), type("D", (), {"item_num": item_num})())
        assert list(m.state_dict().keys()) == [str(k) for k in gold[f"n{n_layers}.sd_keys"]]
        assert list(m.rec_parameter_names()) == [n for n, _ in m.named_parameters()]
        res = m.load_state_dict({k: torch.from_numpy(v) for k, v in R.unpack(gold, "sd", n_layers).items()}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys


def test_init_follows_the_reference():
    torch.manual_seed(3)
    m = LightSANs(_cfg(D=64, H=4, K=3, L=10, n_layers=3, inner=2), type("D", (), {"item_num": 500})())
    a = [lay.multi_head_attention for lay in m.trm_encoder.layer]
    th = a[0].attpooling_key.theta.detach()
    assert 0.8 < float(th.std()) < 1.2                                      # randn, not N(0, 0.02)
    for x in a[1:]:                                                         # one deep-copied layer: the same thetas
        assert torch.equal(x.attpooling_key.theta, a[0].attpooling_key.theta)
        assert torch.equal(x.attpooling_value.theta, a[0].attpooling_value.theta)
    w = m.item_embedding.weight.detach()
    assert w[0].abs().sum() > 0 and 0.015 < float(w.std()) < 0.025          # row 0 drawn too
    assert not a[0].query.bias.any() and torch.equal(a[0].pos_ln.weight, torch.ones(64))
    assert LightSANs.input_type == InputType.AUGSEQ and SUPPORTED["LightSANs"] == "TWOTOWER"


@pytest.mark.parametrize("over,what", [({"MAX_ITEM_LIST_LENGTH": 65}, "MAX_ITEM_LIST_LENGTH"),
                                       ({"embedding_size": 2048, "n_heads": 4}, "embedding_size"),
                                       ({"embedding_size": 96, "n_heads": 16}, "embedding_size"),
                                       ({"k_interests": 17}, "k_interests"), ({"k_interests": 0}, "k_interests")])
def test_model_refuses_shapes_beyond_the_kernel_limits(over, what):
    cfg = dict(_cfg(D=64, H=4, K=3, L=10), **over)
    with pytest.raises(ValueError, match=what):
        LightSANs(cfg, type("D", (), {"item_num": 50})())
    cfg = _cfg(D=1024, H=4, K=16, L=64, n_layers=1)                          # the limits themselves are served
    LightSANs(cfg, type("D", (), {"item_num": 50})())


# ------------------------------------------------------------------------------------------------ data
SRGNN_GOLD = os.path.join(ROOT, "tests", "golden", "srgnn_tiny.npz")


def _data(L, batch=8):
    cfg = {"data_path": GDIR, "dataset": "TinyInter", "MAX_ITEM_LIST_LENGTH": L, "MODEL_INPUT_TYPE": LightSANs.input_type,
           "train_batch_size": batch, "eval_batch_size": 7, "seed": 5}
    d = Data(cfg)
    d.build()
    return cfg, d


def _reference_prefixes():
    """train_feat['item_seq'] of the reference's Data under AUGSEQ on TinyInter.csv (recorded by tools/make_golden_srgnn.py)."""
    g = np.load(SRGNN_GOLD)
    ends = np.cumsum(g["aug.lens"])
    return int(g["aug.L"]), np.split(g["aug.flat"], ends[:-1])


def test_two_tower_rows_are_the_reference_prefixes_with_outside_negatives():
    """Every AUGSEQ prefix of the reference's train_feat is one row: prefix + negative, left-padded to L + 2."""
    L, ref = _reference_prefixes()
    cfg, d = _data(L)
    bt = TwoTowerTrainBatcher(cfg, d)
    assert bt.n == len(ref)
    idx = bt._indices()
    assert sorted(idx.tolist()) == list(range(len(ref)))
    seen = 0
    for hist, target in bt:
        hist, target = hist.numpy(), target.numpy()
        assert hist.dtype == target.dtype == np.int64 and hist.shape[1] == L and target.shape == (len(hist), 2)
        for r in range(len(hist)):
            s = ref[idx[seen + r]]
            row = np.concatenate((hist[r], target[r]))
            k = len(s) + 1
            assert 2 <= len(s) <= L + 1
            assert np.array_equal(row[-k:-1], s) and not row[:-k].any()       # prefix + negative, left-padded to L + 2
            assert 1 <= target[r, 1] < d.item_num and target[r, 1] not in s  # the negative lies outside the prefix
        seen += len(hist)
    assert seen == len(ref)


def test_every_item_of_a_chunk_after_the_first_is_a_positive():
    L, ref = _reference_prefixes()
    cfg, d = _data(L, batch=1000)
    hist, target = next(iter(TwoTowerTrainBatcher(cfg, d)))
    assert len(hist) == len(ref)
    want = sorted(int(s[-1]) for s in ref)
    assert sorted(target[:, 0].tolist()) == want


def test_two_tower_order_and_rank_split_are_the_distributed_samplers():
    cfg, d = _data(4)
    n = len(d.train_feat["seq_start"])
    for world in (1, 2):
        for rank in range(world):
            a = TwoTowerTrainBatcher(cfg, d, rank=rank, world=world)
            a.set_epoch(3)
            g = torch.Generator()
            g.manual_seed(3)
            perm = torch.randperm(n, generator=g).tolist()
            total = -(-n // world) * world
            perm += perm[:total - n]
            assert a._indices().tolist() == perm[rank:total:world]
    a, b = TwoTowerTrainBatcher(cfg, d, rank=0, world=2), TwoTowerTrainBatcher(cfg, d, rank=1, world=2)
    assert set(a._indices().tolist()) | set(b._indices().tolist()) == set(range(n))


def test_two_tower_batcher_refuses_the_seq_build():
    cfg, _ = _data(4)
    d = Data(dict(cfg, MODEL_INPUT_TYPE=InputType.SEQ))
    d.build()
    with pytest.raises(ValueError, match="AUGSEQ"):
        TwoTowerTrainBatcher(cfg, d)


def test_yaml_loads_and_dispatches_to_the_two_tower_path(tmp_path):
    from pixelrec_amd.data import bulid_dataloader, load_data
    from pixelrec_amd.data.dataset import SeqEvalBatcher

    c = Config([os.path.join(ROOT, "configs/IDNet/lightsans.yaml"), os.path.join(ROOT, "configs/overall/ID.yaml")])
    assert c["model"] == "LightSANs" and c["k_interests"] == 3 and c["n_layers"] == 1 and c["n_heads"] == 4
    assert c["embedding_size"] == 512 and c["inner_size"] == 2 and c["MODEL_INPUT_TYPE"] == InputType.AUGSEQ
    over = tmp_path / "o.yaml"
    over.write_text(f"data_path: {GDIR}/\ndataset: TinyInter\nMAX_ITEM_LIST_LENGTH: 4\ntrain_batch_size: 8\n")
    c = Config([os.path.join(ROOT, "configs/IDNet/lightsans.yaml"), os.path.join(ROOT, "configs/overall/ID.yaml"), str(over)])
    d = load_data(c)
    train, valid, test = bulid_dataloader(c, d)
    assert isinstance(train.batcher, TwoTowerTrainBatcher)
    assert isinstance(valid, SeqEvalBatcher) and isinstance(test, SeqEvalBatcher)
    assert "seq_start" in d.train_feat                                       # the AUGSEQ prefixes, as in the reference
    hist, target = next(iter(train))
    assert hist.shape[1] == 4 and target.shape[1] == 2
