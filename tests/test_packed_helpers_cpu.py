"""The host-side helpers of pixelrec_amd/model/packed.py that need no device: the two input forms, the Linear-stack helpers, the
MLPLayers parameter container, the step bracket and the evaluation-cache hook."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from pixelrec_amd.lib import PxrError
from pixelrec_amd.model import packed


class _Data:
    def __init__(self, I):
        self.item_num = I


def _din(hidden=(12, 4), D=8, I=13):
    from pixelrec_amd.model import DIN

    return DIN({"embedding_size": D, "mlp_hidden_size": list(hidden), "dropout_prob": 0.0, "MAX_ITEM_LIST_LENGTH": 4}, _Data(I))


def _curatornet(tmp_path, I=9, F=12, E=8, mult=2):
    from pixelrec_amd.model import CuratorNet

    path = str(tmp_path / "v.npy")
    np.save(path, np.random.default_rng(0).standard_normal((I, F)).astype(np.float32))
    return CuratorNet({"embedding_size": E, "hidden_size": mult, "MAX_ITEM_LIST_LENGTH": 4, "v_feat_path": path}, _Data(I))


# ------------------------------------------------------------------------------------------------------------ input forms
ROWS = torch.tensor([[0, 2, 3, 4, 5, 6], [1, 1, 2, 3, 7, 8]])
TEXT = "X: expected ids, got profile {profile} and tail {tail}"             # a caller's own text: the shapes go where it says


def test_split_tail_takes_the_single_tensor_and_the_pair():
    for n_tail in (1, 2, 3):
        want = (ROWS[:, :-n_tail], ROWS[:, -n_tail:])
        for form in (ROWS, want, list(want), (want[0], want[1].reshape(-1))):          # a flat tail is reshaped per row
            prof, tail = packed.split_tail(form, n_tail, TEXT)
            assert torch.equal(prof, want[0]) and torch.equal(tail, want[1])
            assert prof.is_contiguous() and tail.is_contiguous()


def test_split_tail_rejects_what_the_models_rejected():
    bad = [
        (ROWS.view(2, 1, 6), 2),                                   # wrong rank of the single tensor
        (ROWS[:, :2], 2),                                          # no profile position left (L = 0)
        ((ROWS[:, :4], ROWS[:, 3:]), 2),                           # wrong tail width
        ((ROWS[:, :4], ROWS[:, 4:]), 3),
        ((ROWS[:, :4].reshape(2, 2, 2), ROWS[:, 4:]), 2),          # wrong rank of the profile
        ((ROWS[:, :0], ROWS[:, 4:]), 2),                           # an empty profile
    ]
    for form, n_tail in bad:
        with pytest.raises(ValueError, match=r"^X: expected ids, got profile \(.*\) and tail \(.*\)$"):
            packed.split_tail(form, n_tail, TEXT)
    assert packed.split_tail(ROWS, 2, TEXT, max_len=4)[0].shape == (2, 4)
    with pytest.raises(ValueError, match=r"^X: expected ids, got profile \(2, 4\) and tail \(2, 2\)$"):
        packed.split_tail(ROWS, 2, TEXT, max_len=3)                # CuratorNet's upper bound on L


def _planes(rows):
    return torch.stack((rows[:, :-1], torch.cat((rows[:, :-2], rows[:, -1:]), 1)), 1)     # [B, 2, L + 1]


def test_split_planes_takes_the_two_planes_and_the_pair():
    want = (ROWS[:, :-2], ROWS[:, -2:])
    for form in (_planes(ROWS), want, list(want)):
        prof, tgt = packed.split_planes(form, "X", TEXT)
        assert torch.equal(prof, want[0]) and torch.equal(tgt, want[1])
        assert prof.is_contiguous() and tgt.is_contiguous()


def test_split_planes_rejects_what_the_models_rejected():
    planes = _planes(ROWS)
    for form in (ROWS, planes[:, :1], planes[:, :, :1], planes.unsqueeze(0)):              # wrong rank, one plane, no profile
        with pytest.raises(ValueError, match=r"^X: expected \[B, 2, L \+ 1\] ids"):
            packed.split_planes(form, "X", TEXT)
    unequal = planes.clone()
    unequal[1, 1, 0] += 1
    with pytest.raises(ValueError, match="^X: the two planes .* same profile"):
        packed.split_planes(unequal, "X", TEXT)
    for form in ((ROWS[:, :3], ROWS[:, 3:]), (ROWS[:, :0], ROWS[:, 4:])):                  # wrong target width, empty profile
        with pytest.raises(ValueError, match=r"^X: expected ids, got profile \(2, [03]\) and tail \(2, [23]\)$"):
            packed.split_planes(form, "X", TEXT)
    assert packed.split_planes((ROWS[:, :0], ROWS[:, 4:]), "X", TEXT, min_len=0)[0].shape == (2, 0)


def test_the_models_keep_their_own_conditions(tmp_path):
    from pixelrec_amd.model import ACF, DSSM, FM, WideDeep  # noqa: F401

    with pytest.raises(ValueError, match=r"^DIN: expected \[B, L \+ 2\] ids \(profile, positive, negative\), got profile \(2, 4\) and target "
                                         r"\(2, 3\)$"):
        _din()._split_input((ROWS[:, :4], ROWS[:, 3:]))
    cur = _curatornet(tmp_path)
    with pytest.raises(ValueError, match=r"^CuratorNet: expected .*1\.\.255 positions"):
        cur._split_input(torch.zeros(2, 258, dtype=torch.int64))
    assert cur._split_input(torch.zeros(2, 257, dtype=torch.int64))[0].shape == (2, 255)
    cfg = {"embedding_size": 8, "mlp_hidden_size": [8], "dropout_prob": 0.0, "MAX_ITEM_LIST_LENGTH": 4}
    wd = WideDeep(cfg, _Data(13))
    assert wd._split_input(_planes(ROWS))[1].tolist() == ROWS[:, -2:].tolist()
    with pytest.raises(ValueError, match="MAX_ITEM_LIST_LENGTH = 4"):
        wd._split_input(_planes(ROWS[:, 1:]))
    with pytest.raises(ValueError, match=r"^WideDeep: expected a profile \[B, L\] and targets \[B, 2\] \(positive, negative\), got \(2, 4\) and "
                                         r"\(2, 3\)$"):
        wd._split_input((ROWS[:, :4], ROWS[:, 3:]))
    fm, dssm = FM(cfg, _Data(13)), DSSM({**cfg, "mlp_hidden_size": []}, _Data(13))
    with pytest.raises(ValueError, match="^FM: the two planes"):
        fm._split_input(_planes(ROWS) + torch.tensor([[[0], [1]]]))
    for m in (fm, dssm):                                                              # the texts these models had before the helpers
        with pytest.raises(ValueError, match=rf"^{type(m).__name__}: expected a profile \[B, L\] \(L >= 1\) and targets \[B, 2\] "
                                             r"\(positive, negative\), got \(2, 4\) and \(2, 3\)$"):
            m._split_input((ROWS[:, :4], ROWS[:, 3:]))
    with pytest.raises(ValueError, match=r"^DSSM: expected \[B, L \+ 2\] ids \(profile, positive, negative\), got \(2, 2\)$"):
        dssm._split_input(ROWS[:, :2])
    acf_text = r"^ACF: expected \[B, L \+ 3\] ids \(profile, then 3 trailing columns\), got profile \(2, 4\) and tail \(2, 2\)$"
    with pytest.raises(ValueError, match=acf_text):
        ACF._split_input(None, (ROWS[:, :4], ROWS[:, 4:]), 3)


# ------------------------------------------------------------------------------------------------------------ Linear stacks
def test_linear_specs_and_names_of_a_two_hidden_layer_din():
    m = _din()
    lin = m._linears()
    mlp = m.attention.att_mlp_layers.mlp_layers
    assert [(k, p) for k, p, _ in lin] == [("l0", "attention.att_mlp_layers.mlp_layers.1"), ("l1", "attention.att_mlp_layers.mlp_layers.4"),
                                          ("dense", "attention.dense")]
    specs = packed.linear_specs(lin)
    assert [k for k, _ in specs] == ["l0.w", "l0.b", "l1.w", "l1.b", "dense.w", "dense.b"]
    want = [mlp[1].weight, mlp[1].bias, mlp[4].weight, mlp[4].bias, m.attention.dense.weight, m.attention.dense.bias]
    assert all(p is w for (_, p), w in zip(specs, want))
    assert [tuple(p.shape) for _, p in specs] == [(12, 32), (12,), (4, 12), (4,), (1, 4), (1,)]
    names = {"attention.att_mlp_layers.mlp_layers.1.weight": "l0.w", "attention.att_mlp_layers.mlp_layers.1.bias": "l0.b",
             "attention.att_mlp_layers.mlp_layers.4.weight": "l1.w", "attention.att_mlp_layers.mlp_layers.4.bias": "l1.b",
             "attention.dense.weight": "dense.w", "attention.dense.bias": "dense.b"}
    assert list(packed.linear_names(lin).items()) == list(names.items())
    assert m._flat_specs() == specs
    assert list(m.rec_parameter_names().items()) == list(names.items()) + [("item_embedding.weight", None)]


def test_linear_specs_and_names_of_curatornet(tmp_path):
    m = _curatornet(tmp_path)
    lin = m._linears()
    attrs = ["selu_common1", "selu_common2", "selu_pu1", "selu_pu2", "selu_pu3"]
    assert [(k, p) for k, p, _ in lin] == list(zip(["c1", "c2", "p1", "p2", "p3"], attrs))
    assert all(mod is getattr(m, a) for (_, _, mod), a in zip(lin, attrs))
    specs = packed.linear_specs(lin)
    assert [k for k, _ in specs] == ["c1.w", "c1.b", "c2.w", "c2.b", "p1.w", "p1.b", "p2.w", "p2.b", "p3.w", "p3.b"]
    assert [tuple(p.shape) for _, p in specs] == [(8, 12), (8,), (8, 8), (8,), (16, 16), (16,), (16, 16), (16,), (8, 16), (8,)]
    names = [("selu_common1.weight", "c1.w"), ("selu_common1.bias", "c1.b"), ("selu_common2.weight", "c2.w"),
             ("selu_common2.bias", "c2.b"), ("selu_pu1.weight", "p1.w"), ("selu_pu1.bias", "p1.b"), ("selu_pu2.weight", "p2.w"),
             ("selu_pu2.bias", "p2.b"), ("selu_pu3.weight", "p3.w"), ("selu_pu3.bias", "p3.b")]
    assert list(packed.linear_names(lin).items()) == names == list(m.rec_parameter_names().items())
    assert [n for n, _ in names] == [k for k, p in m.named_parameters() if p.requires_grad]      # the frozen table is not among them


@pytest.mark.parametrize("act", [nn.Sigmoid, nn.ReLU, nn.SELU])
def test_act_mlp_has_the_reference_layout(act):
    mlp = packed._ActMLP([32, 12, 4], act, dropout=0.25)
    assert list(mlp.state_dict().keys()) == ["mlp_layers.1.weight", "mlp_layers.1.bias", "mlp_layers.4.weight", "mlp_layers.4.bias"]
    assert [k for k, _ in mlp.named_parameters()] == list(mlp.state_dict().keys())
    mods = list(mlp.mlp_layers)
    assert [type(x) for x in mods] == [nn.Dropout, nn.Linear, act] * 2 and mods[0].p == mods[3].p == 0.25
    assert (mods[1].in_features, mods[1].out_features, mods[4].in_features, mods[4].out_features) == (32, 12, 12, 4)
    assert list(packed._ActMLP([8], act).state_dict().keys()) == [] == list(packed._ActMLP([], act).state_dict().keys())


def test_constructor_checks():
    assert packed.hidden_sizes(None) == [] == packed.hidden_sizes([])
    assert packed.hidden_sizes(8) == [8] and packed.hidden_sizes((8, "4")) == [8, 4]
    for D in (0, -4, 6, 4100):
        with pytest.raises(ValueError, match=f"embedding_size must be a positive multiple of 4.*got {D}$"):
            packed.check_width16(D)
    packed.check_width16(4096)
    packed.one_process(_din())                                                           # one process here: no complaint


def test_one_process_names_the_model(monkeypatch):
    monkeypatch.setattr(packed, "world_info", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="^DIN runs on one process: data parallelism is not built for this model$"):
        _din()
    with pytest.raises(NotImplementedError, match="^Module runs on one process: .* for the graph models$"):
        packed.one_process(nn.Module(), "the graph models")


# ------------------------------------------------------------------------------------------------------------ the step bracket
def test_take_saved_raises_on_a_fresh_model():
    m = _din()
    with pytest.raises(PxrError, match=r"^backward\(\) without a training-mode forward\(\)$"):
        m._take_saved()
    m._saved = saved = {"B": 1}
    assert m._take_saved() is saved and m._saved is saved
    assert packed.take_saved(m, "table") is saved
    with pytest.raises(PxrError, match=r"^backward\(\) without a training-mode forward\(\)$"):
        packed.take_saved(m, None)                                                     # the pixel pooled models' second condition


def test_step_done_with_the_counter_already_bumped_launches_nothing(monkeypatch):
    from pixelrec_amd import ops

    def no_launch(*a, **k):
        raise AssertionError("counter_add launched")

    monkeypatch.setattr(ops, "counter_add", no_launch)
    m = _din()
    m._saved, before = {"B": 1}, m._step_counter
    m._step_done(bumped=True)
    assert m._saved is None and m._step_counter == before + 1 and m._drop_dev is None
    m._saved = {"B": 1}
    with pytest.raises(AssertionError, match="counter_add launched"):                    # the default advances the device counter
        m._step_done()
    assert m._saved is None and m._step_counter == before + 1                            # cleared first, counted last


# ------------------------------------------------------------------------------------------------------------ evaluation cache
def test_eval_cache_goes_on_train_and_load_but_not_on_eval(tmp_path, monkeypatch):
    order = []

    class Hooks:
        def flush(self):
            order.append("flush")

    m = _din()
    drop = type(m)._drop_eval_cache
    m._drop_eval_cache = lambda: (order.append("drop"), drop(m))[1]
    m.register_table_hooks(Hooks())
    m._eval_cache = cache = ("aq", "Bm", "C")
    assert m.eval()._eval_cache is cache and m.train(False)._eval_cache is cache and order == []
    assert m.train()._eval_cache is None and order == ["drop"]
    m._eval_cache = cache
    del order[:]
    sd = {k: v.clone() for k, v in nn.Module.state_dict(m).items()}
    loaded, plain_load = [], nn.Module.load_state_dict
    monkeypatch.setattr(nn.Module, "load_state_dict", lambda self, *a, **k: (loaded.append(list(order)), plain_load(self, *a, **k))[1])
    m.load_state_dict(sd, strict=True)
    assert loaded == [["flush", "drop"]] and m._eval_cache is None                       # the table is flushed before the load
    cur = _curatornet(tmp_path)
    cur.store_ifeatures = "cached"
    assert cur.eval().store_ifeatures == "cached"
    assert cur.train().store_ifeatures is None


def test_models_without_an_evaluation_cache_keep_their_matrices_on_train():
    from pixelrec_amd.model import MF

    class D:
        user_num, item_num = 5, 7

    m = MF({"embedding_size": 8, "mlp_hidden_size": [], "dropout_prob": 0.0}, D())
    m.store_ifeatures = "kept"
    assert m.train().store_ifeatures == "kept"
    m.load_state_dict(m.state_dict())
    assert m.store_ifeatures == "kept"
