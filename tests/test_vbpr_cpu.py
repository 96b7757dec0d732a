"""VBPR without a GPU: the float64 restatement against the reference's golden fixture, the PAIR registration, the shipped YAML,
the state_dict layout, the two-group optimizer state to and from torch.optim.AdamW's layout, and the errors for fragments and
shapes the native path does not take."""
import os

import numpy as np
import pytest
import torch

from tests import vbpr_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "vbpr_tiny.npz")
ARGS4 = {"modal_lr": 1e-4, "rec_lr": 1e-3, "modal_decay": 0.1, "rec_decay": 0}


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_has_the_cases_it_is_meant_to_have(gold):
    users, items = gold["users"], gold["items"]
    assert (items[..., 0] != items[..., 1]).all()          # no sample's positive is its negative
    u, it = users[0], items[0]
    assert len(set(u.tolist())) < len(u) and 0 in u and 0 in it
    assert set(it[:, 0].tolist()) & set(it[:, 1].tolist())    # one sample's positive is another's negative


def test_float64_restatement_matches_the_golden_fixture(gold):
    P = R.state_from(gold, "sd.")
    users, items, v = gold["users"], gold["items"], gold["v_feat"]
    L, grads = R.loss_and_grads(P, v, users[0], items[0])
    assert abs(L - float(gold["loss"])) <= 1e-6
    assert set(grads) == set(R.NAMES)
    for k, g in grads.items():
        ref = gold["grad." + k]
        assert np.abs(g.numpy() - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()), k
    # user 0 and item 0 are ordinary rows: the batch reads them and their gradient is non-zero
    for k in ("user_id_embedding.weight", "item_id_embedding.weight", "user_modal_embedding.weight"):
        assert np.abs(gold["grad." + k][0]).max() > 0, k
    scores = R.predict(P, v, gold["eval.users"]).numpy()
    assert np.abs(scores - gold["eval.scores"]).max() <= 1e-5
    mlr, mwd, rlr, rwd = (float(x) for x in gold["groups"])
    losses, _, _ = R.adamw(P, v, list(zip(users, items)), (mlr, mwd), (rlr, rwd))
    for s, L in enumerate(losses):
        assert abs(L - float(gold[f"adamw.loss{s}"])) <= 2e-6, s
    for k, val in P.items():
        ref = gold["adamw.final." + k]
        assert np.abs(val.numpy() - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max()), k


def test_vbpr_is_registered_for_the_pair_path():
    from pixelrec_amd.data.utils import SUPPORTED
    from pixelrec_amd.model import VBPR
    from pixelrec_amd.utils.enum_type import InputType

    assert SUPPORTED["VBPR"] == "PAIR"
    assert VBPR.input_type == InputType.PAIR


def test_yaml_loads_with_the_reference_values():
    from pixelrec_amd.config.configurator import Config
    from pixelrec_amd.utils.enum_type import InputType

    c = Config([os.path.join(ROOT, "configs/ViNet/vbpr.yaml")])
    assert c["model"] == "VBPR" and c["embedding_size"] == 4096 and c["dropout_prob"] == 0 and c["seed"] == 2020
    assert c["train_batch_size"] == 512 and c["eval_batch_size"] == 512 and c["epochs"] == 200
    assert c["decay_check_name"] == "projection"
    assert dict(c["optim_args"]) == ARGS4
    assert c["v_feat_path"] == "../dataset/visual_features/RN50.npy" and c["dataset"] == "Pixel200K"
    assert list(c["topk"]) == [5, 10] and c["valid_metric"] == "NDCG@10" and c["stopping_step"] == 30
    assert c["MODEL_INPUT_TYPE"] == InputType.PAIR


class _Data:
    user_num, item_num = 7, 9


def _feat(tmp_path, rows=9, F=12, name="v.npy"):
    path = str(tmp_path / name)
    np.save(path, np.random.default_rng(1).standard_normal((rows, F)).astype(np.float32))
    return path


def _model(path, D=16):
    from pixelrec_amd.model import VBPR

    return VBPR({"embedding_size": D, "mlp_hidden_size": [], "dropout_prob": 0.0, "v_feat_path": path}, _Data())


def test_state_dict_has_the_reference_keys_in_order_and_no_features(gold, tmp_path):
    m = _model(_feat(tmp_path))
    ref = [k[len("sd."):] for k in gold.files if k.startswith("sd.")]
    assert ref == list(R.NAMES)
    assert list(m.state_dict().keys()) == ref
    assert [n for n, _ in m.named_parameters()] == ref and not list(m.named_buffers())      # v_feat: neither parameter nor buffer
    sd = {k: torch.from_numpy(np.asarray(gold["sd." + k])) for k in ref}
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert tuple(m.v_feat.shape) == (9, 12) and m.v_feat.dtype == torch.float32


def test_bad_shapes_raise_value_errors_that_say_which(tmp_path):
    with pytest.raises(ValueError, match="item_num"):
        _model(_feat(tmp_path, rows=8))                    # the feature matrix has one row per item
    with pytest.raises(ValueError, match="multiple of 4"):
        _model(_feat(tmp_path, F=10))
    with pytest.raises(ValueError, match="embedding_size"):
        _model(_feat(tmp_path), D=12)                      # Dh = 6
    with pytest.raises(ValueError, match="embedding_size"):
        _model(_feat(tmp_path), D=2 * 4100)                # Dh > 4096


def _host_packed(m):
    """The layout _ensure_packed builds, on the host (no device needed for the state conversions)."""
    specs = m._flat_specs()
    total = sum(p.numel() for _, p in specs)
    off, views = 0, {}
    for name, p in specs:
        views[name] = (off, p.numel(), tuple(p.shape))
        off += p.numel()
    m._views = views
    table = torch.zeros(1 + 7 + 9 + 7, 8)
    m.lazy_table = lambda: table
    m.flat_parameters = lambda: (torch.zeros(total), torch.zeros(total))
    return total


def test_optimizer_state_round_trips_through_the_torch_layout_with_two_groups(tmp_path):
    """native (flat projection moments + one [1 + U + I + U, Dh] table moment buffer) -> torch.optim.AdamW's layout with the
    reference's two groups (the projections under modal_lr / modal_decay, the three tables under rec_lr / rec_decay, parameter
    indices through the groups in order) -> native again; torch's own loader accepts it."""
    from pixelrec_amd import optim

    m = _model(_feat(tmp_path))
    total = _host_packed(m)
    opt = optim.flat_table_adamw(m, ARGS4, "projection")
    assert isinstance(opt, optim.PxrAdamW) and opt.flat_group == {"lr": 1e-4, "weight_decay": 0.1}
    assert opt.param_groups[0]["lr"] == 1e-3 and opt.param_groups[0]["weight_decay"] == 0.0
    g = torch.Generator().manual_seed(3)
    opt.step_count = 5
    opt._m, opt._v = torch.randn(total, generator=g), torch.rand(total, generator=g)
    opt._tm, opt._tv = torch.randn(24, 8, generator=g), torch.rand(24, 8, generator=g)
    opt._tm[0] = 0
    opt._tv[0] = 0                                         # the spare row carries no state
    opt._ensure_state = lambda: None
    ts = opt.state_dict(layout="torch")
    assert [g_["params"] for g_ in ts["param_groups"]] == [[0, 1], [2, 3, 4]]
    assert (ts["param_groups"][0]["lr"], ts["param_groups"][0]["weight_decay"]) == (1e-4, 0.1)
    assert (ts["param_groups"][1]["lr"], ts["param_groups"][1]["weight_decay"]) == (1e-3, 0.0)
    shapes = [(8, 12), (1, 12), (7, 8), (9, 8), (7, 8)]
    assert [tuple(ts["state"][j]["exp_avg"].shape) for j in range(5)] == shapes
    assert torch.equal(ts["state"][3]["exp_avg_sq"], opt._tv[8:17]) and torch.equal(ts["state"][4]["exp_avg"], opt._tm[17:])
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    topt = torch.optim.AdamW([{"params": params[:2], "lr": 1e-4, "weight_decay": 0.1},
                              {"params": params[2:], "lr": 1e-3, "weight_decay": 0.0}])
    topt.load_state_dict(ts)                               # strict layout: torch's own loader
    assert [g_["params"] for g_ in topt.state_dict()["param_groups"]] == [[0, 1], [2, 3, 4]]
    merged = {"state": ts["state"], "param_groups": [{**ts["param_groups"][1], "params": [0, 1, 2, 3, 4]}]}
    back = optim.torch_to_native_state(merged, m)
    assert back["step"] == 5
    for k, ref in (("m", opt._m), ("v", opt._v), ("table_m", opt._tm), ("table_v", opt._tv)):
        assert torch.equal(back[k], ref), k


def test_one_group_and_unsupported_fragments(tmp_path):
    from pixelrec_amd import optim

    m = _model(_feat(tmp_path))
    _host_packed(m)
    one = optim.flat_table_adamw(m, {"learning_rate": 1e-3, "weight_decay": 0.1}, None)
    assert one.flat_group is None and one.param_groups[0]["lr"] == 1e-3
    # fragments that would separate the two projections from each other, or the three tables from each other
    for frag in ("feature", "bias_projection", "modal", "user", "item_id", "embedding", "weight"):
        with pytest.raises(NotImplementedError, match="'%s'" % frag):
            optim.flat_table_adamw(m, ARGS4, frag)
    lead = optim.flat_table_adamw(m, ARGS4, None)          # no fragment: the reference's empty 'visual_encoder' group comes first
    assert lead.flat_group is None and lead.empty_leading_group == {"lr": 1e-4, "weight_decay": 0.1}


def test_trainer_takes_the_new_optimizer_branch_only_for_a_model_that_declares_it():
    from pixelrec_amd.model import MF, VBPR, SASRec

    assert VBPR.split_flat_table_groups is True
    assert not hasattr(MF, "split_flat_table_groups") and not hasattr(SASRec, "split_flat_table_groups")
