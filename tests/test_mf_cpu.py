"""MF without a GPU: the float64 restatement against the reference's golden fixture (both tower configs), the PAIR registration,
the shipped YAML, and the optimizer-state conversion to and from torch.optim.AdamW's layout over the shared table buffer."""
import os

import numpy as np
import pytest
import torch

from tests import mf_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "mf_tiny.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("cfg", ["c0", "c1"])
def test_float64_restatement_matches_the_golden_fixture(gold, cfg):
    n_layers = len(gold[cfg + ".hidden"])
    P = R.state_from(gold, cfg + ".sd.")
    users, items = gold["users"], gold["items"]
    L, grads = R.loss_and_grads(P, n_layers, users[0], items[0])
    assert abs(L - float(gold[cfg + ".loss"])) <= 1e-6
    for k, g in grads.items():
        ref = gold[cfg + ".grad." + k]
        assert np.abs(g.numpy() - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()), k
    # user 0 and item 0 are ordinary rows: the batch reads them and their gradient is non-zero
    assert np.abs(gold[cfg + ".grad.user_embedding.weight"][0]).max() > 0
    assert np.abs(gold[cfg + ".grad.item_embedding.weight"][0]).max() > 0
    scores = R.predict(P, n_layers, gold["eval.users"]).numpy()          # running statistics as the step left them
    assert np.abs(scores - gold[cfg + ".eval.scores"]).max() <= 1e-5
    P = R.state_from(gold, cfg + ".sd.")
    lr, wd = (float(x) for x in gold["lr_wd"])
    losses, _, _ = R.adamw(P, n_layers, list(zip(users, items)), lr, wd)
    for s, L in enumerate(losses):
        assert abs(L - float(gold[cfg + f".adamw.loss{s}"])) <= 2e-6, s
    for k, v in P.items():
        ref = gold[cfg + ".adamw.final." + k]
        if v.dtype == torch.int64:
            assert int(v) == int(ref), k
        elif R.noise_driven(k):
            assert np.abs(v.numpy() - ref).max() <= 4 * 4 * lr, k
        else:
            assert np.abs(v.numpy() - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max()), k


def test_mf_is_registered_for_the_pair_path():
    from pixelrec_amd.data.utils import SUPPORTED
    from pixelrec_amd.model import MF
    from pixelrec_amd.utils.enum_type import InputType

    assert SUPPORTED["MF"] == "PAIR"
    assert MF.input_type == InputType.PAIR


def test_yaml_loads_with_the_reference_values():
    from pixelrec_amd.config.configurator import Config
    from pixelrec_amd.utils.enum_type import InputType

    c = Config([os.path.join(ROOT, "configs/IDNet/mf.yaml"), os.path.join(ROOT, "configs/overall/ID.yaml")])
    assert c["model"] == "MF" and c["embedding_size"] == 4096 and c["dropout_prob"] == 0 and list(c["mlp_hidden_size"]) == []
    assert c["MODEL_INPUT_TYPE"] == InputType.PAIR


class _Data:
    user_num, item_num = 7, 9


def _model(hidden, D=8):
    from pixelrec_amd.model import MF

    return MF({"embedding_size": D, "mlp_hidden_size": hidden, "dropout_prob": 0.0}, _Data())


def test_state_dict_has_the_reference_keys_in_order(gold):
    for cfg, hidden in (("c0", []), ("c1", [8, 4])):
        m = _model(hidden)
        ref = [k[len(cfg + ".sd."):] for k in gold.files if k.startswith(cfg + ".sd.")]
        assert list(m.state_dict().keys()) == ref
        sd = {k: torch.from_numpy(np.asarray(gold[cfg + ".sd." + k])) for k in ref}
        res = m.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    with pytest.raises(ValueError):
        _model([6, 4])                                     # hidden sizes are multiples of 4


def test_optimizer_state_round_trips_through_the_torch_layout():
    """native (flat tower moments + one [1 + U + I, D] table moment buffer) -> torch.optim.AdamW's per-parameter layout in the
    reference's parameter order (towers, then user_embedding, then item_embedding: [U, D] and [I, D]) -> native again."""
    from pixelrec_amd import optim

    m = _model([8, 4])
    specs = m._flat_specs()
    total = sum(p.numel() for _, p in specs)
    off, views = 0, {}
    for name, p in specs:                                  # the flat layout _ensure_packed builds (no device needed here)
        views[name] = (off, p.numel(), tuple(p.shape))
        off += p.numel()
    m._views = views
    table = torch.zeros(1 + 7 + 9, 8)
    m.lazy_table = lambda: table
    m.flat_parameters = lambda: (torch.zeros(total), torch.zeros(total))
    g = torch.Generator().manual_seed(3)
    native = {"step": 5, "param_groups": [{"lr": 1e-3, "weight_decay": 0.1, "betas": (0.9, 0.999), "eps": 1e-8}],
              "m": torch.randn(total, generator=g), "v": torch.rand(total, generator=g),
              "table_m": torch.randn(17, 8, generator=g), "table_v": torch.rand(17, 8, generator=g)}
    native["table_m"][0] = 0
    native["table_v"][0] = 0                               # the spare row carries no state
    ts = optim.native_to_torch_state(native, m)
    names = optim.reference_rec_parameter_names(m)
    assert names[-2:] == ["user_embedding.weight", "item_embedding.weight"]
    assert names[:4] == ["user_mlp_layers.mlp_layers.1.weight", "user_mlp_layers.mlp_layers.1.bias",
                         "user_mlp_layers.mlp_layers.2.weight", "user_mlp_layers.mlp_layers.2.bias"]
    assert len(ts["state"]) == len(names) == 8 * 2 + 2
    assert tuple(ts["state"][len(names) - 2]["exp_avg"].shape) == (7, 8)
    assert tuple(ts["state"][len(names) - 1]["exp_avg"].shape) == (9, 8)
    assert torch.equal(ts["state"][len(names) - 1]["exp_avg_sq"], native["table_v"][8:])
    back = optim.torch_to_native_state(ts, m)
    assert back["step"] == 5
    for k in ("m", "v", "table_m", "table_v"):
        assert torch.equal(back[k], native[k]), k
