"""MOMF without a GPU: the batcher (PairTrainBatcher's samples with the items as positions into the batch's distinct images, no zero
image in front), the fixture of the reference's own class against the float64 restatement on the torch-module tower's float64
output (which pins the composition: which row of E a position means, the per-occurrence BatchNorm statistics, the absence of the
1e-8), the dedup as a property of the restatement, the registry and the yaml, the state_dict and the optimizer's two groups."""
import os

import numpy as np
import pytest
import torch

from tests import momf_restate as R
from tests.mo_common import FOUR, GOLD, ROOT, fixture_state, my_name, tower_config, trainer_optimizer

TOWER = 2e-5         # per-entry budget of the torch-module tower against the reference's (tests/test_mopool_cpu.py)
CONFIGS = ("c0", "c1")


def _config(D, tune, hidden=()):
    return tower_config(tune, embedding_size=D, mlp_hidden_size=list(hidden), dropout_prob=0)


def stored_state(g, c):
    """The fixture's state_dict of configuration c in its stored key order (the encoder's tensors are stored once)."""
    return {k: torch.from_numpy(g[("enc." if k.startswith("visual_encoder.") else c + ".sd.") + k])
            for k in (str(x) for x in g[c + ".sd.keys"])}


def build_from_fixture(g, c):
    import pixelrec_amd.model as M

    U, I, D = (int(x) for x in g["meta"][:3])

    class DL:
        user_num, item_num = U, I

    m = M.MOMF(_config(D, int(g["meta"][6]), [int(h) for h in g[c + ".hidden"]]), DL())
    m.load_state_dict(fixture_state(g, stored_state(g, c)), strict=True)
    return m


def rec_state(g, c, dtype, stats_after=None):
    """The restatement's P: the state outside the encoder; `stats_after` = j: the BatchNorm statistics batch j left."""
    P = {k: torch.from_numpy(g[c + ".sd." + k]) for k in R.state_names(len(g[c + ".hidden"]))}
    if stats_after is not None:
        for k in (str(x) for x in g[c + ".stats.keys"]):
            P[k] = torch.from_numpy(g[f"{c}.b{stats_after}.stats." + k])
    return {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in P.items()}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "momf_tiny.npz"))


# ------------------------------------------------------------------------------------------------------------ batcher
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from pixelrec_amd.config import Config
    from pixelrec_amd.data import load_data

    d = tmp_path_factory.mktemp("momf")
    (d / "m.yaml").write_text("model: MOMF\nembedding_size: 8\nmlp_hidden_size: []\ndropout_prob: 0\n")
    (d / "o.yaml").write_text(f"seed: 2020\ndata_path: {GOLD}/\ndataset: TinyInter\nMAX_ITEM_LIST_LENGTH: 6\ntrain_batch_size: 4\n"
                              "eval_batch_size: 16\nuse_modality: True\n")
    config = Config([str(d / "m.yaml"), str(d / "o.yaml")])
    data = load_data(config)
    data.build()
    return config, data


def test_batcher_yields_the_pair_batchers_samples_as_positions_into_the_batchs_distinct_images(tiny):
    from pixelrec_amd.data.dataset import MoPairTrainBatcher, PairTrainBatcher

    config, data = tiny
    b, pair = MoPairTrainBatcher(config, data), PairTrainBatcher(config, data)
    assert isinstance(b, PairTrainBatcher) and len(b) == len(pair) and b.n == pair.n
    seen = shared = 0
    for (user, index, image_ids), (user_p, item_p) in zip(b, pair):       # the same seed: the same order and random stream
        B = user.shape[0]
        assert user.dtype == index.dtype == image_ids.dtype == torch.int64 and tuple(index.shape) == (B, 2)
        ids = image_ids.numpy()
        assert (np.diff(ids) > 0).all() and ids[0] >= 1                # strictly ascending (so distinct), no zero image in front
        assert len(ids) <= 2 * B
        assert set(np.unique(index.numpy()).tolist()) == set(range(len(ids)))             # base 0; no image without a reader
        assert torch.equal(user, user_p) and torch.equal(image_ids[index], item_p)        # users, positives and negatives
        shared += int(len(ids) < 2 * B)
        seen += B
    assert seen == pair.n and shared > 0                               # some batch reads an image twice
    first_epoch = [tuple(t.clone() for t in x) for x in b]
    again = [tuple(t.clone() for t in x) for x in b]
    assert all(torch.equal(p, q) for x, y in zip(first_epoch, again) for p, q in zip(x, y))              # same (seed, epoch)
    b.set_epoch(1)
    other = [tuple(t.clone() for t in x) for x in b]
    assert any(p.shape != q.shape or not torch.equal(p, q) for x, y in zip(first_epoch, other) for p, q in zip(x, y))


def test_positions_helper_has_no_zero_row_and_leaves_its_sibling_alone():
    from pixelrec_amd.data.dataset import positions_into_distinct_images, positions_into_distinct_items

    item = np.array([[7, 3], [3, 9], [7, 1]])
    index, image_ids = positions_into_distinct_items(item)
    assert image_ids.tolist() == [1, 3, 7, 9] and index.tolist() == [[2, 1], [1, 3], [2, 0]] and index.dtype == np.int64
    _, with_zero = positions_into_distinct_images(item[:, :1], item)
    assert with_zero.tolist() == [0, 1, 3, 7, 9]                         # the sequence models' helper keeps its zero row


def test_model_is_registered_with_its_batcher_and_the_pair_evaluation(tiny):
    from pixelrec_amd.config import Config
    from pixelrec_amd.data.dataset import MoPairTrainBatcher, PairEvalBatcher
    from pixelrec_amd.data.utils import SUPPORTED, bulid_dataloader
    from pixelrec_amd.utils import get_model
    from pixelrec_amd.utils.enum_type import InputType

    config, data = tiny
    assert SUPPORTED["MOMF"] == "PAIR" and get_model("MOMF").__name__ == "MOMF" and get_model("MOMF").input_type == InputType.PAIR
    train, valid, test = bulid_dataloader(config, data)
    assert isinstance(train.batcher, MoPairTrainBatcher) and isinstance(valid, PairEvalBatcher) and isinstance(test, PairEvalBatcher)
    shipped = Config([os.path.join(ROOT, "configs", "PixelNet", "mf.yaml"), os.path.join(ROOT, "configs", "overall", "ViT.yaml")])
    assert shipped["model"] == "MOMF" and shipped["embedding_size"] == 4096 and shipped["dropout_prob"] == 0
    assert list(shipped["mlp_hidden_size"]) == [] and get_model(shipped["model"]).__name__ == "MOMF"


# ------------------------------------------------------------------------------------------------------------ fixture, restatement
@pytest.mark.parametrize("c", CONFIGS)
def test_fixture_pins_the_composition_on_the_float64_cpu_tower(gold, c):
    """The build's torch-module tower (visual.py's CPU path) in float64 on the fixture's state, then momf_restate in float64 on its
    output -- autograd through both -- against the reference's stored loss, every gradient (the dense user table's included), the
    BatchNorm running statistics after each batch, compute_item and predict: each within its stored ref_err (the reference's own
    float32 distance from float64) plus TOWER."""
    g = gold
    L = len(g[c + ".hidden"])
    m = build_from_fixture(g, c).double().eval()
    store = torch.from_numpy(g["store"].astype(np.float64))
    names = [str(k) for k in g[c + ".param.keys"]]
    stat_keys = [str(k) for k in g[c + ".stats.keys"]]
    rec = R.trainable(R.state_names(L))
    assert names[:len(rec)] == rec and len(names) == len(rec) + 18 and len(stat_keys) == 6 * L
    P = rec_state(g, c, torch.float64)
    for k in rec:
        assert torch.equal(P[k], m.get_parameter(k).detach())
    for j in range(2):
        user, item = g[f"b{j}.user"], g[f"b{j}.item"]
        m.zero_grad()
        Q = {k: (v.clone().requires_grad_(True) if k in rec else v) for k, v in P.items()}
        stats = {}
        loss = R.loss_of(Q, L, m.visual_encoder(store), user, item, stats)      # E = the store's rows: an id IS its row
        loss.backward()
        ref = float(g[f"{c}.b{j}.loss"])
        print(c, "batch", j, "loss", float(loss.detach()), ref, "ref_err", float(g[f"ref_err.{c}.b{j}.loss"]))
        assert abs(float(loss.detach()) - ref) <= TOWER + float(g[f"ref_err.{c}.b{j}.loss"])
        for i, k in enumerate(names):
            got = Q[k].grad if k in Q else m.get_parameter(my_name(k)).grad
            e = float((got - torch.from_numpy(g[f"{c}.b{j}.grad." + k]).double()).abs().max())
            assert e <= TOWER + float(g[f"ref_err.{c}.b{j}.grad"][i]), (k, e)
        for i, k in enumerate(stat_keys):
            e = float((stats[k].double() - torch.from_numpy(g[f"{c}.b{j}.stats." + k]).double()).abs().max())
            assert e <= TOWER + float(g[f"ref_err.{c}.b{j}.stats"][i]), (k, e)
        P.update(stats)
    feat = R.item_features(P, L, m.visual_encoder(store).detach())
    e = float((feat - torch.from_numpy(g[c + ".eval.item_feature"]).double()).abs().max())
    print(c, "item features", e, "ref_err", float(g[f"ref_err.{c}.item_feature"]))
    assert e <= TOWER + float(g[f"ref_err.{c}.item_feature"])
    scores = R.predict(P, L, g["eval.users"], feat)
    e = float((scores - torch.from_numpy(g[c + ".eval.scores"]).double()).abs().max())
    print(c, "scores", e, "ref_err", float(g[f"ref_err.{c}.scores"]))
    assert tuple(scores.shape) == (int(g["meta"][0]), int(g["meta"][1])) and e <= TOWER + float(g[f"ref_err.{c}.scores"])


def test_fixture_batches_hold_the_cases_they_are_there_for(gold):
    g = gold
    U, I, D, B = (int(x) for x in g["meta"][:4])
    assert (U, I, D, B) == (9, 13, 8, 6) and [int(h) for h in g["c0.hidden"]] == [] and [int(h) for h in g["c1.hidden"]] == [12, 8]
    for j in range(2):
        user, item = g[f"b{j}.user"], g[f"b{j}.item"]
        assert user.shape == (B,) and item.shape == (B, 2)
        assert len(set(user.tolist())) < B                                                  # a user that appears twice
        assert len(set(item[:, 0].tolist())) < B                                            # a positive shared by two samples
        assert any(item[b, 0] == item[k, 1] for b in range(B) for k in range(B) if b != k)  # positive here, negative there
        assert (item[:, 0] != item[:, 1]).all() and (item >= 1).all() and int(item.max()) < I and 0 <= int(user.min()) and int(user.max()) < U
    assert float(np.abs(g["store"][0]).max()) == 0
    assert os.path.getsize(os.path.join(GOLD, "momf_tiny.npz")) < 1_000_000


@pytest.mark.parametrize("hidden", [[], [12, 8]])
def test_dedup_does_not_change_the_restated_function(hidden):
    """In float64: the loss on E with shared positions equals the loss on one row per position (E_x[2b + t] = E[index_{b,t}]), and
    the gradient of a row of E that several samples read is the sum of its copies' gradients -- with towers too, because the
    BatchNorm statistics are taken per occurrence in both forms."""
    gen = torch.Generator().manual_seed(len(hidden) + 3)
    U, M, D, B = 7, 9, 8, 6
    L = len(hidden)
    sizes = [D] + hidden
    P = {}
    for k in R.state_names(L):
        if k == R.TABLE:
            P[k] = torch.randn(U, D, generator=gen, dtype=torch.float64) * 0.5
        elif k.endswith("num_batches_tracked"):
            P[k] = torch.zeros((), dtype=torch.int64)
        else:
            layer = int(k.split(".")[2]) // 4
            o, i = sizes[layer + 1], sizes[layer]
            if k.endswith("running_var"):
                P[k] = torch.ones(o, dtype=torch.float64)
            elif int(k.split(".")[2]) % 4 == 1 and k.endswith("weight"):
                P[k] = torch.randn(o, i, generator=gen, dtype=torch.float64) * 0.4
            else:
                P[k] = torch.randn(o, generator=gen, dtype=torch.float64) * 0.1 + (1.0 if k.endswith("2.weight") or k.endswith("6.weight") else 0.0)
    E = torch.randn(M, D, generator=gen, dtype=torch.float64) * 0.5
    user = torch.tensor([0, 3, 3, 5, 1, 6])
    index = torch.tensor([[2, 4], [2, 7], [4, 1], [5, 2], [0, 3], [7, 4]])            # row 2 read three times, 4 three times, 8 never
    loss, grads, _ = R.loss_and_grads(P, L, E, user, index)
    flat = index.view(-1)
    loss_x, grads_x, _ = R.loss_and_grads(P, L, E[flat], user, torch.arange(2 * B).view(B, 2))
    assert abs(loss - loss_x) <= 1e-14
    summed = torch.zeros_like(E).index_add_(0, flat, grads_x[R.E_KEY])
    assert float((grads[R.E_KEY] - summed).abs().max()) <= 1e-14 and float(grads[R.E_KEY][8].abs().max()) == 0
    assert float(grads[R.E_KEY][2].abs().max()) > 0
    for k in R.trainable(list(P)):
        assert float((grads[k] - grads_x[k]).abs().max()) <= 1e-14, k
    assert set(torch.nonzero(grads[R.TABLE].abs().sum(1)).view(-1).tolist()) == set(user.tolist())


# ------------------------------------------------------------------------------------------------------------ model surface
@pytest.mark.parametrize("c", CONFIGS)
def test_state_dict_is_the_references_and_loads_strictly(gold, c):
    g = gold
    m = build_from_fixture(g, c)
    L = len(g[c + ".hidden"])
    keys = list(m.state_dict())
    want = [my_name(str(k)) for k in g[c + ".sd.keys"] if "post_layernorm" not in str(k)]
    n_rec = 7 * 2 * L + 1
    assert keys == want and keys[:n_rec] == R.state_names(L) and keys[n_rec - 1] == "user_embedding.weight"
    assert all(k.startswith("visual_encoder.") for k in keys[n_rec:])
    assert list(m.rec_parameter_names()) == R.trainable(R.state_names(L))               # the towers, then the table
    assert m.rec_parameter_names()["user_embedding.weight"] is None
    assert m.table_parameter_spans() == {"user_embedding.weight": (1, 1 + int(g["meta"][0]))}
    for k, v in fixture_state(g, stored_state(g, c)).items():
        assert torch.equal(m.state_dict()[k], v)
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    assert len(frozen) == int(g["meta"][6]) == len(g["frozen"]) and all("visual_encoder" in n for n in frozen)


def test_fresh_model_is_xavier_normal_before_the_encoder_is_loaded():
    import pixelrec_amd.model as M
    from pixelrec_amd.model.mf import MF, MfTowers

    class DL:
        user_num, item_num = 300, 13

    torch.manual_seed(3)
    m = M.MOMF(_config(64, 37, [80, 40]), DL())
    assert isinstance(m, MfTowers) and issubclass(MF, MfTowers)
    for name, p in list(m.user_mlp_layers.named_parameters()) + list(m.item_mlp_layers.named_parameters()):
        if p.dim() == 2:
            std = (2.0 / sum(p.shape)) ** 0.5
            assert abs(float(p.std()) - std) < 0.15 * std, (name, float(p.std()), std)
        elif name.endswith("bias"):
            assert float(p.abs().max()) == 0
    w = m.user_embedding.weight
    assert tuple(w.shape) == (300, 64) and abs(float(w.std()) - (2.0 / 364) ** 0.5) < 0.05 * (2.0 / 364) ** 0.5
    assert m.out_size == 40 and M.MOMF(_config(64, 37, []), DL()).out_size == 64


@pytest.mark.parametrize("D,hidden", [(10, []), (8, [10]), (8, [12, 0]), (8, [4100]), (4100, [])])
def test_constructor_refuses_widths_the_kernels_cannot_serve(D, hidden):
    import pixelrec_amd.model as M

    class DL:
        user_num, item_num = 9, 13

    with pytest.raises(ValueError):
        M.MOMF(_config(D, 37, hidden), DL())


def test_reference_input_form_maps_to_one_position_per_image():
    import pixelrec_amd.model as M

    user = torch.tensor([4, 1, 4])
    item = torch.arange(3 * 2 * 3 * 2 * 2, dtype=torch.float32).view(3, 2, 3, 2, 2)
    u, index, images = M.MOMF._reference_form(user, item)
    assert index.tolist() == [[0, 1], [2, 3], [4, 5]] and torch.equal(images, item.flatten(0, 1)) and u is user
    with pytest.raises(ValueError):
        M.MOMF._reference_form(user[:2], item)


def test_four_optim_args_give_the_encoder_group_and_a_rec_group_with_the_table(gold):
    from pixelrec_amd.optim import OptimizerGroup, PxrAdamW, VisualAdamW, has_lazy_table, reference_rec_parameter_names, table_spans

    m = build_from_fixture(gold, "c1")
    opt = trainer_optimizer(m, FOUR)
    assert isinstance(opt, OptimizerGroup)
    vis, rec = opt._split()
    assert isinstance(vis, VisualAdamW) and isinstance(rec, PxrAdamW) and rec.has_table is True and has_lazy_table(m)
    assert [len(vis._trainable()), len(reference_rec_parameter_names(m))] == [18, 17]
    assert table_spans(m) == {"user_embedding.weight": (1, 10)}
    assert (vis.param_groups[0]["lr"], vis.param_groups[0]["weight_decay"]) == (1e-4, 0.0)
    assert (rec.param_groups[0]["lr"], rec.param_groups[0]["weight_decay"]) == (3e-4, 0.1)
    one = trainer_optimizer(build_from_fixture(gold, "c0"), {"learning_rate": 2e-4, "weight_decay": 0.05})
    assert isinstance(one, PxrAdamW) and (one.param_groups[0]["lr"], one.param_groups[0]["weight_decay"]) == (2e-4, 0.05)
