"""MODIN without a GPU: the batcher (CuratorTrainBatcher's samples as positions into the batch's distinct images), the fixture of
the reference's own class against the float64 restatement on the torch-module tower's float64 output (which pins the composition:
which row of E an index means, what 0 means, the mask, 1 / sqrt(D), the absence of a regulariser), the restatement against DIN's,
the state_dict, the constructor's limits and the optimizer's two groups."""
import os

import numpy as np
import pytest
import torch

from tests import din_restate as DR
from tests import modin_restate as R
from tests.mo_common import FOUR, GOLD, fixture_state, my_name, tower_config, trainer_optimizer

TOWER = 2e-5         # per-entry budget of the torch-module tower against the reference's (tests/test_mopool_cpu.py)


def _config(D, L, tune, hidden=(12, 4)):
    return tower_config(tune, embedding_size=D, mlp_hidden_size=list(hidden), dropout_prob=0, MAX_ITEM_LIST_LENGTH=L)


def build_from_fixture(g):
    import pixelrec_amd.model as M

    I, D, L = (int(x) for x in g["meta"][:3])

    class DL:
        item_num = I

    m = M.MODIN(_config(D, L, int(g["meta"][6]), [int(h) for h in g["hidden"]]), DL())
    m.load_state_dict(fixture_state(g), strict=True)
    return m


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "modin_tiny.npz"))


# ------------------------------------------------------------------------------------------------------------ batcher
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from pixelrec_amd.config import Config
    from pixelrec_amd.data import load_data

    d = tmp_path_factory.mktemp("modin")
    (d / "m.yaml").write_text("model: MODIN\nembedding_size: 8\nmlp_hidden_size: [12, 4]\ndropout_prob: 0\n")
    (d / "o.yaml").write_text(f"seed: 2020\ndata_path: {GOLD}/\ndataset: TinyInter\nMAX_ITEM_LIST_LENGTH: 6\ntrain_batch_size: 4\n"
                              "eval_batch_size: 16\nuse_modality: True\n")
    config = Config([str(d / "m.yaml"), str(d / "o.yaml")])
    data = load_data(config)
    data.build()
    return config, data


def test_batcher_yields_curators_samples_as_positions_into_the_batchs_distinct_images(tiny):
    from pixelrec_amd.data.dataset import CuratorTrainBatcher, MoTowerTrainBatcher

    config, data = tiny
    b, cur = MoTowerTrainBatcher(config, data), CuratorTrainBatcher(config, data)
    assert isinstance(b, CuratorTrainBatcher) and len(b) == len(cur) and b.n == cur.n
    L, bs = 6, 4
    order = cur._indices()
    assert np.array_equal(b._indices(), order)
    rng = np.random.default_rng([2020, 0, 0])                      # (seed, epoch, rank)
    seen = 0
    for k, (index, image_ids) in enumerate(b):
        rows = order[k * bs:(k + 1) * bs]
        assert index.dtype == torch.int64 and image_ids.dtype == torch.int64 and tuple(index.shape) == (len(rows), L + 2)
        ids = image_ids.numpy()
        assert ids[0] == 0 and (np.diff(ids) > 0).all()            # 0 first, the rest strictly ascending (so distinct)
        assert 0 <= int(index.min()) and int(index.max()) < len(ids)
        assert set(np.unique(index.numpy()).tolist()) | {0} == set(range(len(ids)))        # no image listed without a reader
        profile, target = cur.make_batch(rows, rng)                # the same chunks, the same rng stream
        items = ids[index.numpy()]
        assert np.array_equal(items[:, :L], profile) and np.array_equal(items[:, L:], target)
        assert (items[:, L:] >= 1).all()
        seen += len(rows)
    assert seen == cur.n
    first_epoch = [(i.clone(), j.clone()) for i, j in b]
    again = [(i.clone(), j.clone()) for i, j in b]
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(first_epoch, again))     # same (seed, epoch)
    b.set_epoch(1)
    other = [(i.clone(), j.clone()) for i, j in b]
    assert any(x[0].shape != y[0].shape or not torch.equal(x[0], y[0]) for x, y in zip(first_epoch, other))  # two epochs differ


def test_model_is_registered_with_its_batcher_and_the_sequence_evaluation(tiny):
    from pixelrec_amd.data.dataset import MoTowerTrainBatcher, SeqEvalBatcher
    from pixelrec_amd.data.utils import SUPPORTED, bulid_dataloader
    from pixelrec_amd.utils import get_model

    config, data = tiny
    assert SUPPORTED["MODIN"] == "SEQ" and get_model("MODIN").__name__ == "MODIN"
    train, valid, test = bulid_dataloader(config, data)
    assert isinstance(train.batcher, MoTowerTrainBatcher) and isinstance(valid, SeqEvalBatcher) and isinstance(test, SeqEvalBatcher)


# ------------------------------------------------------------------------------------------------------------ fixture, restatement
def test_fixture_pins_the_composition_on_the_float64_cpu_tower(gold):
    """The build's torch-module tower (visual.py's CPU path) in float64 on the fixture's state, then modin_restate in float64 on its
    output -- autograd through both -- against the reference's stored loss, all 24 gradients, item features and predict: each
    within its stored ref_err (the reference's own float32 distance from float64) plus TOWER."""
    g = gold
    m = build_from_fixture(g).double().eval()
    store = torch.from_numpy(g["store"].astype(np.float64))
    att = R.names(len(g["hidden"]))
    P = {k: m.get_parameter(k) for k in att}
    feat = m.visual_encoder(store)
    err = float((feat.detach() - torch.from_numpy(g["eval.item_feature"]).double()).abs().max())
    print("item features: float64 CPU tower vs reference", err, "ref_err", float(g["ref_err.item_feature"]))
    assert err <= TOWER + float(g["ref_err.item_feature"])
    assert float(feat.detach()[0].abs().max()) > 0                  # the zero image's encoding is not zero
    names = [str(k) for k in g["param.keys"]]
    assert len(names) == 24 and names[:6] == att
    for j in range(2):
        items = g[f"b{j}.items"]
        m.zero_grad()
        loss = R.loss_of(P, m.visual_encoder(store), items)         # E = the store's rows: an id IS its row, 0 the zero image
        loss.backward()
        ref = float(g[f"b{j}.loss"])
        print("batch", j, "loss", float(loss), ref, "ref_err", float(g[f"ref_err.b{j}.loss"]))
        assert abs(float(loss) - ref) <= TOWER + float(g[f"ref_err.b{j}.loss"])
        for k in names:
            got, want = m.get_parameter(my_name(k)).grad, torch.from_numpy(g[f"b{j}.grad." + k]).double()
            e = float((got - want).abs().max())
            assert e <= TOWER + float(g[f"ref_err.b{j}.grad." + k]), (k, e)
        # the regulariser DIN adds is absent: with it the loss would sit 0.01 ||emb||_2 / B higher, far outside the budget
        emb = feat.detach()[torch.from_numpy(items)]
        assert 0.01 * float(torch.norm(emb, 2)) / len(items) > 100 * (TOWER + float(g[f"ref_err.b{j}.loss"]))
    win = g["eval.windows"]
    with torch.no_grad():
        P64 = {k: v.detach() for k, v in P.items()}
        s_ref_form = R.predict(P64, feat.detach(), R.reference_form(win, feat.shape[0]))
        s_windows = R.predict(P64, feat.detach(), win)
    assert torch.equal(s_ref_form, s_windows)                       # the two input forms of predict are one function
    e = float((s_ref_form - torch.from_numpy(g["eval.scores"]).double()).abs().max())
    print("scores", e, "ref_err", float(g["ref_err.scores"]))
    assert e <= TOWER + float(g["ref_err.scores"])
    assert float(s_ref_form[5].abs().max()) == 0                    # the all-padding window


def test_fixture_batches_hold_the_cases_they_are_there_for(gold):
    g = gold
    L = int(g["meta"][2])
    for j in range(2):
        items = g[f"b{j}.items"]
        prof, tgt = items[:, :L], items[:, L:]
        assert sorted((prof != 0).sum(1).tolist()) == [0, 1, 2, 3, 4, 4]                    # full, 1..3 pads, all padding
        assert any(len(set(r[r != 0].tolist())) < int((r != 0).sum()) for r in prof)        # a repeat inside a profile
        assert set(prof[prof != 0].tolist()) & set(tgt.reshape(-1).tolist())                # history here, target there
        assert any(int(t[0]) in set(p.tolist()) for p, t in zip(prof, tgt))                 # a positive in its own profile
        assert (tgt != 0).all() and (tgt[:, 0] != tgt[:, 1]).all() and int(items.max()) < int(g["meta"][0])
    assert (g["eval.windows"][5] == 0).all() and tuple(g["eval.scores"].shape) == (8, int(g["meta"][0]))
    assert os.path.getsize(os.path.join(GOLD, "modin_tiny.npz")) < 1_000_000


def test_restatement_is_dins_loss_without_the_regulariser():
    """modin_restate.loss + 0.01 ||emb||_2 / B == din_restate.loss_of on a table equal to E, in float64 to 1e-12 (both read row 0
    as it stands at a padded position and mask it afterwards)."""
    gen = torch.Generator().manual_seed(5)
    M, D, hidden = 9, 8, [12, 4]
    sizes = [4 * D] + hidden + [1]
    P = {}
    for i, k in enumerate(R.names(len(hidden))):
        a, b = sizes[i // 2], sizes[i // 2 + 1]
        P[k] = (torch.randn(b, a, generator=gen, dtype=torch.float64) * 0.3) if k.endswith("weight") else torch.randn(b, generator=gen, dtype=torch.float64) * 0.1
    E = torch.randn(M, D, generator=gen, dtype=torch.float64) * 0.5
    rows = torch.tensor([[1, 2, 3, 4, 5, 6], [0, 2, 2, 7, 7, 1], [0, 0, 0, 0, 3, 4], [0, 0, 0, 5, 5, 2]])
    mine = float(R.loss_of(P, E, rows))
    emb = E[rows]
    theirs = float(DR.loss_of({**P, DR.TABLE: E}, rows))
    assert abs(mine + 0.01 * float(torch.norm(emb, 2)) / rows.shape[0] - theirs) <= 1e-12
    loss, grads = R.loss_and_grads(P, E, rows)
    assert loss == mine and set(grads) == set(P) | {R.E_KEY} and float(grads[R.E_KEY][8].abs().max()) == 0
    assert float(grads[R.E_KEY][0].abs().max()) == 0                # row 0 is read under the mask only: no gradient


# ------------------------------------------------------------------------------------------------------------ model surface
def test_state_dict_is_the_references_and_loads_strictly(gold):
    g = gold
    m = build_from_fixture(g)
    keys = list(m.state_dict())
    want = [my_name(str(k)) for k in g["sd.keys"] if "post_layernorm" not in str(k)]
    assert keys == want and keys[:6] == R.names(2) and all(k.startswith("visual_encoder.") for k in keys[6:])
    assert [n for n, _ in m.named_parameters()] == keys              # no buffer
    assert list(m.rec_parameter_names()) == keys[:6]                 # the attention tensors only: no table entry
    for k, v in fixture_state(g).items():
        assert torch.equal(m.state_dict()[k], v)
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    assert len(frozen) == int(g["meta"][6]) == len(g["frozen"]) and all("visual_encoder" in n for n in frozen)


def test_fresh_attention_is_xavier_normal_with_zero_biases():
    import pixelrec_amd.model as M

    class DL:
        item_num = 13

    torch.manual_seed(3)
    m = M.MODIN(_config(64, 10, 37, [80, 40]), DL())
    for name, p in m.attention.named_parameters():
        if name.endswith("bias"):
            assert float(p.abs().max()) == 0
        else:
            out_f, in_f = p.shape
            std = (2.0 / (in_f + out_f)) ** 0.5
            assert abs(float(p.std()) - std) < 0.15 * std + (0.5 * std if p.numel() < 100 else 0), (name, float(p.std()), std)
    assert m.dropout_prob == 0 and m.mlp_hidden_size == [80, 40] and m.fused_topk_supported is True


@pytest.mark.parametrize("D,hidden", [(8, []), (8, [10]), (8, [12, 0]), (10, [12, 4]), (8, [4100])])
def test_constructor_refuses_widths_the_kernels_cannot_serve(D, hidden):
    import pixelrec_amd.model as M

    class DL:
        item_num = 13

    with pytest.raises(ValueError):
        M.MODIN(_config(D, 4, 37, hidden), DL())


def test_reference_input_form_maps_to_positions_behind_the_zero_image():
    import pixelrec_amd.model as M

    items = torch.tensor([[0, 3, 5, 7], [2, 2, 9, 1]])
    modal = torch.arange(2 * 4 * 3 * 2 * 2, dtype=torch.float32).view(2, 4, 3, 2, 2)
    index, images = M.MODIN._reference_form(modal, items)
    assert index.tolist() == [[0, 2, 3, 4], [5, 6, 7, 8]]            # 1 + b (L + 2) + j where items != 0, else 0
    assert tuple(images.shape) == (9, 3, 2, 2) and float(images[0].abs().max()) == 0 and torch.equal(images[1:], modal.flatten(0, 1))
    with pytest.raises(ValueError):
        M.MODIN._reference_form(modal, items[:, :3])


def test_four_optim_args_give_the_encoder_group_and_a_rec_group_without_a_table(gold):
    from pixelrec_amd.optim import OptimizerGroup, PxrAdamW, VisualAdamW, has_lazy_table, reference_rec_parameter_names

    m = build_from_fixture(gold)
    opt = trainer_optimizer(m, FOUR)
    assert isinstance(opt, OptimizerGroup)
    vis, rec = opt._split()
    assert isinstance(vis, VisualAdamW) and isinstance(rec, PxrAdamW) and rec.has_table is False and not has_lazy_table(m)
    assert [len(vis._trainable()), len(reference_rec_parameter_names(m))] == [18, 6]
    assert (vis.param_groups[0]["lr"], vis.param_groups[0]["weight_decay"]) == (1e-4, 0.0)
    assert (rec.param_groups[0]["lr"], rec.param_groups[0]["weight_decay"]) == (3e-4, 0.1)
    one = trainer_optimizer(build_from_fixture(gold), {"learning_rate": 2e-4, "weight_decay": 0.05})
    assert isinstance(one, PxrAdamW) and (one.param_groups[0]["lr"], one.param_groups[0]["weight_decay"]) == (2e-4, 0.05)
