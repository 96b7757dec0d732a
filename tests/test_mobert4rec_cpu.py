"""MOBERT4Rec without a GPU: the batcher (BERT4RecTrainBatcher's batches as positions into the batch's distinct images, the mask
token standing for the ones image), the fixture of the reference's own class against the float64 restatement on the torch-module
tower's float64 output (which pins the composition: which row of E an index means, what 0 means, that padded inputs are inert, the
key-padding mask, the mask row in predict), the two input forms of the restatement, the state_dict, the config and the model's
small surfaces."""
import os

import numpy as np
import pytest
import torch

from tests import mobert4rec_restate as R
from tests.mo_common import FOUR, GOLD, ROOT, fixture_state, my_name, tower_config, trainer_optimizer

N_BLOCK = 35          # position_embedding + 2 layers x 16 + LayerNorm x 2


def _config(D, L, tune, heads=2, inner=2, layers=2, p_drop=0.0):
    return tower_config(tune, n_layers=layers, n_heads=heads, embedding_size=D, inner_size=inner, hidden_dropout_prob=p_drop,
                        attn_dropout_prob=p_drop, hidden_act="gelu", layer_norm_eps=1e-12, initializer_range=0.02, mask_ratio=0.6,
                        MAX_ITEM_LIST_LENGTH=L)


def restate_cfg(g):
    return {"n_layers": int(g["meta"][9]), "n_heads": int(g["meta"][7]), "layer_norm_eps": 1e-12, "hidden_act": "gelu"}


def build_from_fixture(g, p_drop=0.0):
    import pixelrec_amd.model as M

    I, D, L = (int(x) for x in g["meta"][:3])

    class DL:
        item_num = I

    m = M.MOBERT4Rec(_config(D, L, int(g["meta"][6]), int(g["meta"][7]), int(g["meta"][8]), int(g["meta"][9]), p_drop), DL())
    m.load_state_dict(fixture_state(g, R.golden_state(g)), strict=True)
    return m


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "mobert4rec_tiny.npz"))


# ------------------------------------------------------------------------------------------------------------ batcher
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from pixelrec_amd.config import Config
    from pixelrec_amd.data import load_data

    d = tmp_path_factory.mktemp("mobert4rec")
    (d / "m.yaml").write_text("model: MOBERT4Rec\nembedding_size: 32\nn_layers: 2\nn_heads: 2\ninner_size: 2\nmask_ratio: 0.6\n")
    (d / "o.yaml").write_text(f"seed: 2020\ndata_path: {GOLD}/\ndataset: TinyInter\nMAX_ITEM_LIST_LENGTH: 6\ntrain_batch_size: 4\n"
                              "eval_batch_size: 16\nuse_modality: True\n")
    config = Config([str(d / "m.yaml"), str(d / "o.yaml")])
    data = load_data(config)
    data.build()
    return config, data


def test_batcher_yields_bert4recs_batches_as_positions_into_the_batchs_distinct_images(tiny):
    from pixelrec_amd.data.dataset import BERT4RecTrainBatcher, MoBert4RecTrainBatcher

    config, data = tiny
    b, ref = MoBert4RecTrainBatcher(config, data), BERT4RecTrainBatcher(config, data)
    assert isinstance(b, BERT4RecTrainBatcher) and len(b) == len(ref) and b.n == ref.n
    I, P = data.item_num, 7
    n_masked = 0
    for (index, masked, image_ids), (items, masked_ref) in zip(b, ref):            # the same seed, epoch and rank
        assert index.dtype == masked.dtype == image_ids.dtype == torch.int64
        assert tuple(index.shape) == (items.shape[0], 3, P) and tuple(masked.shape) == (items.shape[0], P)
        ids = image_ids.numpy()
        assert ids[0] == 0 and ids[1] == I and (np.diff(ids[2:]) > 0).all() and (ids[2:] > 0).all() and (ids[2:] < I).all()
        assert 0 <= int(index.min()) and int(index.max()) < len(ids)
        assert set(np.unique(index.numpy()).tolist()) | {0, 1} == set(range(len(ids)))     # no image listed without a reader
        assert np.array_equal(ids[index.numpy()], items.numpy()) and torch.equal(masked, masked_ref)
        idx, mk = index.numpy(), masked.numpy()
        assert (mk[idx[:, 1] == 0] == 0).all()                                    # padding is never masked
        assert not (idx[:, 1:] == 1).any()                                        # the mask row appears in plane 0 only ...
        assert ((idx[:, 0] == 1) == (mk != 0)).all()                              # ... exactly at the masked positions
        assert ((idx[:, 2] != 0) == (mk != 0)).all()
        it = items.numpy()
        for s in range(len(it)):                                                  # negatives lie outside their sequence
            own = set(it[s, 1][it[s, 1] != 0].tolist())
            assert not own & set(it[s, 2][it[s, 2] != 0].tolist())
        n_masked += int(mk.sum())
    assert n_masked > 0
    first = [tuple(x.clone() for x in t) for t in b]
    again = [tuple(x.clone() for x in t) for t in b]
    assert all(torch.equal(x, y) for s, t in zip(first, again) for x, y in zip(s, t))
    b.set_epoch(1)
    other = [tuple(x.clone() for x in t) for t in b]
    assert any(x[0].shape != y[0].shape or not torch.equal(x[0], y[0]) for x, y in zip(first, other))       # two epochs differ


def test_mapping_puts_the_zero_and_the_mask_row_first_whether_read_or_not():
    from pixelrec_amd.data.dataset import positions_into_distinct_images_masked

    items = np.array([[[0, 5, 9], [0, 5, 3], [0, 0, 7]]])
    index, ids = positions_into_distinct_images_masked(items, 9)
    assert ids.tolist() == [0, 9, 3, 5, 7] and index.tolist() == [[[0, 3, 1], [0, 3, 2], [0, 0, 4]]]
    index, ids = positions_into_distinct_images_masked(np.array([[[4, 2], [4, 2], [0, 0]]]), 9)          # nothing masked, no padding
    assert ids.tolist() == [0, 9, 2, 4] and index.tolist() == [[[3, 2], [3, 2], [0, 0]]]


def test_model_is_registered_with_its_batcher_and_the_sequence_evaluation(tiny):
    from pixelrec_amd.data.dataset import MoBert4RecTrainBatcher, SeqEvalBatcher
    from pixelrec_amd.data.utils import SUPPORTED, bulid_dataloader
    from pixelrec_amd.utils import get_model

    config, data = tiny
    assert SUPPORTED["MOBERT4Rec"] == "SEQ" and get_model("MOBERT4Rec").__name__ == "MOBERT4Rec"
    train, valid, test = bulid_dataloader(config, data)
    assert isinstance(train.batcher, MoBert4RecTrainBatcher) and isinstance(valid, SeqEvalBatcher) and isinstance(test, SeqEvalBatcher)


def test_shipped_yaml_selects_the_class_and_the_batcher():
    from pixelrec_amd.config import Config
    from pixelrec_amd.data.utils import SUPPORTED
    from pixelrec_amd.utils import get_model

    config = Config([os.path.join(ROOT, "configs", "PixelNet", "bert4rec.yaml"), os.path.join(ROOT, "configs", "overall", "ViT.yaml")])
    assert config["model"] == "MOBERT4Rec" and get_model(config["model"]).__name__ == "MOBERT4Rec" and SUPPORTED[config["model"]] == "SEQ"
    got = {k: config[k] for k in ("n_layers", "n_heads", "embedding_size", "inner_size", "hidden_dropout_prob", "attn_dropout_prob",
                                  "hidden_act", "layer_norm_eps", "initializer_range", "mask_ratio")}
    assert got == {"n_layers": 2, "n_heads": 4, "embedding_size": 512, "inner_size": 1, "hidden_dropout_prob": 0.1,
                   "attn_dropout_prob": 0.1, "hidden_act": "gelu", "layer_norm_eps": 1e-12, "initializer_range": 0.02, "mask_ratio": 0.6}
    assert config["use_modality"] and len(config["optim_args"]) == 4


# ------------------------------------------------------------------------------------------------------------ fixture, restatement
def _catalogue(g, dtype):
    store = R.golden_store(g).to(dtype)
    return torch.cat((store, torch.ones_like(store[:1])))           # [store | ones image]: an id IS its row, the mask token too


def test_fixture_pins_the_composition_on_the_float64_cpu_tower(gold):
    """The build's torch-module tower (visual.py's CPU path) in float64 on the fixture's state, then mobert4rec_restate in float64 on
    its output -- autograd through both, each image encoded once, padded inputs reading row 0 -- against the reference's stored
    loss, all 53 gradients, item features and predict: each within its stored ref_err (the reference's own float32 distance from
    float64) plus 1e-12 relative."""
    g = gold
    m = build_from_fixture(g).double().eval()
    cfg = restate_cfg(g)
    cat = _catalogue(g, torch.float64)
    I = int(g["meta"][0])
    blk = R.names(cfg["n_layers"])
    P = {k: m.get_parameter(k) for k in blk}
    feat = m.visual_encoder(cat)
    want = torch.from_numpy(g["eval.item_feature"]).double()
    err = float((feat.detach() - want).abs().max())
    print("item features: float64 CPU tower vs reference", err, "ref_err", float(g["ref_err.item_feature"]))
    assert tuple(feat.shape) == (I + 1, int(g["meta"][1])) and err <= float(g["ref_err.item_feature"]) + 1e-12 * float(want.abs().max())
    assert float(feat.detach()[0].abs().max()) > 0                  # the zero image's encoding is not zero
    names = [str(k) for k in g["param.keys"]]
    assert len(names) == N_BLOCK + 18 and set(blk) <= set(names)
    for j in range(2):
        items, masked = g[f"b{j}.items"], g[f"b{j}.masked_index"]
        m.zero_grad()
        loss = R.loss_of(P, m.visual_encoder(cat), items, masked, cfg)
        loss.backward()
        ref = float(g[f"b{j}.loss"])
        print("batch", j, "loss", float(loss.detach()), ref, "ref_err", float(g[f"ref_err.b{j}.loss"]))
        assert abs(float(loss.detach()) - ref) <= float(g[f"ref_err.b{j}.loss"]) + 1e-12 * abs(ref)
        # (relative to the batch's largest gradient entry: a key bias's gradient cancels to ~1e-11 by the softmax's shift invariance,
        # and two float64 evaluations differ by 2^-53 of the terms that cancel, not of what is left of them)
        scale = max(float(np.abs(g[f"b{j}.grad." + k]).max()) for k in names)
        for k in names:
            got, w = m.get_parameter(my_name(k)).grad, torch.from_numpy(g[f"b{j}.grad." + k]).double()
            e = float((got - w).abs().max())
            assert e <= float(g[f"ref_err.b{j}.grad." + k]) + 1e-12 * scale, (k, e)
        # the reference form (one row per position behind a zero image) and the positional form are one float64 function: the same
        # rows are read and the same terms summed, in another order -> 1e-12 relative
        E = feat.detach()
        it = torch.from_numpy(items)
        rows = torch.cat((E[:1], torch.stack((E[it[:, 0]], E[it[:, 1]], E[it[:, 2]]), dim=2).flatten(0, 2)))
        Pd = {k: v.detach() for k, v in P.items()}
        a = float(R.loss_of(Pd, rows, R.reference_positions(it[:, 0], masked), masked, cfg))
        b = float(R.loss_of(Pd, E, items, masked, cfg))
        assert abs(a - b) <= 1e-12 * max(1.0, abs(b)) and abs(b - float(loss.detach())) <= 1e-12
    win = g["eval.windows"]
    s = R.predict({k: v.detach() for k, v in P.items()}, feat.detach(), win, cfg, I)
    w = torch.from_numpy(g["eval.scores"]).double()
    e = float((s - w).abs().max())
    print("scores", e, "ref_err", float(g["ref_err.scores"]))
    assert tuple(s.shape) == (8, I) and e <= float(g["ref_err.scores"]) + 1e-12 * float(w.abs().max())


def test_fixture_batches_hold_the_cases_they_are_there_for(gold):
    g = gold
    I, P = int(g["meta"][0]), int(g["meta"][2]) + 1
    for j in range(2):
        items, mk = g[f"b{j}.items"], g[f"b{j}.masked_index"]
        assert items.shape == (6, 3, P) and mk.shape == (6, P)
        real = items[:, 1] != 0
        assert sorted(real.sum(1).tolist()) == [2, 3, 4, 4, 5, 5]                           # full, and 1 / 2 / 3 padded positions
        assert (mk[~real] == 0).all() and ((items[:, 0] == I) == (mk != 0)).all() and ((items[:, 2] != 0) == (mk != 0)).all()
        assert any(mk[b].sum() == 0 for b in range(6)) and any(mk[b].sum() == real[b].sum() for b in range(6))
        unmasked_in = [set(items[b, 0][(items[b, 0] != 0) & (items[b, 0] != I)].tolist()) for b in range(6)]
        negs = [set(items[b, 2][items[b, 2] != 0].tolist()) for b in range(6)]
        masked_pos = [set(items[b, 1][mk[b] != 0].tolist()) for b in range(6)]
        assert any(unmasked_in[a] & negs[b] for a in range(6) for b in range(6) if a != b)          # an input here, a negative there
        assert any(masked_pos[a] & unmasked_in[b] for a in range(6) for b in range(6) if a != b)    # a masked positive here, an input there
        for b in range(6):
            assert not negs[b] & set(items[b, 1][real[b]].tolist())
    assert tuple(g["eval.scores"].shape) == (8, I) and tuple(g["eval.item_feature"].shape) == (I + 1, int(g["meta"][1]))
    assert os.path.getsize(os.path.join(GOLD, "mobert4rec_tiny.npz")) < 1_000_000


def test_padded_inputs_are_inert_in_the_restatement():
    """What decision 1 rests on, in float32 and float64: replacing the row that padded inputs read (by its content: in the
    positional form the index is the key mask as well) changes neither the loss bits nor any gradient bit, and that row's own
    gradient is exactly 0."""
    gen = torch.Generator().manual_seed(11)
    D, P, M, cfg = 8, 5, 9, {"n_layers": 2, "n_heads": 2, "layer_norm_eps": 1e-12}
    for dt in (torch.float32, torch.float64):
        prm = {}
        for k in R.names(2):
            if k.startswith("position"):
                shape = (P, D)
            elif "dense_1" in k:
                shape = (2 * D, D) if k.endswith("weight") else (2 * D,)
            elif "dense_2.weight" in k:
                shape = (D, 2 * D)
            else:
                shape = (D, D) if (k.endswith("weight") and "LayerNorm" not in k) else (D,)
            prm[k] = (torch.randn(*shape, generator=gen, dtype=torch.float64) * 0.3).to(dt)
        E = (torch.randn(M, D, generator=gen, dtype=torch.float64) * 0.5).to(dt)
        index = torch.tensor([[[0, 0, 1, 3, 1], [0, 0, 2, 3, 4], [0, 0, 5, 0, 6]], [[0, 1, 4, 1, 2], [0, 3, 4, 5, 2], [0, 6, 0, 7, 0]]])
        masked = (index[:, 2] != 0).long()
        E2 = E.clone()
        E2[0] = E[1] * 1.5 + 0.25                                   # padded positions now read something else
        l0, g0 = R.loss_and_grads(prm, E, index, masked, cfg)
        l1, g1 = R.loss_and_grads(prm, E2, index, masked, cfg)
        assert l0 == l1 and float(g1[R.E_KEY][0].abs().max()) == 0 and float(g0[R.E_KEY][0].abs().max()) == 0
        assert float(g0[R.E_KEY][8].abs().max()) == 0 and float(g0[R.E_KEY][1:8].abs().max(1).values.min()) > 0
        for k in g0:
            assert torch.equal(g0[k], g1[k]), k


# ------------------------------------------------------------------------------------------------------------ model surface
def test_state_dict_is_the_references_and_loads_strictly(gold):
    g = gold
    m = build_from_fixture(g)
    keys = list(m.state_dict())
    want = [my_name(str(k)) for k in g["sd.keys"] if "post_layernorm" not in str(k)]
    blk = R.names(2)
    assert keys == want and keys[-N_BLOCK:] == blk and all(k.startswith("visual_encoder.") for k in keys[:-N_BLOCK])
    assert keys[-N_BLOCK] == "position_embedding.weight" and keys[-2:] == ["LayerNorm.weight", "LayerNorm.bias"]
    assert [n for n, _ in m.named_parameters()] == keys              # no buffer
    assert list(m.rec_parameter_names()) == blk
    for k, v in fixture_state(g, R.golden_state(g)).items():
        assert torch.equal(m.state_dict()[k], v)
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    assert len(frozen) == int(g["meta"][6]) == len(g["frozen"]) and all("visual_encoder" in n for n in frozen)
    assert tuple(m.position_embedding.weight.shape) == (int(g["meta"][2]) + 1, int(g["meta"][1])) and m.mask_token == m.item_num == 13


def test_forward_on_the_cpu_says_hip_device_only(gold):
    from pixelrec_amd.lib import PxrError

    m = build_from_fixture(gold)
    index = torch.zeros(2, 3, 5, dtype=torch.int64)
    with pytest.raises(PxrError, match="HIP device only"):
        m((index, torch.zeros(3, 3, 64, 64), torch.zeros(2, 5, dtype=torch.int64)))
    with pytest.raises(PxrError, match="HIP device only"):
        m.loss_from_embeddings(torch.zeros(3, 32), index, torch.zeros(2, 5, dtype=torch.int64))


def test_extra_item_images_is_one_all_ones_image_and_the_catalogue_needs_its_row(gold):
    m = build_from_fixture(gold)
    img = m.extra_item_images(6, 4, "cpu")
    assert tuple(img.shape) == (1, 3, 6, 4) and img.dtype == torch.float32 and bool((img == 1).all())
    with pytest.raises(ValueError):
        m.encode_last(torch.zeros(2, 4, dtype=torch.int64), torch.zeros(13, 32))           # no mask row
    with pytest.raises(ValueError):
        m.set_item_feature(torch.zeros(13, 32))
    feat = torch.arange(14 * 32, dtype=torch.float32).view(14, 32)
    m.set_item_feature(feat)
    assert torch.equal(m.scoring_item_matrix(), feat[:13])


def test_reference_input_form_maps_to_one_row_per_position_behind_the_zero_image(gold):
    m = build_from_fixture(gold)
    input_ids = torch.tensor([[0, 3, 13, 7, 13], [2, 13, 9, 1, 4]])
    masked = torch.tensor([[0, 0, 1, 0, 1], [0, 1, 0, 0, 0]])
    modal = torch.arange(2 * 15 * 3 * 2 * 2, dtype=torch.float32).view(2, 15, 3, 2, 2)
    index, images = m._reference_form(input_ids, modal, masked)
    assert index.tolist() == [[[0, 4, 7, 10, 13], [0, 0, 8, 0, 14], [0, 0, 9, 0, 15]],
                              [[16, 19, 22, 25, 28], [0, 20, 0, 0, 0], [0, 21, 0, 0, 0]]]
    assert torch.equal(index, R.reference_positions(input_ids, masked))
    assert tuple(images.shape) == (31, 3, 2, 2) and float(images[0].abs().max()) == 0 and torch.equal(images[1:], modal.flatten(0, 1))
    with pytest.raises(ValueError):
        m._reference_form(input_ids, modal[:, :14], masked)


def test_four_optim_args_give_the_encoder_group_and_a_rec_group_without_a_table(gold):
    from pixelrec_amd.optim import OptimizerGroup, PxrAdamW, VisualAdamW, reference_rec_parameter_names

    m = build_from_fixture(gold)
    opt = trainer_optimizer(m, FOUR)
    assert isinstance(opt, OptimizerGroup)
    vis, rec = opt._split()
    assert isinstance(vis, VisualAdamW) and isinstance(rec, PxrAdamW) and rec.has_table is False
    assert [len(vis._trainable()), len(reference_rec_parameter_names(m))] == [18, N_BLOCK]
    assert reference_rec_parameter_names(m) == R.names(2)
    assert (vis.param_groups[0]["lr"], vis.param_groups[0]["weight_decay"]) == (1e-4, 0.0)
    assert (rec.param_groups[0]["lr"], rec.param_groups[0]["weight_decay"]) == (3e-4, 0.1)
