"""BERT4Rec without a GPU: the test-side restatement (tests/bert4rec_restate.py) against the golden vectors the reference's own
BERT4Rec produced (tools/make_golden_bert4rec.py -> tests/golden/bert4rec_tiny.npz), the model contract (state_dict keys, the
registry), and properties of the host batcher (pixelrec_amd/data/dataset.py BERT4RecTrainBatcher)."""
import os
import random

import numpy as np
import pytest
import torch

from tests import bert4rec_restate as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bert4rec_tiny.npz")


def _golden():
    z = np.load(GOLDEN, allow_pickle=False)
    meta = dict(zip(("item_num", "D", "L", "H", "inner", "n_layers", "B", "seed"), [int(x) for x in z["meta"]]))
    return meta, z


def _cfg(meta):
    return {"n_layers": meta["n_layers"], "n_heads": meta["H"], "layer_norm_eps": 1e-12}


def test_golden_fixture_covers_the_edge_cases():
    meta, z = _golden()
    items, mask = z["items"], z["masked_index"]
    P, tok = meta["L"] + 1, meta["item_num"]
    assert items.shape == (meta["B"], 3, P) and mask.shape == (meta["B"], P)
    assert (items[:, 1] == 0).any() and (mask.sum(1) == 0).any()          # padded windows; one without a masked position
    assert ((items[:, 0] == tok) == (mask == 1)).all()
    g = z["grad.item_embedding.weight"]
    assert np.abs(g[0]).max() == 0 and np.abs(g[tok]).max() > 0            # row 0 untouched, the mask-token row trained


def test_restatement_matches_reference_loss_and_gradients():
    meta, z = _golden()
    p = R.golden_params(z)
    loss, g = R.loss_and_grads(p, torch.from_numpy(z["items"]), torch.from_numpy(z["masked_index"]), _cfg(meta))
    assert abs(float(loss) - float(z["loss"])) <= 1e-6 * max(1.0, abs(float(z["loss"])))
    for k, v in g.items():
        ref = torch.from_numpy(z["grad." + k])
        assert (v - ref).abs().max().item() <= 1e-7 + 1e-5 * ref.abs().max().item(), k


def test_restatement_matches_reference_predict_and_adamw():
    meta, z = _golden()
    p = R.golden_params(z)
    feat = p["item_embedding.weight"][:meta["item_num"]]
    scores = R.predict(p, torch.from_numpy(z["eval.item_seq"]), feat, _cfg(meta), meta["item_num"])
    assert (scores - torch.from_numpy(z["eval.scores"])).abs().max().item() <= 1e-5
    batches = [(torch.from_numpy(i), torch.from_numpy(m)) for i, m in zip(z["adamw.items"], z["adamw.masks"])]
    losses, final = R.adamw_trajectory(p, batches, _cfg(meta))
    for s, l in enumerate(losses):
        assert abs(l - float(z[f"adamw.loss{s}"])) <= 1e-5 * max(1.0, abs(l))
    for k, v in final.items():
        assert (v - torch.from_numpy(z["adamw.final." + k])).abs().max().item() <= 1e-6, k


def _model_cfg(meta):
    return {"n_layers": meta["n_layers"], "n_heads": meta["H"], "embedding_size": meta["D"], "inner_size": meta["inner"],
            "hidden_dropout_prob": 0.0, "attn_dropout_prob": 0.0, "hidden_act": "gelu", "layer_norm_eps": 1e-12,
            "initializer_range": 0.02, "MAX_ITEM_LIST_LENGTH": meta["L"], "mask_ratio": 0.4, "seed": 2020}


def test_model_state_dict_keys_and_shapes_are_the_references():
    from pixelrec_amd.model import BERT4Rec
    from pixelrec_amd.utils import get_model

    meta, z = _golden()

    class DL:
        item_num = meta["item_num"]

    m = BERT4Rec(_model_cfg(meta), DL())
    sd = m.state_dict()
    ref = {k[3:]: z[k].shape for k in z.files if k.startswith("sd.")}
    assert set(sd.keys()) == set(ref.keys())
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in ref.items()}
    m.load_state_dict(R.golden_params(z), strict=True)
    assert get_model("BERT4Rec") is BERT4Rec


def test_data_pipeline_registers_bert4rec():
    from pixelrec_amd.data import utils as U

    assert U.SUPPORTED["BERT4Rec"] == "SEQ"


class _DL:
    def __init__(self, seqs, item_num):
        self.item_num = item_num
        self.train_feat = {"item_seq": seqs}


def _batcher(L=20, n=400, item_num=500, ratio=0.3, seed=3):
    from pixelrec_amd.data.dataset import BERT4RecTrainBatcher

    rng = np.random.default_rng(seed)
    seqs = [list(rng.choice(np.arange(1, item_num), size=int(rng.integers(2, L + 2)), replace=False)) for _ in range(n)]
    cfg = {"MAX_ITEM_LIST_LENGTH": L, "train_batch_size": 64, "seed": 7, "mask_ratio": ratio, "device_sampler": None}
    return BERT4RecTrainBatcher(cfg, _DL(seqs, item_num)), seqs


def test_batcher_shapes_dtypes_and_masking_properties():
    b, seqs = _batcher()
    P, N = 21, 500
    n_real = n_masked = 0
    for items, mask in b:
        assert items.dtype == torch.int64 and mask.dtype == torch.int64
        assert items.shape[1:] == (3, P) and mask.shape == (items.shape[0], P)
        it, mk = items.numpy(), mask.numpy().astype(bool)
        inp, pos, neg = it[:, 0], it[:, 1], it[:, 2]
        real = pos != 0
        assert not (mk & ~real).any()                                  # padding is never masked
        assert (inp[mk] == N).all() and (inp[~mk] == pos[~mk]).all()   # masked slots hold the mask token item_num
        assert (neg[mk] != 0).all() and (neg[~mk] == 0).all()          # a negative exactly where masked
        assert ((neg[:, :, None] == pos[:, None, :]).any(-1) & mk).sum() == 0   # negatives outside the sequence
        assert ((neg >= 0) & (neg < N)).all()
        n_real += int(real.sum()); n_masked += int(mk.sum())
    frac = n_masked / n_real
    assert abs(frac - 0.3) < 0.02, frac


def test_batcher_matches_the_reference_dataset_in_distribution():
    """The literal per-sample dataset (the reference's BERT4RecTrainDataset) and the vectorised batcher: same layout, same
    masked fraction."""
    from pixelrec_amd.data.dataset import BERT4RecTrainDataset

    b, seqs = _batcher(ratio=0.6)
    ds = BERT4RecTrainDataset({"MAX_ITEM_LIST_LENGTH": 20, "mask_ratio": 0.6}, _DL(seqs, 500))
    random.seed(0)
    n_real = n_masked = 0
    for i in range(len(ds)):
        items, mask = ds[i]
        assert items.shape == (3, 21) and mask.shape == (21,)
        real = items[1] != 0
        assert not (mask.bool() & ~real).any()
        assert (items[0][mask.bool()] == 500).all()
        n_real += int(real.sum()); n_masked += int(mask.sum())
    assert abs(n_masked / n_real - 0.6) < 0.03
