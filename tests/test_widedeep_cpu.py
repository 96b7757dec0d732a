"""WideDeep without a GPU: the two forms of the float64 restatement (literal reference form; split first layer, cancelled head,
factorised scoring) against each other and against the golden fixture of the reference's own WideDeep, the registry and batcher
wiring, the constructor's and forward's error cases, and the state_dict layout.  Every test needs pixelrec_amd.model.WideDeep."""
import os

import numpy as np
import pytest
import torch

from tests import widedeep_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "widedeep_tiny.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


class _Data:
    item_num = 13


def _cfg(D=8, hidden=(12, 4), L=4, p=0):
    return {"embedding_size": D, "mlp_hidden_size": list(hidden), "dropout_prob": p, "MAX_ITEM_LIST_LENGTH": L}


def _model(**kw):
    from pixelrec_amd.model import WideDeep

    return WideDeep(_cfg(**kw), _Data())


def test_fixture_has_the_cases_it_is_meant_to_have(gold):
    from pixelrec_amd.model import WideDeep  # noqa: F401  (the fixture belongs to this model)

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
    assert (gold["grad." + R.DEEP][0] == 0).all() and (gold["grad." + R.WIDE][0] == 0).all()
    assert gold["sd." + R.DEEP][0].any() and gold["sd." + R.WIDE][0].any()         # the init overwrote both padding rows
    assert float(gold["sd." + R.WBIAS][0]) != 0 and float(gold["sd." + R.PRED_B][0]) != 0
    w = gold["eval.windows"]
    assert w.shape == (8, L) and ((w != 0).sum(1) == 0).sum() == 1
    assert [str(k) for k in gold["sd.keys"]] == R.names(2)
    assert gold["sd." + R.lin(0) + ".weight"].shape == (12, (L + 1) * D)            # the first Linear is [(L + 1) D -> h_1]


def _random_state(I, D, L, hidden, g):
    P = {R.WBIAS: torch.randn(1, generator=g, dtype=torch.float64) * 0.3, R.WIDE: torch.randn(I, 1, generator=g, dtype=torch.float64) * 0.3,
         R.DEEP: torch.randn(I, D, generator=g, dtype=torch.float64) * 0.5}
    sizes = [(L + 1) * D] + list(hidden) + [1]
    keys = R.names(len(hidden))
    for i, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        P[keys[3 + 2 * i]] = torch.randn(b, a, generator=g, dtype=torch.float64) * (2.0 / (a + b)) ** 0.5
        P[keys[4 + 2 * i]] = torch.randn(b, generator=g, dtype=torch.float64) * 0.1
    return P


@pytest.mark.parametrize("hidden", [[4], [12, 4], [16, 8, 4]])
def test_the_two_forms_agree_in_float64(hidden, gold):
    """Loss, every gradient and the scores of the literal form and of the native form (split first layer, cancelled head,
    factorised scoring) to 1e-12.  The literal form's gradients of the two cancelled biases are sums of +c_b and -c_b."""
    from pixelrec_amd.model import WideDeep  # noqa: F401

    g = torch.Generator().manual_seed(3 + len(hidden))
    I, D, L = 13, 8, 4
    P = _random_state(I, D, L, hidden, g)
    for rows in gold["rows"][:2]:
        (la, ga), (lb, gb) = R.loss_and_grads(P, rows, "literal"), R.loss_and_grads(P, rows, "native")
        assert abs(la - lb) <= 1e-12
        for k in P:
            assert float((ga[k] - gb[k]).abs().max()) <= 1e-12, k
        assert float(gb[R.WBIAS].abs().max()) == 0 == float(gb[R.PRED_B].abs().max())
        assert float(ga[R.DEEP][0].abs().max()) == 0 == float(ga[R.WIDE][0].abs().max())
        hist = set(rows[:, :L].reshape(-1).tolist()) - set(rows[:, L:].reshape(-1).tolist()) - {0}
        assert hist and all(float(ga[R.WIDE][i].abs().max()) <= 1e-15 for i in hist)   # a history-only item: no wide gradient
    win = gold["eval.windows"]
    lit, fac = R.predict_literal(P, win), R.predict_factorised(P, win)
    assert float((lit - fac).abs().max()) <= 1e-12


def test_float64_restatement_matches_the_golden_fixture(gold):
    """The reference ran in float32: its distance from the float64 restatement is float32 rounding (a few 1e-7 on scores of
    magnitude 3); 2e-6 relative is far below any mistake in the arithmetic.  Both forms are compared.
    The trajectory's final weights are the exception.  Adam divides a gradient by (its running magnitude + eps 1e-8), so an entry
    whose gradient is 0 or of the order of eps in exact arithmetic -- the two cancelled biases, a wide entry that is only ever a
    history item (a sum of +c_b and -c_b), first-layer weights behind a ReLU that is almost always off -- moves by up to lr per
    step on float32 rounding residue and hardly at all in float64 (measured here: 4.3e-6 on the first Linear's weight, 7.0e-6 on
    wide_bias against the native form, which does not move it).  The yardstick for the final weights is therefore the reference's
    own float32 error: twice the distance of the float32 literal restatement from float64 on the same batches, or 1e-6 relative
    if that is larger; and never more than Adam's own bound of lr per step."""
    from pixelrec_amd.model import WideDeep  # noqa: F401

    lr, wd = (float(x) for x in gold["optim"])
    P32 = R.state_from(gold, "sd.", torch.float32)
    R.adamw(P32, list(gold["rows"]), lr, wd, "literal")
    for form in ("literal", "native"):
        P = R.state_from(gold, "sd.", torch.float64)
        loss, g = R.loss_and_grads(P, gold["rows"][0], form)
        assert abs(loss - float(gold["loss"])) <= 1e-6
        for k in R.names(2):
            ref = gold["grad." + k]
            assert np.abs(g[k].numpy() - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()), k
        s = (R.predict_literal if form == "literal" else R.predict_factorised)(P, gold["eval.windows"])
        ref = torch.from_numpy(gold["eval.scores"]).double()
        assert float((s - ref).abs().max()) <= 2e-6 * float(ref.abs().max())
        losses = R.adamw(P, list(gold["rows"]), lr, wd, form)
        for i, v in enumerate(losses):
            assert abs(v - float(gold[f"adamw.loss{i}"])) <= 1e-6
        for k in R.names(2):
            ref = gold["adamw.final." + k]
            d32 = float((P32[k].double() - P[k]).abs().max())
            err = np.abs(P[k].numpy() - ref).max()
            print(form, k, "error", err, "float32 restatement", d32)
            assert err <= max(1e-6 * max(1.0, np.abs(ref).max()), 2 * d32), k
            assert err <= 4 * lr                                                   # Adam moves an entry by at most lr per step
        # row 0 of both tables is decayed though it never gets a gradient: 4 steps of p <- p (1 - lr wd)
        for k in (R.DEEP, R.WIDE):
            r0 = torch.from_numpy(gold["sd." + k][0]).double() * (1 - lr * wd) ** 4
            assert float((P[k][0] - r0).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------------------ wiring
CFG = {"MAX_ITEM_LIST_LENGTH": 4, "train_batch_size": 7, "eval_batch_size": 5, "seed": 11, "device_sampler": None,
       "eval_vectorized": None, "eval_num_workers": 0}


def test_widedeep_is_registered_and_the_yaml_parses():
    from pixelrec_amd.config.configurator import Config
    from pixelrec_amd.data.dataset import CuratorTrainBatcher, SeqEvalBatcher
    from pixelrec_amd.data.utils import SUPPORTED, bulid_dataloader
    from pixelrec_amd.model import WideDeep
    from pixelrec_amd.utils.enum_type import InputType
    from pixelrec_amd.utils.utils import get_model
    from tests.test_din_cpu import _Synth

    assert SUPPORTED["WideDeep"] == "SEQ" and WideDeep.input_type == InputType.SEQ and get_model("WideDeep") is WideDeep
    data = _Synth()
    train, valid, test = bulid_dataloader(dict(CFG, model="WideDeep"), data)
    assert type(train.batcher) is CuratorTrainBatcher and type(valid) is SeqEvalBatcher and type(test) is SeqEvalBatcher
    # one sample per chunk: the chunk without its last item, the last item, a negative outside the chunk
    chunks = [[int(i) for i in s] for s in data.train_feat["item_seq"]]
    got = []
    for prof, target in train:
        assert prof.dtype == target.dtype == torch.int64 and prof.shape[1] == 4 and target.shape[1] == 2
        for p, (pos, neg) in zip(prof.tolist(), target.tolist()):
            chunk = [i for i in p if i] + [pos]
            got.append(chunk)
            assert 1 <= neg < data.item_num and neg not in chunk
    assert sorted(got) == sorted(chunks)
    c = Config([os.path.join(ROOT, "configs/IDNet/widedeep.yaml"), os.path.join(ROOT, "configs/overall/ID.yaml")])
    assert c["model"] == "WideDeep" and c["embedding_size"] == 64 and list(c["mlp_hidden_size"]) == [128, 64] and c["dropout_prob"] == 0
    assert c["MAX_ITEM_LIST_LENGTH"] == 10 and dict(c["optim_args"]) == {"learning_rate": 1e-4, "weight_decay": 0.1}
    assert c["MODEL_INPUT_TYPE"] == InputType.SEQ


def test_constructor_and_forward_error_cases():
    from pixelrec_amd.model import WideDeep

    for hidden in ([], [6], [12, 5], [4100], [0]):
        with pytest.raises(ValueError):
            WideDeep(_cfg(hidden=hidden), _Data())
    for D in (0, 6, 4100):
        with pytest.raises(ValueError):
            WideDeep(_cfg(D=D), _Data())
    with pytest.raises(NotImplementedError):
        WideDeep(_cfg(p=0.1), _Data())
    m = _model().train()
    m._ensure_packed = lambda: None                          # the checks below come before anything touches the device
    inp = R.planes(torch.tensor([[0, 3, 4, 5, 6, 7], [1, 2, 3, 4, 8, 9]]))
    bad = inp.clone()
    bad[1, 1, 2] = 11                                        # the negative's plane holds another profile
    with pytest.raises(ValueError, match="same profile"):
        m(bad)
    with pytest.raises(ValueError):
        m(inp[:, :1])                                        # one plane
    with pytest.raises(ValueError, match="MAX_ITEM_LIST_LENGTH"):
        m((torch.zeros(2, 5, dtype=torch.int64), torch.ones(2, 2, dtype=torch.int64)))


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
    assert torch.equal(m.deep_item_embedding.weight.data, sd[R.DEEP]) and torch.equal(m.wide_item_embedding.weight.data, sd[R.WIDE])
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != R.PRED_B}, strict=True)
    assert list(_model(hidden=(16,)).state_dict().keys()) == R.names(1)
    assert list(_model(hidden=(16, 8, 4)).state_dict().keys()) == R.names(3)
    assert list(m.table_parameter_spans()) == [R.DEEP] and m.table_parameter_spans()[R.DEEP] == (1, 14)


def test_init_is_xavier_normal_with_zero_biases_and_nonzero_padding_rows():
    torch.manual_seed(0)

    class Big:
        item_num = 4001

    from pixelrec_amd.model import WideDeep

    m = WideDeep(_cfg(D=64, hidden=(128, 64), L=10), Big())
    sd = m.state_dict()
    for k, v in sd.items():
        if k.endswith("bias"):
            assert float(v.abs().max()) == 0, k
        else:
            fan_out, fan_in = v.shape
            std = (2.0 / (fan_in + fan_out)) ** 0.5
            if v.numel() >= 4000:
                assert abs(float(v.std()) / std - 1) < 0.05, k
    assert sd[R.DEEP][0].abs().max() > 0 and sd[R.WIDE][0].abs().max() > 0
    assert sd[R.lin(0) + ".weight"].shape == (128, 11 * 64)
