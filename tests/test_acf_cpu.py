"""ACF without a GPU: the float64 restatement against the reference's golden fixture (and what it shows about the two `w` biases
and the empty profile), the batchers against literal per-sample loops, the model's construction, state_dict layout and errors,
and the shipped YAML."""
import os

import numpy as np
import pytest
import torch

from tests import acf_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "acf_tiny.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_has_the_cases_it_is_meant_to_have(gold):
    L = int(gold["meta"][6])
    for rows in gold["rows"]:
        prof, pos, neg, uid = rows[:, :L], rows[:, L], rows[:, L + 1], rows[:, L + 2]
        assert len(set(uid.tolist())) < len(uid) and 0 in uid                     # a repeated user, user 0
        assert set(prof[prof != 0].tolist()) & set(pos.tolist()) & set(neg.tolist())   # profile / positive / negative of three rows
        assert (prof == 0).all(1).any() and (prof != 0).all(1).any()              # an empty and a full profile
        assert any(len(set(p[p != 0].tolist())) < int((p != 0).sum()) for p in prof)   # the same item twice in one profile
        assert (pos != neg).all() and (pos != 0).all() and (neg != 0).all()


def test_float64_restatement_matches_the_golden_fixture(gold):
    """Bounds: float32 rounding of the reference's own float32 run (a chain of five GEMMs and two softmaxes at magnitudes <= 1:
    1e-6 absolute on the loss and relative to the largest entry on the gradients)."""
    P = R.state_from(gold, "sd.")
    v, rows = gold["v_feat"], gold["rows"]
    L, grads = R.loss_and_grads(P, v, rows[0])
    assert abs(L - float(gold["loss"])) <= 1e-6
    assert set(grads) == set(R.NAMES) and len(R.NAMES) == 18
    for k, g in grads.items():
        ref = gold["grad." + k]
        assert np.abs(g.numpy() - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()), k
    assert np.abs(gold["grad.item_model.weight"][0]).max() == 0                   # the padding row never receives a gradient
    for k in R.BOUNDED:                                                           # zero in exact arithmetic, noise in float32
        assert np.abs(gold["grad." + k]).max() <= 1e-7 and grads[k].abs().max() <= 1e-15
    scores = R.predict(P, v, gold["eval.windows"]).numpy()
    assert np.abs(scores - gold["eval.scores"]).max() <= 1e-5
    lr, wd = (float(x) for x in gold["hyper"])
    losses, _, _ = R.adamw(P, v, list(rows), lr, wd)
    for s, Ls in enumerate(losses):
        assert abs(Ls - float(gold[f"adamw.loss{s}"])) <= 2e-6, s


def test_the_two_w_biases_change_no_output(gold):
    P = R.state_from(gold, "sd.")
    v, rows, win = gold["v_feat"], gold["rows"][0], gold["eval.windows"]
    L0, s0 = float(R.loss(P, v, rows)), R.predict(P, v, win)
    for k in R.BOUNDED:
        P[k] = P[k] + 1.0
    L1, s1 = float(R.loss(P, v, rows)), R.predict(P, v, win)
    assert abs(L1 - L0) <= 1e-14 and (s1 - s0).abs().max() <= 1e-13               # the softmax's own rounding


def test_an_empty_profile_is_finite_and_gives_alpha_no_gradient(gold):
    P = R.state_from(gold, "sd.")
    L = int(gold["meta"][6])
    rows = torch.from_numpy(gold["rows"][0])
    empty = rows[(rows[:, :L] == 0).all(1)][:1]
    assert len(empty) == 1
    user, beta, alpha = R.user_vectors(P, gold["v_feat"], empty[:, :L], empty[:, -1], want=True)
    assert torch.isfinite(user).all() and (alpha == 0).all()
    Lv, g = R.loss_and_grads(P, gold["v_feat"], empty)
    assert np.isfinite(Lv) and all(torch.isfinite(x).all() for x in g.values())
    # alpha's operands: w_p, w_x, w and everything below w_x(pooled) get exactly nothing from this row
    for k in R.NAMES:
        if any(t in k for t in ("w_p.", "user_model.w_x.", "user_model.w.", "feats.")):
            assert g[k].abs().max() == 0, k
    assert g["user_model.w_u.weight"].abs().max() > 0


# ------------------------------------------------------------------------------------------------------------ batchers
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


CFG = {"MAX_ITEM_LIST_LENGTH": 4, "train_batch_size": 7, "eval_batch_size": 5, "seed": 11}


def _literal_samples(data, L):
    out = []
    for uid, seq in zip(data.train_feat["user_id"], data.train_feat["item_seq"]):
        seq = [int(i) for i in seq]
        for j, item in enumerate(seq):
            prof = seq[:j] + seq[j + 1:]
            out.append((tuple([0] * (L - len(prof)) + prof), item, int(uid)))
    return out


def test_train_batcher_matches_a_literal_per_sample_loop():
    from pixelrec_amd.data.dataset import SampleAcfTrainBatcher

    data, L = _Synth(), CFG["MAX_ITEM_LIST_LENGTH"]
    lit = _literal_samples(data, L)
    chunks = {(int(u), int(i)): set(int(x) for x in s) for u, s in zip(data.train_feat["user_id"], data.train_feat["item_seq"]) for i in s}
    assert any(len(s) == 1 for s in data.train_feat["item_seq"])                  # single-item chunks exist in the synthetic data
    for epoch in (0, 1):
        b = SampleAcfTrainBatcher(CFG, data)
        b.set_epoch(epoch)
        assert b.n == len(lit) == sum(len(s) for s in data.train_feat["item_seq"])
        got = []
        for prof, tail in b:
            assert prof.dtype == tail.dtype == torch.int64 and prof.shape[1] == L and tail.shape[1] == 3
            for p, (pos, neg, uid) in zip(prof.tolist(), tail.tolist()):
                got.append((tuple(p), pos, uid))
                assert 1 <= neg < data.item_num and neg not in chunks[(uid, pos)]
        assert sorted(got) == sorted(lit)
        assert any(all(x == 0 for x in p) for p, _, _ in got)                     # the empty profiles are kept
    # rank split: disjoint and complete (padding by wrapping may repeat a few samples, as DistributedSampler does)
    parts = []
    for r in range(3):
        b = SampleAcfTrainBatcher(CFG, data, rank=r, world=3)
        parts.append([(tuple(p), t[0], t[2]) for prof, tail in b for p, t in zip(prof.tolist(), tail.tolist())])
    assert len({len(p) for p in parts}) == 1 and sum(len(p) for p in parts) == -(-len(lit) // 3) * 3
    assert set(sum(parts, [])) == set(lit)
    idx = [SampleAcfTrainBatcher(CFG, data, rank=r, world=3)._indices().tolist() for r in range(3)]
    flat = sum(idx, [])
    assert set(flat) == set(range(len(lit))) and len(flat) - len(set(flat)) == len(flat) - len(lit)


def test_eval_batcher_is_the_sequence_batcher_plus_the_user_ids():
    from pixelrec_amd.data.dataset import AcfEvalBatcher, SeqEvalBatcher

    data, L = _Synth(), CFG["MAX_ITEM_LIST_LENGTH"]
    uids = np.fromiter(data.user_seq.keys(), dtype=np.int64)
    for phase in ("valid", "test"):
        a, s = AcfEvalBatcher(CFG, data, phase=phase), SeqEvalBatcher(CFG, data, phase=phase)
        assert len(a) == len(s)
        n = 0
        for (wa, ha, pa, ta), (ws, hs, ps, ts) in zip(a, s):
            assert wa.shape == (ws.shape[0], L + 1) and wa.dtype == torch.int64
            assert torch.equal(wa[:, :L], ws) and torch.equal(wa[:, L], torch.from_numpy(uids[n:n + len(ws)]))
            assert torch.equal(ha[0], hs[0]) and torch.equal(ha[1], hs[1]) and torch.equal(pa, ps) and torch.equal(ta, ts)
            n += len(ws)
        assert n == len(uids)


# ------------------------------------------------------------------------------------------------------------ the model
class _Data:
    user_num, item_num = 7, 11


def _feat(tmp_path, shape=(11, 2, 2, 12), name="v.npy"):
    path = str(tmp_path / name)
    np.save(path, np.random.default_rng(1).standard_normal(shape).astype(np.float32))
    return path


def _model(path, E=8):
    from pixelrec_amd.model import ACF

    return ACF({"embedding_size": E, "v_feat_path": path, "MAX_ITEM_LIST_LENGTH": 4}, _Data())


def test_state_dict_has_the_reference_keys_in_order_and_loads_the_fixture(gold, tmp_path):
    m = _model(_feat(tmp_path))
    ref = [str(k) for k in gold["sd.keys"]]
    assert ref == list(R.STATE_KEYS) and len(ref) == 19
    assert list(m.state_dict().keys()) == ref
    assert [n for n, _ in m.named_parameters()] == list(R.NAMES) and not list(m.named_buffers())
    assert list(m.rec_parameter_names()) == list(R.NAMES)
    assert m.item_model.weight is m.user_model.profile_embedding.weight
    sd = {k: torch.from_numpy(np.asarray(gold["sd." + k])) for k in ref}
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.item_model.weight.data, sd["item_model.weight"]) and m.item_model.weight.data[0].abs().max() > 0
    assert tuple(m.v_feat.shape) == (11, 2, 2, 12) and m.regions == 4 and m.feature_dim == 12


def test_init_is_kaiming_with_zero_biases(tmp_path):
    torch.manual_seed(0)
    m = _model(_feat(tmp_path, shape=(11, 2, 2, 400)), E=64)
    for n, p in m.named_parameters():
        if n.endswith("bias"):
            assert p.abs().max() == 0, n
    w = m.user_model.feats.dim_reductor.weight
    assert abs(float(w.data.std()) - (2.0 / 400) ** 0.5) < 0.1 * (2.0 / 400) ** 0.5


def test_bad_feature_files_raise_value_errors_that_name_the_file(tmp_path):
    with pytest.raises(ValueError, match="v2.npy"):
        _model(_feat(tmp_path, shape=(11, 48), name="v2.npy"))                    # a 2-D (VBPR-style) feature matrix
    with pytest.raises(ValueError, match="item_num"):
        _model(_feat(tmp_path, shape=(10, 2, 2, 12)))
    with pytest.raises(ValueError, match="multiple of 4"):
        _model(_feat(tmp_path, shape=(11, 2, 2, 10)))
    with pytest.raises(ValueError, match="embedding_size"):
        _model(_feat(tmp_path), E=6)


def test_forward_on_the_cpu_raises_instead_of_falling_back(gold, tmp_path):
    from pixelrec_amd.lib import PxrError

    m = _model(_feat(tmp_path)).train()
    with pytest.raises(PxrError):
        m(torch.from_numpy(gold["rows"][0]))
    with pytest.raises(PxrError):
        m.eval().predict(torch.from_numpy(gold["eval.windows"]), None)


def test_ops_reject_cpu_tensors():
    from pixelrec_amd import ops
    from pixelrec_amd.lib import PxrError

    with pytest.raises(PxrError):
        ops.acf_rows(torch.zeros(2, 3, dtype=torch.int64), None, torch.zeros(2, dtype=torch.int64), 5, 5)
    with pytest.raises(PxrError):
        ops.acf_item_fwd(torch.zeros(2, 8), torch.zeros(6, 8), torch.zeros(6, 8), torch.zeros(6, 8), torch.zeros(8),
                         torch.zeros(2, 3, dtype=torch.int64))


def test_kernel_shape_limits_fail_loudly_without_a_gpu():
    from pixelrec_amd import lib

    L = lib.load()
    one = 16                                  # (a non-null, 16-byte aligned address: the checks run before any launch)
    assert L.pxr_acf_region_fwd_f32(one, one, one, one, one, 2, 3, 2000, 8, one, one, None) == -1
    assert b"regions" in L.pxr_last_error()
    assert L.pxr_acf_item_fwd_f32(one, one, one, one, one, one, 2, 3, 6, one, one, None) == -1
    assert b"E % 4" in L.pxr_last_error()
    from pixelrec_amd import ops

    segs = (ops._CRowSegment * 3)()                 # profile: a null id list with a positive count | no items | two users
    segs[0].count, segs[0].n, segs[0].base, segs[0].pad0 = 4, 5, 1, 1
    segs[1].n, segs[1].base, segs[1].pad0 = 5, 1, 1
    segs[2].ids, segs[2].count, segs[2].n, segs[2].base = one, 2, 5, 6
    assert L.pxr_table_rows_i64(segs, 3, one, None, None) == -1
    assert b"null id list" in L.pxr_last_error()


def test_acf_is_registered_and_the_yaml_parses():
    from pixelrec_amd.config.configurator import Config
    from pixelrec_amd.data.utils import SUPPORTED
    from pixelrec_amd.model import ACF
    from pixelrec_amd.utils.enum_type import InputType
    from pixelrec_amd.utils.utils import get_model

    assert SUPPORTED["ACF"] == "SEQ" and ACF.input_type == InputType.SEQ and get_model("ACF") is ACF
    c = Config([os.path.join(ROOT, "configs/ViNet/acf.yaml")])
    assert c["model"] == "ACF" and c["embedding_size"] == 512 and c["MAX_ITEM_LIST_LENGTH"] == 10 and c["seed"] == 2020
    assert c["train_batch_size"] == 512 and c["eval_batch_size"] == 512 and c["epochs"] == 200
    assert dict(c["optim_args"]) == {"learning_rate": 1e-4, "weight_decay": 0.01}
    assert c["v_feat_path"] == "../dataset/visual_features/RN50_layer4.npy" and c["dataset"] == "Pixel200K"
    assert list(c["topk"]) == [5, 10] and c["valid_metric"] == "NDCG@10" and c["stopping_step"] == 30
    assert c["MODEL_INPUT_TYPE"] == InputType.SEQ
