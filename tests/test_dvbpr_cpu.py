"""DVBPR without a GPU: the index maps of csrc/conv2d.hip (restated in tests/dvbpr_restate.py with the kernels' arithmetic) against
torch's unfold / fold / max_pool2d autograd on every shape the GPU kernel tests use, the layer table, the fixture against the
float64 restatement, the wiring, the state_dict layout and the inert padding mode."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dvbpr_restate as R
from tests.mo_common import GOLD, ROOT

# (n, Cin, H, W, Cout, kh, kw, sh, sw): the smallest shapes that reach the edges (tests/test_gpu_conv2d.py runs the kernels on them)
CONV_SHAPES = [
    (2, 3, 23, 33, 8, 11, 11, 1, 4),     # conv1's geometry: K = 363 -> a pad column; W-stride remainder: the last two columns unread
    (3, 8, 9, 7, 12, 5, 5, 1, 1),        # a plain 5x5
    (2, 4, 6, 5, 4, 3, 3, 1, 1),         # a plain 3x3
    (1, 4, 3, 3, 4, 3, 3, 1, 1),         # one output pixel
    (5, 4, 20, 19, 8, 3, 3, 1, 1),       # the chunking case: a budget of two images' columns gives chunks of 2, 2 and 1
    (2, 4, 11, 12, 4, 3, 3, 2, 3),       # strides in both directions: windows that do not overlap in W (every element is still read)
    (2, 4, 12, 13, 4, 3, 3, 2, 3),       # the same with a remainder in both directions: the last row and the last column unread
]
POOL_SHAPES = [(2, 4, 7, 5), (1, 4, 2, 2), (2, 8, 6, 6)]      # (n, C, H, W): odd sizes (a dropped row and column), one window, even
FIXTURE = os.path.join(GOLD, "dvbpr_tiny.npz")


def conv_input(shape, seed=0):
    n, C, H, W = shape[:4]
    return torch.randn(n, C, H, W, generator=torch.Generator().manual_seed(seed))


def pool_input(shape, seed=0, ties=False):
    """A ReLU'd activation; ties: every window of channel 0 gets its maximum planted twice (positive), every window of channel 1 is 0."""
    y = torch.relu(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)))
    if ties:
        n, C, H, W = shape
        for h in range(0, H - 1, 2):
            for w in range(0, W - 1, 2):
                y[:, 0, h, w + 1] = y[:, 0, h + 1, w] = 3.0 + h + w      # second and third of the window tie above everything else
                y[:, 1, h:h + 2, w:w + 2] = 0.0                           # a tie at 0: ReLU'(0) = 0, nothing flows
    return y


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_im2col_map_is_unfold_bit_for_bit(shape):
    n, C, H, W, _, kh, kw, sh, sw = shape
    x = conv_input(shape)
    col = R.im2col_map(x.numpy(), kh, kw, sh, sw)
    K = C * kh * kw
    ref = F.unfold(x, (kh, kw), stride=(sh, sw)).transpose(1, 2).reshape(-1, K)
    assert col.shape == (ref.shape[0], (K + 3) // 4 * 4)
    assert np.array_equal(col[:, :K].view(np.int32), ref.numpy().view(np.int32))
    assert np.array_equal(col[:, K:].view(np.int32), np.zeros_like(col[:, K:]).view(np.int32))      # +0.0, not -0.0


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_col2im_map_is_fold(shape):
    n, C, H, W, _, kh, kw, sh, sw = shape
    Ho, Wo = R.out_hw(H, W, kh, kw, sh, sw)
    K = C * kh * kw
    ldk = (K + 3) // 4 * 4
    # integer values: every sum is exact, so the comparison is independent of fold's summation order
    dcol = torch.randint(-8, 9, (n * Ho * Wo, ldk), generator=torch.Generator().manual_seed(1)).double()
    dx = R.col2im_map(dcol.numpy(), n, C, H, W, kh, kw, sh, sw)
    ref = F.fold(dcol[:, :K].reshape(n, Ho * Wo, K).transpose(1, 2), (H, W), (kh, kw), stride=(sh, sw))
    assert np.array_equal(dx, ref.numpy())
    unread = ~R.covered(H, W, kh, kw, sh, sw)
    assert np.array_equal(dx[:, :, unread].view(np.int64), np.zeros_like(dx[:, :, unread]).view(np.int64))
    if shape[7:] == (1, 4):
        assert unread[:, -2:].all() and not unread[:, :-2].any()        # the last two columns are read by no window
    if shape[2:4] == (11, 12):
        assert not unread.any()
    if shape[2:4] == (12, 13):
        assert unread[-1, :].all() and unread[:, -1].all() and not unread[:-1, :-1].any()


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_pool_maps_are_torch(shape, ties):
    y = pool_input(shape, ties=ties)
    x = y.clone().requires_grad_(True)
    p = F.max_pool2d(torch.relu(x), 2)
    dp = torch.randn(p.shape, generator=torch.Generator().manual_seed(2))
    p.backward(dp)
    assert np.array_equal(R.pool_fwd_map(y.numpy()).view(np.int32), p.detach().numpy().view(np.int32))
    dy = R.pool_bwd_map(y.numpy(), dp.numpy())
    assert np.array_equal(dy.view(np.int32), x.grad.numpy().view(np.int32))
    n, C, H, W = shape
    assert not dy[:, :, 2 * (H // 2):, :].any() and not dy[:, :, :, 2 * (W // 2):].any()
    if ties:
        assert (dy[:, 0, 0, 1] == dp.numpy()[:, 0, 0, 0]).all() and not dy[:, 0, 1, 0].any()      # the first of the tie wins
        assert not dy[:, 1].any()


def test_layer_table_comes_out_of_the_geometry():
    from pixelrec_amd.model.cnnf import cnnf_flat_features, cnnf_geometry

    g = cnnf_geometry()
    assert [(d["ho"], d["wo"]) for d in g] == [(214, 54), (103, 23), (49, 9), (47, 7), (45, 5)]
    assert [(d["hp"], d["wp"]) for d in g] == [(107, 27), (51, 11), (49, 9), (47, 7), (22, 2)]
    assert [(d["cin"], d["cout"], d["kh"], d["kw"], d["sh"], d["sw"], d["pool"]) for d in g] == \
        [(c[0], c[1], c[2], c[2], c[3][0], c[3][1], c[4]) for c in R.CONVS]
    assert cnnf_flat_features() == R.FLAT == 11264
    from pixelrec_amd import ops

    # one image's columns: 16.8 MB at conv1, 15.2 MB at conv2
    mb = [d["ho"] * d["wo"] * ops.conv2d_ldk(d["cin"], d["kh"], d["kw"]) * 4 / 1e6 for d in g]
    assert round(mb[0], 1) == 16.8 and round(mb[1], 1) == 15.2
    assert ops.conv2d_ldk(3, 11, 11) == 364
    assert ops.conv2d_chunk_images(5, 18 * 17, 36, 2 * 18 * 17 * 36 * 4) == 2 and ops.conv2d_chunk_images(5, 10, 4, 1) == 1
    with pytest.raises(ValueError):
        ops.conv2d_out_hw(3, 3, 4, 3, 1, 1)
    with pytest.raises(ValueError):
        ops.conv2d_out_hw(3, 3, 3, 3, 0, 1)


def load_fixture():
    g = np.load(FIXTURE)
    U, I, Dh, B, seed = (int(v) for v in g["meta"])
    state = R.make_state(seed, Dh, U, I)
    assert list(state) == [str(k) for k in g["sd.keys"]]
    sums = R.state_sums(state)
    assert np.allclose(sums, g["sd.sums"], rtol=1e-12, atol=0), "the weight recipe no longer reproduces the fixture's weights"
    return g, state, R.expand_images(g["store"]), (U, I, Dh, B)


def test_fixture_is_small_and_the_restatement_equals_it():
    assert os.path.getsize(FIXTURE) < 1_000_000
    g, state, images, (U, I, Dh, B) = load_fixture()
    assert g["store"].dtype == np.uint8 and g["store"].shape == (I, 28, 28, 3)
    close = lambda a, b: np.allclose(np.asarray(a), b, rtol=1e-9, atol=1e-13)
    for j in range(2):
        user, item = g[f"b{j}.user"], g[f"b{j}.item_id"]
        ids, index = R.dedup(item)
        assert len(ids) == 5 and item.shape == (B, 2)                     # one image shared between a positive and a negative
        P = {k: v.double().requires_grad_(True) for k, v in state.items()}
        loss = R.loss_of(P, R.cnnf(P, images[torch.from_numpy(ids)]), user, item, index)      # each distinct image once
        loss.backward()
        assert close(loss.detach(), g[f"b{j}.loss"][0])
        for k in state:
            gr = P[k].grad
            if f"b{j}.grad.{k}" in g:
                assert close(gr, g[f"b{j}.grad.{k}"]), k
            elif f"b{j}.rows.{k}" in g:
                rows = np.unique(user if "users" in k else item.reshape(-1))
                assert close(gr[torch.from_numpy(rows)], g[f"b{j}.rows.{k}"]), k
                assert float(gr.abs().sum()) == float(gr[torch.from_numpy(rows)].abs().sum())
            else:
                assert close(gr.norm(), g[f"b{j}.norm.{k}"][0]), k
                assert close(gr.reshape(-1)[torch.from_numpy(R.sample_index(gr.numel()))], g[f"b{j}.sample.{k}"]), k
    with torch.no_grad():
        P = {k: v.double() for k, v in state.items()}
        feat = R.cnnf(P, images)
        assert close(feat, g["eval.item_feature"]) and close(R.predict(P, np.arange(U), feat), g["eval.scores"])
    assert all(("ref_err." + k) in g for k in g.files if k[0] == "b" and "." in k and k.split(".")[1] in ("loss", "grad", "rows", "norm", "sample"))


def test_padding_mode_is_inert():
    _, state, images, _ = load_fixture()
    with torch.no_grad():
        a = R.cnnf(state, images[:2], padding_mode="replicate")
        b = R.cnnf(state, images[:2], padding_mode="zeros")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and float(a.abs().max()) > 0


def test_wiring():
    from pixelrec_amd.config import Config
    from pixelrec_amd.data.dataset import MoPairTrainBatcher, PairEvalBatcher
    from pixelrec_amd.data.utils import LOADERS, SUPPORTED, _TrainLoader
    from pixelrec_amd.model import DVBPR
    from pixelrec_amd.utils import get_model
    from pixelrec_amd.utils.enum_type import InputType

    assert get_model("DVBPR") is DVBPR and DVBPR.input_type == InputType.PAIR
    assert SUPPORTED["DVBPR"] == "PAIR" and LOADERS["DVBPR"] == (MoPairTrainBatcher, PairEvalBatcher, _TrainLoader)
    cfg = Config([os.path.join(ROOT, "configs", "PixelNet", "dvbpr.yaml"), os.path.join(ROOT, "configs", "overall", "ViT.yaml")])
    assert cfg["model"] == "DVBPR" and cfg["embedding_size"] == 4096 and cfg["dropout_prob"] == 0.5
    assert cfg["conv_workspace_mb"] == 1024 and cfg["use_modality"] and len(cfg["optim_args"]) == 4
    # the batcher's (user, index, image_ids) -> (user, item_id, index): item_id = image_ids[index]
    item = torch.tensor([[1, 4], [4, 7], [2, 8]])
    ids, index = R.dedup(item.numpy())
    user = torch.tensor([0, 3, 5])
    u, item_id, idx = DVBPR.batch_ids((user, torch.from_numpy(index), torch.from_numpy(ids)))
    assert torch.equal(u, user) and torch.equal(item_id, item) and torch.equal(idx, torch.from_numpy(index))


class _Data:
    def __init__(self, U, I):
        self.user_num, self.item_num = U, I


def build_model(U, I, Dh, dropout=0.0, **extra):
    from pixelrec_amd.model import DVBPR

    return DVBPR({"embedding_size": 2 * Dh, "dropout_prob": dropout, "seed": 2020, **extra}, _Data(U, I))


def test_state_dict_has_the_reference_layout():
    g, state, _, (U, I, Dh, _) = load_fixture()
    m = build_model(U, I, Dh)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in g["sd.keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in g["sd.shapes"]]
    assert dict(R.state_shapes(Dh, U, I)) == {k: tuple(v.shape) for k, v in sd.items()}
    m.load_state_dict(state, strict=True)
    assert [n for n, _ in m.visual_encoder.named_parameters()] == [k[len(R.ENC):] for k in state if k.startswith(R.ENC)]
    assert list(m.table_parameter_spans()) == list(state)[16:] and list(m.rec_parameter_names()) == list(state)[16:]
    assert m.table_parameter_spans()["gamma_items.weight"] == (1 + 2 * U, 1 + 2 * U + I)
    # tables uniform(0, 1), xavier-uniform weights (dvbpr.py:40-46, 139-143)
    fresh = build_model(U, I, Dh)
    for k in list(state)[16:]:
        t = fresh.state_dict()[k]
        assert 0.0 <= float(t.min()) and float(t.max()) < 1.0 and 0.3 < float(t.mean()) < 0.7
    w = fresh.state_dict()[R.ENC + "fcs.1.weight"]
    assert float(w.abs().max()) <= np.sqrt(6.0 / 1024) and float(w.abs().max()) > 0.99 * np.sqrt(6.0 / 1024)


def test_cpu_inputs_are_refused():
    from pixelrec_amd.lib import PxrError

    m = build_model(7, 9, 16)
    with pytest.raises(ValueError):
        m.visual_encoder(torch.zeros(2, 3, 64, 64))
    with pytest.raises(PxrError):
        m.visual_encoder(torch.zeros(2, 3, 224, 224))
    with pytest.raises(ValueError):
        build_model(7, 9, 16, conv_workspace_mb=0)
