"""The frozen ViT prefix cached per item (model/prefix_cache.py): the gather fused with the first live block's LayerNorm
(pxr_ln_gather_fwd_f32), the tower's forward cut at the first trainable block, the encoder / MOSASRec / Trainer over item ids.

Bit identities are against the launches the id form replaces (embed_gather -> ln_residual_fwd; the image form on the same ids);
the accuracy bars are those of tests/test_gpu_mosasrec.py against the oracle on HF's CLIPVisionModel, fed store.batch(ids)."""
import functools

import pytest
import torch

from oracle import mosasrec_oracle as MO
from oracle import sasrec_oracle as O
from tests.mo_common import bits, tower_config

pytestmark = pytest.mark.gpu

D, L, NH, NL, B = 64, 6, 2, 2, 3
TOWERS = ("clip-vit-tiny-test", "clip-vit-tiny64-test")     # materialised attention / fused attention with fp16 planes
TUNE = {0: 5, 1: 21, 2: 37, 3: 53}                          # first trainable block k -> tune_scale (5 embedding tensors, 16 per block)
BAD_INDEX = 1                                               # PXR_STATUS_BAD_INDEX


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel
def _both(cache, ids, T, gamma, beta, pf):
    from pixelrec_amd import ops

    n, H = ids.numel(), gamma.numel()
    fused = ops.ln_gather_fwd(cache, ids, T, gamma, beta, 1e-5, save=True, planes=pf)
    x = ops.embed_gather(cache, ids).view(n, T, H)
    two = (x,) + tuple(ops.ln_residual_fwd(x, None, gamma, beta, 1e-5, save=True, planes=pf))
    return fused, two


def _assert_same(fused, two):
    for name, a, b in zip(("x_out", "y", "xhat", "rstd"), fused, two):
        assert torch.equal(bits(a), bits(b)), name
    if len(fused) == 5:
        assert fused[4].fmt == two[4].fmt and (fused[4].pr, fused[4].ps) == (two[4].pr, two[4].ps)
        assert torch.equal(fused[4].buf.view(torch.int16), two[4].buf.view(torch.int16)), "raw plane buffers"


@pytest.mark.parametrize("H,T,n", [(64, 5, 1), (128, 17, 7), (768, 50, 3), (1024, 257, 2)])
def test_gather_layernorm_equals_gather_then_layernorm(H, T, n):
    """x_out, xhat, rstd, fp32 y and the raw plane buffers (bf16x3 and two-plane fp16) of the fused launch == embed_gather followed
    by ln_residual_fwd, on n ids and on seven ids that hold a repeat, id 0 and id N-1."""
    from pixelrec_amd import ops

    N = 11
    g = torch.Generator().manual_seed(H + T)
    cache = torch.randn(N, T * H, generator=g).cuda()
    gamma, beta = (1 + 0.1 * torch.randn(H, generator=g)).cuda(), (0.1 * torch.randn(H, generator=g)).cuda()
    pattern = [0, N - 1, 0, 4, 4, 2, N - 1]
    ops.raise_on_bad_indices()
    for ids in {tuple(pattern[:n]), tuple(pattern)}:
        ids = torch.tensor(ids, dtype=torch.int64).cuda()
        for pf in (False, True, "h2"):
            fused, two = _both(cache, ids, T, gamma, beta, pf)
            _assert_same(fused, two)
            assert torch.equal(fused[0].view(ids.numel(), -1), cache[ids])
    ops.raise_on_bad_indices()                               # every id was inside the cache


def test_gather_layernorm_flags_and_clamps_a_bad_id():
    from pixelrec_amd import ops

    N, T, H = 6, 5, 64
    g = torch.Generator().manual_seed(2)
    cache = torch.randn(N, T * H, generator=g).cuda()
    gamma, beta = torch.ones(H).cuda(), torch.zeros(H).cuda()
    ops.raise_on_bad_indices()
    ids = torch.tensor([-1, N, 2], dtype=torch.int64).cuda()
    x, y, _, _ = ops.ln_gather_fwd(cache, ids, T, gamma, beta, 1e-5)
    assert int(ops.device_status().item()) & BAD_INDEX
    with pytest.raises(IndexError):
        ops.raise_on_bad_indices()
    clamped = torch.tensor([0, N - 1, 2]).cuda()
    assert torch.equal(x.view(3, -1), cache[clamped])        # the rows read are the clamped ones
    ref = ops.ln_gather_fwd(cache, clamped, T, gamma, beta, 1e-5)
    assert torch.equal(y, ref[1])
    ops.raise_on_bad_indices()


def test_gather_layernorm_reaches_past_2_31_elements():
    """A cache of just over 2^31 elements (8.6 GB, uninitialised but for rows 0 and N-1): both rows come back."""
    from pixelrec_amd import ops

    T, H = 50, 768
    N = (1 << 31) // (T * H) + 1
    assert N * T * H > (1 << 31)
    if torch.cuda.mem_get_info()[0] < 16 * 1024 ** 3:
        pytest.skip("less than 16 GB of free device memory")
    g = torch.Generator().manual_seed(3)
    cache = torch.empty(N, T * H, dtype=torch.float32, device="cuda")
    rows = torch.randn(2, T * H, generator=g).cuda()
    cache[0], cache[N - 1] = rows[0], rows[1]
    gamma, beta = (1 + 0.1 * torch.randn(H, generator=g)).cuda(), (0.1 * torch.randn(H, generator=g)).cuda()
    ids = torch.tensor([N - 1, 0], dtype=torch.int64).cuda()
    fused = ops.ln_gather_fwd(cache, ids, T, gamma, beta, 1e-5, planes="h2")
    assert torch.equal(fused[0].view(2, -1), rows.flip(0))
    x = rows.flip(0).contiguous().view(2, T, H)
    _assert_same(fused, (x,) + tuple(ops.ln_residual_fwd(x, None, gamma, beta, 1e-5, planes="h2")))
    assert torch.equal(ops.embed_gather(cache, ids), rows.flip(0))      # the plain-gather route (only the head trains)
    ops.raise_on_bad_indices()
    del cache


# ------------------------------------------------------------------------------------------------------------------ the towers
def _encoder(name, k=2, seed=7):
    from pixelrec_amd.model import visual

    torch.manual_seed(seed)
    cfg = {"encoder_name": name, "encoder_source": "transformers", "embedding_size": 32, "pretrain_path": None,
           "fine_tune_arg": {"tune_scale": TUNE[k], "pre_trained": False, "activation": "relu", "dnn_layers": [], "method": "mean"}}
    enc = visual.load_model(cfg)
    for p in enc.parameters():
        if p.dim() == 1:
            p.data.add_(0.1 * torch.randn_like(p))
    enc = enc.cuda()
    enc._native.ensure_packed()
    assert enc._native.first_trainable_block() == k
    return enc


def _forward_before_the_split(tower, images, need_grad):
    """NativeTower.forward as it stood before it was cut at the first trainable block: the embeddings, ONE loop over every block,
    the mean head (Linear + ReLU + token mean)."""
    from pixelrec_amd import ops

    tower.ensure_packed()
    e = tower.enc
    vm = "item_encoder.vision_model."
    H, heads, d, T, p = tower._shape()
    n, c, Hi, Wi = images.shape
    first = tower.first_trainable_block() if need_grad else 10 ** 9
    patches = images.view(n, c, Hi // p, p, Wi // p, p).permute(0, 2, 4, 1, 3, 5).reshape(-1, c * p * p).contiguous()
    pe = ops.linear_fwd(patches, tower.view(vm + "embeddings.patch_embedding.weight").view(H, -1), None).view(n, T - 1, H)
    x0 = ops.vit_embed(pe, tower.view(vm + "embeddings.class_embedding"), tower.view(vm + "embeddings.position_embedding.weight"))
    x, _, _ = ops.ln_residual_fwd(x0, None, tower.view(vm + "pre_layrnorm.weight"), tower.view(vm + "pre_layrnorm.bias"), 1e-5, save=False)
    blocks = []
    for i in range(len(e.item_encoder.vision_model.encoder.layers)):
        x, s = tower._block_fwd(i, x, keep=need_grad and i >= first)
        blocks.append(s)
    head = e.head_layers()
    act = ops.linear_epi(x, tower.view(head[0][0]), tower.view(head[0][1]), ops.EPI_BIAS_RELU)
    out = ops.token_mean(act)
    saved = dict(n=n, first=first, blocks=blocks, x_last=x, head_in=x, act=act, act_relu=True, xh_p=None, rs_p=None, head=head,
                 hidden=[], patches=None, xh0=None, rs0=None, head_planes=None) if need_grad else None
    return out, saved


# ------------------------------------------------------------------------------------------------------------------ 2. the split
@pytest.mark.parametrize("need_grad", [True, False])
@pytest.mark.parametrize("name", TOWERS)
def test_split_forward_is_the_forward(name, need_grad):
    enc = _encoder(name)
    tower = enc._native
    g = torch.Generator().manual_seed(11)
    images = torch.randn(5, 3, 64, 64, generator=g).cuda()
    d_out = torch.randn(5, 32, generator=g).cuda()
    runs = []
    for fwd in (lambda: _forward_before_the_split(tower, images, need_grad),
                lambda: tower.forward_from(tower.forward_prefix(images), need_grad),
                lambda: tower.forward(images, need_grad)):
        with torch.no_grad():
            out, saved = fwd()
            assert (saved is not None) == need_grad
            gflat = None
            if need_grad:
                assert saved["first"] == 2
                tower.gflat.zero_()
                tower.backward(d_out, saved)
                gflat = tower.gflat.clone()
        runs.append((out.clone(), gflat))
    for out, gflat in runs[1:]:
        assert torch.equal(bits(out), bits(runs[0][0]))
        if need_grad:
            assert torch.equal(bits(gflat), bits(runs[0][1])) and float(gflat.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------ 3. batch invariance
@pytest.mark.parametrize("name", TOWERS)
def test_prefix_of_an_image_does_not_depend_on_its_batch(name):
    """forward_prefix of one image: alone, at positions 0 and 4 of a batch of 5, inside a chunk of 100 (the cache's fill) -- the
    same bits, so the cached step computes what the uncached one does."""
    enc = _encoder(name)
    tower = enc._native
    g = torch.Generator().manual_seed(13)
    images = torch.randn(100, 3, 64, 64, generator=g).cuda()
    with torch.no_grad():
        alone = tower.forward_prefix(images[7:8])[0].clone()
        five = tower.forward_prefix(images[[7, 1, 2, 3, 7]].contiguous())
        chunk = tower.forward_prefix(images)
    assert alone.shape == five.shape[1:] and float(alone.abs().max()) > 0
    assert torch.equal(bits(five[0]), bits(alone)), "position 0 of 5"
    assert torch.equal(bits(five[4]), bits(alone)), "position 4 of 5"
    assert torch.equal(bits(chunk[7]), bits(alone)), "inside a chunk of 100"


# ------------------------------------------------------------------------------------------------------------------ 4. the model
def _build(name, k):
    from pixelrec_amd.model import MOSASRec
    from pixelrec_amd.model.visual import ENCODER_SHAPES

    class DL:
        item_num = 50

    torch.manual_seed(1)
    hf = MO.hf_clip_vision(*ENCODER_SHAPES[name])
    cfg = tower_config(TUNE[k], n_layers=NL, n_heads=NH, embedding_size=D, inner_size=2, hidden_dropout_prob=0.0, attn_dropout_prob=0.0,
                       hidden_act="gelu", layer_norm_eps=1e-12, initializer_range=0.02, MAX_ITEM_LIST_LENGTH=L, encoder_name=name)
    m = MOSASRec(cfg, DL())
    m.visual_encoder.item_encoder.load_state_dict(
        {k_: v for k_, v in MO.hf_state_to_reference_names(hf).items() if "post_layernorm" not in k_}, strict=True)
    seq = {k_: v for k_, v in O.synth_params(50, D, L, NL, 2, seed=4).items() if k_ != "item_embedding.weight"}
    m.load_state_dict(seq, strict=False)
    return m, hf, seq


def _store():
    from pixelrec_amd.data.images import ImageStore

    return ImageStore.synthetic(50, 64, 5, "cuda")


def _batch():
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(1, 50, (B, 2 * (L + 1)), generator=g)
    ids[0, :8] = 0                                          # left-padded sequence: pad images, masked targets
    ids[1, 3] = ids[1, 5]                                   # an item twice in one batch
    mask = torch.ones(B, L, dtype=torch.int64)
    mask[0, :3] = 0
    return ids.cuda(), mask.cuda()


def _grads(m):
    return {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}


@functools.lru_cache(maxsize=None)
def _oracle(name, k):
    """(loss, {this build's parameter name: gradient}) of the HF-based oracle on store.batch(ids); computed once per tower and k."""
    m, hf, seq = _build(name, k)
    ids, mask = _batch()
    images = _store().batch(ids).cpu()
    rec_w = m.visual_encoder.rec_fc[0].weight.detach().clone().requires_grad_(True)
    rec_b = m.visual_encoder.rec_fc[0].bias.detach().clone().requires_grad_(True)
    for p in hf.parameters():
        p.requires_grad_(True)
    hf.train(False)
    sp = {k_: v.clone().requires_grad_(True) for k_, v in seq.items()}
    emb = MO.mean_item_encoder(hf, rec_w, rec_b, images.flatten(0, 1)).view(B, -1, 2, D)
    ref = MO.forward_loss(sp, emb, mask.cpu(), {"n_layers": NL, "n_heads": NH, "layer_norm_eps": 1e-12})
    ref.backward()
    grads = {k_: v.grad for k_, v in sp.items()}
    grads["visual_encoder.rec_fc.0.weight"], grads["visual_encoder.rec_fc.0.bias"] = rec_w.grad, rec_b.grad
    for n, p in hf.named_parameters():
        if p.grad is not None:
            grads["visual_encoder.item_encoder.vision_model." + n] = p.grad
    return float(ref.detach()), grads


def _assert_matches_oracle(m, loss, ref_loss, ref, k):
    """The comparison and the bounds of tests/test_gpu_mosasrec.py::test_loss_and_gradients_match_oracle."""
    assert abs(float(loss) - ref_loss) < 3e-5 * max(1.0, abs(ref_loss))
    checked = 0
    for n, p in m.named_parameters():
        if n.startswith("visual_encoder.rec_fc"):
            r = ref[n]
            assert (p.grad.cpu() - r).abs().max().item() < 1e-5 + 3e-4 * r.abs().max().item(), n
        elif n.startswith("visual_encoder"):
            if p.requires_grad and n not in ref:        # post_layernorm: trainable but unused by method 'mean'
                assert p.grad is None
            elif p.requires_grad:
                r = ref[n]
                assert (p.grad.cpu() - r).abs().max().item() <= 1e-6 + 5e-4 * r.abs().max().item(), n
                checked += 1
            else:
                assert p.grad is None
        else:
            r = ref[n]
            assert (p.grad.cpu() - r).abs().max().item() <= 5e-6 + 3e-4 * r.abs().max().item(), n
    assert checked == 16 * (3 - k)


@pytest.mark.parametrize("k", [2, 1, 3])
@pytest.mark.parametrize("name", TOWERS)
def test_model_over_ids_matches_the_oracle_and_the_image_form(name, k, monkeypatch):
    """(a) MOSASRec over item ids against the oracle fed store.batch(ids), the bounds of the image form's test; (b) loss and every
    gradient bit-equal to the image form on the same ids; and the unfused route (PXR_PREFIX_FUSED_LN=0) gives the same bits.
    k = 3: only the head trains, the plain gather feeds it."""
    from pixelrec_amd import ops

    ids, mask = _batch()
    store = _store()
    ref_loss, ref = _oracle(name, k)
    out = {}
    for form in ("images", "ids", "ids-unfused"):
        monkeypatch.setenv("PXR_PREFIX_FUSED_LN", "0" if form == "ids-unfused" else "1")
        m = _build(name, k)[0].cuda().train()
        if form != "images":
            assert m.visual_encoder.build_prefix_cache(store)
            cache = m.visual_encoder.prefix_cache
            assert cache.k == k and cache.table.shape[0] == store.n and float(cache.table[0].abs().max()) > 0    # row 0: the zero image's prefix
        loss = m((store.batch(ids) if form == "images" else ids, mask))
        loss.backward()
        ops.raise_on_bad_indices()
        _assert_matches_oracle(m, loss.detach(), ref_loss, ref, k)                  # (a), and the image form's own bar
        out[form] = (loss.detach().clone(), _grads(m))
    for form in ("ids", "ids-unfused"):                                             # (b)
        assert torch.equal(bits(out[form][0]), bits(out["images"][0])), form
        assert out[form][1].keys() == out["images"][1].keys()
        for n, gr in out["images"][1].items():
            assert torch.equal(bits(out[form][1][n]), bits(gr)), (form, n)


def test_model_over_ids_equals_the_image_form_without_planes(monkeypatch):
    """PXR_PLANES=0: the blocks on the fp32-input GEMMs (the fill writes the table through linear_epi's `out`, the gather + LayerNorm
    launch returns fp32 y) -- ids and images give the same bits there too."""
    from pixelrec_amd import ops

    monkeypatch.setenv("PXR_PLANES", "0")
    ids, mask = _batch()
    store = _store()
    out = {}
    for form in ("images", "ids"):
        m = _build(TOWERS[0], 2)[0].cuda().train()
        assert not m.visual_encoder._native._planes_on()
        if form == "ids":
            assert m.visual_encoder.build_prefix_cache(store)
        loss = m((store.batch(ids) if form == "images" else ids, mask))
        loss.backward()
        out[form] = (loss.detach().clone(), _grads(m))
    ops.raise_on_bad_indices()
    assert torch.equal(bits(out["ids"][0]), bits(out["images"][0]))
    for n, gr in out["images"][1].items():
        assert torch.equal(bits(out["ids"][1][n]), bits(gr)), n


def test_no_frozen_prefix_no_cache():
    m = _build(TOWERS[0], 0)[0].cuda()
    assert m.visual_encoder.build_prefix_cache(_store()) is False and m.visual_encoder.prefix_cache is None


def test_encoder_over_ids_of_any_shape_and_bad_ids():
    from pixelrec_amd import ops

    m = _build(TOWERS[0], 2)[0].cuda().eval()
    store = _store()
    enc = m.visual_encoder
    assert enc.build_prefix_cache(store, chunk=16)           # 50 items: three full chunks and a rest
    ids = torch.tensor([[0, 49, 7], [7, 3, 1]]).cuda()
    with torch.no_grad():
        feat = m.compute_item(ids)
        ref = m.compute_item(store.batch(ids.flatten()))
    assert feat.shape == (6, D) and torch.equal(bits(feat), bits(ref))
    ops.raise_on_bad_indices()
    with torch.no_grad():
        bad = m.compute_item(torch.tensor([-3, 50, 7]).cuda())
    with pytest.raises(IndexError):
        ops.raise_on_bad_indices()
    with torch.no_grad():
        assert torch.equal(bits(bad), bits(m.compute_item(torch.tensor([0, 49, 7]).cuda())))      # clamped


# ------------------------------------------------------------------------------------------------------------------ 5. lifecycle
def test_cache_lifecycle():
    from pixelrec_amd import ops
    from pixelrec_amd.lib import PxrError

    m = _build(TOWERS[0], 2)[0].cuda().train()
    enc, store = m.visual_encoder, _store()
    ids, mask = _batch()
    ops.raise_on_bad_indices()

    def refused():
        with pytest.raises(PxrError):
            m((ids, mask))
        assert int(ops.device_status().item()) == 0          # raised in front of every launch

    enc._native.ensure_packed()                               # (the tower's own flat buffers: allocated at its first use, cache or not)
    free0 = torch.cuda.memory_allocated()
    assert enc.build_prefix_cache(store, budget_bytes=1) is False and enc.prefix_cache is None
    assert torch.cuda.memory_allocated() == free0            # nothing was allocated
    refused()
    m((store.batch(ids), mask)).backward()                   # the image form still runs
    # load_state_dict: the weights may have changed
    assert enc.build_prefix_cache(store)
    m((ids, mask)).backward()
    m.load_state_dict(m.state_dict())
    assert enc.prefix_cache is None
    refused()
    # a frozen block starts to train: k moves
    assert enc.build_prefix_cache(store)
    p = enc.item_encoder.vision_model.encoder.layers[1].mlp.fc1.bias
    p.requires_grad = True
    refused()
    p.requires_grad = False
    m((ids, mask)).backward()
    # another store
    other = _store()
    enc.prefix_cache.store = other
    refused()
    enc.prefix_cache.store = store
    m((ids, mask)).backward()
    enc.drop_prefix_cache()
    assert enc.prefix_cache is None
    refused()
    with pytest.raises(PxrError):
        enc(ids.cpu())
    ops.raise_on_bad_indices()


# ------------------------------------------------------------------------------------------------------------------ 6. hipGraph
def test_id_step_replayed_from_a_hip_graph_equals_the_eager_steps(monkeypatch):
    """tests/test_gpu_mosasrec.py::_pixelnet_graph_equals_eager over item ids: seven id batches, dropout 0.1, both optimizer
    groups inside the capture."""
    from pixelrec_amd.graph import GraphedTrainStep
    from pixelrec_amd.optim import OptimizerGroup, PxrAdamW, VisualAdamW

    monkeypatch.setenv("PXR_SEQ_H2_STALE", "0")
    g = torch.Generator().manual_seed(9)
    store = _store()
    batches = [(torch.randint(0, 50, (B, 2 * (L + 1)), generator=g).cuda(), torch.ones(B, L, dtype=torch.int64).cuda()) for _ in range(7)]
    one = torch.ones((), device="cuda")

    def run(graph):
        m = _build(TOWERS[0], 2)[0].cuda().train()
        m.hidden_dropout_prob = m.attn_dropout_prob = 0.1
        assert m.visual_encoder.build_prefix_cache(store)
        opt = OptimizerGroup(VisualAdamW(m.visual_encoder, lr=1e-3, weight_decay=0.01), PxrAdamW(m, lr=1e-3, weight_decay=0.1))
        losses, gs = [], None
        for i, (ids, mk) in enumerate(batches):
            if graph and i >= 2:
                if gs is None:
                    gs = GraphedTrainStep(m, opt, ids, mk, warmup=1)     # (its eager warm-up step trains on batch 2 as well)
                    continue
                losses.append(float(gs(ids, mk)))
            else:
                opt.zero_grad()
                loss = m((ids, mk))
                loss.backward(one)
                opt.step()
                losses.append(float(loss.detach()))
        assert m.visual_encoder.prefix_cache is not None                 # the optimizer moves trainable blocks only
        return losses, {k: v.detach().clone() for k, v in m.state_dict().items()}, [o.step_count for o in opt.opts]

    le, se, ne = run(False)
    lg, sg, ng = run(True)
    assert ne == ng == [len(batches)] * 2
    assert le[:2] == lg[:2] and le[3:] == lg[2:]
    for k in se:
        assert torch.equal(se[k], sg[k]), k


# ------------------------------------------------------------------------------------------------------------------ 7. Trainer
def _trainer_run(tmp_path, tag, extra):
    """tests/test_gpu_mosasrec.py::test_pixelnet_trainer_end_to_end's setup, one epoch -> (epoch loss, item_feature, checkpoint, trainer)."""
    from pixelrec_amd.config import Config
    from pixelrec_amd.data import bulid_dataloader, load_data
    from pixelrec_amd.parallel import DataParallel
    from pixelrec_amd.trainer import Trainer
    from pixelrec_amd.utils import get_model, init_seed
    from tests.golden_util import GOLDEN_DIR

    d = tmp_path / tag
    d.mkdir()
    my, ov = d / "m.yaml", d / "o.yaml"
    my.write_text("model: MOSASRec\nn_layers: 2\nn_heads: 2\nembedding_size: 32\ninner_size: 2\nhidden_dropout_prob: 0.1\n"
                  "attn_dropout_prob: 0.1\nhidden_act: 'gelu'\nlayer_norm_eps: 1e-12\ninitializer_range: 0.02\n")
    ov.write_text(f"seed: 2020\nstate: INFO\nuse_modality: True\nreproducibility: True\ncheckpoint_dir: '{d}/saved'\n"
                  f"log_path: '{d}/log'\nshow_progress: False\nMAX_ITEM_LIST_LENGTH: 6\ndata_path: {GOLDEN_DIR}/\n"
                  "dataset: TinyInter\nimage_path: 'synthetic:64'\nencoder_name: 'clip-vit-tiny-test'\n"
                  "encoder_source: 'transformers'\nepochs: 1\ntrain_batch_size: 8\n"
                  "fine_tune_arg: {tune_scale: 37, pre_trained: True, activation: 'relu', dnn_layers: [], method: 'mean'}\n"
                  "optim_args: {modal_lr: 0.001, rec_lr: 0.001, modal_decay: 0, rec_decay: 0.1}\n"
                  "eval_batch_size: 16\ntopk: [5,10]\nmetrics: ['Recall', 'NDCG']\nvalid_metric: NDCG@10\n"
                  "metric_decimal_place: 7\neval_step: 1\nstopping_step: 30\n" + extra)
    config = Config([str(my), str(ov)])
    config["device"] = torch.device("cuda", 0)
    init_seed(2020, True)
    dataload = load_data(config)
    train, valid, test = bulid_dataloader(config, dataload)
    model = get_model(config["model"])(config, dataload).to(config["device"])
    trainer = Trainer(config, DataParallel(model))
    trainer.fit(train, valid, saved=True)
    feat = trainer.item_feature.clone()                      # the validation pass of the epoch encoded the catalogue
    ck = torch.load(trainer.saved_model_file, map_location="cpu", weights_only=False)
    return trainer.train_loss_dict[0], feat, ck, trainer, test


def test_trainer_with_the_prefix_cache_end_to_end(tmp_path):
    plain_loss, plain_feat, plain_ck, t0, _ = _trainer_run(tmp_path, "plain", "")
    assert t0.model.module.visual_encoder.prefix_cache is None          # the key is missing: images, as ever
    loss, feat, ck, t1, test = _trainer_run(tmp_path, "cached", "prefix_cache: True\n")
    enc = t1.model.module.visual_encoder
    assert enc.prefix_cache is not None and enc.prefix_cache.k == 2 and t1._prefix_cache() is enc.prefix_cache
    assert feat.shape == plain_feat.shape and (feat - plain_feat).abs().max().item() <= 3e-5
    assert abs(loss - plain_loss) <= 3e-5 * abs(plain_loss)
    out = t1.evaluate(test, load_best_model=True)                        # (load_state_dict drops the cache: this pass reads images)
    assert set(out) == {"recall@5", "recall@10", "ndcg@5", "ndcg@10"} and enc.prefix_cache is None
    assert any(k.startswith("visual_encoder.item_encoder.vision_model.encoder.layers.2.") for k in ck["state_dict"])
    # a budget of nothing: refused, and the run is the uncached one
    _, _, ck0, t2, _ = _trainer_run(tmp_path, "refused", "prefix_cache: True\nprefix_cache_gb: 0\n")
    assert t2.model.module.visual_encoder.prefix_cache is None
    assert ck0["state_dict"].keys() == plain_ck["state_dict"].keys()
    for k, v in plain_ck["state_dict"].items():
        assert torch.equal(ck0["state_dict"][k], v), k
