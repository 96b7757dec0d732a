"""Segment sums of the table gradient with very long segments cut into parts (csrc/embed_grad.hip: segsum_parts_kernel /
segsum_big_kernel behind pxr_sasrec_occ_segsum_split).  Reference: the scatter-add of nn.Embedding's backward over the three id
tensors of sasrec.py:68,88-92 (inputs: d x0; targets: +coef * out; negatives: -coef * out; padding id 0 dropped)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _batch(B, L, n_items, heavy, seed):
    rng = np.random.default_rng(seed)
    items = rng.integers(1, n_items, size=(B, 2, L + 1))
    hot = rng.random((B, 2, L + 1))
    for k, (item, frac) in enumerate(heavy):
        items[(hot >= sum(f for _, f in heavy[:k])) & (hot < sum(f for _, f in heavy[:k + 1]))] = item
    items[:, 0, :3][rng.random((B, 3)) < 0.4] = 0          # left padding
    return torch.from_numpy(items).cuda()


def _dense_ref(items, dx0, out, coef, n_items):
    B, _, W = items.shape
    L, D = W - 1, out.shape[-1]
    g = torch.zeros(n_items, D, dtype=torch.float64, device="cuda")
    g.index_add_(0, items[:, 0, :L].reshape(-1), dx0.double().view(-1, D))
    g.index_add_(0, items[:, 0, 1:].reshape(-1), (coef.double().view(-1, 1) * out.double().view(-1, D)))
    g.index_add_(0, items[:, 1, 1:].reshape(-1), -(coef.double().view(-1, 1) * out.double().view(-1, D)))
    g[0] = 0
    return g


@pytest.mark.parametrize("B,L,D,heavy", [(256, 50, 512, [(7, 0.30), (11, 0.05), (13, 0.035)]),      # ~11 500 / 1 900 / 1 300 occurrences
                                         (300, 20, 256, [(5, 0.5)]),
                                         (64, 50, 512, [(9, 0.08)]),                               # ~770 occurrences: nothing above the split
                                         (700, 50, 384, [(3, 0.02), (4, 0.0125)])])                 # D = 384: 5 groups of 96 lanes
def test_split_segment_sums_equal_the_one_launch_sums(B, L, D, heavy):
    from pixelrec_amd import ops

    n_items = 5000
    items = _batch(B, L, n_items, heavy, seed=B + D)
    g = torch.Generator(device="cuda").manual_seed(1)
    dx0 = torch.randn(B, L, D, device="cuda", generator=g)
    out = torch.randn(B, L, D, device="cuda", generator=g)
    coef = torch.randn(B, L, device="cuda", generator=g)
    cap = B * (2 * L + 1)
    ws = torch.empty(ops.occ_ws_bytes(B, L), dtype=torch.uint8, device="cuda")
    need2 = ops.occ_split_ws_bytes(B, L, D)
    assert need2 > 0
    ws2 = torch.zeros(need2, dtype=torch.uint8, device="cuda")
    one, two, again = (ops.SparseRows(cap, D, "cuda") for _ in range(3))
    for sp, w2 in ((one, None), (two, ws2), (again, ws2)):
        sp.rows.fill_(float("nan"))
        ops.occ_sort(items, L, None, n_items, sp, ws)
        ops.sasrec_occ_segsum(ws, dx0, out, coef, n_items, sp, 1.0, ws2=w2)
        assert int(ws2[:8].view(torch.int32)[0]) == 0          # the cursor is back at zero after every call
    n = one.count()
    assert n == two.count() == again.count() and torch.equal(one.idx[:n], two.idx[:n])
    assert torch.equal(two.rows[:n], again.rows[:n])           # bit-reproducible
    ref = _dense_ref(items, dx0, out, coef, n_items)[one.idx[:n]]
    cnt = torch.bincount(torch.cat([items[:, 0, :L].reshape(-1), items[:, 0, 1:].reshape(-1), items[:, 1, 1:].reshape(-1)]), minlength=n_items)[one.idx[:n]]
    big = cnt > 1024
    assert int(big.sum()) == sum(1 for _, f in heavy if f * 3 * B * L * 0.95 > 1024)
    assert torch.equal(one.rows[:n][~big], two.rows[:n][~big])  # rows below the split: the same kernel path, the same bits
    scale = ref.abs().max(dim=1, keepdim=True).values.clamp_min(1.0)
    e1 = ((one.rows[:n].double() - ref).abs() / scale).max().item()
    e2 = ((two.rows[:n].double() - ref).abs() / scale).max().item()
    assert e2 < 3e-6 and e2 <= 2 * e1 + 1e-7, (e1, e2)
    assert torch.isfinite(two.rows[:n]).all()


def test_training_step_uses_the_split_route_for_big_batches_only(monkeypatch):
    from pixelrec_amd import synth
    from pixelrec_amd.model import SASRec

    cfg = {"n_layers": 1, "n_heads": 2, "embedding_size": 256, "inner_size": 1, "hidden_dropout_prob": 0.0, "attn_dropout_prob": 0.0,
           "hidden_act": "gelu", "layer_norm_eps": 1e-12, "initializer_range": 0.02, "MAX_ITEM_LIST_LENGTH": 50, "seed": 1}

    class DL:
        item_num = 3000

    rng = np.random.default_rng(0)
    losses = {}
    for B in (32, 256):
        for env in ("0", "auto"):
            monkeypatch.setenv("PXR_SEGSUM_SPLIT", env)
            torch.manual_seed(0)
            m = SASRec(cfg, DL()).cuda().train()
            items, mask = synth.train_batch(3000, B, 50, np.random.default_rng(B), synth.ZipfItems(3000))
            loss = m((torch.from_numpy(items).cuda(), torch.from_numpy(mask).cuda()))
            loss.backward()
            assert (m._occ_ws2 is not None) == (env == "auto" and B == 256)
            losses[B, env] = m.sparse_table_grad.to_dense(3000)
        a, b = losses[B, "0"], losses[B, "auto"]
        assert (a - b).abs().max().item() <= 2e-6 * max(1.0, a.abs().max().item())
