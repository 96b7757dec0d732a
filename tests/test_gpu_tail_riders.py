"""Tail riders: the closing reductions of a backward pass (LayerNorm dgamma|dbeta, bias and position column sums, the dropout
counter bump, the loss sum) run on extra workgroups of the segment-sum launch of the table gradient (csrc/reduce_multi.cuh,
csrc/embed_grad.hip) instead of as launches of their own.  Nothing in the arithmetic moves, so every comparison here is
PXR_TAIL_RIDERS=0 against =1 in one process with torch.equal."""
import numpy as np
import pytest
import torch

CFG = {"n_layers": 2, "n_heads": 2, "embedding_size": 64, "inner_size": 2, "hidden_dropout_prob": 0.1, "attn_dropout_prob": 0.1,
       "hidden_act": "gelu", "layer_norm_eps": 1e-12, "initializer_range": 0.02, "MAX_ITEM_LIST_LENGTH": 5, "seed": 2020}
N_ITEMS, B, L = 50, 3, 5


class DL:
    item_num = N_ITEMS


def _batch(shift=0):
    """items [3, 2, 6], mask [3, 5].  Row 7: five occurrences (three inputs, two targets).  Row 3: an input and a target of sequence
    0 and a negative of sequence 1.  Sequence 2 has two items (one input, one target), the rest is padding."""
    items = np.zeros((B, 2, L + 1), dtype=np.int64)
    mask = np.zeros((B, L), dtype=np.int64)
    items[0, 0] = [7, 7, 7, 3, 9, 11]
    items[0, 1, 1:] = [12, 13, 15, 16, 14]
    items[1, 0] = [20, 21, 22, 23, 24, 25]
    items[1, 1, 1:] = [3, 31, 32, 33, 34]
    items[2, 0, 4:] = [40, 41]
    items[2, 1, 5] = 42
    mask[0] = mask[1] = 1
    mask[2, 4] = 1
    if shift:      # another batch of the same geometry: every id moved, padding kept
        items = np.where(items > 0, (items + shift - 1) % (N_ITEMS - 1) + 1, 0)
    return torch.from_numpy(items), torch.from_numpy(mask)


def _model(cfg=CFG, defer_loss=False):
    from pixelrec_amd.model import SASRec
    from pixelrec_amd.optim import PxrAdamW

    torch.manual_seed(11)
    model = SASRec(cfg, DL()).cuda().train()
    model.defer_weight_grad_join = True           # every backward below is followed by opt.step(): the rows_apply_handle route
    model.defer_loss_reduce = defer_loss
    opt = PxrAdamW(model, lr=1e-3, weight_decay=0.1, table_update="lazy")
    return model, opt


def _state(model, opt, loss):
    torch.cuda.synchronize()
    out = {"loss": loss.detach().clone().view(1), "gflat": model.flat_parameters()[1].clone(), "drop": model._drop_dev.clone()}
    out.update({"p." + k: v.detach().clone() for k, v in model.state_dict().items()})
    out.update({"o." + k: v.detach().clone() for k, v in opt.state_dict().items() if torch.is_tensor(v)})
    out.update(tm=opt._tm.clone(), tv=opt._tv.clone(), last=opt._last.clone())
    return out


def _one_step(monkeypatch, knob, cfg=CFG, defer_loss=False, steps=1):
    monkeypatch.setenv("PXR_TAIL_RIDERS", knob)
    model, opt = _model(cfg, defer_loss)
    for k in range(steps):
        items, mask = (t.cuda() for t in _batch(3 * k))
        opt.zero_grad()
        loss = model((items, mask))
        loss.backward()
        opt.step()
    return _state(model, opt, loss)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- 1. one training step -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])      # bf16x3 = the default mode, whose sequence block runs on h2 planes
def test_one_training_step_is_bit_identical(monkeypatch, mode):
    """Loss, every gradient of the flat buffer (LN, biases, positions), the touched table rows with moments and last[], the dropout
    step counter, after two steps (the second one runs the stale-scale h2 path): knob off == knob on."""
    from pixelrec_amd import ops

    prev = ops.set_gemm_mode(mode)
    try:
        off = _one_step(monkeypatch, "0", steps=2)
        on = _one_step(monkeypatch, "1", steps=2)
    finally:
        ops.set_gemm_mode(prev)
    _same(off, on)
    assert int(on["drop"]) == 2 and float(on["gflat"].abs().sum()) > 0 and int((on["last"] == 2).sum()) > 0


# ---- 2. odd rider geometry (ops level) -----------------------------------------------------------------------------------------
def _carrier(D):
    """A phase-2 call at the batch of test 1 and width D, with everything it reads."""
    from pixelrec_amd import ops

    items = _batch()[0].cuda()
    g = torch.Generator(device="cuda").manual_seed(D)
    dx0, out = (torch.randn(B, L, D, device="cuda", generator=g) for _ in range(2))
    coef = torch.randn(B, L, device="cuda", generator=g)
    sp = ops.SparseRows(B * (2 * L + 1), D, "cuda", packed=True)
    ws = torch.empty(ops.occ_ws_bytes(B, L), dtype=torch.uint8, device="cuda")
    ops.occ_sort(items, L, None, N_ITEMS, sp, ws)
    return lambda rider=None: (ops.sasrec_occ_segsum(ws, dx0, out, coef, N_ITEMS, sp, 1.0, rider=rider), sp)[1]


def _problems(n, D, seed):
    """n partial buffers: LayerNorm-shaped ones ([P, 2D] -> dgamma | dbeta) alternating with single-output ones of other widths."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    probs = []
    for i in range(n):
        if i % 2 == 0:
            P, N = 3 + 5 * i, 2 * D
            outs = (torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda"), D)
        else:
            P, N = 130 + i, D + 1 + i                     # P > 128: the unrolled part of the column sum; N no multiple of 16
            outs = (torch.zeros(N, device="cuda"), None, 0)
        probs.append((torch.randn(P, N, device="cuda", generator=g), P, N, *outs))
    return probs


def _collect(probs):
    from pixelrec_amd import ops

    d = ops.DeferredReductions()
    for part, P, N, oa, ob, split in probs:
        d.add(part, P, N, oa, ob, split)
    return d


def _outputs(probs):
    torch.cuda.synchronize()
    return [t.clone() for p in probs for t in (p[3], p[4]) if t is not None]


@pytest.mark.gpu
@pytest.mark.parametrize("D,n", [(24, 1), (8, 1), (24, 16), (24, 17)])
def test_rider_geometry(D, n):
    """2D = 48 columns are three column groups (the second rider block runs one and idles on its other half), 2D = 16 a single
    one; 16 problems fill a rider, 17 do not fit one and flush(prepare=True) leaves them to the stand-alone launches."""
    from pixelrec_amd import ops

    run = _carrier(D)
    ref_rows = run().rows.clone()
    bump = torch.full((1,), 41, dtype=torch.int64, device="cuda")
    ref = _problems(n, D, 5)
    assert _collect(ref).flush(bump=bump) is True
    want = _outputs(ref)

    got = _problems(n, D, 5)
    d = _collect(got)
    rider = d.flush(bump=bump, prepare=True)
    if n > 16:
        assert rider is None and len(d.items) == n        # untouched: the caller flushes as usual
        assert d.flush(bump=bump) is True
        sp = run()
    else:
        assert isinstance(rider, ops.TailRider) and not d.items and len(rider.items) == n
        assert all(float(t.abs().sum()) == 0 for t in _outputs(got))      # prepared, not launched
        sp = run(rider)
    have = _outputs(got)
    assert len(want) == len(have) and all(torch.equal(a, b) for a, b in zip(want, have))
    assert torch.equal(sp.rows, ref_rows)                  # the carrier's sums do not notice their rider
    assert int(bump) == 43


@pytest.mark.gpu
def test_rider_with_the_loss_sum_alone():
    """A rider of no reductions and one loss problem (B = 300 rows: more than the 256 summing threads)."""
    from pixelrec_amd import ops

    Bq, Lq = 300, 11
    lossrow = torch.randn(Bq * Lq, device="cuda")
    loss = torch.full((1,), float("nan"), device="cuda")
    _carrier(8)(ops.TailRider(loss=(lossrow, Bq, Lq, loss)))
    rows = lossrow.view(Bq, Lq).cpu().double().sum(1)
    assert abs(float(loss) - float(rows.sum() / Bq)) < 1e-4


# ---- 3. loss deferral ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_deferred_loss_equals_the_forward_sum(monkeypatch):
    off = _one_step(monkeypatch, "1", defer_loss=False)
    on = _one_step(monkeypatch, "1", defer_loss=True)
    knob_off = _one_step(monkeypatch, "0", defer_loss=True)       # flag on, riders off: the forward sums the loss itself
    _same(off, on)
    _same(off, knob_off)


@pytest.mark.gpu
def test_deferral_leaves_eval_and_no_grad_forwards_alone(monkeypatch):
    monkeypatch.setenv("PXR_TAIL_RIDERS", "1")
    model, opt = _model(defer_loss=True)
    items, mask = (t.cuda() for t in _batch())
    with torch.no_grad():
        a = model((items, mask)).clone()
    model.eval()
    b = model((items, mask)).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(a) and torch.equal(a, b) and float(a) > 0
    # a training forward with the flag: the loss is whatever the backward's tail writes -- the plain forward's, bit for bit
    model.train()
    loss = model((items, mask))
    loss.backward(); opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and float(loss) > 0


@pytest.mark.gpu
def test_a_tail_without_carrier_still_fills_the_loss(monkeypatch):
    """The split route of the segment sums (forced: PXR_SEGSUM_SPLIT=1 needs D >= 256) is three launches and carries nothing: the
    forward sums the loss itself, the reductions run on their own, and the knob changes nothing."""
    monkeypatch.setenv("PXR_SEGSUM_SPLIT", "1")
    cfg = dict(CFG, embedding_size=256)
    monkeypatch.setenv("PXR_TAIL_RIDERS", "1")
    model, opt = _model(cfg, defer_loss=True)
    items, mask = (t.cuda() for t in _batch())
    loss = model((items, mask))
    assert model._occ_ws2 is not None and not model._tail_has_carrier()
    torch.cuda.synchronize()
    filled = loss.detach().clone()                 # before backward
    loss.backward(); opt.step()
    on = _state(model, opt, loss)
    assert torch.equal(filled.view(1), on["loss"]) and float(filled) > 0
    off = _one_step(monkeypatch, "0", cfg=cfg, defer_loss=True)
    _same(off, on)


# ---- 4. captured step -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("knob", ["1", "0"])
def test_three_replays_equal_three_eager_steps(monkeypatch, knob):
    from pixelrec_amd.graph import GraphedTrainStep

    monkeypatch.setenv("PXR_TAIL_RIDERS", knob)
    batches = [tuple(t.cuda() for t in _batch(s)) for s in (0, 3, 6, 9)]

    def flags(m):      # what GraphedTrainStep sets on its model, for the eager twin
        m.defer_loss_reduce = True
        if getattr(m, "_split_env", None) is None:
            m.split_catch_up = True
        m.trust_optimizer_planes = True
        m.h2_stale_scales = True

    model, opt = _model()
    gstep = GraphedTrainStep(model, opt, *batches[0], warmup=1)
    assert model.defer_loss_reduce
    g_losses = [gstep(*b).clone() for b in batches[1:]]
    torch.cuda.synchronize()
    g_sd = {k: v.detach().clone() for k, v in model.state_dict().items()}

    model, opt = _model()
    flags(model)
    e_losses = []
    for b in batches:
        opt.zero_grad()
        loss = model(b)
        loss.backward()
        opt.step()
        e_losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    e_sd = model.state_dict()
    assert all(torch.equal(a.view(1), b.view(1)) for a, b in zip(g_losses, e_losses[1:]))
    assert g_sd.keys() == e_sd.keys()
    for k in g_sd:
        assert torch.equal(g_sd[k], e_sd[k]), k


# ---- 5. CPU only ----------------------------------------------------------------------------------------------------------------
def test_prepare_mode_launches_nothing(monkeypatch):
    """flush(prepare=True) on host tensors, with the library out of reach: it only hands the problems over."""
    from pixelrec_amd import lib, ops

    def no_library():
        raise AssertionError("prepare mode reached for the library")

    monkeypatch.setattr(lib, "load", no_library)
    d = ops.DeferredReductions()
    assert d.flush(prepare=True) is None                   # nothing collected
    outs = [torch.zeros(4) for _ in range(16)]
    for o in outs:
        d.add(torch.ones(3, 4), 3, 4, o)
    bump = torch.zeros(1, dtype=torch.int64)
    rider = d.flush(bump=bump, prepare=True)
    assert isinstance(rider, ops.TailRider) and len(rider.items) == 16 and rider.bump is bump and rider.loss is None and not d.items
    assert int(bump) == 0 and all(float(o.sum()) == 0 for o in outs)
    arg, keep = rider.c_arg()
    assert arg.value and keep.n == 16 and keep.P[15] == 3 and keep.N[0] == 4 and keep.out_b[0] is None and keep.loss is None
    for o in outs + [torch.zeros(4)]:
        d.add(torch.ones(3, 4), 3, 4, o)
    assert d.flush(bump=bump, prepare=True) is None and len(d.items) == 17      # more than one rider holds: left for flush()
    assert ops.TailRider().c_arg() == (None, None)


def test_rider_descriptor_matches_the_header():
    """ops._CTailRider lays its fields out as include/pxr.h declares pxr_tail_rider (names, order, array lengths)."""
    import os
    import re

    from pixelrec_amd import ops

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pxr.h")).read()
    body = re.search(r"typedef struct pxr_tail_rider \{(.*?)\} pxr_tail_rider;", text, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            m = re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*(\[(\d+)\])?\s*$", part.strip())
            names.append((m.group(1), int(m.group(3)) if m.group(3) else 1))
    fields = [(n, getattr(t, "_length_", 1)) for n, t in ops._CTailRider._fields_]
    assert names == fields


def test_a_step_with_collectives_has_no_carrier():
    """A row exchange hooked behind the segment sums (parallel.GradSync), the split workspace of big batches and BERT4Rec each
    keep the reductions as launches of their own: the forward then defers nothing."""
    from pixelrec_amd.model import SASRec

    m = SASRec(CFG, DL())
    assert m._tail_has_carrier()
    m._sparse_ready_hook = lambda: None
    assert not m._tail_has_carrier()
    m._sparse_ready_hook = None
    m._occ_ws2 = torch.zeros(1)
    assert not m._tail_has_carrier()
