"""DVBPR on the MI355X, at 224 x 224 with at most 6 images a step (9 in evaluation): the native step against the float64 values of
tests/golden/dvbpr_tiny.npz (the REFERENCE's own class, tools/make_golden_dvbpr.py) in both input forms, the head alone, dropout
with regenerated masks, the optimizer, main.py.

The 4x rule.  Yardstick of a stored tensor = the reference's own float32 error |reference float32 - reference float64|, the maximum
over the tensor, stored in the fixture (for the scalar loss max(that, 2^-23 |loss|)).  The native result may err from the float64
value by at most 4 x the yardstick -- the factor tests/test_gpu_gemm_b3.py gives one fp32 path over another.
Every comparison prints `DVBPR_RATIO name error/yardstick`.

One floor, and the ratio that forced it.  The stored L2 norm of a large weight gradient is a scalar like the loss, and its yardstick is
ONE draw of the reference's error, not a maximum over a tensor: for b0's fcs.0.weight it is 1.75e-8 (2.1e-8 of the norm, a fifth of
what the other eleven norms have, 6.8e-8 .. 1.5e-7), and the native norm, off by 7.6e-8 (9.3e-8 of the norm, like the others), measured
4.33 x that on the MI355X in the batcher form (3.72 x in the reference form).  So the norms get the loss's own floor, max(ref_err,
2^-23 |norm|); nothing else has a floor.  Largest ratios measured on the MI355X with it: 2.63 (b1.rows.theta_users.weight),
2.23 (b0.sample fcs.1.weight; 2.34 in the batcher form), 1.52 (b0.rows.theta_users.weight), 1.44 (eval.item_feature), 1.36
(b1.grad fcs.2.weight); loss 0.67, scores 0.48; with dropout 0.5: 1.83 (fcs.1.weight), 1.37, 1.34, loss 1.19.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import dropout_rng
from pixelrec_amd import ops
from tests import dvbpr_restate as R
from tests.mo_common import FOUR, GOLD, ROOT, assert_optimizer_state_round_trips, assert_two_fresh_models_agree, bits
from tests.test_dvbpr_cpu import build_model, load_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR = 4.0
TABLES = ("theta_users.weight", "gamma_users.weight", "gamma_items.weight")


def build_from_fixture(dropout=0.0):
    g, state, images, (U, I, Dh, B) = load_fixture()
    m = build_model(U, I, Dh, dropout)
    m.load_state_dict(state, strict=True)
    return m.to(DEV).train()


def batch_input(g, images, j, form):
    user, item = torch.from_numpy(g[f"b{j}.user"]), torch.from_numpy(g[f"b{j}.item_id"])
    if form == "reference":
        return user.to(DEV), item.to(DEV), images[item].to(DEV)                    # [B, 2, 3, 224, 224]
    ids, index = R.dedup(item.numpy())
    ids = torch.from_numpy(ids)
    return user.to(DEV), torch.from_numpy(index).to(DEV), images[ids].to(DEV), ids.to(DEV)


def native_step(m, inp):
    """-> (loss, {state_dict key: gradient on the host}); the tables' gradient dense, from the sparse rows."""
    loss = m(inp)
    loss.backward()
    grads = {R.ENC + n: p.grad.detach().cpu().clone() for n, p in m.visual_encoder.named_parameters()}
    dense = m.sparse_table_grad.to_dense(m.lazy_table().shape[0]).cpu()
    for k, (lo, hi) in m.table_parameter_spans().items():
        grads[k] = dense[lo:hi]
    ops.raise_on_bad_indices(loss.device)
    return loss.detach().cpu(), grads


def check(name, got, want, yard, worst):
    err = float((got.double() - torch.as_tensor(want).double()).abs().max())
    ratio = err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))
    print(f"DVBPR_RATIO {name} {ratio:.3f}   (error {err:.3e}, yardstick {yard:.3e})")
    worst.append((ratio, name))


def compare_with_stored(g, j, loss, grads, worst):
    lw = float(g[f"b{j}.loss"][0])
    check(f"b{j}.loss", loss, lw, max(float(g[f"ref_err.b{j}.loss"]), 2.0 ** -23 * abs(lw)), worst)
    user, item = g[f"b{j}.user"], g[f"b{j}.item_id"]
    for k, gr in grads.items():
        if f"b{j}.grad.{k}" in g:
            check(f"b{j}.grad.{k}", gr, g[f"b{j}.grad.{k}"], float(g[f"ref_err.b{j}.grad.{k}"]), worst)
        elif k in TABLES:
            rows = torch.from_numpy(np.unique(user if "users" in k else item.reshape(-1)))
            check(f"b{j}.rows.{k}", gr[rows], g[f"b{j}.rows.{k}"], float(g[f"ref_err.b{j}.rows.{k}"]), worst)
            rest = torch.ones(gr.shape[0], dtype=torch.bool)
            rest[rows] = False
            assert not gr[rest].any()                                             # no other row has a gradient
        else:
            nw = float(g[f"b{j}.norm.{k}"][0])                                     # a scalar, like the loss: the same floor (module docstring)
            check(f"b{j}.norm.{k}", gr.double().norm().reshape(1), nw, max(float(g[f"ref_err.b{j}.norm.{k}"]), 2.0 ** -23 * nw), worst)
            idx = torch.from_numpy(R.sample_index(gr.numel()))
            check(f"b{j}.sample.{k}", gr.reshape(-1)[idx], g[f"b{j}.sample.{k}"], float(g[f"ref_err.b{j}.sample.{k}"]), worst)


def assert_within(worst):
    worst.sort(reverse=True)
    print("DVBPR_WORST " + ", ".join(f"{n} {r:.3f}" for r, n in worst[:5]))
    bad = [(n, r) for r, n in worst if not r <= FACTOR]
    assert not bad, f"more than {FACTOR} x the reference's own float32 error: {bad[:8]}"


@pytest.mark.parametrize("form", ["batcher", "reference"])
def test_fixture(form):
    """Loss, every stored gradient / sample / norm, compute_item and the scores (predict, and the packed fused-scoring operands)
    against the fixture's float64 values under the 4x rule.  Largest ratios measured on the MI355X: see README.md "DVBPR"."""
    g, state, images, (U, I, Dh, B) = load_fixture()
    m = build_from_fixture()
    worst = []
    for j in range(2):
        loss, grads = native_step(m, batch_input(g, images, j, form))
        assert set(grads) == set(state)
        compare_with_stored(g, j, loss, grads, worst)
    m.eval()
    feat = m.compute_item(images.to(DEV))
    check("eval.item_feature", feat.cpu(), g["eval.item_feature"], float(g["ref_err.eval.item_feature"]), worst)
    users = torch.arange(U, device=DEV)
    check("eval.scores", m.predict(users, feat).cpu(), g["eval.scores"], float(g["ref_err.eval.scores"]), worst)
    m.set_item_feature(feat)
    q, items = m.encode_last(users)[1].cpu().double(), m.scoring_item_matrix().cpu().double()
    assert q.shape[1] == items.shape[1] == ops.vbpr_packed_width(Dh) and not items[:, 2 * Dh:].any()     # a zero bias column
    check("eval.scores.packed", q @ items.t(), g["eval.scores"], float(g["ref_err.eval.scores"]), worst)
    assert_within(worst)


def test_both_input_forms_and_the_dedup_are_one_function():
    """The reference form encodes 2B = 6 images, the batcher form the M = 5 distinct ones and sums the copies' gradients: with
    dropout 0 both are within 4 x the yardstick of the same float64 values (test_fixture), so within 8 x of each other."""
    g, state, images, _ = load_fixture()
    a = native_step(build_from_fixture(), batch_input(g, images, 0, "batcher"))
    b = native_step(build_from_fixture(), batch_input(g, images, 0, "reference"))
    assert abs(float(a[0]) - float(b[0])) <= 2 * FACTOR * max(float(g["ref_err.b0.loss"]), 2.0 ** -23 * float(a[0]))
    for k in a[1]:
        key = [f"ref_err.b0.{kind}.{k}" for kind in ("grad", "rows", "sample") if f"ref_err.b0.{kind}.{k}" in g][0]
        idx = torch.from_numpy(R.sample_index(a[1][k].numel())) if "sample" in key else None
        x, y = (a[1][k].reshape(-1)[idx], b[1][k].reshape(-1)[idx]) if idx is not None else (a[1][k], b[1][k])
        if k in TABLES:
            rows = torch.from_numpy(np.unique(g["b0.user"] if "users" in k else g["b0.item_id"].reshape(-1)))
            x, y = x[rows], y[rows]
        assert float((x.double() - y.double()).abs().max()) <= 2 * FACTOR * float(g[key]), k


def test_two_fresh_models_give_the_same_bits():
    g, state, images, _ = load_fixture()
    assert_two_fresh_models_agree(build_from_fixture, lambda m, j: native_step(m, batch_input(g, images, j, "batcher")),
                                  1 + len(state))


# ------------------------------------------------------------------------------------------------------------ the head alone
def head_case(Dh, seed):
    """U = 6, I = 8, B = 5, M = 7: a repeated user, an item and a position shared by a positive and a negative, position 0 in use,
    position 6 read by nobody.  Values scaled so that x_b is O(1)."""
    g = torch.Generator().manual_seed(seed)
    U, I, B, M = 6, 8, 5, 7
    P = {"theta_users.weight": torch.rand(U, Dh, generator=g) / Dh ** 0.5, "gamma_users.weight": torch.rand(U, Dh, generator=g) / Dh ** 0.5,
         "gamma_items.weight": torch.rand(I, Dh, generator=g)}
    E = torch.randn(M, Dh, generator=g)
    user = torch.tensor([0, 3, 3, 5, 1])
    item = torch.tensor([[1, 4], [4, 7], [2, 0], [6, 1], [0, 2]])
    index = torch.tensor([[0, 3], [3, 5], [1, 0], [4, 2], [5, 1]])
    return (U, I, B, M), P, E, user, item, index


@pytest.mark.parametrize("Dh", [16, 2048])
def test_head_alone_against_float64(Dh):
    """loss_from_embeddings against float64 autograd.  Bounds from the arithmetic: x_b is four dot products of Dh terms, summed per lane
    in Dh / 64 + 1 steps and then through a 6-level tree: |dx| <= (Dh / 16 + 8) 2^-24 S with S = the largest sum of |terms| of an x_b;
    |d loss| <= |dx| + 2^-22; a coefficient c_b = -sigmoid(-x_b) / B errs by at most |dx| / (4 B) + a few ulp, and a gradient row sums at
    most 2B terms c_b v: |d grad| <= (|dx| / 4 + 2^-21) 2 max|v|."""
    (U, I, B, M), P, E, user, item, index = head_case(Dh, 7 + Dh)
    m = build_model(U, I, Dh)
    sd = m.state_dict()
    sd.update(P)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).train()
    Ed = E.to(DEV).requires_grad_(True)
    loss = m.loss_from_embeddings(Ed, user.to(DEV), item.to(DEV), index.to(DEV))
    loss.backward()
    dense = m.sparse_table_grad.to_dense(m.lazy_table().shape[0]).cpu()
    ops.raise_on_bad_indices(Ed.device)
    P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
    E64 = E.double().requires_grad_(True)
    loss64 = R.loss_of(P64, E64, user, item, index)
    loss64.backward()
    gu, tu, gi, e = P["gamma_users.weight"][user].double(), P["theta_users.weight"][user].double(), P["gamma_items.weight"][item].double(), E[index].double()
    S = float(((gu[:, None] * gi).abs().sum(-1) + (tu[:, None] * e).abs().sum(-1)).sum(-1).max())
    dx = (Dh / 16 + 8) * 2.0 ** -24 * S
    assert abs(float(loss) - float(loss64)) <= dx + 2.0 ** -22
    vmax = max(float(v.abs().max()) for v in list(P.values()) + [E])
    tol = (dx / 4 + 2.0 ** -21) * 2 * vmax
    dE = Ed.grad.cpu()
    assert float((dE.double() - E64.grad).abs().max()) <= tol
    assert float(dE[0].abs().max()) > 0 and float(E64.grad[0].abs().max()) > 0      # position 0 is a real image: its gradient is there
    assert not dE[6].any() and torch.equal(bits(dE[6]), torch.zeros(Dh, dtype=torch.int32))      # a row nobody reads: +0.0
    for k, (lo, hi) in m.table_parameter_spans().items():
        assert float((dense[lo:hi].double() - P64[k].grad).abs().max()) <= tol, k
    assert not dense[0].any()


def test_bad_ids_raise_index_error():
    (U, I, B, M), P, E, user, item, index = head_case(16, 1)
    m = build_model(U, I, 16).to(DEV).train()
    Ed = E.to(DEV)
    with torch.no_grad():
        float(m.loss_from_embeddings(Ed, user.to(DEV), item.to(DEV), index.to(DEV)))
        ops.raise_on_bad_indices(Ed.device)                                        # clean ids: nothing raised
        for what, (u, it, ix) in {"position": (user, item, index.clone().index_put_((torch.tensor(2), torch.tensor(1)), torch.tensor(M))),
                                  "negative position": (user, item, index.clone().index_put_((torch.tensor(0), torch.tensor(0)), torch.tensor(-1))),
                                  "user": (user.clone().index_put_((torch.tensor(1),), torch.tensor(U)), item, index),
                                  "item": (user, item.clone().index_put_((torch.tensor(4), torch.tensor(0)), torch.tensor(I)), index)}.items():
            m.loss_from_embeddings(Ed, u.to(DEV), it.to(DEV), ix.to(DEV))
            with pytest.raises(IndexError):
                ops.raise_on_bad_indices(Ed.device)
    with pytest.raises(ValueError):
        m.loss_from_embeddings(Ed, user.to(DEV), item.to(DEV)[:, :1], index.to(DEV))
    with pytest.raises(ValueError):
        m.visual_encoder(torch.zeros(2, 3, 64, 64, device=DEV))


# ------------------------------------------------------------------------------------------------------------ dropout
def test_dropout_matches_the_restatement_with_regenerated_masks():
    """dropout_prob = 0.5: the masks of step 0 regenerated by oracle/dropout_rng (stream k for fcs.k, element index i * width + j over the
    [M, width] output, seed 2020 + 0 backward passes) go into the float64 restatement; yardstick = the float32 restatement's distance
    from it under the same masks, the 4x rule as in test_fixture.  compute_item in eval mode has the dropout-0 model's bits."""
    g, state, images, (U, I, Dh, B) = load_fixture()
    p = 0.5
    m = build_from_fixture(dropout=p)
    j = 0
    inp = batch_input(g, images, j, "batcher")
    loss, grads = native_step(m, inp)
    ids, index = R.dedup(g[f"b{j}.item_id"])
    M = len(ids)
    masks = [torch.from_numpy(dropout_rng.keep_mask(2020, k, (M, w), p)) for k, w in enumerate((R.FC, R.FC, Dh))]
    assert all(0.2 < float(mk.float().mean()) < 0.8 for mk in masks)
    runs = {}
    for dtype in (torch.float32, torch.float64):
        P = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in state.items()}
        l = R.loss_of(P, R.cnnf(P, images[torch.from_numpy(ids)], masks=masks, p=p), g[f"b{j}.user"], g[f"b{j}.item_id"], index)
        l.backward()
        runs[dtype] = (l.detach().double(), {k: P[k].grad.double() for k in P})
    l32, g32 = runs[torch.float32]
    l64, g64 = runs[torch.float64]
    assert abs(float(l64) - float(g["b0.loss"][0])) > 1e-4                         # the masks changed the function
    worst = []
    check("drop.loss", loss, l64, max(abs(float(l32 - l64)), 2.0 ** -23 * abs(float(l64))), worst)
    for k in state:
        check("drop.grad." + k, grads[k], g64[k], float((g32[k] - g64[k]).abs().max()), worst)
    assert_within(worst)
    m.eval()
    plain = build_from_fixture().eval()
    x = images[:3].to(DEV)
    assert torch.equal(bits(m.compute_item(x)), bits(plain.compute_item(x)))


# ------------------------------------------------------------------------------------------------------------ the optimizer
def test_one_optimizer_step_moves_the_batch_rows_and_the_encoder():
    """Four optim_args: OptimizerGroup(VisualAdamW over 16 encoder tensors, PxrAdamW over the tables).  One step changes every encoder
    tensor and, with rec_decay 0, exactly the batch's rows of the three tables; the lazy and the dense table schedule give the same bits
    (with the shipped decay too); the torch-layout state has groups [16, 3] and round-trips through torch.optim.AdamW."""
    from pixelrec_amd.optim import OptimizerGroup, PxrAdamW, VisualAdamW
    from tests.mo_common import trainer_optimizer

    g, state, images, (U, I, Dh, B) = load_fixture()
    inp = lambda: batch_input(g, images, 0, "batcher")
    user, item = g["b0.user"], g["b0.item_id"]

    def run(opt_of):
        m = build_from_fixture()
        opt = opt_of(m)
        opt.zero_grad()
        m(inp()).backward()
        opt.step()
        opt.flush()
        return m, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}

    m, after = run(lambda m: trainer_optimizer(m, {**FOUR, "rec_decay": 0.0}))
    assert isinstance(trainer_optimizer(build_from_fixture(), FOUR), OptimizerGroup)
    for k, v in state.items():
        moved = (after[k] != v).reshape(v.shape[0], -1).any(dim=1)
        if k in TABLES:
            rows = np.unique(user if "users" in k else item.reshape(-1))
            assert sorted(torch.nonzero(moved).reshape(-1).tolist()) == rows.tolist(), k
        else:
            assert bool((after[k] != v).any()), k
    lazy = run(lambda m: trainer_optimizer(m, FOUR))[1]
    dense = run(lambda m: OptimizerGroup(VisualAdamW(m.visual_encoder, lr=FOUR["modal_lr"], weight_decay=FOUR["modal_decay"]),
                                         PxrAdamW(m, lr=FOUR["rec_lr"], weight_decay=FOUR["rec_decay"], table_update="dense")))[1]
    for k in state:
        assert torch.equal(bits(lazy[k]), bits(dense[k])), k
    assert_optimizer_state_round_trips(build_from_fixture, lambda m: m(inp()).backward(), [16, 3], list(range(19)),
                                       rec=lambda m: [m.get_parameter(k) for k in TABLES])


# ------------------------------------------------------------------------------------------------------------ main.py
def test_main_py_trains_evaluates_and_the_checkpoint_reloads(tmp_path):
    """main.py with configs/PixelNet/dvbpr.yaml's keys on TinyInter with synthetic 224 x 224 images, two epochs, in a subprocess under
    its own timeout (the overlay is this test's: mo_common.run_main_py is written for 64-pixel images): finite losses that change,
    Recall@10 and NDCG@10 from the reloaded checkpoint, whose keys are the reference's, in its order, and load with strict=True."""
    from pixelrec_amd.config import Config
    from pixelrec_amd.data import load_data
    from pixelrec_amd.utils import get_model

    shipped = open(os.path.join(ROOT, "configs", "PixelNet", "dvbpr.yaml")).read()
    assert re.findall(r"^(\w+):", shipped, flags=re.M) == ["model", "embedding_size", "dropout_prob", "conv_workspace_mb"]
    my, ov = tmp_path / "m.yaml", tmp_path / "o.yaml"
    my.write_text("model: DVBPR\nembedding_size: 32\ndropout_prob: 0.5\nconv_workspace_mb: 64\n")
    ov.write_text(f"seed: 2020\nstate: INFO\nuse_modality: True\nreproducibility: True\ncheckpoint_dir: '{tmp_path}/saved'\n"
                  f"log_path: '{tmp_path}/log'\nshow_progress: False\nMAX_ITEM_LIST_LENGTH: 6\ndata_path: {GOLD}/\n"
                  "dataset: TinyInter\nimage_path: 'synthetic:224'\nencoder_name: 'clip-vit-tiny-test'\n"
                  "encoder_source: 'transformers'\nepochs: 2\ntrain_batch_size: 32\n"
                  "fine_tune_arg: {tune_scale: 37, pre_trained: True, activation: 'relu', dnn_layers: [], method: 'mean'}\n"
                  "optim_args: {modal_lr: 0.0001, rec_lr: 0.001, modal_decay: 0, rec_decay: 0.1}\n"
                  "eval_batch_size: 16\ntopk: [5,10]\nmetrics: ['Recall', 'NDCG']\nvalid_metric: NDCG@10\n"
                  "metric_decimal_place: 7\neval_step: 1\nstopping_step: 30\n")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "OMP_NUM_THREADS")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--device", "0", "--config_file", str(my), str(ov)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    epochs = [float(x) for x in re.findall(r"epoch \d+ training \[time: [0-9.]+s, train loss: ([0-9.]+)\]", out)]
    assert len(epochs) == 2 and all(np.isfinite(e) for e in epochs) and epochs[0] != epochs[1], out[-3000:]
    assert "Loading model structure and parameters from" in out, out[-3000:]
    for metric in ("recall@10", "ndcg@10"):
        mm = re.search(r"test result: .*?'%s', ([0-9.]+)\)" % metric, out)
        assert mm is not None and 0.0 <= float(mm.group(1)) <= 1.0, out[-2000:]
    print("epoch losses", epochs, re.search(r"test result: .*", out).group(0))
    files = os.listdir(tmp_path / "saved")
    assert len(files) == 1
    ck = torch.load(tmp_path / "saved" / files[0], map_location="cpu", weights_only=False)
    config = Config([str(my), str(ov)])
    data = load_data(config)
    data.build()
    assert list(ck["state_dict"]) == list(R.state_shapes(16, data.user_num, data.item_num))
    assert {k: tuple(v.shape) for k, v in ck["state_dict"].items()} == dict(R.state_shapes(16, data.user_num, data.item_num))
    assert [len(x["params"]) for x in ck["optimizer"]["param_groups"]] == [16, 3]          # the reference's two groups
    fresh = get_model("DVBPR")(config, data)
    fresh.load_state_dict(ck["state_dict"], strict=True)
