"""NextItNet (pixelrec_amd/model/nextitnet.py) against the reference's own outputs (tests/golden/nextitnet_tiny.npz, written by
oracle/make_golden_nextitnet.py from REC.model.IDNet.nextitnet.NextItNet) and, at a wider shape with the lazy table optimizer,
against torch.optim.AdamW on the oracle."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "nextitnet_tiny.npz"))
N, E, K, BLOCKS, L, B = [int(x) for x in G["dims"]]
DIL = [int(d) for d in G["dilations"]]


def _config(final, e=E, blocks=BLOCKS, dil=None, l=L, k=K):
    return {"embedding_size": e, "block_num": blocks, "dilations": list(dil or DIL), "kernel_size": k, "reg_weight": 0.0,
            "final_layer": final, "MAX_ITEM_LIST_LENGTH": l, "seed": 2020}


@pytest.mark.parametrize("case", ["plain", "final"])
def test_nextitnet_matches_the_reference(case):
    from pixelrec_amd.model import NextItNet

    class DL:
        item_num = N

    m = NextItNet(_config(case == "final"), DL())
    pre = case + "/param/"
    ref = {k[len(pre):]: torch.from_numpy(G[k]) for k in G.files if k.startswith(pre)}
    assert list(m.state_dict().keys()) == list(ref.keys())                     # the reference's names AND order
    m.load_state_dict(ref, strict=True)
    m = m.cuda().train()
    items, mask = torch.from_numpy(G["items"]).cuda(), torch.from_numpy(G["masked_index"]).cuda()
    loss = m((items, mask))
    loss.backward()
    assert abs(float(loss.detach()) - float(G[case + "/loss"])) < 5e-6
    for name, p in m.named_parameters():
        want = torch.from_numpy(G[f"{case}/grad/{name}"])
        if name == "item_embedding.weight":
            sp = m.sparse_table_grad
            n = int(sp.n)
            got = torch.zeros_like(want)
            got[sp.idx[:n].cpu()] = sp.rows[:n].cpu()
        else:
            got = p.grad.cpu()
        err = (got - want).abs().max().item()
        assert err <= 2e-6 + 2e-5 * want.abs().max().item(), (name, err)
    m.eval()
    with torch.no_grad():
        scores = m.predict(torch.from_numpy(G["item_seq"]).cuda(), m.compute_item_all())
        assert (scores.cpu() - torch.from_numpy(G[case + "/scores"])).abs().max().item() < 2e-5
        assert abs(float(m((items, mask))) - float(G[case + "/loss"])) < 5e-6


def test_causal_im2col_and_col2im_are_transposes_of_each_other():
    from pixelrec_amd import ops
    g = torch.Generator().manual_seed(0)
    for (b, l, c, k, d) in ((3, 7, 8, 3, 1), (2, 10, 12, 3, 4), (2, 5, 4, 2, 8), (1, 9, 16, 4, 2)):
        x = torch.randn(b, l, c, generator=g)
        y = torch.randn(b, l, c * k, generator=g)
        xc = ops.causal_im2col(x.cuda(), k, d).cpu()
        want = torch.zeros(b, l, c, k)
        for j in range(k):
            s = (k - 1 - j) * d
            if s < l:
                want[:, s:, :, j] = x[:, :l - s]
        assert torch.equal(xc, want.reshape(b, l, c * k))
        dx = ops.causal_col2im(y.cuda(), k, d).cpu()
        assert abs(float((xc * y).sum()) - float((x * dx).sum())) < 1e-3 * max(1.0, float((xc * y).abs().sum()))   # <A x, y> == <x, A^T y>


def test_nextitnet_training_steps_follow_torch_adamw_on_the_oracle():
    """emb 64, kernel 3, 2 x [1, 4] dilations (the shipped pattern), L = 10, 500 items: four PxrAdamW steps (sparse table
    gradient, lazy schedule) against torch.optim.AdamW over the oracle."""
    from oracle import nextitnet_oracle as NO
    from pixelrec_amd.model import NextItNet
    from pixelrec_amd.optim import PxrAdamW

    n, e, l, b = 500, 64, 10, 8
    dil = [1, 4]
    rng = np.random.default_rng(6)

    class DL:
        item_num = n

    torch.manual_seed(3)
    m = NextItNet(_config(False, e=e, blocks=2, dil=dil, l=l), DL())
    ref = {k: v.detach().clone().double().requires_grad_(True) for k, v in m.state_dict().items()}
    m = m.cuda().train()
    opt = PxrAdamW(m, lr=1e-3, weight_decay=0.1)
    topt = torch.optim.AdamW(list(ref.values()), lr=1e-3, weight_decay=0.1)
    for step in range(4):
        items = torch.from_numpy(rng.integers(1, n, size=(b, 2, l + 1)).astype(np.int64))
        mask = torch.ones(b, l, dtype=torch.int64)
        items[0, 0, :3] = 0; mask[0, :3] = 0
        loss = m((items.cuda(), mask.cuda()))
        loss.backward()
        opt.step()
        topt.zero_grad()
        rl = NO.forward_loss(ref, items, mask, dil * 2)
        rl.backward()
        ref["item_embedding.weight"].grad[0] = 0
        topt.step()
        assert abs(float(loss.detach()) - float(rl.detach())) < 2e-5 * max(1.0, abs(float(rl.detach()))), step
    sd = m.state_dict()
    for k, v in ref.items():
        diff = (sd[k].cpu().double() - v.detach()).abs()
        # Single-step gradients agree with the oracle to ~1e-7 at this shape (checked below in
        # test_nextitnet_single_step_gradients_at_the_shipped_dilations) and one
        # PxrAdamW step from equal state and gradients equals torch.optim.AdamW (tests/test_gpu_sasrec.py).  Over several steps
        # Adam normalises every element's step to ~lr whatever the gradient's size: where a gradient is at rounding level (conv
        # taps that mostly see the zero padding left of a 10-step sequence) its SIGN is noise on either side, those weights part
        # by up to 2 lr per step and perturb every later gradient.  So the element-wise statement after 4 steps is the trivial
        # one (nobody moved further than 4 lr + decay), the tight ones are the per-step LOSS agreement above and the mean drift.
        assert diff.max().item() < 4.5e-3, k
        assert diff.mean().item() < 2e-5, (k, diff.mean().item())


def test_trainer_runs_nextitnet_end_to_end(tmp_path):
    """IDNet/nextitnet.yaml-shaped run on TinyInter: Trainer.fit (hipGraph replay), fused top-k evaluation, reference-layout
    checkpoint."""
    from pixelrec_amd.config import Config
    from pixelrec_amd.data import bulid_dataloader, load_data
    from pixelrec_amd.optim import reference_rec_parameter_names
    from pixelrec_amd.parallel import DataParallel
    from pixelrec_amd.trainer import Trainer
    from pixelrec_amd.utils import get_model

    golden_dir = os.path.join(os.path.dirname(__file__), "golden")
    my, ov = tmp_path / "m.yaml", tmp_path / "o.yaml"
    my.write_text("model: NextItNet\nembedding_size: 32\nkernel_size: 3\nblock_num: 2\ndilations: [1,4]\nfinal_layer: False\n")
    ov.write_text(f"seed: 2020\nstate: INFO\nuse_modality: False\nreproducibility: True\ncheckpoint_dir: '{tmp_path}/saved'\n"
                  f"log_path: '{tmp_path}/log'\nshow_progress: False\nMAX_ITEM_LIST_LENGTH: 6\ndata_path: {golden_dir}/\n"
                  "dataset: TinyInter\nepochs: 3\ntrain_batch_size: 8\noptim_args: {learning_rate: 0.003, weight_decay: 0.1}\n"
                  "eval_batch_size: 16\ntopk: [5,10]\nmetrics: ['Recall', 'NDCG']\nvalid_metric: NDCG@10\n"
                  "metric_decimal_place: 7\neval_step: 1\nstopping_step: 30\n")
    config = Config([str(my), str(ov)])
    config["device"] = torch.device("cuda", 0)
    dataload = load_data(config)
    train, valid, test = bulid_dataloader(config, dataload)
    model = get_model(config["model"])(config, dataload)
    trainer = Trainer(config, DataParallel(model.to(config["device"])))
    trainer.fit(train, valid, saved=True)
    losses = [trainer.train_loss_dict[e] for e in sorted(trainer.train_loss_dict)]
    assert len(losses) == 3 and losses[-1] < losses[0]
    res = trainer.evaluate(test, load_best_model=True)
    assert set(res) == {"recall@5", "recall@10", "ndcg@5", "ndcg@10"}
    ck = torch.load(trainer.saved_model_file, map_location="cpu", weights_only=False)
    names = reference_rec_parameter_names(trainer.model.module)
    assert names == list(ck["state_dict"].keys()) and names[1] == "residual_blocks.0.conv1.weight" and len(names) == 1 + 4 * 8
    tparams = [torch.nn.Parameter(ck["state_dict"][k].clone()) for k in names]
    topt = torch.optim.AdamW(tparams, lr=1.0, weight_decay=0.5)
    topt.load_state_dict(ck["optimizer"])
    assert topt.state[tparams[1]]["exp_avg"].shape == tparams[1].shape == (32, 32, 1, 3)


def test_nextitnet_single_step_gradients_at_the_shipped_dilations():
    """One step at emb 64, dilations 2 x [1, 4] (second convolutions at 2 and 8, L = 10: taps that only ever see the left
    padding), every non-table gradient against the fp64 oracle: the measured error is ~1e-7."""
    from oracle import nextitnet_oracle as NO
    from pixelrec_amd.model import NextItNet

    n, e, l, b = 500, 64, 10, 8
    dil = [1, 4]

    class DL:
        item_num = n

    torch.manual_seed(3)
    m = NextItNet(_config(False, e=e, blocks=2, dil=dil, l=l), DL())
    ref = {k: v.detach().clone().double().requires_grad_(True) for k, v in m.state_dict().items()}
    m = m.cuda().train()
    rng = np.random.default_rng(6)
    items = torch.from_numpy(rng.integers(1, n, size=(b, 2, l + 1)).astype(np.int64))
    mask = torch.ones(b, l, dtype=torch.int64)
    loss = m((items.cuda(), mask.cuda()))
    loss.backward()
    rl = NO.forward_loss(ref, items, mask, dil * 2)
    rl.backward()
    assert abs(float(loss.detach()) - float(rl.detach())) < 2e-6 * abs(float(rl.detach()))
    for name, p in m.named_parameters():
        if name == "item_embedding.weight":
            continue
        want = ref[name].grad
        err = (p.grad.cpu().double() - want).abs().max().item()
        assert err < 2e-6 * max(1.0, want.abs().max().item()), (name, err)
    dead = ref["residual_blocks.1.conv2.weight"].grad[:, :, 0, 0]            # dilation 8, tap 0 reaches back 16 > L positions
    assert float(dead.abs().max()) == 0.0
    assert float(m.residual_blocks[1].conv2.weight.grad[:, :, 0, 0].abs().max()) == 0.0


@pytest.mark.parametrize("case", ["one_position", "kernel_size_1"])
def test_nextitnet_single_step_with_dead_taps_and_a_one_tap_kernel(case):
    """L = 1 with dilations [1, 4], kernel 3: every tap but the last only ever sees the left padding (its weight gradient is
    exactly zero); kernel_size = 1: im2col and col2im are copies and the dilation is moot.  Loss and every gradient of one step,
    the table's included, against the float64 oracle."""
    from oracle import nextitnet_oracle as NO
    from pixelrec_amd.model import NextItNet

    n, e, b = 60, 16, 3
    l, k = (1, 3) if case == "one_position" else (5, 1)
    dil = [1, 4]

    class DL:
        item_num = n

    torch.manual_seed(4)
    m = NextItNet(_config(False, e=e, blocks=1, dil=dil, l=l, k=k), DL())
    ref = {kk: v.detach().clone().double().requires_grad_(True) for kk, v in m.state_dict().items()}
    assert ref["residual_blocks.1.conv2.weight"].shape == (e, e, 1, k)
    m = m.cuda().train()
    rng = np.random.default_rng(9)
    items = torch.from_numpy(rng.integers(1, n, size=(b, 2, l + 1)).astype(np.int64))
    mask = torch.ones(b, l, dtype=torch.int64)
    loss = m((items.cuda(), mask.cuda()))
    loss.backward()
    rl = NO.forward_loss(ref, items, mask, dil)
    rl.backward()
    assert abs(float(loss.detach()) - float(rl.detach())) < 2e-6 * abs(float(rl.detach()))
    for name, p in m.named_parameters():
        want = ref[name].grad.clone()
        if name == "item_embedding.weight":
            sp = m.sparse_table_grad
            cnt = int(sp.n)
            got = torch.zeros(n, e)
            got[sp.idx[:cnt].cpu()] = sp.rows[:cnt].cpu()
            want[0] = 0
        else:
            got = p.grad.cpu()
        err = (got.double() - want).abs().max().item()
        assert err < 2e-6 * max(1.0, want.abs().max().item()), (name, err)
        if case == "one_position" and name.endswith(("conv1.weight", "conv2.weight")):
            assert float(want[..., :k - 1].abs().max()) == 0.0 and float(got[..., :k - 1].abs().max()) == 0.0, name
            assert float(want[..., k - 1].abs().max()) > 0.0, name
