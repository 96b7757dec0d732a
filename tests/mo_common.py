"""What the tests of the models trained from pixels share (tests/test_mo*_cpu.py, tests/test_gpu_mo*.py): the fixture naming, the
tiny tower's config, the Trainer's optimizer for a bare model, the constants of csrc/occ_sort.cuh and csrc/embed_grad.hip, and the three test bodies
that differ between the models in a few constants only -- the main.py run, the two-fresh-models loop and the optimizer state's
round trip.  A plain helper module like tests/segsum_cases.py: no test, no fixture."""
import os
import re
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PFX = "visual_encoder.item_encoder."
FOUR = {"modal_lr": 1e-4, "rec_lr": 3e-4, "modal_decay": 0.0, "rec_decay": 0.1}
LRS = [(1e-4, 0.0), (3e-4, 0.1)]           # FOUR as the (lr, weight_decay) of the two groups


def bits(t):
    return t.contiguous().view(torch.int32)


def my_name(k):
    """A fixture key (transformers-5.x names) -> this build's parameter name (`vision_model.` in the encoder's names)."""
    return (PFX + "vision_model." + k[len(PFX):]) if k.startswith(PFX) else k


def fixture_state(g, state=None):
    """The fixture's state_dict under this build's names, without the unused post_layernorm pair.  `state`: the stored one where
    the fixture does not hold it as plain float arrays."""
    if state is None:
        state = {k: torch.from_numpy(g["sd." + k]) for k in (str(x) for x in g["sd.keys"])}
    return {my_name(k): v for k, v in state.items() if "post_layernorm" not in k}


def tower_config(tune, **model_keys):
    """A model's config over the tiny test tower with `tune` frozen encoder tensors: the keys every pixel model's config shares,
    then the model's own."""
    return {"seed": 2020, "encoder_name": "clip-vit-tiny-test", "encoder_source": "transformers", "pretrain_path": None,
            "fine_tune_arg": {"tune_scale": tune, "pre_trained": True, "activation": "relu", "dnn_layers": [], "method": "mean"},
            **model_keys}


class _Wrap:
    def __init__(self, m):
        self.module = m


def trainer_optimizer(m, optim_args):
    from pixelrec_amd.trainer import Trainer

    t = Trainer.__new__(Trainer)
    t.optim_args, t.model, t.config = optim_args, _Wrap(m), {"decay_check_name": None}
    return t._build_optimizer()


def sort_constants():
    """(FP_MAX_N of csrc/occ_sort.cuh, SEG_SHORT, SEG_CHUNK of csrc/embed_grad.hip)."""
    read = lambda f: open(os.path.join(ROOT, "pixelrec_amd", "csrc", f)).read()
    sort, seg = read("occ_sort.cuh"), read("embed_grad.hip")
    val = lambda k, src: int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1))
    mult = int(re.search(r"constexpr int FP_MAX_N = (\d+) \* RS_TILE;", sort).group(1))
    assert "enabled && n <= FP_MAX_N" in sort                      # use_fused_sort's cut-over
    return mult * val("RS_THREADS", sort) * val("RS_ITEMS", sort), val("SEG_SHORT", seg), val("SEG_CHUNK", seg)


def run_main_py(tmp_path, model_yaml, max_len=6, timeout=600):
    """main.py on TinyInter with synthetic 64 x 64 images and the tiny tower, two epochs: finite losses that change, Recall@10 and
    NDCG@10 reported from the reloaded checkpoint -> (output, epoch losses, checkpoint, config, data); the caller checks the
    checkpoint's keys and loads it into a fresh model."""
    from pixelrec_amd.config import Config
    from pixelrec_amd.data import load_data

    my, ov = tmp_path / "m.yaml", tmp_path / "o.yaml"
    my.write_text(model_yaml)
    ov.write_text(f"seed: 2020\nstate: INFO\nuse_modality: True\nreproducibility: True\ncheckpoint_dir: '{tmp_path}/saved'\n"
                  f"log_path: '{tmp_path}/log'\nshow_progress: False\nMAX_ITEM_LIST_LENGTH: {max_len}\ndata_path: {GOLD}/\n"
                  "dataset: TinyInter\nimage_path: 'synthetic:64'\nencoder_name: 'clip-vit-tiny-test'\n"
                  "encoder_source: 'transformers'\nepochs: 2\ntrain_batch_size: 8\n"
                  "fine_tune_arg: {tune_scale: 37, pre_trained: True, activation: 'relu', dnn_layers: [], method: 'mean'}\n"
                  "optim_args: {modal_lr: 0.001, rec_lr: 0.001, modal_decay: 0, rec_decay: 0.1}\n"
                  "eval_batch_size: 16\ntopk: [5,10]\nmetrics: ['Recall', 'NDCG']\nvalid_metric: NDCG@10\n"
                  "metric_decimal_place: 7\neval_step: 1\nstopping_step: 30\n")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "OMP_NUM_THREADS")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--device", "0", "--config_file", str(my), str(ov)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=timeout)
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
    return out, epochs, ck, config, data


def assert_two_fresh_models_agree(build, step, n_per_step):
    """Two models from `build()` run `step(m, j)` -> (loss, {name: gradient}) on batches 0 and 1: `n_per_step` tensors a step, two
    different losses, and the same bits from both models."""
    runs = []
    for _ in range(2):
        m = build()
        out = []
        for j in range(2):
            loss, grads = step(m, j)
            out += [loss] + [grads[k] for k in sorted(grads)]
        runs.append(out)
    assert len(runs[0]) == len(runs[1]) == 2 * n_per_step
    assert float(runs[0][0]) != float(runs[0][n_per_step])          # two batches, two losses
    for x, y in zip(*runs):
        assert torch.equal(bits(x), bits(y))


def assert_optimizer_state_round_trips(build, step, groups, with_state, lrs=LRS, rec=None, moved=None):
    """Four optim_args on `build()`: the encoder group and a rec group without a table, `groups` parameters; one `step(m)` and one
    optimizer step, after which `moved(set of moved keys, set of trainable keys)` makes the model's own assertions; the
    torch-layout state has entries `with_state` and loads into torch.optim.AdamW over the reference's two groups (`rec(m)`: the rec
    group's parameters in the reference's registration order; default: every parameter outside the encoder) and back."""
    from pixelrec_amd.optim import OptimizerGroup

    m = build()
    opt = trainer_optimizer(m, FOUR)
    assert isinstance(opt, OptimizerGroup)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    opt.zero_grad()
    step(m)
    opt.step()
    after = m.state_dict()
    if moved is not None:
        moved({k for k in before if not torch.equal(before[k], after[k])}, {n for n, p in m.named_parameters() if p.requires_grad})
    sd = opt.state_dict(layout="torch")
    assert [len(x["params"]) for x in sd["param_groups"]] == groups and sorted(sd["state"]) == with_state
    assert [(x["lr"], x["weight_decay"]) for x in sd["param_groups"]] == lrs
    enc = [p for n, p in m.named_parameters() if "visual_encoder" in n and p.requires_grad]
    recs = rec(m) if rec is not None else [p for n, p in m.named_parameters() if "visual_encoder" not in n]
    if rec is not None:
        assert [tuple(sd["state"][groups[0] + i]["exp_avg"].shape) for i in range(groups[1])] == [tuple(p.shape) for p in recs]
    tor = torch.optim.AdamW([{"params": enc, "lr": 1.0, "weight_decay": 0.5}, {"params": recs, "lr": 2.0, "weight_decay": 0.25}])
    tor.load_state_dict(sd)                                         # the layout the reference stores
    assert [(x["lr"], x["weight_decay"]) for x in tor.param_groups] == lrs
    opt2 = trainer_optimizer(build(), {**FOUR, "modal_lr": 5.0, "rec_lr": 7.0})
    opt2.load_state_dict(tor.state_dict())
    sd2 = opt2.state_dict(layout="torch")
    assert [x["params"] for x in sd2["param_groups"]] == [x["params"] for x in sd["param_groups"]]
    assert [(x["lr"], x["weight_decay"]) for x in sd2["param_groups"]] == lrs
    assert sorted(sd2["state"]) == with_state
    for i in with_state:
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sd2["state"][i][key].cpu(), sd["state"][i][key].cpu()), (i, key)
