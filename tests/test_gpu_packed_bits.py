"""The flat-buffer layout and the training bits of every model family that packs its parameters (pixelrec_amd/model/packed.py)
against tests/golden/packed_model_bits.json, which was recorded with `python tests/test_gpu_packed_bits.py --record FILE` on the
build of the commit BEFORE the packing, the parameter views, the lazy-table surface and the autograd bridge got one definition
(eight copies of the pack loop, ten of the bridge).  Sharing that host code changes no layout, no launch and no operand, so per
case the `_views` dict, the state-dict key list, the float32 bit pattern of the loss of each of three PxrAdamW steps and, after
the third step and a flush, the u32 checksums of the flat buffer, the flat gradient buffer and the table must be equal.

The recorder runs every case twice.  A case whose two runs on the recording build differ in any bit is listed under
"first_step_only" in the golden file and compared on `_views`, keys and the first loss only; the families whose sources promise
run-to-run identity (MF, VBPR, ACF, DIN, CuratorNet, WideDeep, DSSM, FM) may not be listed (asserted below).

Cases: each family at the shape, the weights and the batches of its own fixture under tests/golden/ (built by the `_gold_model`
helpers of its GPU test):
  * mf/plain   mlp_hidden_size [] -- the flat buffer is the 4-element placeholder;
  * mf/towers  mlp_hidden_size [8, 4] -- BatchNorm buffers advance on the device;
  * mf/reload  the towers again: the state dict after step 1 goes into a model that was packed, moved to the CPU and back (a
               repack) and trains two more steps under a new optimizer;
  * vbpr       three table spans;
  * acf        every tensor on a 16-byte boundary, the one-element biases of the two `w` Linears in mid-buffer;
  * din        hidden (12, 4): the one-element `dense.b`;
  * curatornet aligned, no table;
  * srgnn      step 2: `_p(..., span=2)` fused views;
  * lightgcn   three layers: the flat buffer is the table;
  * sasrec     two layers (SeqRecCore's pack);
  * widedeep   the wide table and its bias in the flat buffer, the deep table lazy;
  * dssm/plain, fm   no flat parameter: pooling fused with the pair head;
  * dssm/mlp   hidden [8, 12, 8] with dropout_prob 0.25: the device step counter decides the second and third steps' masks;
  * gru4rec, nextitnet, lightsans, bert4rec   the sequence blocks on SeqRecCore's bracket (their fixture's one batch three times
               where it holds only one).

Every case also records "steps": [m._step_counter, int(m._drop_dev)] after the last step -- the host and the device count of
completed backward passes, [3, 3] ([2, 2] for mf/reload's second model) -- compared in full for a "first_step_only" case too.
The second group of cases and the "steps" field were recorded on the build of the commit BEFORE the step bracket
(`_take_saved` / `_step_done`), the Linear-stack helpers and the input, scoring and evaluation-cache helpers moved into packed.py."""
import json
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "packed_model_bits.json")
STEPS = 3
MUST_BE_FULL = ("mf/plain", "mf/towers", "mf/reload", "vbpr", "acf", "din", "curatornet", "widedeep", "dssm/plain", "dssm/mlp", "fm")


def _gold(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + "_tiny.npz"))


def _adamw(m, lr=1e-3, wd=0.1):
    from pixelrec_amd.optim import PxrAdamW

    return PxrAdamW(m, lr=lr, weight_decay=wd)


def _lazy_table(m):
    return m.lazy_table()


# ---- per family: the model in train() as its GPU test's helper builds it (tmp: a directory for the feature files), and
# (optimizer, the batches of the steps, the table to checksum | None) for a model
def _mf_model(cfg):
    def make(tmp):
        from tests import test_gpu_mf as T

        return T._gold_model(_gold("mf"), cfg)
    return make


def _vbpr_model(tmp):
    from tests import test_gpu_vbpr as T

    return T._gold_model(_gold("vbpr"), tmp)


def _acf_model(tmp):
    from tests import test_gpu_acf as T

    return T._gold_model(_gold("acf"), tmp)


def _din_model(tmp):
    from tests import test_gpu_din as T

    m = T._gold_model(_gold("din"))
    assert m.mlp_hidden_size == [12, 4]
    return m


def _curatornet_model(tmp):
    from tests import test_gpu_curatornet as T

    return T._gold_model(_gold("curatornet"), tmp)


def _srgnn_model(tmp):
    from tests import test_gpu_srgnn as T

    return T._model(_gold("srgnn"), 2)


def _lightgcn_model(tmp):
    from tests import test_gpu_lightgcn as T

    return T._gold_model(_gold("lightgcn"), 3)[0]


def _sasrec_model(tmp, dev="cuda"):
    from tests import test_gpu_sasrec as T
    from tests.golden_util import load_case

    meta, _ = load_case("tiny")
    assert meta["n_layers"] == 2
    return T._model(meta, dev=dev)[0].train()


def _widedeep_model(tmp):
    from tests import test_gpu_widedeep as T

    return T._gold_model(_gold("widedeep"))


def _pool_model(fixture, p=0.0):
    def make(tmp):
        from tests import test_gpu_pool as T

        kind, hidden = T.CASES[fixture + "_tiny"]
        return T._gold_model(kind, hidden, _gold(fixture), p=p)
    return make


def _gru4rec_model(tmp):
    from pixelrec_amd.model import GRU4Rec
    from tests import test_gpu_gru4rec as T

    m = GRU4Rec(T._config(), type("DL", (), {"item_num": T.N})())
    m.load_state_dict({k[6:]: torch.from_numpy(T.G[k]) for k in T.G.files if k.startswith("param/")}, strict=True)
    return m.cuda().train()


def _nextitnet_model(tmp):
    from pixelrec_amd.model import NextItNet
    from tests import test_gpu_nextitnet as T

    m = NextItNet(T._config(False), type("DL", (), {"item_num": T.N})())
    m.load_state_dict({k[12:]: torch.from_numpy(T.G[k]) for k in T.G.files if k.startswith("plain/param/")}, strict=True)
    return m.cuda().train()


def _lightsans_model(tmp):
    from tests import test_gpu_lightsans as T

    return T._model(_gold("lightsans"), 2)


def _bert4rec_model(tmp):
    from tests import test_gpu_bert4rec as T

    return T._model(*T._golden())[0].train()


MODELS = {"mf/plain": _mf_model("c0"), "mf/towers": _mf_model("c1"), "vbpr": _vbpr_model, "acf": _acf_model, "din": _din_model,
          "curatornet": _curatornet_model, "srgnn": _srgnn_model, "lightgcn": _lightgcn_model, "sasrec": _sasrec_model, "widedeep": _widedeep_model,
          "dssm/plain": _pool_model("dssm"), "dssm/mlp": _pool_model("dssm_mlp", p=0.25), "fm": _pool_model("fm"),
          "gru4rec": _gru4rec_model, "nextitnet": _nextitnet_model, "lightsans": _lightsans_model, "bert4rec": _bert4rec_model}
CASES = sorted(list(MODELS) + ["mf/reload"])


def _pairs(g):
    users, items = torch.from_numpy(g["users"]).cuda(), torch.from_numpy(g["items"]).cuda()
    return [(users[s], items[s]) for s in range(STEPS)]


def _rows(g):
    rows = torch.from_numpy(g["rows"]).cuda()
    return [rows[s] for s in range(STEPS)]


def _training(name, m):
    if name.startswith("mf/"):
        return _adamw(m), _pairs(_gold("mf")), _lazy_table
    if name == "vbpr":
        from tests.test_gpu_vbpr import _opt

        return _opt(m), _pairs(_gold("vbpr")), _lazy_table
    if name == "acf":
        from tests.test_gpu_acf import _opt

        return _opt(m), _rows(_gold("acf")), _lazy_table
    if name == "din":
        from tests.test_gpu_din import _opt

        return _opt(m), _rows(_gold("din")), _lazy_table
    if name == "curatornet":
        from tests.test_gpu_curatornet import _opt

        return _opt(m), _rows(_gold("curatornet")), None
    if name == "srgnn":
        from tests.test_gpu_srgnn import _batch

        return _adamw(m, lr=1e-2), [_batch(_gold("srgnn"), s) for s in range(STEPS)], lambda m: m.embedding.weight.data
    if name == "lightgcn":
        return _adamw(m), _pairs(_gold("lightgcn")), lambda m: m.item_embedding.weight.data
    if name == "widedeep":
        from tests.test_gpu_widedeep import _opt, _split

        g = _gold("widedeep")
        return _opt(m), [_split(torch.from_numpy(g["rows"][s]).cuda(), m.max_seq_length) for s in range(STEPS)], _lazy_table
    if name in ("dssm/plain", "dssm/mlp", "fm"):
        from tests.test_gpu_pool import _inp, _opt

        g = _gold({"dssm/plain": "dssm", "dssm/mlp": "dssm_mlp", "fm": "fm"}[name])
        return _opt(m), [_inp(type(m).__name__, g["rows"][s]) for s in range(STEPS)], _lazy_table
    if name in ("gru4rec", "nextitnet"):
        g = _gold(name)
        batch = (torch.from_numpy(g["items"]).cuda(), torch.from_numpy(g["masked_index"]).cuda())
        return _adamw(m), [batch] * STEPS, lambda m: m.item_embedding.weight.data
    if name == "lightsans":
        g = _gold("lightsans")
        return _adamw(m), [torch.from_numpy(g[f"b{s}.items"]).cuda() for s in range(STEPS)], lambda m: m.item_embedding.weight.data
    if name == "bert4rec":
        z = _gold("bert4rec")
        batches = [(torch.from_numpy(z["adamw.items"][s]).cuda(), torch.from_numpy(z["adamw.masks"][s]).cuda()) for s in range(STEPS)]
        return _adamw(m, lr=1e-4), batches, lambda m: m.item_embedding.weight.data
    from tests.golden_util import load_case

    _, z = load_case("tiny")
    batches = [(torch.from_numpy(z["adamw.items"][s]).cuda(), torch.from_numpy(z["adamw.masks"][s]).cuda()) for s in range(STEPS)]
    return _adamw(m, lr=1e-4), batches, lambda m: m.item_embedding.weight.data


def _u32_sum(t):
    return int((t.detach().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF).sum().item()) & 0xFFFFFFFF


def _loss_bits(loss):
    return int(loss.detach().to(torch.float32).reshape(1).view(torch.int32).item()) & 0xFFFFFFFF


def _train(m, opt, batches):
    bits = []
    for b in batches:
        opt.zero_grad()
        loss = m(b)
        loss.backward()
        opt.step()
        bits.append(_loss_bits(loss))
    return bits


def _record(m, opt, losses, table_of):
    from pixelrec_amd import ops

    if hasattr(opt, "flush"):
        opt.flush()
    torch.cuda.synchronize()
    ops.raise_on_bad_indices("cuda")
    flat, gflat = m.flat_parameters()
    sums = {"flat": _u32_sum(flat), "gflat": _u32_sum(gflat)}
    if table_of is not None:
        sums["table"] = _u32_sum(table_of(m))
    return {"views": {k: [int(off), int(n), [int(x) for x in shape]] for k, (off, n, shape) in m._views.items()},
            "keys": list(m.state_dict().keys()), "loss_bits": losses, "sums": sums,
            "steps": [int(m._step_counter), int(m._drop_dev)]}


def run_case(name):
    with tempfile.TemporaryDirectory() as tmp:
        if name != "mf/reload":
            m = MODELS[name](tmp)
            opt, batches, table_of = _training(name, m)
            return _record(m, opt, _train(m, opt, batches), table_of)
        a = MODELS["mf/towers"](tmp)
        opt, batches, table_of = _training(name, a)
        _train(a, opt, batches[:1])
        sd = {k: v.detach().cpu().clone() for k, v in a.state_dict().items()}
        b = MODELS["mf/towers"](tmp)
        flat0 = b.flat_parameters()[0]                      # packed once ...
        b.cpu().load_state_dict(sd, strict=True)
        b.cuda().train()
        opt_b = _adamw(b)
        losses = _train(b, opt_b, batches[1:])
        assert b.flat_parameters()[0].data_ptr() != flat0.data_ptr()     # ... and again after the round trip
        return _record(b, opt_b, losses, table_of)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_compares_the_deterministic_families_in_full(golden):
    assert sorted(golden["cases"]) == CASES
    assert not set(golden["first_step_only"]) & set(MUST_BE_FULL)


@pytest.mark.parametrize("name", CASES)
def test_layout_keys_and_training_bits_are_kept(name, golden):
    want, got = golden["cases"][name], run_case(name)
    print(name, json.dumps(got, sort_keys=True))
    assert got["views"] == want["views"]
    assert got["keys"] == want["keys"]
    assert got["steps"] == want["steps"] == [len(got["loss_bits"])] * 2
    if name in golden["first_step_only"]:
        assert got["loss_bits"][0] == want["loss_bits"][0]
        return
    assert got["loss_bits"] == want["loss_bits"]
    assert got["sums"] == want["sums"]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: test_gpu_packed_bits.py --record FILE"
    cases, loose = {}, []
    for name in CASES:
        cases[name], again = run_case(name), run_case(name)
        if again != cases[name]:
            loose.append(name)
    assert not set(loose) & set(MUST_BE_FULL), loose
    with open(sys.argv[2], "w") as f:                    # one case per line
        f.write('{"first_step_only": ' + json.dumps(loose) + ',\n"cases": {\n'
                + ",\n".join(f"{json.dumps(k)}: {json.dumps(cases[k], sort_keys=True)}" for k in CASES) + "\n}}\n")
