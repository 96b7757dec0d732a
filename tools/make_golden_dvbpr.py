"""Generates tests/golden/dvbpr_tiny.npz by running the REFERENCE's DVBPR (REC/model/PixelNet/dvbpr.py) unmodified, imported through
oracle/ref_shim.py, once in float32 and once in float64.  Run where the reference is present:
    python tools/make_golden_dvbpr.py

Tiny shape: U = 7 users, I = 9 items, Dh = 16 (embedding_size 32), dropout 0, a store of 9 images, two batches of B = 3 in each of
which one image is the positive of one sample and the negative of another (6 positions, M = 5 distinct images).  The images are
stored as uint8 [9, 28, 28, 3] and expanded by tests/dvbpr_restate.expand_images (pixel repetition x 8, then (x / 255 - 0.5) / 0.5).
The weights are NOT stored -- fcs.0.weight alone is 23 MB: tests/dvbpr_restate.make_state rebuilds them from
np.random.RandomState(seed), and the fixture holds the seed and a float64 sum and sum of squares per tensor.

The reference's forward gets its own input form (user [B], item_id [B, 2], item_modal [B, 2, 3, 224, 224]), one image per position, in
training mode.  Stored, all from the FLOAT64 run: per batch the loss, the gradient of every bias, of convs.0.weight, of fcs.2.weight
and of the touched table rows in full, and for the other six weights the L2 norm and a strided sample of 1024 elements
(dvbpr_restate.sample_index); compute_item over the store and predict for all users.  Under ref_err.* the same entry's |float32 run -
float64 run| as ONE number (the maximum over the tensor): the reference's own float32 error, the tests' yardstick.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import dvbpr_restate as R  # noqa: E402

C = dict(U=7, I=9, Dh=16, B=3, seed=1234)
FULL = ("convs.0.weight", "fcs.2.weight")       # weight gradients kept whole


class FakeData:
    user_num = C["U"]
    item_num = C["I"]


def batches():
    """Two (user [3], item_id [3, 2]): in each, one item is a positive and a negative, 5 distinct items; batch 1 repeats a user."""
    return [(np.array([0, 3, 5], dtype=np.int64), np.array([[1, 4], [4, 7], [2, 8]], dtype=np.int64)),
            (np.array([6, 2, 6], dtype=np.int64), np.array([[0, 3], [5, 0], [6, 1]], dtype=np.int64))]


def run(ref_cls, state, images, dtype):
    torch.manual_seed(0)
    model = ref_cls({"dropout_prob": 0.0, "embedding_size": 2 * C["Dh"], "device": "cpu"}, FakeData())
    assert list(model.state_dict()) == list(state), list(model.state_dict())
    model.load_state_dict(state, strict=True)
    model = model.to(dtype)
    model.weight = model.weight.to(dtype)           # the [[1], [-1]] of dvbpr.py:34 is a plain attribute
    model.train()
    img = images.to(dtype)
    out = {}
    for j, (user, item) in enumerate(batches()):
        model.zero_grad()
        u, it = torch.from_numpy(user), torch.from_numpy(item)
        loss = model((u, it, img[it]))
        loss.backward()
        out[f"b{j}.loss"] = loss.detach().double().reshape(1)
        for n, p in model.named_parameters():
            g = p.grad.detach().double()
            if n.startswith(R.ENC):
                short = n[len(R.ENC):]
                if n.endswith("bias") or short in FULL:
                    out[f"b{j}.grad.{n}"] = g
                else:
                    out[f"b{j}.norm.{n}"] = g.norm().reshape(1)
                    out[f"b{j}.sample.{n}"] = g.reshape(-1)[torch.from_numpy(R.sample_index(g.numel()))]
            else:
                rows = np.unique(user if "users" in n else item.reshape(-1))
                untouched = np.setdiff1d(np.arange(g.shape[0]), rows)
                assert float(g[untouched].abs().max()) == 0.0
                out[f"b{j}.rows.{n}"] = g[torch.from_numpy(rows)]
    model.eval()
    with torch.no_grad():
        feat = model.compute_item(img)
        out["eval.item_feature"] = feat.double()
        out["eval.scores"] = model.predict(torch.arange(C["U"]), feat).double()
    return out


def main():
    ref_shim.import_reference()
    ref_cls = __import__("REC.model.PixelNet.dvbpr", fromlist=["DVBPR"]).DVBPR
    rs = np.random.RandomState(C["seed"] + 1)
    store = rs.randint(0, 256, size=(C["I"], 28, 28, 3)).astype(np.uint8)
    images = R.expand_images(store)
    state = R.make_state(C["seed"], C["Dh"], C["U"], C["I"])
    r32, r64 = run(ref_cls, state, images, torch.float32), run(ref_cls, state, images, torch.float64)
    out = {"meta": np.array([C["U"], C["I"], C["Dh"], C["B"], C["seed"]]), "store": store, "sd.keys": np.array(list(state)),
           "sd.shapes": np.array([",".join(str(d) for d in v.shape) for v in state.values()]), "sd.sums": R.state_sums(state)}
    for j, (user, item) in enumerate(batches()):
        out[f"b{j}.user"], out[f"b{j}.item_id"] = user, item
    worst = {}
    for k, v in r64.items():
        out[k] = v.numpy().copy()
        err = float((r32[k] - v).abs().max())
        out["ref_err." + k] = np.array(err)
        kind = k.split(".")[1] if k[0] == "b" else k
        worst[kind] = max(worst.get(kind, 0.0), err)
    print("DVBPR reference float32 vs float64: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    path = os.path.join(ROOT, "tests", "golden", "dvbpr_tiny.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1_000_000, size
    print(f"wrote {path} ({size / 1024:.0f} KiB), losses {[float(out[f'b{j}.loss'][0]) for j in range(2)]}")


if __name__ == "__main__":
    main()
