"""Generates tests/golden/curatornet_tiny.npz by running the REFERENCE's CuratorNet (REC/model/ViNet/curatornet.py) unmodified,
imported through oracle/ref_shim.py.  Run where the reference is present:   python tools/make_golden_curatornet.py

Tiny shape: item_num = 9, F = 12, embedding_size = 8, hidden_size = 2 (profile tower 16 wide), L = 4, B = 6, four batches of
[profile (L) | positive | negative] rows.  Every batch holds a full profile, profiles with one, two and three padded positions, an
all-padding profile and a profile that repeats an item; one item is the positive of one sample and the negative of another, and no
sample's positive equals its negative.  `selu_common1.bias` is zero in the stored initial state, so a padded position's first
pre-activation is EXACTLY 0: the x == 0 case of the SELU derivative (scale * alpha, torch's backward).

Stored: the feature matrix, the initial state_dict, the loss and the ten gradients of one training step, compute_item_all, predict
for eight windows (one of them all padding), and a 4-step torch.optim.AdamW trajectory from the initial state under acf.yaml's
optim_args (learning_rate 1e-4, weight_decay 0.01): losses, final state_dict.

The fixture is only worth comparing against if rounding cannot flip a discrete choice, so the generator checks in float64 (with
tests/curatornet_restate.py) and moves on to the next seed when a check fails:
  * every max over L is more than 1e-4 above the runner-up, except where the tied positions hold the same item;
  * every pre-activation that is not exactly 0 is larger than 1e-4 in magnitude;
  * every entry of the ten gradients is non-zero.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import curatornet_restate as R  # noqa: E402

C = dict(item_num=9, F=12, E=8, hidden=2, L=4, B=6, lr=1e-4, wd=0.01)
MARGIN = 1e-4


class FakeData:
    item_num = C["item_num"]


def batch(rng):
    I, L, B = C["item_num"], C["L"], C["B"]
    prof = np.zeros((B, L), dtype=np.int64)
    for b, n_real in enumerate((4, 3, 2, 1, 0, 4)):      # full, one / two / three padded, all padding, (repeated item below)
        prof[b, L - n_real:] = rng.choice(np.arange(1, I), size=n_real, replace=False)
    prof[5, 2] = prof[5, 0]                               # a repeated item inside a profile
    pos = rng.integers(1, I, size=B)
    neg = rng.integers(1, I, size=B)
    neg[2] = pos[0]                                       # the positive of one sample is the negative of another
    for b in range(B):                                    # no sample whose positive equals its negative
        while neg[b] == pos[b] or (b == 2 and pos[b] == pos[0]):
            if b == 2:
                pos[b] = rng.integers(1, I)
            else:
                neg[b] = rng.integers(1, I)
    return np.concatenate((prof, pos[:, None], neg[:, None]), axis=1)


def pre_activations(P, ids):
    """Every Linear's pre-activation for the rows `ids` [B, L + 2] read, plus the pooling's inputs [B, L, E]."""
    feat = P["embedding.weight"]
    ids = torch.as_tensor(ids)
    z1 = feat[ids] @ P["selu_common1.weight"].T + P["selu_common1.bias"]
    z2 = R.selu(z1) @ P["selu_common2.weight"].T + P["selu_common2.bias"]
    h = R.selu(z2)[:, :C["L"]]
    out, x = [z1, z2], R.pool(h)[0]
    for lin in ("selu_pu1", "selu_pu2", "selu_pu3"):
        z = x @ P[lin + ".weight"].T + P[lin + ".bias"]
        out.append(z)
        x = R.selu(z)
    return out, h


def comparable(P, rows_list):
    for ids in rows_list:
        zs, h = pre_activations(P, ids)
        for z in zs:
            z = z.abs()
            if ((z != 0) & (z <= MARGIN)).any():
                return False
        prof = torch.as_tensor(ids)[:, :C["L"]]
        top, arg = h.max(dim=1)
        for l in range(C["L"]):                           # runner-up positions: a different item must be > MARGIN below
            other = prof[:, l].unsqueeze(1) != torch.gather(prof, 1, arg)
            if (other & (top - h[:, l] <= MARGIN)).any():
                return False
    return True


def build(seed):
    from REC.model.ViNet.curatornet import CuratorNet

    rng = np.random.default_rng(seed)
    batches = [batch(rng) for _ in range(4)]
    windows = np.zeros((8, C["L"]), dtype=np.int64)
    for b, n_real in enumerate((4, 4, 3, 2, 1, 0, 4, 3)):  # one window is all padding
        windows[b, C["L"] - n_real:] = rng.integers(1, C["item_num"], size=n_real)
    v_feat = rng.standard_normal((C["item_num"], C["F"])).astype(np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "v_feat.npy")
        np.save(path, v_feat)
        cfg = {"embedding_size": C["E"], "hidden_size": C["hidden"], "device": "cpu", "v_feat_path": path}
        torch.manual_seed(seed)
        model = CuratorNet(cfg, FakeData())
    with torch.no_grad():
        model.selu_common1.bias.zero_()
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    assert list(sd0) == list(R.KEYS)
    P = {k: v.double() for k, v in sd0.items()}
    pad_rows = np.concatenate((windows, windows[:, :2]), axis=1)
    if not comparable(P, batches + [pad_rows]):
        return None
    store = {"meta": np.array([C[k] for k in ("item_num", "F", "E", "hidden", "L", "B")] + [seed]),
             "optim": np.array([C["lr"], C["wd"]]), "v_feat": v_feat, "rows": np.stack(batches), "eval.windows": windows}
    for k, v in sd0.items():
        store["sd." + k] = v.numpy().copy()
    model.train()
    model.zero_grad()
    loss = model(torch.from_numpy(batches[0]))
    loss.backward()
    store["loss"] = np.array(loss.item(), dtype=np.float32)
    assert model.embedding.weight.grad is None
    for k in R.NAMES:
        g = model.get_parameter(k).grad.numpy().copy()
        if (g == 0).any():
            return None
        store["grad." + k] = g
    _, g64 = R.loss_and_grads(P, batches[0][:, :C["L"]], batches[0][:, C["L"]:])
    if any((g == 0).any() for g in g64.values()):
        return None
    model.eval()
    with torch.no_grad():
        feat = model.compute_item_all()
        store["eval.item_all"] = feat.numpy().copy()
        store["eval.scores"] = model.predict(torch.from_numpy(windows), feat).numpy().copy()
    model.train()
    model.load_state_dict(sd0, strict=True)
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=C["lr"], weight_decay=C["wd"])
    for s, rows in enumerate(batches):
        opt.zero_grad()
        l = model(torch.from_numpy(rows))
        l.backward()
        opt.step()
        store[f"adamw.loss{s}"] = np.array(l.item(), dtype=np.float32)
    for k, v in model.state_dict().items():
        store["adamw.final." + k] = v.numpy().copy()
    # how far the reference's float32 arithmetic is from the float64 restatement on these inputs (for the record)
    L64, _ = R.loss_and_grads(P, batches[0][:, :C["L"]], batches[0][:, C["L"]:])
    gerr = max(float(np.abs(g64[k].numpy() - store["grad." + k]).max() / max(1.0, np.abs(store["grad." + k]).max())) for k in R.NAMES)
    print(f"seed {seed}: reference fp32 vs float64 restatement: loss {abs(L64 - float(store['loss'])):.2e}, gradients {gerr:.2e}")
    return store


def main():
    ref_shim.import_reference()
    for seed in range(41, 141):
        store = build(seed)
        if store is not None:
            break
        print(f"seed {seed}: a comparability check failed, trying the next seed")
    else:
        raise SystemExit("no seed passed the comparability checks")
    path = os.path.join(ROOT, "tests", "golden", "curatornet_tiny.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB), loss={float(store['loss']):.6f}")


if __name__ == "__main__":
    main()
