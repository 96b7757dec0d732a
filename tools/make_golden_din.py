"""Generates tests/golden/din_tiny.npz by running the REFERENCE's DIN (REC/model/IDNet/din.py) unmodified, imported through
oracle/ref_shim.py.  Run where the reference is present:   python tools/make_golden_din.py

Tiny shape: item_num = 13, embedding_size = 8, mlp_hidden_size = [12, 4], L = 4, B = 6, four batches of [profile (L) | positive |
negative] rows.  Every batch holds a full profile, profiles with one, two and three padded positions, an all-padding profile and
a profile that repeats an item; one item is the positive of one sample and the negative of another, and no sample's positive
equals its negative.

Stored: the initial state_dict, the loss and the seven gradients of one training step (the table's row 0 exactly zero), predict
through the reference's [B, N, L + 1] form for eight windows (one of them all padding), and a 4-step torch.optim.AdamW trajectory
from the initial state under configs/overall/ID.yaml's optim_args (learning_rate 1e-4, weight_decay 0.1): losses, final state_dict
(row 0 and never-touched rows included).

The fixture is only worth comparing against if rounding cannot flip a ranking, so the generator checks in float64 (with
tests/din_restate.py) and moves on to the next seed when a check fails:
  * among the unmasked items of every non-padding window, adjacent float64 scores down to rank K + 1 (K = 10) are more than
    MARGIN = 1e-5 apart -- the margin the id comparisons of tests/test_gpu_din.py rely on;
  * no gradient entry of the attention tensors is zero.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import din_restate as R  # noqa: E402

C = dict(item_num=13, D=8, hidden=[12, 4], L=4, B=6, lr=1e-4, wd=0.1, K=10)
MARGIN = 1e-5


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


def reference_form(windows, item_num):
    """CandiEvalDataset's id tensor [B, item_num, L + 1]: the window repeated per candidate, the candidate id last."""
    B, L = windows.shape
    out = np.zeros((B, item_num, L + 1), dtype=np.int64)
    out[:, :, :L] = windows[:, None, :]
    out[:, :, L] = np.arange(item_num)[None, :]
    return out


def rankings_comparable(P, windows):
    s = R.predict_factorised(P, windows)
    s[:, 0] = float("-inf")
    top = torch.sort(s, dim=-1, descending=True).values[:, :C["K"] + 1]
    for b in range(len(windows)):
        if (windows[b] != 0).any() and bool(((top[b, :-1] - top[b, 1:]) <= MARGIN).any()):
            return False
    return True


def build(seed):
    from REC.model.IDNet.din import DIN

    rng = np.random.default_rng(seed)
    batches = [batch(rng) for _ in range(4)]
    windows = np.zeros((8, C["L"]), dtype=np.int64)
    for b, n_real in enumerate((4, 4, 3, 2, 1, 0, 4, 3)):  # one window is all padding
        windows[b, C["L"] - n_real:] = rng.integers(1, C["item_num"], size=n_real)
    cfg = {"embedding_size": C["D"], "mlp_hidden_size": list(C["hidden"]), "device": "cpu", "dropout_prob": 0}
    torch.manual_seed(seed)
    model = DIN(cfg, FakeData())
    names = R.names(len(C["hidden"]))
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    assert list(sd0) == names, list(sd0)
    assert [n for n, _ in model.named_parameters()] == names
    P = {k: v.double() for k, v in sd0.items()}
    if not rankings_comparable(P, windows):
        return None
    store = {"meta": np.array([C["item_num"], C["D"], C["L"], C["B"], C["K"], seed] + list(C["hidden"])),
             "optim": np.array([C["lr"], C["wd"]]), "rows": np.stack(batches), "eval.windows": windows,
             "sd.keys": np.array(names)}
    for k, v in sd0.items():
        store["sd." + k] = v.numpy().copy()
    model.train()
    model.zero_grad()
    loss = model(torch.from_numpy(batches[0]))
    loss.backward()
    store["loss"] = np.array(loss.item(), dtype=np.float32)
    for k in names:
        g = model.get_parameter(k).grad.numpy().copy()
        if k != R.TABLE and (g == 0).any():
            return None
        store["grad." + k] = g
    assert (store["grad." + R.TABLE][0] == 0).all()
    L64, g64 = R.loss_and_grads(P, batches[0])
    if any((g64[k] == 0).any() for k in names if k != R.TABLE):
        return None
    model.eval()
    with torch.no_grad():
        feat = model.compute_item_all()
        scores = model.predict(torch.from_numpy(reference_form(windows, C["item_num"])), feat)
        store["eval.scores"] = scores.numpy().copy()
    assert (store["eval.scores"][5] == 0).all()           # the all-padding window scores exactly 0 everywhere
    s64 = R.predict_literal(P, windows)
    f64 = R.predict_factorised(P, windows)
    model.train()
    model.load_state_dict(sd0, strict=True)
    opt = torch.optim.AdamW(list(model.parameters()), lr=C["lr"], weight_decay=C["wd"])
    for s, rows in enumerate(batches):
        opt.zero_grad()
        l = model(torch.from_numpy(rows))
        l.backward()
        opt.step()
        store[f"adamw.loss{s}"] = np.array(l.item(), dtype=np.float32)
    for k, v in model.state_dict().items():
        store["adamw.final." + k] = v.numpy().copy()
    gerr = max(float(np.abs(g64[k].numpy() - store["grad." + k]).max() / max(1.0, np.abs(store["grad." + k]).max())) for k in names)
    print(f"seed {seed}: reference fp32 vs float64 restatement: loss {abs(L64 - float(store['loss'])):.2e}, gradients {gerr:.2e}, "
          f"predict {float((s64 - torch.from_numpy(store['eval.scores']).double()).abs().max()):.2e} on scores up to "
          f"{float(s64.abs().max()):.2e}; factorised vs literal float64 {float((f64 - s64).abs().max()):.2e}")
    return store


def main():
    ref_shim.import_reference()
    for seed in range(61, 161):
        store = build(seed)
        if store is not None:
            break
        print(f"seed {seed}: a comparability check failed, trying the next seed")
    else:
        raise SystemExit("no seed passed the comparability checks")
    path = os.path.join(ROOT, "tests", "golden", "din_tiny.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB), loss={float(store['loss']):.6f}")


if __name__ == "__main__":
    main()
