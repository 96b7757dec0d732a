"""Generates tests/golden/dssm_tiny.npz, dssm_mlp_tiny.npz and fm_tiny.npz by running the REFERENCE's DSSM and FM
(REC/model/IDNet/dssm.py, fm.py) unmodified, imported through oracle/ref_shim.py.  Run where the reference is present:
    python tools/make_golden_pool.py

Tiny shape: item_num = 13, embedding_size = 8, L = 4, six samples per batch, four batches of [profile (L) | positive | negative]
rows; the DSSM MLP case uses mlp_hidden_size = [8, 12, 8].  Every batch holds a full profile, profiles with one, two and three
padded positions, an all-padding profile and a profile that repeats an item; the positive of sample 0 also sits in its own
profile; one item is the positive of one sample and the negative of another; no sample's positive equals its negative.

The reference's forward begins with `inputs = inputs[0].unsqueeze(0)`: it sees ONE row.  The generator therefore calls it once per
row of a batch (a one-row batch), averages the six losses and the six gradients in float64 and stores that -- the loss and the
gradient of the mean over every row, which is what the native models compute.

Stored per model: the initial state_dict with its key list, the loss and the gradients of step one (the table's row 0 exactly
zero), the reference's loss and gradients on the first row of that batch alone (one.*: a one-row batch, no averaging), predict for eight windows (one of them all padding), a 4-step torch.optim.AdamW trajectory (configs/overall/ID.yaml's
learning_rate 1e-4, weight_decay 0.1) of the per-batch averaged gradients -- losses and final state_dict -- and, under ref_err.*,
the distance of every one of these from the float64 restatement (tests/pool_restate.py; FM: the literal formula, which is what the
reference computes).  These distances are the reference's own float32 error; the tests take them as the tolerance.

A fixture is only worth comparing against if rounding cannot flip a ranking or a ReLU, so the generator checks in float64 and moves
on to the next seed when a check fails:
  * among the unmasked items of every non-padding window, adjacent float64 scores down to rank K + 1 (K = 10) are more than
    MARGIN = 1e-5 apart;
  * (MLP case) at the initial state no ReLU pre-activation of the four batches and the eight windows lies within 1e-4 of 0, and
    along the float64 trajectory none lies within 1e-6 of 0.  A row with an all-padding profile is exempt in the first layer: its
    pre-activation is the bias itself, the same number in every precision (exactly 0 at the initial state, where relu' is 0 in
    the reference and in the kernels alike); the same holds further down while the layer input stays exactly zero.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import pool_restate as R  # noqa: E402

C = dict(item_num=13, D=8, L=4, B=6, lr=1e-4, wd=0.1, K=10)
MARGIN = 1e-5
CASES = {"dssm_tiny": ("DSSM", []), "dssm_mlp_tiny": ("DSSM", [8, 12, 8]), "fm_tiny": ("FM", [])}


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
    pos[0] = prof[0, 1]                                   # a positive that also sits in its own profile
    neg[2] = pos[0]                                       # the positive of one sample is the negative of another
    for b in range(B):                                    # no sample whose positive equals its negative
        while neg[b] == pos[b]:
            if b == 2:
                pos[b] = rng.integers(1, I)
            else:
                neg[b] = rng.integers(1, I)
    return np.concatenate((prof, pos[:, None], neg[:, None]), axis=1)


def rankings_comparable(kind, P, windows):
    s = R.predict(kind, P, windows).clone()
    s[:, 0] = float("-inf")
    top = torch.sort(s, dim=-1, descending=True).values[:, :C["K"] + 1]
    for b in range(len(windows)):
        if (windows[b] != 0).any() and bool(((top[b, :-1] - top[b, 1:]) <= MARGIN).any()):
            return False
    return True


def relus_stable(P, profiles, margin):
    """No pre-activation of the DSSM MLP within `margin` of 0.  A row whose layer input is exactly zero (an all-padding profile, and
    what zero biases make of it further down) is exempt: its pre-activation is the bias itself, the same number in every precision
    -- it only must not be a nonzero number below 1e-9."""
    x = R.pooled(P[R.TABLE], torch.as_tensor(profiles), True)
    for i in range(R.n_layers_of(P)):
        z = x @ P[f"mlp_layers.mlp_layers.{3 * i + 1}.weight"].T + P[f"mlp_layers.mlp_layers.{3 * i + 1}.bias"]
        exempt = (x == 0).all(1)
        if bool(exempt.any()) and bool(((z[exempt] != 0) & (z[exempt].abs() <= 1e-9)).any()):
            return False
        if bool((~exempt).any()) and float(z[~exempt].abs().min()) <= margin:
            return False
        x = torch.relu(z)
    return True


def ref_input(kind, rows):
    return R.fm_form(rows) if kind == "FM" else torch.as_tensor(rows)


def ref_mean_step(model, kind, rows, names):
    """The reference's loss and gradients of every row on its own, averaged in float64."""
    inp = ref_input(kind, rows)
    loss = 0.0
    grads = {k: torch.zeros_like(model.get_parameter(k), dtype=torch.float64) for k in names}
    for b in range(len(rows)):
        model.zero_grad()
        l = model(inp[b:b + 1])
        l.backward()
        loss += float(l.detach().double())
        for k in names:
            g = model.get_parameter(k).grad
            if g is not None:
                grads[k] += g.double()
    n = len(rows)
    return loss / n, {k: g / n for k, g in grads.items()}


def build(name, kind, hidden, seed):
    REC = __import__("REC.model.IDNet." + kind.lower(), fromlist=[kind])
    Model = getattr(REC, kind)
    rng = np.random.default_rng(seed)
    batches = [batch(rng) for _ in range(4)]
    windows = np.zeros((8, C["L"]), dtype=np.int64)
    for b, n_real in enumerate((4, 4, 3, 2, 1, 0, 4, 3)):  # one window is all padding
        windows[b, C["L"] - n_real:] = rng.integers(1, C["item_num"], size=n_real)
    cfg = {"embedding_size": C["D"], "mlp_hidden_size": list(hidden), "device": "cpu", "dropout_prob": 0,
           "MAX_ITEM_LIST_LENGTH": C["L"]}
    torch.manual_seed(seed)
    model = Model(cfg, FakeData())
    nl = max(0, len(hidden) - 1)
    keys, names = R.names(kind, nl), R.param_names(kind, nl)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    assert list(sd0) == keys, list(sd0)
    assert [n for n, _ in model.named_parameters()] == names
    P = {k: v.double() for k, v in sd0.items()}
    if not rankings_comparable(kind, P, windows):
        return None
    if nl and not relus_stable(P, np.concatenate([b[:, :-2] for b in batches] + [windows]), 1e-4):
        return None
    store = {"meta": np.array([C["item_num"], C["D"], C["L"], C["B"], C["K"], seed] + list(hidden)),
             "optim": np.array([C["lr"], C["wd"]]), "rows": np.stack(batches), "eval.windows": windows, "sd.keys": np.array(keys),
             "param.keys": np.array(names)}
    for k, v in sd0.items():
        store["sd." + k] = v.numpy().copy()
    model.train()
    loss, grads = ref_mean_step(model, kind, batches[0], names)
    L64, g64 = R.loss_and_grads(kind, P, batches[0], literal=True)
    store["loss"] = np.array(loss)                     # the float64 mean of six float32 losses
    store["ref_err.loss"] = np.array(abs(loss - L64))
    for k in names:
        store["grad." + k] = grads[k].numpy().copy()   # float64 means, as handed to AdamW after one rounding
        store["ref_err.grad." + k] = np.array(float((grads[k] - g64[k]).abs().max()))
    assert (store["grad." + R.TABLE][0] == 0).all()
    # a one-row batch: the reference's own forward on it, no averaging
    one = batches[0][:1]
    model.zero_grad()
    l1 = model(ref_input(kind, one))
    l1.backward()
    L1, g1 = R.loss_and_grads(kind, P, one, literal=True)
    store["one.loss"] = np.array(l1.item(), dtype=np.float32)
    store["ref_err.one.loss"] = np.array(abs(float(l1.detach().double()) - L1))
    for k in names:
        g = model.get_parameter(k).grad
        g = torch.zeros_like(model.get_parameter(k)) if g is None else g
        store["one.grad." + k] = g.numpy().copy()
        store["ref_err.one.grad." + k] = np.array(float((g.double() - g1[k]).abs().max()))
    model.eval()
    with torch.no_grad():
        scores = model.predict(torch.from_numpy(windows), model.compute_item_all())
    store["eval.scores"] = scores.numpy().copy()
    assert (store["eval.scores"][5] == 0).all() or nl      # the all-padding window pools to exactly 0
    s64 = R.predict(kind, P, windows)
    store["ref_err.scores"] = np.array(float((s64 - scores.double()).abs().max()))
    # the trajectory: torch.optim.AdamW on the per-batch averaged gradients
    model.train()
    model.load_state_dict(sd0, strict=True)
    opt = torch.optim.AdamW(list(model.parameters()), lr=C["lr"], weight_decay=C["wd"])
    T = {k: v.clone() for k, v in P.items()}
    l64s, _ = R.adamw(kind, T, batches, C["lr"], C["wd"], literal=True)
    Tchk = {k: v.clone() for k, v in P.items()}
    for s, rows in enumerate(batches):
        if nl and not relus_stable(Tchk, rows[:, :-2], 1e-6):
            return None
        l, g = ref_mean_step(model, kind, rows, names)
        opt.zero_grad()
        for k in names:
            model.get_parameter(k).grad = g[k].float()
        opt.step()
        store[f"adamw.loss{s}"] = np.array(l)
        store[f"ref_err.loss{s}"] = np.array(abs(l - l64s[s]))
        Tchk = {k: v.detach().double().clone() for k, v in model.state_dict().items()}       # the next step's state
    for k, v in model.state_dict().items():
        store["adamw.final." + k] = v.numpy().copy()
        store["ref_err.final." + k] = np.array(float((v.double() - T[k]).abs().max()))
    gerr = max(float(store["ref_err.grad." + k]) for k in names)
    ferr = max(float(store["ref_err.final." + k]) for k in keys)
    print(f"{name} seed {seed}: reference fp32 vs float64 restatement: loss {float(store['ref_err.loss']):.2e}, gradients {gerr:.2e}, "
          f"predict {float(store['ref_err.scores']):.2e} on scores up to {float(s64.abs().max()):.2e}, trajectory losses "
          f"{max(float(store[f'ref_err.loss{s}']) for s in range(4)):.2e}, final state {ferr:.2e}")
    return store


def main():
    ref_shim.import_reference()
    for name, (kind, hidden) in CASES.items():
        for seed in range(61, 161):
            store = build(name, kind, hidden, seed)
            if store is not None:
                break
            print(f"{name} seed {seed}: a comparability check failed, trying the next seed")
        else:
            raise SystemExit(f"{name}: no seed passed the comparability checks")
        path = os.path.join(ROOT, "tests", "golden", name + ".npz")
        np.savez_compressed(path, **store)
        print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB), loss={float(store['loss']):.6f}")


if __name__ == "__main__":
    main()
