"""Generates tests/golden/widedeep_tiny.npz by running the REFERENCE's WideDeep (REC/model/IDNet/widedeep.py) unmodified, imported
through oracle/ref_shim.py.  Run where the reference is present:   python tools/make_golden_widedeep.py

The reference sizes its first Linear by embedding_size * MAX_ITEM_LIST_LENGTH while its datasets deliver MAX_ITEM_LIST_LENGTH + 1
ids per row, so the model is built with MAX_ITEM_LIST_LENGTH = L + 1: exactly the shapes pixelrec_amd.model.WideDeep has for a
history of L items.

Tiny shape: item_num = 13, embedding_size = 8, mlp_hidden_size = [12, 4], L = 4, B = 6, four batches of [profile (L) | positive |
negative] rows (fed to the reference as its [B, 2, L + 1] planes).  Every batch holds a full profile, profiles with one, two and
three padded positions, an all-padding profile and a profile that repeats an item; one item is the positive of one sample and the
negative of another, and no sample's positive equals its negative.  The reference initialises every bias to 0; the generator
overwrites the biases (wide_bias and the predict bias included) with small random values so that predict's values depend on them.

Stored: the initial state_dict with its key order, the loss and all nine gradients of one training step (row 0 of both tables
exactly zero; the gradients of wide_bias and of the predict bias as the reference's float32 arithmetic gives them -- rounding
residue of a sum that is exactly zero), predict through the reference's [B, N, L + 1] form for eight windows (one of them all
padding), and a 4-step torch.optim.AdamW trajectory from the initial state under configs/overall/ID.yaml's optim_args
(learning_rate 1e-4, weight_decay 0.1): losses and the final state_dict.

The fixture is only worth comparing against if rounding cannot flip a ranking, so the generator checks in float64 (with
tests/widedeep_restate.py) that among the unmasked items of every window adjacent scores down to rank K + 1 (K = 10) are more than
MARGIN = 1e-5 apart -- the margin the id comparisons of tests/test_gpu_widedeep.py rely on -- and moves on to the next seed
otherwise.

    python tools/make_golden_widedeep.py --measure

prints instead the figure tests/test_gpu_widedeep.py records as FUSED_MEASURED: the largest error of the reference's own float32
predict against float64 over the inputs of the fused top-k test (widedeep_restate.topk_grid), relative to the largest |score| of
the case, and how many (user, rank) cells float64 alone would excuse under four times that figure.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import widedeep_restate as R  # noqa: E402

C = dict(item_num=13, D=8, hidden=[12, 4], L=4, B=6, lr=1e-4, wd=0.1, K=10)
MARGIN = 1e-5


def reference_model(item_num, D, hidden, L):
    from REC.model.IDNet.widedeep import WideDeep

    class FakeData:
        pass

    FakeData.item_num = item_num
    cfg = {"embedding_size": D, "mlp_hidden_size": list(hidden), "device": "cpu", "dropout_prob": 0, "MAX_ITEM_LIST_LENGTH": L + 1,
           "method": None}
    return WideDeep(cfg, FakeData())


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
    return not bool(((top[:, :-1] - top[:, 1:]) <= MARGIN).any())


def build(seed):
    rng = np.random.default_rng(seed)
    batches = [batch(rng) for _ in range(4)]
    windows = np.zeros((8, C["L"]), dtype=np.int64)
    for b, n_real in enumerate((4, 4, 3, 2, 1, 0, 4, 3)):  # one window is all padding
        windows[b, C["L"] - n_real:] = rng.integers(1, C["item_num"], size=n_real)
    torch.manual_seed(seed)
    model = reference_model(C["item_num"], C["D"], C["hidden"], C["L"])
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("bias"):
                p.copy_(torch.randn(p.shape) * 0.1)
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
    loss = model(R.planes(batches[0]))
    loss.backward()
    store["loss"] = np.array(loss.item(), dtype=np.float32)
    for k in names:
        store["grad." + k] = model.get_parameter(k).grad.numpy().copy()
    assert (store["grad." + R.DEEP][0] == 0).all() and (store["grad." + R.WIDE][0] == 0).all()
    L64, g64 = R.loss_and_grads(P, batches[0])
    model.eval()
    with torch.no_grad():
        scores = model.predict((torch.from_numpy(reference_form(windows, C["item_num"])), None), None)
        store["eval.scores"] = scores.numpy().copy()
    s64 = R.predict_literal(P, windows)
    f64 = R.predict_factorised(P, windows)
    model.train()
    model.load_state_dict(sd0, strict=True)
    opt = torch.optim.AdamW(list(model.parameters()), lr=C["lr"], weight_decay=C["wd"])
    for s, rows in enumerate(batches):
        opt.zero_grad()
        l = model(R.planes(rows))
        l.backward()
        opt.step()
        store[f"adamw.loss{s}"] = np.array(l.item(), dtype=np.float32)
    for k, v in model.state_dict().items():
        store["adamw.final." + k] = v.numpy().copy()
    gerr = max(float(np.abs(g64[k].numpy() - store["grad." + k]).max() / max(1.0, np.abs(store["grad." + k]).max())) for k in names)
    print(f"seed {seed}: reference fp32 vs float64 restatement: loss {abs(L64 - float(store['loss'])):.2e}, gradients {gerr:.2e}, "
          f"predict {float((s64 - torch.from_numpy(store['eval.scores']).double()).abs().max()):.2e} on scores up to "
          f"{float(s64.abs().max()):.2e}; factorised vs literal float64 {float((f64 - s64).abs().max()):.2e}; the cancelled biases' "
          f"reference gradients {float(store['grad.' + R.WBIAS][0]):.2e}, {float(store['grad.' + R.PRED_B][0]):.2e}")
    return store


def measure():
    """The reference's own float32 predict against float64 over the fused top-k test's inputs."""
    worst, worst_case, cells, excused_at = 0.0, None, 0, []
    cases = []
    for item_num, hidden, D, L, B in R.topk_grid():
        P, win, hist = R.topk_case(item_num, B, D, L, hidden)
        model = reference_model(item_num, D, hidden, L)
        model.load_state_dict(P, strict=True)
        model.eval()
        with torch.no_grad():
            s32 = model.predict((torch.from_numpy(reference_form(win.numpy(), item_num)), None), None)
        s64 = R.predict_literal({k: v.double() for k, v in P.items()}, win)
        rel = float((s32.double() - s64).abs().max()) / float(s64.abs().max())
        if rel > worst:
            worst, worst_case = rel, (item_num, hidden, D, L, B)
        cases.append((s64, R.topk_histories(s64, hist)))
    print(f"FUSED_MEASURED = {worst:.3e}   (case item_num, hidden, D, L, B = {worst_case})")
    smallest = float("inf")
    for s64, hist in cases:
        _, masked = R.masked_topk(s64, hist, 1)
        v = torch.topk(masked, min(R.TOPK_K + 1, masked.shape[1]), -1).values
        scale = float(s64.abs().max())
        for b in range(v.shape[0]):
            for r in range(R.TOPK_K):
                if v[b, r] == float("-inf"):
                    continue
                cells += 1
                gaps = ([float(v[b, r - 1] - v[b, r])] if r > 0 else []) + \
                       ([float(v[b, r] - v[b, r + 1])] if r + 1 < v.shape[1] and v[b, r + 1] > float("-inf") else [])
                if gaps:
                    smallest = min(smallest, min(gaps) / scale)
                    excused_at.append(min(gaps) / scale)
    tol = 4 * worst
    print(f"under 4 x that = {tol:.3e}: float64 alone excuses {sum(1 for g in excused_at if g <= tol)} of {cells} cells; smallest "
          f"normalised gap {smallest:.3e}")


def main():
    ref_shim.import_reference()
    if "--measure" in sys.argv:
        return measure()
    for seed in range(71, 171):
        store = build(seed)
        if store is not None:
            break
        print(f"seed {seed}: a comparability check failed, trying the next seed")
    else:
        raise SystemExit("no seed passed the comparability checks")
    path = os.path.join(ROOT, "tests", "golden", "widedeep_tiny.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB), loss={float(store['loss']):.6f}")


if __name__ == "__main__":
    main()
