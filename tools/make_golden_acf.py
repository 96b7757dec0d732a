"""Generates tests/golden/acf_tiny.npz by running the REFERENCE's ACF (REC/model/ViNet/acf.py) unmodified, imported through
oracle/ref_shim.py.  Run where the reference is present:   python tools/make_golden_acf.py

Tiny shape: user_num = 7, item_num = 11, embedding_size = 8, F = 12, a 2 x 2 region map, L = 4, B = 6.  Every batch holds a
repeated user, user 0, an item that is in one row's profile, another row's positive and a third row's negative, a row with an
empty profile, a row with a full profile, and the same item twice in one profile.  Stored: the region features, the initial
state_dict (19 keys), the loss and the 18 gradients of one training step, the predict scores after compute_item_all, and a 4-step
torch.optim.AdamW trajectory from the initial state (learning_rate 1e-3 -- the shipped 1e-4 moves nothing in 4 steps -- weight
decay 0.01): losses, final state_dict.  Arrays the reference read or produced only.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

C = dict(user_num=7, item_num=11, E=8, F=12, h=2, w=2, L=4, B=6, seed=47, lr=1e-3, wd=0.01)


class FakeData:
    user_num, item_num = C["user_num"], C["item_num"]


def left_pad(seq, L):
    return [0] * (L - len(seq)) + list(seq)


def batch(rng):
    """[B, L + 3] rows [profile | positive | negative | user id] with the cases listed above."""
    I, L, B = C["item_num"], C["L"], C["B"]
    shared = int(rng.integers(1, I))
    rows = []
    for b in range(B):
        n = int(rng.integers(1, L + 1))
        prof = [int(i) for i in rng.integers(1, I, size=n)]
        pos, neg, uid = int(rng.integers(1, I)), int(rng.integers(1, I)), int(rng.integers(0, C["user_num"]))
        if b == 0:
            prof[-1] = shared                                # `shared` in a profile ...
        if b == 1:
            pos, uid = shared, rows[0][-1]                   # ... the positive of another row (and a repeated user) ...
        if b == 2:
            neg, uid = shared, 0                             # ... and the negative of a third (user 0)
        if b == 3:
            prof = []                                        # an empty profile
        if b == 4:
            prof = [int(i) for i in rng.integers(1, I, size=L)]          # a full profile ...
            prof[1] = prof[3]                                # ... with the same item twice
        while neg == pos:
            neg = int(rng.integers(1, I))
        rows.append(left_pad(prof, L) + [pos, neg, uid])
    return np.asarray(rows, dtype=np.int64)


def main():
    ref_shim.import_reference()
    from REC.model.ViNet.acf import ACF

    rng = np.random.default_rng(C["seed"])
    batches = [batch(rng) for _ in range(4)]
    v_feat = rng.standard_normal((C["item_num"], C["h"], C["w"], C["F"])).astype(np.float32)
    windows = np.asarray([left_pad([3, 5], C["L"]) + [1], left_pad([], C["L"]) + [2], [1, 2, 3, 4, 0], [6, 6, 7, 10, 5],
                          left_pad([9], C["L"]) + [1]], dtype=np.int64)
    store = {"meta": np.array([C[k] for k in ("user_num", "item_num", "E", "F", "h", "w", "L", "B", "seed")]),
             "hyper": np.array([C["lr"], C["wd"]]), "v_feat": v_feat, "rows": np.stack(batches), "eval.windows": windows}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "v_feat.npy")
        np.save(path, v_feat)
        cfg = {"embedding_size": C["E"], "device": "cpu", "v_feat_path": path, "MAX_ITEM_LIST_LENGTH": C["L"]}
        torch.manual_seed(C["seed"])
        model = ACF(cfg, FakeData())
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    store["sd.keys"] = np.array(list(sd0))
    for k, v in sd0.items():
        store["sd." + k] = v.numpy().copy()
    model.train()
    model.zero_grad()
    loss = model(torch.from_numpy(batches[0]))
    loss.backward()
    store["loss"] = np.array(loss.item(), dtype=np.float32)
    for k, v in model.named_parameters():
        store["grad." + k] = v.grad.numpy().copy()
    model.eval()
    with torch.no_grad():
        store["eval.scores"] = model.predict(torch.from_numpy(windows), model.compute_item_all()).numpy()
    model.train()
    model.load_state_dict(sd0, strict=True)
    opt = torch.optim.AdamW(model.parameters(), lr=C["lr"], weight_decay=C["wd"])
    for s, rows in enumerate(batches):
        opt.zero_grad()
        l = model(torch.from_numpy(rows))
        l.backward()
        opt.step()
        store[f"adamw.loss{s}"] = np.array(l.item(), dtype=np.float32)
    for k, v in model.state_dict().items():
        store["adamw.final." + k] = v.numpy().copy()
    path = os.path.join(ROOT, "tests", "golden", "acf_tiny.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB), loss={float(store['loss']):.6f}, "
          f"{len(sd0)} state keys, {len(list(model.named_parameters()))} parameters")


if __name__ == "__main__":
    main()
