"""Generates tests/golden/vbpr_tiny.npz by running the REFERENCE's VBPR (REC/model/ViNet/vbpr.py) unmodified, imported through
oracle/ref_shim.py.  Run where the reference is present:   python tools/make_golden_vbpr.py

Tiny shape: user_num = 7, item_num = 9, embedding_size = 16 (Dh = 8), F = 12, B = 6.  The batches repeat users and items, include
user 0 and item 0 (ordinary trainable rows in VBPR: no padding id), one item is the positive of one sample and the negative of
another, and no sample's positive equals its negative (the reference's sampler never draws one; there the item gradients cancel
to rounding noise).  Stored: the feature matrix, the initial state_dict, the loss and every gradient of one training step, the
predict scores after compute_item_all, and a 4-step torch.optim.AdamW trajectory from the initial state under the shipped
two-group settings (decay_check_name 'projection': modal_lr 1e-4, modal_decay 0.1; the rest rec_lr 1e-3, rec_decay 0, groups built
as reference trainer.py:73-91 builds them): losses, final state_dict.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

C = dict(user_num=7, item_num=9, D=16, F=12, B=6, seed=31, modal_lr=1e-4, modal_decay=0.1, rec_lr=1e-3, rec_decay=0.0)
FRAGMENT = "projection"


class FakeData:
    user_num, item_num = C["user_num"], C["item_num"]


def batch(rng):
    B, I = C["B"], C["item_num"]
    user = rng.integers(0, C["user_num"], size=B)
    user[1] = user[0]                                     # a repeated user
    user[4] = 0                                           # user 0 is an ordinary row
    pos = rng.integers(0, I, size=B)
    neg = rng.integers(0, I, size=B)
    neg[2] = pos[0]                                       # the positive of one sample is the negative of another
    pos[3] = pos[0]
    pos[5] = 0                                            # item 0 is an ordinary row
    for b in range(B):                                    # the sampler never draws the positive as the negative
        while neg[b] == pos[b]:
            neg[b] = (neg[b] + 1 + rng.integers(0, I - 1)) % I
    return user.astype(np.int64), np.stack([pos, neg], axis=1).astype(np.int64)


def main():
    ref_shim.import_reference()
    from REC.model.ViNet.vbpr import VBPR

    rng = np.random.default_rng(C["seed"])
    batches = [batch(rng) for _ in range(4)]
    assert all((b[1][:, 0] != b[1][:, 1]).all() for b in batches)
    assert batches[0][1][2, 1] == batches[0][1][0, 0]
    v_feat = rng.standard_normal((C["item_num"], C["F"])).astype(np.float32)
    store = {"meta": np.array([C[k] for k in ("user_num", "item_num", "D", "F", "B", "seed")]),
             "groups": np.array([C["modal_lr"], C["modal_decay"], C["rec_lr"], C["rec_decay"]]), "v_feat": v_feat,
             "users": np.stack([b[0] for b in batches]), "items": np.stack([b[1] for b in batches]),
             "eval.users": np.array([1, 2, 3, 4, 5, 6, 0, 3], dtype=np.int64)}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "v_feat.npy")
        np.save(path, v_feat)
        cfg = {"embedding_size": C["D"], "mlp_hidden_size": [], "dropout_prob": 0.0, "device": "cpu", "v_feat_path": path}
        torch.manual_seed(C["seed"])
        model = VBPR(cfg, FakeData())
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    for k, v in sd0.items():
        store["sd." + k] = v.numpy().copy()
    model.train()
    user, item = (torch.from_numpy(x) for x in batches[0])
    model.zero_grad()
    loss = model((user, item))
    loss.backward()
    store["loss"] = np.array(loss.item(), dtype=np.float32)
    for k, v in model.named_parameters():
        store["grad." + k] = v.grad.numpy().copy()
    model.eval()
    with torch.no_grad():
        feat = model.compute_item_all()
        store["eval.scores"] = model.predict(torch.from_numpy(store["eval.users"]), feat).numpy()
    model.train()
    model.load_state_dict(sd0, strict=True)
    inside = [p for n, p in model.named_parameters() if FRAGMENT in n]
    outside = [p for n, p in model.named_parameters() if FRAGMENT not in n]
    opt = torch.optim.AdamW([{"params": inside, "lr": C["modal_lr"], "weight_decay": C["modal_decay"]},
                             {"params": outside, "lr": C["rec_lr"], "weight_decay": C["rec_decay"]}])
    for s, (u, it) in enumerate(batches):
        opt.zero_grad()
        l = model((torch.from_numpy(u), torch.from_numpy(it)))
        l.backward()
        opt.step()
        store[f"adamw.loss{s}"] = np.array(l.item(), dtype=np.float32)
    for k, v in model.state_dict().items():
        store["adamw.final." + k] = v.numpy().copy()
    path = os.path.join(ROOT, "tests", "golden", "vbpr_tiny.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB), loss={float(store['loss']):.6f}")


if __name__ == "__main__":
    main()
