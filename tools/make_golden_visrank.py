"""Generates tests/golden/visrank_tiny.npz by running the REFERENCE's VISRANK (REC/model/ViNet/visrank.py) unmodified on the CPU,
imported through oracle/ref_shim.py.  Run where the reference is present:   python tools/make_golden_visrank.py

Tiny shape: item_num = 80, F = 12.  Histories of length 1, 3 and 60 (the 60 exercises predict's user[-50:]; the items it drops stay
in the full history the trainer masks), and one of length 5 that repeats an item.  Methods: average_top_k with top_num 1 and 3,
maximum, and a mean method ('mean': any other string).  Stored: the feature matrix, the histories and, per (method, history), the
scores predict returned -- nothing else.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

C = dict(item_num=80, F=12, seed=47)
METHODS = [("average_top_k", 1), ("average_top_k", 3), ("maximum", 0), ("mean", 0)]


class FakeData:
    item_num = C["item_num"]


def histories(rng):
    I = C["item_num"]
    h60 = rng.permutation(np.arange(1, I))[:60]
    rep = rng.permutation(np.arange(1, I))[:4]
    return [rng.integers(1, I, size=1), rng.permutation(np.arange(1, I))[:3], h60, np.array([rep[0], rep[1], rep[0], rep[2], rep[3]])]


def main():
    ref_shim.import_reference()
    from REC.model.ViNet.visrank import VISRANK

    rng = np.random.default_rng(C["seed"])
    v_feat = rng.standard_normal((C["item_num"], C["F"])).astype(np.float32)
    hists = [np.asarray(h, dtype=np.int64) for h in histories(rng)]
    store = {"meta": np.array([C["item_num"], C["F"], C["seed"]]), "v_feat": v_feat,
             "methods": np.array([m for m, _ in METHODS]), "top_nums": np.array([t for _, t in METHODS])}
    for i, h in enumerate(hists):
        store[f"hist{i}"] = h
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "v_feat.npy")
        np.save(path, v_feat)
        for mi, (method, top_num) in enumerate(METHODS):
            model = VISRANK({"method": method, "top_num": top_num, "device": "cpu", "v_feat_path": path}, FakeData())
            assert list(model.state_dict().keys()) == ["placeholder"]
            for i, h in enumerate(hists):
                store[f"scores.{mi}.{i}"] = model.predict(torch.from_numpy(h), None).numpy().astype(np.float32)
    path = os.path.join(ROOT, "tests", "golden", "visrank_tiny.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
