"""Generates tests/golden/bert4rec_tiny.npz by running the REFERENCE's BERT4Rec (REC/model/IDNet/bert4rec.py) unmodified,
imported through oracle/ref_shim.py.  Run where the reference is present:   python tools/make_golden_bert4rec.py

Tiny case: item_num = 97, D = 32, L = 8 (9 positions), 2 heads, inner 2, 2 layers, B = 5, dropout 0 (eval mode).  The batch has
left-padded windows, one full window, one window with no masked position, a mask token in every other window; negatives are
drawn outside their sequence.  Stored: inputs, state_dict, loss, every parameter gradient (dense; the table's mask-token row is
nonzero and row 0 zero), predict scores, and a 4-step torch.optim.AdamW trajectory (losses + final parameters).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from oracle.sasrec_oracle import synth_params  # noqa: E402

C = dict(item_num=97, D=32, L=8, H=2, inner=2, n_layers=2, B=5, seed=41, mask_ratio=0.4)


def ref_config():
    return {"n_layers": C["n_layers"], "n_heads": C["H"], "embedding_size": C["D"], "inner_size": C["inner"],
            "hidden_dropout_prob": 0.0, "attn_dropout_prob": 0.0, "hidden_act": "gelu", "layer_norm_eps": 1e-12,
            "initializer_range": 0.02, "MAX_ITEM_LIST_LENGTH": C["L"], "mask_ratio": C["mask_ratio"], "device": "cpu"}


def make_batch(rng, lens, no_mask_row=None):
    """Windows of the given lengths masked like BERT4RecTrainDataset.reconstruct_train_data (trainset.py:445-468)."""
    P, N, tok = C["L"] + 1, C["item_num"], C["item_num"]
    B = len(lens)
    items = np.zeros((B, 3, P), dtype=np.int64)
    mask = np.zeros((B, P), dtype=np.int64)
    for b, n in enumerate(lens):
        seq = rng.choice(np.arange(1, N), size=n, replace=False)
        m = rng.random(n) < C["mask_ratio"]
        if b == no_mask_row:
            m[:] = False
        elif not m.any():
            m[rng.integers(n)] = True
        neg = np.zeros(n, dtype=np.int64)
        for t in np.nonzero(m)[0]:
            while True:
                x = int(rng.integers(1, N))
                if x not in seq:
                    neg[t] = x
                    break
        items[b, 0, P - n:] = np.where(m, tok, seq)
        items[b, 1, P - n:] = seq
        items[b, 2, P - n:] = neg
        mask[b, P - n:] = m
    return items, mask


def main():
    ref_shim.import_reference()
    from REC.model.IDNet.bert4rec import BERT4Rec

    torch.manual_seed(C["seed"])
    rng = np.random.default_rng(C["seed"])

    class DL:
        item_num = C["item_num"]

    model = BERT4Rec(ref_config(), DL())
    params = synth_params(C["item_num"] + 1, C["D"], C["L"] + 1, C["n_layers"], C["inner"], seed=C["seed"])
    res = model.load_state_dict(params, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.eval()
    store = {"meta": np.array([C[k] for k in ("item_num", "D", "L", "H", "inner", "n_layers", "B", "seed")])}
    for k, v in model.state_dict().items():
        store["sd." + k] = v.numpy().copy()

    lens = [3, C["L"] + 1, 6, 2, 5]
    items, mask = make_batch(rng, lens, no_mask_row=3)
    store["items"], store["masked_index"] = items, mask
    model.zero_grad()
    loss = model((torch.from_numpy(items), torch.from_numpy(mask)))
    loss.backward()
    store["loss"] = np.array(loss.item(), dtype=np.float32)
    for k, v in model.named_parameters():
        store["grad." + k] = v.grad.numpy().copy()
    g = model.item_embedding.weight.grad
    assert float(g[0].abs().max()) == 0.0 and float(g[C["item_num"]].abs().max()) > 0.0

    # predict on windows of the last L items (left-padded), scored against compute_item_all()
    item_seq = np.zeros((6, C["L"]), dtype=np.int64)
    for b, n in enumerate([1, 3, C["L"], 5, 2, 7]):
        item_seq[b, C["L"] - n:] = rng.choice(np.arange(1, C["item_num"]), size=n, replace=False)
    store["eval.item_seq"] = item_seq
    with torch.no_grad():
        store["eval.scores"] = model.predict(torch.from_numpy(item_seq), model.compute_item_all()).numpy()

    # 4 AdamW steps (lr 1e-4, wd 0.1), the first on the batch above
    batches = [(items, mask)] + [make_batch(rng, list(rng.integers(2, C["L"] + 2, size=C["B"]))) for _ in range(3)]
    store["adamw.items"] = np.stack([b[0] for b in batches])
    store["adamw.masks"] = np.stack([b[1] for b in batches])
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.1)
    for s, (it, mk) in enumerate(batches):
        opt.zero_grad()
        l = model((torch.from_numpy(it), torch.from_numpy(mk)))
        l.backward()
        opt.step()
        store[f"adamw.loss{s}"] = np.array(l.item(), dtype=np.float32)
    for k, v in model.state_dict().items():
        store["adamw.final." + k] = v.numpy().copy()

    path = os.path.join(ROOT, "tests", "golden", "bert4rec_tiny.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB), loss={float(store['loss']):.6f}")


if __name__ == "__main__":
    main()
