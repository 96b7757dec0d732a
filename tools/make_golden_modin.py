"""Generates tests/golden/modin_tiny.npz by running the REFERENCE's MODIN (REC/model/PixelNet/modin.py) unmodified, imported
through oracle/ref_shim.py.  Run where the reference is present:
    python tools/make_golden_modin.py

The reference's `load_model` cannot run offline (it downloads the CLIP checkpoint).  It is replaced -- in the imported module's
namespace only, the way tools/make_golden_mopool.py does it -- by a function that builds the same tiny random CLIP tower
(ENCODER_SHAPES["clip-vit-tiny-test"]), freezes the first `tune_scale` named parameters (5 + 16 * 2: block 2 and rec_fc train) and
wraps it in the reference's own MeanItemEncoder.  Everything downstream is the reference's code.

Tiny shape: 13 items, a 13-image store of 64 x 64 fp16-exact images (row 0 the zero image), embedding_size 8, L = 4,
mlp_hidden_size [12, 4], six samples per batch, two batches.  The pixels are multiples of 1 / 16 and the initial weights multiples
of 2^-10 (random all the same): that is what keeps the file under 1 MB.  A batch is `items` [6, L + 2] = [profile | positive |
negative] ids into the store (0 = padding); the reference's forward gets (store[items], items), one image per position.  Each
batch holds a full profile, profiles with one, two and three padded positions, an all-padding profile, a profile that repeats an
item, an item that is history in one sample and a target in another, and a positive that sits in its own profile.

Stored: the state_dict with its key list (the reference's names under the installed transformers), per batch the loss and the
gradient of every trainable parameter (6 attention tensors, 18 encoder tensors), compute_item over the store, predict in the
reference's [B, item_num, L + 1] form for eight windows (one all padding), and, under ref_err.*, the distance of each of these from
the float64 restatement: tests/modin_restate.py on the float64 encoder output (the same modules in double).  These distances are
the reference's own float32 error; the tests add them to their budgets.

A fixture is only worth comparing against if rounding cannot flip a ranking, so the generator checks in float64 and moves on to the
next seed when the check fails: among the unmasked items of every non-padding window, adjacent float64 scores down to rank K + 1
(K = 10) are more than MARGIN = 1e-5 apart.
"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import modin_restate as R  # noqa: E402

SHAPE = (64, 3, 4, 128, 64, 32)      # hidden, layers, heads, mlp, image, patch  (= ENCODER_SHAPES["clip-vit-tiny-test"])
TUNE = 5 + 16 * 2                    # freeze embeddings + blocks 0, 1; train block 2 and rec_fc
C = dict(item_num=13, D=8, L=4, B=6, K=10, hidden=[12, 4])
MARGIN = 1e-5
ENC = "visual_encoder."


class FakeData:
    item_num = C["item_num"]


def batch(rng):
    """items [B, L + 2] of ids into the store (0 = padding)."""
    I, L, B = C["item_num"], C["L"], C["B"]
    used = np.arange(1, I)
    prof = np.zeros((B, L), dtype=np.int64)
    for b, n_real in enumerate((4, 3, 2, 1, 0, 4)):      # full, one / two / three padded, all padding, (repeated item below)
        prof[b, L - n_real:] = rng.choice(used, size=n_real, replace=False)
    prof[5, 2] = prof[5, 0]                               # a repeated item inside a profile
    pos = rng.choice(used, size=B)
    neg = rng.choice(used, size=B)
    pos[0] = prof[0, 1]                                   # the positive of sample 0 sits in its own profile ...
    neg[2] = pos[0]                                       # ... and is the negative of sample 2: history here, target there
    for b in range(B):                                    # no sample whose positive equals its negative
        while neg[b] == pos[b]:
            if b == 2:
                pos[b] = rng.choice(used)
            else:
                neg[b] = rng.choice(used)
    return np.concatenate((prof, pos[:, None], neg[:, None]), axis=1)


def rankings_comparable(P64, feat64, windows):
    s = R.predict(P64, feat64, windows).clone()
    s[:, 0] = float("-inf")
    top = torch.sort(s, dim=-1, descending=True).values[:, :C["K"] + 1]
    for b in range(len(windows)):
        if (windows[b] != 0).any() and bool(((top[b, :-1] - top[b, 1:]) <= MARGIN).any()):
            return False
    return True


def build(seed):
    from transformers import CLIPVisionConfig, CLIPVisionModel

    ref_mod = __import__("REC.model.PixelNet.modin", fromlist=["MODIN"])
    from REC.model.layers import MeanItemEncoder

    def load_model(config):
        hidden, n_layers, heads, inter, image, patch = SHAPE
        cfg = CLIPVisionConfig(hidden_size=hidden, intermediate_size=inter, num_hidden_layers=n_layers,
                               num_attention_heads=heads, image_size=image, patch_size=patch)
        model = CLIPVisionModel(cfg)
        for index, (_, p) in enumerate(model.named_parameters()):       # load.py:97-99
            if index < config["fine_tune_arg"]["tune_scale"]:
                p.requires_grad = False
        return MeanItemEncoder(item_encoder=model, input_dim=hidden, output_dim=config["embedding_size"],
                               act_name="relu", dnn_layers=[])                         # load.py:116-117

    ref_mod.load_model = load_model
    I, D, L = C["item_num"], C["D"], C["L"]
    config = {"embedding_size": D, "mlp_hidden_size": list(C["hidden"]), "dropout_prob": 0, "device": "cpu", "MAX_ITEM_LIST_LENGTH": L,
              "fine_tune_arg": {"tune_scale": TUNE, "pre_trained": True, "activation": "relu", "dnn_layers": [], "method": "mean"}}
    torch.manual_seed(seed)
    model = ref_mod.MODIN(config, FakeData())
    with torch.no_grad():                                               # make biases / LN affine non-trivial
        for n, p in model.named_parameters():
            if n.endswith("bias") or "layer_norm" in n or "layrnorm" in n:
                p.add_(0.05 * torch.randn_like(p))
        for p in model.parameters():                                    # every weight a multiple of 2^-10 (exact in float32): the
            p.copy_(torch.round(p * 1024) / 1024)                       # random tensors then deflate to a quarter of their size
    model.eval()                                                        # (no dropout anywhere; eval keeps HF's modules quiet)
    keys = list(model.state_dict())
    att = [k for k in keys if not k.startswith(ENC)]
    assert att == R.names(len(C["hidden"])) and keys[:len(att)] == att, att
    g = torch.Generator().manual_seed(seed)
    store_img = (torch.round(torch.randn(I, 3, SHAPE[4], SHAPE[4], generator=g) * 16) / 16).half()     # multiples of 1 / 16
    store_img[0] = 0.0
    images = store_img.float()
    rng = np.random.default_rng(seed)
    batches = [batch(rng) for _ in range(2)]
    windows = np.zeros((8, L), dtype=np.int64)
    for b, n_real in enumerate((4, 4, 3, 2, 1, 0, 4, 3)):               # one window is all padding
        windows[b, L - n_real:] = rng.integers(1, I, size=n_real)

    enc64 = copy.deepcopy(model.visual_encoder).double()
    P64 = {k: model.state_dict()[k].double() for k in att}
    with torch.no_grad():
        feat64 = enc64(images.double())
    if not rankings_comparable(P64, feat64, windows):
        return None
    # post_layernorm is trainable by index and unused under method 'mean': it never receives a gradient and is left out
    names = [n for n, p in model.named_parameters() if p.requires_grad and "post_layernorm" not in n]
    assert len(names) == 6 + 18, len(names)
    out = {"meta": np.array([I, D, L, C["B"], C["K"], seed, TUNE]), "hidden": np.array(C["hidden"]), "shape": np.array(SHAPE),
           "store": store_img.numpy(), "sd.keys": np.array(keys), "param.keys": np.array(names), "eval.windows": windows,
           "frozen": np.array([n for n, p in model.named_parameters() if not p.requires_grad])}
    for k, v in model.state_dict().items():
        out["sd." + k] = v.numpy().copy()
    worst = {"loss": 0.0, "grad": 0.0}
    for j, items in enumerate(batches):
        it = torch.from_numpy(items)
        modal = images[it]                                              # [B, L + 2, 3, H, W]: one image per position
        model.zero_grad()
        loss = model((modal, it))
        loss.backward()
        enc64.zero_grad()
        Q64 = {k: v.clone().requires_grad_(True) for k, v in P64.items()}
        loss64 = R.loss_of(Q64, enc64(images.double()), items)          # the same function on the store's rows, each encoded once
        loss64.backward()
        g64 = {ENC + n: p.grad for n, p in enc64.named_parameters()}
        g64.update({k: v.grad for k, v in Q64.items()})
        out[f"b{j}.items"] = items
        out[f"b{j}.loss"] = loss.detach().numpy().copy()
        out[f"ref_err.b{j}.loss"] = np.array(abs(float(loss.detach().double()) - float(loss64.detach())))
        worst["loss"] = max(worst["loss"], float(out[f"ref_err.b{j}.loss"]))
        for n in names:
            gr = model.get_parameter(n).grad
            assert gr is not None, n
            out[f"b{j}.grad." + n] = gr.numpy().copy()
            e = float((gr.double() - g64[n]).abs().max())
            out[f"ref_err.b{j}.grad." + n] = np.array(e)
            worst["grad"] = max(worst["grad"], e)
    ref_seq = R.reference_form(windows, I)
    with torch.no_grad():
        feat = model.compute_item(images)
        scores = model.predict(ref_seq, feat)
    out["eval.item_feature"] = feat.numpy().copy()
    out["ref_err.item_feature"] = np.array(float((feat.double() - feat64).abs().max()))
    out["eval.scores"] = scores.numpy().copy()
    s64 = R.predict(P64, feat64, ref_seq)
    out["ref_err.scores"] = np.array(float((s64 - scores.double()).abs().max()))
    assert (out["eval.scores"][5] == 0).all()                           # the all-padding window scores exactly 0
    print(f"MODIN seed {seed}: reference fp32 vs float64 restatement: loss {worst['loss']:.2e}, gradients {worst['grad']:.2e}, item "
          f"features {float(out['ref_err.item_feature']):.2e}, predict {float(out['ref_err.scores']):.2e} on scores up to "
          f"{float(s64.abs().max()):.2e}; {len(names)} trainable of {len(keys)} tensors")
    return out


def main():
    # resolve transformers' lazy modules BEFORE the inert torchvision stub exists (its availability probe needs a real module
    # spec); these are the names REC/model/load.py imports
    from transformers import BeitModel, CLIPVisionModel, SwinConfig, SwinModel, ViTMAEModel  # noqa: F401

    ref_shim.import_reference()
    for seed in range(71, 171):
        out = build(seed)
        if out is not None:
            break
        print(f"modin_tiny seed {seed}: the ranking-margin check failed, trying the next seed")
    else:
        raise SystemExit("modin_tiny: no seed passed the ranking-margin check")
    path = os.path.join(ROOT, "tests", "golden", "modin_tiny.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1_000_000, size
    print(f"wrote {path} ({size / 1024:.0f} KiB), losses {[float(out[f'b{j}.loss']) for j in range(2)]}")


if __name__ == "__main__":
    main()
