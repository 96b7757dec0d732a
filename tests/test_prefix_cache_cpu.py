"""The prefix cache's host side (model/prefix_cache.py; no GPU): budget arithmetic, where the tower is cut, the id form's refusal
of a CPU tensor, the Trainer's default, and the new entry's binding."""
import os
import re

import pytest
import torch

from tests.mo_common import ROOT, tower_config


def _encoder(tune):
    from pixelrec_amd.model import visual

    return visual.load_model(tower_config(tune, embedding_size=32))


def test_bytes_per_item_of_the_shipped_shapes():
    from pixelrec_amd.model.prefix_cache import bytes_per_item
    from pixelrec_amd.model.visual import ENCODER_SHAPES

    want = {"clip-vit-base-patch32": (50, 768, 153_600), "clip-vit-base-patch16": (197, 768, 605_184),
            "clip-vit-large-patch14": (257, 1024, 1_052_672)}
    for name, (T, H, nbytes) in want.items():
        hidden, _, _, _, image, patch = ENCODER_SHAPES[name]
        assert ((image // patch) ** 2 + 1, hidden) == (T, H)
        assert bytes_per_item(T, H) == nbytes
    # Pixel200K (96 001 items): 14.7 / 58.1 / 101 GB
    assert [round(96_001 * want[n][2] / 1e9, 1) for n in want] == [14.7, 58.1, 101.1]


@pytest.mark.parametrize("tune,k", [(5, 0), (21, 1), (37, 2), (53, 3)])
def test_first_trainable_block_of_the_tiny_tower(tune, k):
    enc = _encoder(tune)
    assert enc._native.first_trainable_block() == k
    assert enc.prefix_cache is None                          # off by default


def test_ids_on_the_cpu_are_refused():
    from pixelrec_amd.lib import PxrError

    enc = _encoder(37)
    with pytest.raises(PxrError, match="HIP"):
        enc(torch.tensor([1, 2, 3]))
    with pytest.raises(PxrError):
        enc.build_prefix_cache(_CpuStore())                  # the cache lives beside a store on the device


class _CpuStore:
    n = 4
    images = torch.zeros(4, 64, 64, 3, dtype=torch.uint8)


def test_trainer_without_the_key_stays_on_images():
    from pixelrec_amd.trainer import Trainer

    class Module:
        visual_encoder = None

    class Wrap:
        module = Module()

    for config in ({}, {"prefix_cache": False}, {"prefix_cache": None}, {"prefix_cache_gb": 4}):
        t = Trainer.__new__(Trainer)
        t.config, t.model, t.use_modality = config, Wrap(), True
        assert t._prefix_cache() is None                     # (asks for neither the store nor the encoder)
    t = Trainer.__new__(Trainer)
    t.config, t.model, t.use_modality = {"prefix_cache": True}, Wrap(), False
    assert t._prefix_cache() is None                         # an id model


def test_binding_declares_the_entry_with_the_headers_arguments():
    from pixelrec_amd import lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pxr.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+pxr_ln_gather_fwd_f32\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    assert m is not None
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    res, argtypes = lib._SIGNATURES["pxr_ln_gather_fwd_f32"]
    assert len(args) == len(argtypes) == 18
    assert [i for i, a in enumerate(args) if re.search(r"\bint64_t\b", a) and "*" not in a] == [1, 14, 15]    # n_items, the planes' strides
    assert hasattr(lib.load(), "pxr_ln_gather_fwd_f32")
