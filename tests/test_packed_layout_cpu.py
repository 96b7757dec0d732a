"""The flat-buffer layout without a device: pixelrec_amd.model.packed.flat_layout, fed each family's `_flat_specs()` and
alignment, must reproduce the `_views` that tests/golden/packed_model_bits.json recorded on the build before the packing was
shared; and the members the surrounding code probes for by attribute must be present exactly where they were."""
import json

import pytest
import torch

from tests import test_gpu_packed_bits as P

LAZY_TABLE = {"mf/plain", "mf/towers", "vbpr", "acf", "din", "widedeep", "dssm/plain", "dssm/mlp", "fm"}
ALIGNED = {"acf", "din", "curatornet", "widedeep", "dssm/plain", "dssm/mlp", "fm"}


@pytest.fixture(scope="module")
def golden():
    with open(P.GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.fixture
def on_cpu(monkeypatch):
    """The GPU tests' model helpers end in .cuda(): here the model stays where it was built"""
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, device=None: self)


@pytest.mark.parametrize("name", sorted(P.MODELS))
def test_layout_and_probed_members(name, golden, on_cpu, tmp_path):
    from pixelrec_amd.lib import PxrError
    from pixelrec_amd.model.packed import flat_layout

    m = P.MODELS[name](tmp_path, "cpu") if name == "sasrec" else P.MODELS[name](tmp_path)
    assert m.flat_align == (4 if name in ALIGNED else 1)
    views, total = flat_layout([(k, tuple(p.shape)) for k, p in m._flat_specs()], m.flat_align)
    want = golden[name]["views"]
    assert {k: [off, n, list(shape)] for k, (off, n, shape) in views.items()} == want
    assert total == max((off + -(-n // m.flat_align) * m.flat_align for off, n, _ in want.values()), default=0)
    assert all(off % m.flat_align == 0 for off, _, _ in views.values())
    # what optim.py and graph.py probe for
    assert hasattr(m, "table_parameter_spans") == hasattr(m, "lazy_table") == (name in LAZY_TABLE)
    assert hasattr(m, "running_state_buffers") == name.startswith("mf/")
    assert hasattr(m, "split_flat_table_groups") == (name == "vbpr")
    assert hasattr(m, "item_table_attr") == (name == "srgnn")
    assert hasattr(m, "rec_parameter_names") == (name not in ("sasrec", "bert4rec"))
    assert hasattr(m, "sparse_table_grad") == hasattr(m, "register_table_hooks") == (name not in ("curatornet", "lightgcn"))
    # the bases register nothing: the reference's keys, in its order
    assert list(m.state_dict().keys()) == golden[name]["keys"]
    assert [k for k, _ in m.named_parameters()] == [k for k in golden[name]["keys"] if k in dict(m.named_parameters())]
    with pytest.raises(PxrError, match="no CPU fallback"):
        m.flat_parameters()
    assert list(m.state_dict().keys()) == golden[name]["keys"] and m._flat is None


def test_layout_function():
    from pixelrec_amd.model.packed import flat_layout

    specs = [("a", (3, 2)), ("b", (1,)), ("c", ()), ("d", (5,))]
    assert flat_layout(specs) == ({"a": (0, 6, (3, 2)), "b": (6, 1, (1,)), "c": (7, 1, ()), "d": (8, 5, (5,))}, 13)
    assert flat_layout(specs, 4) == ({"a": (0, 6, (3, 2)), "b": (8, 1, (1,)), "c": (12, 1, ()), "d": (16, 5, (5,))}, 24)
    assert flat_layout([]) == ({}, 0)
