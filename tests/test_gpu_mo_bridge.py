"""packed.EncoderRows on the GPU, under each model that reaches its native step through `loss_from_embeddings`: the head at the
smallest shape the model's own GPU file uses, once on a leaf E and once on the same E as a plain tensor."""
import numpy as np
import pytest
import torch

from pixelrec_amd import ops
from tests.mo_common import bits

pytestmark = pytest.mark.gpu


def _mobert4rec():
    import tests.test_gpu_mobert4rec as T

    m, index, masked, E = T._head_case()
    return m, E, (index, masked), index


def _modin():
    import tests.test_gpu_modin as T

    m, prof, tgt, E, index, _ = T._head_case(*T.HEAD_SHAPES[0])
    return m, E, (prof, tgt), index


def _mosrgnn():
    import tests.test_gpu_mosrgnn as T

    m, seq, tgt, E = T._case(*T.SHAPES[0])
    seq, tgt = torch.from_numpy(seq).cuda(), torch.from_numpy(tgt).cuda()
    return m, E, (seq, tgt), torch.cat((seq, tgt), 1)


def _mopool(name):
    import tests.test_gpu_mopool as T

    B, L, D, n_rows = 3, 4, 8, 9                                    # the first case of its test_head_without_the_tower_matches_float64
    m = T._tiny_model(name, D, L)
    prof, tgt = (t.cuda() for t in T._edge_index(B, L, n_rows, 7 * B + L))
    E = (torch.randn(n_rows, D, generator=torch.Generator().manual_seed(D + B)) * 0.5).cuda()
    return m, E, (prof, tgt), torch.cat((prof, tgt), 1)


CASES = {"MOBERT4Rec": _mobert4rec, "MODIN": _modin, "MOSRGNN": _mosrgnn, "MODSSM": lambda: _mopool("MODSSM"),
         "MOFM": lambda: _mopool("MOFM")}


@pytest.mark.parametrize("name", list(CASES))
def test_leaf_and_plain_e_run_the_same_step(name):
    """Two fresh identical models, one call each: E.requires_grad_(True), then the same E as a plain tensor (the anchored route).
    The same loss bits and the same flat gradient buffer; dE arrives on the leaf as [M, D] with +0.0 in row 0 and in every row
    nobody reads; nothing is left in `_train_table` or `_saved`."""
    results = []
    for leaf in (True, False):
        m, E, args, index = CASES[name]()
        assert type(m).__name__ == name and not E.requires_grad
        E = E.clone().requires_grad_(leaf)
        loss = m.loss_from_embeddings(E, *args)
        assert loss.dim() == 0 and loss.requires_grad and m._train_table is not None
        loss.backward()
        getattr(m, "join_weight_grads", lambda: None)()
        ops.raise_on_bad_indices()
        assert m._train_table is None and m._saved is None
        flat = m.flat_parameters()[1].clone() if hasattr(m, "flat_parameters") else None
        results.append((loss.detach().clone(), flat, E))
        if leaf:
            read = torch.zeros(E.shape[0], dtype=torch.bool, device="cuda")
            read[index.reshape(-1)] = True
            read[0] = False
            assert E.grad.shape == E.shape and not bool(read[-1]) and bool(read.any())
            assert int(bits(E.grad[~read]).abs().max()) == 0 and float(E.grad[read].abs().max()) > 0
        else:
            assert E.grad is None
    (l0, f0, E0), (l1, f1, E1) = results
    assert torch.equal(bits(E0.detach()), bits(E1)) and torch.equal(bits(l0), bits(l1))
    assert (f0 is None) == (name in ("MODSSM", "MOFM"))
    if f0 is not None:
        assert torch.equal(bits(f0), bits(f1)) and float(f0.abs().max()) > 0
    assert np.isfinite(float(l0))
