"""packed.EncoderRows without a GPU: the mixin between the visual encoder's output and the native step, on a stub model in pure
torch.  The stub calls `_encoded_step` directly -- `_check_rows` refuses the CPU by design."""
import pytest
import torch
import torch.nn as nn

from pixelrec_amd.lib import PxrError
from pixelrec_amd.model import packed

M, D = 5, 4


class _Stub(packed.EncoderRows, nn.Module):
    """loss = sum(table * w); `_backward_train` returns gsd * known, which is NOT that loss's gradient: what arrives on E is what
    the model returned, not something autograd derived."""

    def __init__(self):
        super().__init__()
        self.visual_encoder = nn.Linear(3, D)
        self._saved = None
        self.known = torch.arange(M * D, dtype=torch.float32).view(M, D) - 7.0
        self.seen, self.backwards = [], 0

    def loss(self, E, w):
        return self._encoded_step(E, E.detach().contiguous(), w)

    def _forward_train(self, w):
        self.seen.append(self._train_table)
        self._saved = dict(w=w)
        return (self._train_table * w).sum().view(1)

    def _backward_train(self, gsd):
        saved, table = self._take_table()
        assert set(saved) == {"w"} and table is self.seen[-1]
        self._saved = None
        self.backwards += 1
        return gsd * self.known


def _E():
    return torch.randn(2 * M, D, generator=torch.Generator().manual_seed(3))[::2]       # not contiguous


def test_gradient_of_e_is_what_backward_train_returned():
    m, E, w = _Stub(), _E().requires_grad_(True), torch.full((M, D), 0.5)
    loss = m.loss(E, w)
    assert loss.dim() == 0 and loss.requires_grad and float(loss) == float((E.detach() * w).sum())
    (3 * loss).backward()
    assert m.backwards == 1 and torch.equal(E.grad, 3 * m.known)
    assert m._train_table is None and m._saved is None


def test_plain_tensor_still_drives_the_backward_once():
    m, E, w = _Stub(), _E(), torch.ones(M, D)
    loss = m.loss(E, w)
    assert loss.requires_grad and not E.requires_grad
    loss.backward()
    assert m.backwards == 1 and E.grad is None and m._train_table is None
    assert m._anchor.device == E.device and m._anchor.requires_grad and float(m._anchor) == 0
    anchor = m._anchor
    m.loss(E, w).backward()
    assert m._anchor is anchor and m.backwards == 2                 # made once, lazily, on E's device


@pytest.mark.parametrize("grad", [True, False])
def test_table_is_e_detached_contiguous_and_no_alias_of_the_anchored_tensor(grad):
    m, E = _Stub(), _E().requires_grad_(grad)
    E.data[0, 0] = -0.0                                              # (E + anchor * 0 would turn this into +0.0)
    m.loss(E, torch.ones(M, D))
    table = m._train_table
    assert table is m.seen[0] and not table.requires_grad and table.grad_fn is None and table.is_contiguous()
    assert torch.equal(table.view(torch.int32), E.detach().contiguous().view(torch.int32))
    assert table.data_ptr() != E.data_ptr() and not E.is_contiguous()


def test_second_take_table_raises():
    m, E = _Stub(), _E().requires_grad_(True)
    with pytest.raises(PxrError, match=r"backward\(\) without"):
        m._take_table()                                             # a fresh model
    m.loss(E, torch.ones(M, D)).backward()
    with pytest.raises(PxrError, match=r"backward\(\) without"):
        m._take_table()
    m._saved = dict(w=None)                                         # something in _saved, no table: still refused
    with pytest.raises(PxrError, match=r"backward\(\) without"):
        m._take_table()
    m.loss(E, torch.ones(M, D))
    with pytest.raises(PxrError, match=r"backward\(\) without"):
        m._take_table(None)                                         # what else the forward must have left
    assert m._train_table is not None                               # a refused take leaves the table where it is


def test_check_rows():
    m = _Stub()
    for bad in (torch.zeros(M), torch.zeros(1, M, D), torch.zeros(M, D, dtype=torch.float64), torch.zeros(M, D + 1)):
        with pytest.raises(ValueError, match=r"_Stub: E must be float32 \[M, 4\], got"):
            m._check_rows(bad, D)
    with pytest.raises(PxrError, match="HIP device only"):
        m._check_rows(torch.zeros(M, D), D)


def test_mixin_registers_nothing_and_defines_no_probed_member():
    m = _Stub()
    enc = {"visual_encoder.weight", "visual_encoder.bias"}
    assert set(m.state_dict()) == enc and {n for n, _ in m.named_parameters()} == enc and not list(m.named_buffers())
    m.loss(_E(), torch.ones(M, D)).backward()                        # the lazy anchor is no parameter either
    assert set(m.state_dict()) == enc and {n for n, _ in m.named_parameters()} == enc and not list(m.named_buffers())
    for probed in ("modal_inputs", "set_item_feature", "scoring_item_matrix", "extra_item_images"):
        assert not hasattr(m, probed) and not hasattr(packed.EncoderRows, probed)
    x = torch.ones(2, 3, requires_grad=True)
    out = m.compute_item(x)
    assert not out.requires_grad and torch.equal(out, m.visual_encoder(x).detach())


def test_store_modal_inputs_fetches_each_listed_image_once():
    class Store:
        def batch(self, ids):
            return ids.float() * 2

    index, ids = torch.tensor([[0, 1, 2]]), torch.tensor([0, 7, 9])
    got = packed.store_modal_inputs(Store(), (index, ids))
    assert got[0] is index and got[1].tolist() == [0.0, 14.0, 18.0]
