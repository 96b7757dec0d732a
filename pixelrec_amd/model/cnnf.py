"""CNN-F -- the image encoder of DVBPR (reference code/REC/model/PixelNet/dvbpr.py:92-143), trained from pixels on the im2col
convolution kernels of csrc/conv2d.hip and the library GEMMs.  Five Conv2d + ReLU, three of them under MaxPool2d(2), then three
Linears, EACH -- the last included -- followed by ReLU and Dropout(dropout):

    layer                kernel, stride      output     after pool
    conv1   3 ->  64     11x11, (1, 4)       214 x 54   107 x 27
    conv2  64 -> 256      5x5                103 x 23    51 x 11      (floor mode drops the last row and the last column)
    conv3 256 -> 256      3x3                 49 x  9    --
    conv4 256 -> 256      3x3                 47 x  7    --
    conv5 256 -> 256      3x3                 45 x  5    22 x  2
    flatten (c, h, w) = 11264 -> fc 512 -> fc 512 -> fc hidden_dim

There is no padding (`padding_mode='replicate'` with padding 0 is inert) and the first stride is 1 in H, 4 in W (dvbpr.py:101).
`cnnf_geometry()` computes the table from the shapes.

A convolution is ops.conv2d_relu_fwd / ops.conv2d_bwd: chunks of whole images through im2col + GEMM (+ col2im), the chunk size from
ONE byte budget for the column workspace (`conv_workspace_mb`, default 1024; one image's columns are 16.8 MB at conv1 and 15.2 MB at
conv2).  Activations are NHWC, so a conv GEMM's [n Ho Wo, Cout] output is the next layer's input as it stands; the image itself is
read NCHW through its strides; the LAST pool writes (c, h, w) order, which is what `fcs.0.weight` multiplies in the reference, so
every parameter keeps the reference's shape and a reference checkpoint loads with strict=True.  The backward recomputes the columns
from the saved input of each layer instead of keeping them.  conv1 has no data gradient (its input is the image): none is computed.

K = 363: conv1's K = 3 * 11 * 11 is no multiple of 4, and the GEMMs need leading dimensions that are.  The parameter stays [64, 3, 11,
11]; every forward copies it into a padded [64, 364] operand (93 KB, last column zero), the weight gradient is computed in that padded
shape and its first 363 columns are copied back into the parameter's gradient.

Dropout: ops.dropout, the library's counter hash.  Mask k (k = 0, 1, 2 for fcs.k) has stream id k and seed `seed` + the number of
backward passes so far; its element index is the row-major index i * width_k + j into the [n, width_k] output of fcs.k, where n is
the number of images of THIS call and i the image's row in it (for DVBPR: the batch's distinct images, ascending id).
oracle/dropout_rng.keep_mask(seed + step, k, (n, width_k), p) restates it.

Parameters live in one flat buffer with a gradient twin that every backward overwrites (`_native`: `ensure_packed()`, `flat`,
`gflat`, `segments`, `views` -- what optim.VisualAdamW reads of vit_native.NativeTower).  `convs` / `fcs` are nn.Conv2d / nn.Linear
modules used as parameter containers (names, shapes and default bias init of the reference); they are never called.  HIP device only.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..lib import PxrError

IMAGE = (3, 224, 224)
# (Cin, Cout, kh, kw, sh, sw, pooled): dvbpr.py:101-105,118
CNNF_CONVS = ((3, 64, 11, 11, 1, 4, True), (64, 256, 5, 5, 1, 1, True), (256, 256, 3, 3, 1, 1, False),
              (256, 256, 3, 3, 1, 1, False), (256, 256, 3, 3, 1, 1, True))


def cnnf_geometry(H: int = IMAGE[1], W: int = IMAGE[2]):
    """-> [dict(cin, cout, kh, kw, sh, sw, pool, h, w, ho, wo, hp, wp)] per conv layer: input size, conv output, and the size handed to
    the next layer (the pooled one where the layer is pooled)."""
    out = []
    for cin, cout, kh, kw, sh, sw, pool in CNNF_CONVS:
        ho, wo = ops.conv2d_out_hw(H, W, kh, kw, sh, sw)
        hp, wp = (ho // 2, wo // 2) if pool else (ho, wo)
        out.append(dict(cin=cin, cout=cout, kh=kh, kw=kw, sh=sh, sw=sw, pool=pool, h=H, w=W, ho=ho, wo=wo, hp=hp, wp=wp))
        H, W = hp, wp
    return out


def cnnf_flat_features(H: int = IMAGE[1], W: int = IMAGE[2]) -> int:
    g = cnnf_geometry(H, W)[-1]
    return g["cout"] * g["hp"] * g["wp"]


class _CnnfTower:
    """Flat packing + native forward / backward of a CNNF (`enc`)."""

    def __init__(self, enc):
        self.enc = enc
        self.flat = self.gflat = None
        self.views = {}          # name (relative to enc) -> (offset, numel, shape)
        self.segments = []       # [(lo, hi)] flat ranges that receive gradients and optimizer updates
        self.geom = cnnf_geometry()
        self.step_count = 0      # completed backward passes: host mirror ...
        self._step_dev = None    # ... and device counter (the dropout seed offset)
        self._w0p = self._g0p = None

    def ensure_packed(self):
        first = self.enc.convs[0].weight
        if self.flat is not None and self.flat.device == first.device and first.data_ptr() == self.flat.data_ptr():
            return
        dev = first.device
        if dev.type != "cuda":
            raise PxrError("the native image encoder runs on a HIP device only (no CPU fallback)")
        specs = list(self.enc.named_parameters())
        pad4 = lambda n: (n + 3) & ~3                       # every tensor starts 16-byte aligned
        total = sum(pad4(p.numel()) for _, p in specs)
        flat = torch.zeros(total, dtype=torch.float32, device=dev)
        gflat = torch.zeros(total, dtype=torch.float32, device=dev)
        off, views, segs = 0, {}, []
        for name, p in specs:
            n = p.numel()
            flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = flat[off:off + n].view(p.shape)
            views[name] = (off, n, tuple(p.shape))
            if p.requires_grad:
                p.grad = gflat[off:off + n].view(p.shape)
                if segs and segs[-1][1] == off:
                    segs[-1] = (segs[-1][0], off + pad4(n))
                else:
                    segs.append((off, off + pad4(n)))
            off += pad4(n)
        self.flat, self.gflat, self.views, self.segments = flat, gflat, views, segs
        c0 = CNNF_CONVS[0]
        ldk = ops.conv2d_ldk(c0[0], c0[2], c0[3])
        self._w0p = torch.zeros(c0[1], ldk, dtype=torch.float32, device=dev)      # the pad column stays zero
        self._g0p = torch.empty(c0[1], ldk, dtype=torch.float32, device=dev)
        self._step_dev = torch.full((1,), self.step_count, dtype=torch.int64, device=dev)

    def view(self, name, grad=False):
        off, n, shape = self.views[name]
        return (self.gflat if grad else self.flat)[off:off + n].view(shape)

    def _conv_weight(self, l):
        """The GEMM's B operand of conv layer l: weight.view(Cout, K), through the padded copy where K % 4 != 0."""
        cin, cout, kh, kw = CNNF_CONVS[l][:4]
        K = cin * kh * kw
        w = self.view(f"convs.{l}.weight").view(cout, K)
        if K % 4 == 0:
            return w
        self._w0p[:, :K].copy_(w)            # refreshed every forward: the optimizer has moved the parameter
        return self._w0p

    # ------------------------------------------------------------------------------------------ forward
    def forward(self, images, need_grad: bool, train: bool):
        """images float32 [n, 3, 224, 224] on the HIP device -> (E [n, hidden_dim], what the backward needs | None)."""
        e = self.enc
        ws = e.conv_workspace_bytes
        x = images
        convs = []
        for l, (cin, cout, kh, kw, sh, sw, pool) in enumerate(CNNF_CONVS):
            wp = self._conv_weight(l)
            y, der = ops.conv2d_relu_fwd(x, wp, self.view(f"convs.{l}.bias"), kh, kw, sh, sw, ws, save_der=need_grad and not pool)
            convs.append((x, y if pool else None, der, wp))
            x = ops.maxpool2x2_fwd(y, chw=(l == len(CNNF_CONVS) - 1)) if pool else y
        h = x.reshape(x.shape[0], -1)                       # (c, h, w) order: the last pool wrote NCHW
        p = e.dropout_prob if train else 0.0
        fcs = []
        for k in range(len(e.fcs)):
            a, d = ops.linear_fwd(h, self.view(f"fcs.{k}.weight"), self.view(f"fcs.{k}.bias"), act="relu")
            fcs.append((h, d))
            h = ops.dropout(a, p, e.drop_seed, k, step_dev=self._step_dev) if p > 0 else a
        return h, (dict(convs=convs, fcs=fcs, p=p) if need_grad else None)

    # ------------------------------------------------------------------------------------------ backward
    def backward(self, dE, saved):
        """dE [n, hidden_dim] -> every parameter's gradient into the flat gradient buffer (overwritten)."""
        e = self.enc
        ws = e.conv_workspace_bytes
        p = saved["p"]
        G = lambda name: self.view(name, grad=True)
        g = dE.contiguous()
        problems = []
        for k in range(len(e.fcs) - 1, -1, -1):
            h_in, d = saved["fcs"][k]
            if p > 0:
                g = ops.dropout(g, p, e.drop_seed, k, step_dev=self._step_dev)      # the mask's backward is itself
            if k == len(e.fcs) - 1:
                dz = ops.mul(g, d)
            else:
                dz = g                                                                # (the ReLU mask was applied by the GEMM below)
            problems.append((dz, h_in, G(f"fcs.{k}.weight"), G(f"fcs.{k}.bias")))
            # the input gradient, times the ReLU derivative of the layer below (it commutes with that layer's dropout mask: both
            # are elementwise factors, the derivative 0 or 1)
            g = ops.linear_bwd_input(dz, self.view(f"fcs.{k}.weight"), mul=saved["fcs"][k - 1][1] if k > 0 else None)
        ops.grouped_linear_bwd_weight(problems)
        last = self.geom[-1]
        g = g.view(g.shape[0], last["cout"], last["hp"], last["wp"])                 # d pool5, (c, h, w) order
        for l in range(len(CNNF_CONVS) - 1, -1, -1):
            cin, cout, kh, kw, sh, sw, pool = CNNF_CONVS[l]
            x, y, der, wp = saved["convs"][l]
            if pool:
                dz = ops.maxpool2x2_relu_bwd(y, g)
            else:
                dz = ops.mul(g.permute(0, 2, 3, 1), der.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
            padded = wp is self._w0p
            gw = self._g0p if padded else G(f"convs.{l}.weight").view(cout, -1)
            g = ops.conv2d_bwd(dz, x, wp, kh, kw, sh, sw, gw, G(f"convs.{l}.bias"), ws, need_dx=l > 0)
            if padded:
                K = cin * kh * kw
                G(f"convs.{l}.weight").view(cout, K).copy_(gw[:, :K])                # compact the padded weight gradient back
        ops.counter_add(self._step_dev, 1)
        self.step_count += 1


class _CnnfFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images, anchor, tower, train):
        out, saved = tower.forward(images, need_grad=True, train=train)
        ctx.tower, ctx.saved = tower, saved
        return out

    @staticmethod
    def backward(ctx, d_out):
        if ctx.saved is None:
            raise PxrError("CNNF: backward() ran twice over one forward()")
        ctx.tower.backward(d_out, ctx.saved)
        ctx.saved = None
        return None, None, None, None


class CNNF(nn.Module):
    """dvbpr.py:92-143 CNNF(hidden_dim, fc_dim, weights=None, dropout): the shipped geometry only."""

    def __init__(self, hidden_dim=2048, fc_dim=512, dropout=0.5, conv_workspace_mb=1024, seed=2020):
        super().__init__()
        if hidden_dim <= 0 or hidden_dim % 4 or fc_dim <= 0 or fc_dim % 4:
            raise ValueError(f"CNNF: hidden_dim and fc_dim must be positive multiples of 4 (16-byte vector accesses); got "
                             f"{hidden_dim} and {fc_dim}")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"CNNF: dropout must lie in [0, 1), got {dropout}")
        if float(conv_workspace_mb) <= 0:
            raise ValueError(f"CNNF: conv_workspace_mb must be positive, got {conv_workspace_mb}")
        self.hidden_dim, self.fc_dim = int(hidden_dim), int(fc_dim)
        self.dropout_prob = float(dropout)
        self.drop_seed = int(seed)
        self.conv_workspace_bytes = int(float(conv_workspace_mb) * (1 << 20))
        self.convs = nn.ModuleList([nn.Conv2d(cin, cout, (kh, kw), stride=(sh, sw)) for cin, cout, kh, kw, sh, sw, _ in CNNF_CONVS])
        self.fcs = nn.ModuleList([nn.Linear(i, o) for i, o in ((cnnf_flat_features(), fc_dim), (fc_dim, fc_dim), (fc_dim, hidden_dim))])
        self.reset_parameters()
        self._native = _CnnfTower(self)
        self._anchor = None

    def reset_parameters(self):
        """dvbpr.py:139-143: xavier-uniform weights; the biases keep torch's defaults."""
        for m in list(self.convs) + list(self.fcs):
            nn.init.xavier_uniform_(m.weight)

    def encode(self, x, train: bool):
        """x [*, 3, 224, 224] float32 on the HIP device -> [n, hidden_dim]; train: dropout on.  Under autograd (and with a trainable
        parameter) the result carries the native backward."""
        if not isinstance(x, torch.Tensor) or x.dim() < 3 or tuple(x.shape[-3:]) != IMAGE or not x.is_floating_point():
            raise ValueError(f"CNNF: images must be float [*, 3, 224, 224] (dvbpr.py:123), got "
                             f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
        if x.device.type != "cuda":
            raise PxrError("the native image encoder runs on a HIP device only (no CPU fallback)")
        tower = self._native
        tower.ensure_packed()
        x = x.reshape(-1, *IMAGE).to(torch.float32).contiguous()
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if self._anchor is None or self._anchor.device != x.device:
                self._anchor = torch.zeros((), dtype=torch.float32, device=x.device, requires_grad=True)
            return _CnnfFn.apply(x, self._anchor, tower, bool(train))
        out, _ = tower.forward(x, need_grad=False, train=bool(train))
        return out

    def forward(self, x):
        return self.encode(x, self.training)
