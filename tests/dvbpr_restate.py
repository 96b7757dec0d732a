"""A helper, not a test: DVBPR restated from its formulas in plain torch (float32 or float64, whatever the parameters are), the
frozen weight recipe its fixture is built from, and the index maps of csrc/conv2d.hip in numpy with the kernels' own arithmetic.

    CNN-F: five Conv2d + ReLU (no padding; first stride 1 in H, 4 in W), MaxPool2d(2) behind layers 1, 2 and 5, flatten in
           (c, h, w) order, three Linears EACH followed by ReLU and dropout
    x_b  = <gamma_u[user_b], gamma_i[item_b,0] - gamma_i[item_b,1]> + <theta_u[user_b], E[p_b] - E[n_b]>
    loss = -mean_b log sigmoid(x_b)
    predict = gamma_u gamma_i^T + theta_u item_feature^T
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

# (Cin, Cout, k, (stride h, stride w), pooled)
CONVS = ((3, 64, 11, (1, 4), True), (64, 256, 5, (1, 1), True), (256, 256, 3, (1, 1), False), (256, 256, 3, (1, 1), False),
         (256, 256, 3, (1, 1), True))
FLAT, FC = 256 * 22 * 2, 512
ENC = "visual_encoder."
SAMPLE = 1024            # elements of the strided sample the fixture keeps of a large weight gradient


def state_shapes(Dh, U, I):
    """{state_dict key: shape} in the reference's registration order."""
    out = OrderedDict()
    for l, (cin, cout, k, _, _) in enumerate(CONVS):
        out[f"{ENC}convs.{l}.weight"] = (cout, cin, k, k)
        out[f"{ENC}convs.{l}.bias"] = (cout,)
    for l, (i, o) in enumerate(((FLAT, FC), (FC, FC), (FC, Dh))):
        out[f"{ENC}fcs.{l}.weight"] = (o, i)
        out[f"{ENC}fcs.{l}.bias"] = (o,)
    out["theta_users.weight"] = (U, Dh)
    out["gamma_users.weight"] = (U, Dh)
    out["gamma_items.weight"] = (I, Dh)
    return out


def make_state(seed, Dh, U, I):
    """The fixture's weights, rebuilt instead of stored (fcs.0.weight alone is 23 MB): one np.random.RandomState(seed) stream -- frozen
    across NumPy versions -- read in state_dict order, random_sample() in [0, 1) per element; a weight w = (2 r - 1) * sqrt(6 / (fan_in
    + fan_out)) (xavier-uniform bounds), a bias b = (2 r - 1) / sqrt(fan_in), a table row = r (uniform(0, 1)); rounded to float32.
    -> OrderedDict of float32 tensors."""
    rs = np.random.RandomState(seed)
    out = OrderedDict()
    fan = None
    for name, shape in state_shapes(Dh, U, I).items():
        r = rs.random_sample(shape)
        if not name.startswith(ENC):
            v = r
        elif name.endswith("weight"):
            rec = int(np.prod(shape[2:])) if len(shape) > 2 else 1
            fan = shape[1] * rec
            v = (2.0 * r - 1.0) * np.sqrt(6.0 / (fan + shape[0] * rec))
        else:
            v = (2.0 * r - 1.0) / np.sqrt(fan)
        out[name] = torch.from_numpy(v.astype(np.float32))
    return out


def state_sums(state):
    """[(float64 sum, float64 sum of squares)] per tensor, in order: what the fixture holds to pin the recipe."""
    return np.array([[float(v.double().sum()), float((v.double() ** 2).sum())] for v in state.values()])


def expand_images(u8):
    """uint8 [n, 28, 28, 3] -> float32 [n, 3, 224, 224]: every pixel repeated 8 x 8, then (x / 255 - 0.5) / 0.5 in float64, rounded once."""
    x = torch.from_numpy(np.asarray(u8)).double().permute(0, 3, 1, 2)
    x = x.repeat_interleave(8, dim=2).repeat_interleave(8, dim=3)
    return ((x / 255.0 - 0.5) / 0.5).float()


def cnnf(P, images, masks=None, p=0.0, padding_mode="replicate", taps=None):
    """images [n, 3, 224, 224] -> E [n, Dh] with the parameters P (their dtype).  masks: three boolean keep masks [n, width_k], applied
    as h * mask / (1 - p) behind fcs.k (None: no dropout).  padding_mode: the reference's nn.Conv2d option; with padding 0 it pads by
    nothing.  taps: a list that receives every layer's output."""
    x = images.reshape(-1, 3, 224, 224).to(P[ENC + "convs.0.weight"].dtype)
    for l, (_, _, _, stride, pool) in enumerate(CONVS):
        if padding_mode != "zeros":
            x = F.pad(x, (0, 0, 0, 0), mode=padding_mode)
        x = F.relu(F.conv2d(x, P[f"{ENC}convs.{l}.weight"], P[f"{ENC}convs.{l}.bias"], stride=stride))
        if pool:
            x = F.max_pool2d(x, 2)
        if taps is not None:
            taps.append(x)
    x = x.reshape(-1, FLAT)
    for l in range(3):
        x = F.relu(F.linear(x, P[f"{ENC}fcs.{l}.weight"], P[f"{ENC}fcs.{l}.bias"]))
        if masks is not None and p > 0:
            x = x * masks[l].to(x.dtype) / (1.0 - p)
    return x


def loss_of(P, E, user, item_id, index):
    """The head: E [M, Dh], user [B], item_id [B, 2], index [B, 2] (positions into E) -> loss."""
    user, item_id, index = (torch.as_tensor(np.asarray(t), dtype=torch.int64) for t in (user, item_id, index))
    gu, tu = P["gamma_users.weight"][user], P["theta_users.weight"][user]
    gi = P["gamma_items.weight"][item_id]                                     # [B, 2, Dh]
    e = E[index]
    s = (gu[:, None, :] * gi).sum(-1) + (tu[:, None, :] * e).sum(-1)          # [B, 2]
    return -torch.mean(F.logsigmoid(s[:, 0] - s[:, 1]))


def predict(P, users, feat):
    users = torch.as_tensor(np.asarray(users), dtype=torch.int64)
    return P["gamma_users.weight"][users] @ P["gamma_items.weight"].t() + P["theta_users.weight"][users] @ feat.t()


def dedup(item_id):
    """item_id [B, 2] -> (image_ids [M] ascending, index [B, 2] with item_id = image_ids[index]): MoPairTrainBatcher's form."""
    ids, inv = np.unique(np.asarray(item_id).reshape(-1), return_inverse=True)
    return ids.astype(np.int64), inv.reshape(-1, 2).astype(np.int64)


def sample_index(numel):
    """The fixed strided sample of a large tensor: SAMPLE flat indices, evenly spread, ascending."""
    return (np.arange(SAMPLE, dtype=np.int64) * numel) // SAMPLE


# ---------------------------------------------------------------------------------------------- index maps of csrc/conv2d.hip
def out_hw(H, W, kh, kw, sh, sw):
    return (H - kh) // sh + 1, (W - kw) // sw + 1


def im2col_map(x, kh, kw, sh, sw):
    """x [n, C, H, W] (numpy) -> col [n Ho Wo, ldk]: thread t owns col.flat[4t .. 4t + 3]; row = t / (ldk / 4) = (img, ho, wo), k = (c, i,
    j); k >= K gets +0.0 -- the kernel's arithmetic, one vector lane at a time."""
    n, C, H, W = x.shape
    Ho, Wo = out_hw(H, W, kh, kw, sh, sw)
    K = C * kh * kw
    ldk = (K + 3) // 4 * 4
    t = np.arange(n * Ho * Wo * (ldk // 4), dtype=np.int64)
    row, k0 = t // (ldk // 4), (t % (ldk // 4)) * 4
    img, r = row // (Ho * Wo), row % (Ho * Wo)
    ho, wo = r // Wo, r % Wo
    col = np.zeros((n * Ho * Wo, ldk), dtype=x.dtype)
    for q in range(4):
        k = k0 + q
        ok = k < K
        c, ij = k // (kh * kw), k % (kh * kw)
        i, j = ij // kw, ij % kw
        v = np.zeros(t.shape, dtype=x.dtype)
        v[ok] = x[img[ok], c[ok], ho[ok] * sh + i[ok], wo[ok] * sw + j[ok]]
        col[row, k] = v
    return col


def col2im_map(dcol, n, C, H, W, kh, kw, sh, sw):
    """dcol [n Ho Wo, ldk] -> dx [n, C, H, W]: one thread per element, the windows that read it summed kh outer, kw inner in dcol's
    dtype; +0.0 where none does."""
    Ho, Wo = out_hw(H, W, kh, kw, sh, sw)
    img, c, h, w = np.meshgrid(np.arange(n), np.arange(C), np.arange(H), np.arange(W), indexing="ij")
    s = np.zeros((n, C, H, W), dtype=dcol.dtype)
    for i in range(kh):
        hh = h - i
        for j in range(kw):
            ww = w - j
            ok = (hh >= 0) & (hh % sh == 0) & (hh // sh < Ho) & (ww >= 0) & (ww % sw == 0) & (ww // sw < Wo)
            rows = (img[ok] * Ho + hh[ok] // sh) * Wo + ww[ok] // sw
            s[ok] = s[ok] + dcol[rows, c[ok] * kh * kw + i * kw + j]
    return s


def covered(H, W, kh, kw, sh, sw):
    """bool [H, W]: the input elements some window reads."""
    Ho, Wo = out_hw(H, W, kh, kw, sh, sw)
    m = np.zeros((H, W), dtype=bool)
    for ho in range(Ho):
        for wo in range(Wo):
            m[ho * sh:ho * sh + kh, wo * sw:wo * sw + kw] = True
    return m


def _argmax4(a, b, c, d):
    """Winner of a 2 x 2 window in row-major order, the first of equal values: a later one replaces the maximum only when greater."""
    m, k = a.copy(), np.zeros(a.shape, dtype=np.int64)
    for idx, v in ((1, b), (2, c), (3, d)):
        g = v > m
        m[g], k[g] = v[g], idx
    return m, k


def pool_fwd_map(y):
    n, C, H, W = y.shape
    Hp, Wp = H // 2, W // 2
    v = y[:, :, :2 * Hp, :2 * Wp]
    return _argmax4(v[:, :, 0::2, 0::2], v[:, :, 0::2, 1::2], v[:, :, 1::2, 0::2], v[:, :, 1::2, 1::2])[0]


def pool_bwd_map(y, dp):
    """y [n, C, H, W] (ReLU'd), dp [n, C, H // 2, W // 2] -> dy: dp of the window where the element is its first maximum and y > 0,
    else +0.0; dropped rows / columns +0.0."""
    n, C, H, W = y.shape
    Hp, Wp = H // 2, W // 2
    v = y[:, :, :2 * Hp, :2 * Wp]
    m, k = _argmax4(v[:, :, 0::2, 0::2], v[:, :, 0::2, 1::2], v[:, :, 1::2, 0::2], v[:, :, 1::2, 1::2])
    dy = np.zeros_like(y)
    for idx, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        win = (k == idx) & (m > 0)
        dy[:, :, a:2 * Hp:2, b:2 * Wp:2] = np.where(win, dp, 0).astype(y.dtype)
    return dy
