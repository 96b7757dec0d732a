"""The bits of every entry point that runs on the code shared by the sequence path: the masked BPR loss head (csrc/bpr_head.cuh:
the id pair of a row, the two table rows, the loss term, the coefficient, the cf (p - n) row) in its stand-alone
and its LayerNorm-fused form, the id clamp with its status flag (checked_id), the four-wide dropout (pxr_drop4) and the 256-thread
block sum, against tests/golden/seq_head_bits.json, which was recorded with `python tests/test_gpu_seq_head_bits.py --record FILE`
on the build of the commit BEFORE that code was shared (four copies of the head, five of the clamp, five of the dropout pattern,
two of the block sum).  Sharing changes no product, no order of a sum and no clamp, so per case every integer output must be equal
in full, and so must the two u32 sums of every float output's bit patterns (tests/golden_util.py: rec_bits).

Inputs (torch.Generator().manual_seed on the CPU, all finite), one set per (D, B, L, id layout):
  * D in 4, 260, 772, 1028, 2052: VEC = 1, 2, 4, 8, 16 float4s per lane of the LayerNorm kernels; every width above 4 leaves a
    ragged last lane group; 1028 and 2052 are the first widths of VEC 8 and 16, where the fused and the stand-alone forward differ;
  * (B, L) in (1, 1), (3, 13), (50, 5): 250 rows leave a ragged last workgroup of four waves;
  * both id layouts: SASRec's shifted [B, 2, L+1] windows and BERT4Rec's aligned [B, 3, L] planes;
  * dropout p in 0 and 0.1 with stream_id 3 and a device step counter of 5;
  * x, res at scale 0.5, gamma near 1, beta near 0; `out`, the stand-alone head's input, is LayerNorm(x + res) computed in fp64;
  * a table of 11 rows at scale 0.02.  Position 0 scores against row 1 = out[0] * 200 / |out[0]|^2 and position 1 (when there is
    one) against row 2 = -out[1] * 200 / |out[1]|^2, both with the small row 3 as the negative: pos - neg is +200 and -200 up to
    the negative's share (asserted below in fp64), so the naive sigmoid meets exp(-200) = 0 and exp(200) = inf, and every output
    stays finite (-log(1e-8) on the loss, a coefficient of 0).  The other ids are 0 and 3 .. 10;
  * the mask has zeros; with B > 1 the last sequence is masked out whole (the cf == 0 branch, which reads no table row);
  * the backward entries read scores, xhat and rstd computed on the CPU, and run with grad_scale 1 and no device scale, and with
    grad_scale 0.3 and a device scale of 0.7;
  * the WideDeep and DIN heads (their loss kernels hold the block sum): B = 1, 50 and 300, the last beyond one pass of 256 threads;
  * flagged ids, one case per id-checking entry at D 260, (3, 13): one id of -1 and one of n_table among the targets and among the
    negatives (input_ln_fwd, embed_gather: among the inputs); PXR_STATUS_BAD_INDEX must be set, the clamped outputs must match the
    golden (the backward entries, which clamp without flagging, included), and the case clears its bit.
ops.raise_on_bad_indices after every case shows that no status bit is left set, on the recording build as well.

Not covered: the RPW = 2 and STAGE instantiations of ln_fwd_kernel, which process-wide environment knobs select."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
from tests.golden_util import rec_bits as _rec  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "seq_head_bits.json")
N_TABLE = 11
WIDTHS = (4, 260, 772, 1028, 2052)
SHAPES = ((1, 1), (3, 13), (50, 5))
LAYOUTS = ("sasrec", "bert")
DROPS = (0.0, 0.1)
SCALES = {"g1": (1.0, None), "g0.3x0.7": (0.3, 0.7)}
EPS = 1e-12
SEED, STREAM, STEP = 1234567, 3, 5
BAD_INDEX = 1                                              # PXR_STATUS_BAD_INDEX


def _clean():
    from pixelrec_amd import ops

    ops.raise_on_bad_indices("cuda")


class Inputs:
    """the inputs of one (D, B, L, layout), on the CPU; .g(name) is the tensor on the GPU"""

    def __init__(self, D, B, L, layout):
        g = torch.Generator().manual_seed(100000 * D + 100 * B + L)       # the layouts share everything but the shape of `items`
        self.D, self.B, self.L = D, B, L
        self.x = torch.randn(B, L, D, generator=g) * 0.5
        self.res = torch.randn(B, L, D, generator=g) * 0.5
        self.gamma = 1.0 + torch.randn(D, generator=g) * 0.1
        self.beta = torch.randn(D, generator=g) * 0.1
        self.posemb = torch.randn(L, D, generator=g) * 0.02
        self.dy = torch.randn(B, L, D, generator=g) * 0.02
        table = torch.randn(N_TABLE, D, generator=g) * 0.02
        ids = torch.randint(2, N_TABLE, (3, B, L), generator=g)
        ids[ids == 2] = 0
        spare = torch.randint(3, N_TABLE, (B,), generator=g)
        mask = (torch.rand(B, L, generator=g) < 0.7).to(torch.int64)
        z = (self.x + self.res).double()
        mean = z.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((z - mean) ** 2).mean(-1, keepdim=True) + EPS)
        xhat = (z - mean) * rstd
        self.xhat, self.rstd = xhat.float(), rstd.float().reshape(B * L)
        self.out = (xhat * self.gamma.double() + self.beta.double()).float()
        inp, pos, neg = ids[0], ids[1], ids[2]
        o = self.out.view(B * L, D).double()
        pos.view(-1)[0], neg.view(-1)[0] = 1, 3
        table[1] = (o[0] * (200.0 / float((o[0] * o[0]).sum()))).float()
        mask.view(-1)[0] = 1
        if B * L > 1:
            pos.view(-1)[1], neg.view(-1)[1] = 2, 3
            table[2] = (-o[1] * (200.0 / float((o[1] * o[1]).sum()))).float()
            mask.view(-1)[1] = 1
            mask[0, L - 1] = 0
        if B > 1:
            mask[B - 1] = 0
        self.table, self.mask, self.pos_ids, self.neg_ids, self.in_ids = table, mask, pos, neg, inp
        self.set_layout(layout, spare)
        self.pos64 = (o * table[pos.view(-1)].double()).sum(-1)
        self.neg64 = (o * table[neg.view(-1)].double()).sum(-1)
        self.x64 = self.pos64 - self.neg64
        self.pos, self.neg = self.pos64.float().view(B, L), self.neg64.float().view(B, L)
        self._gpu = {}

    def set_layout(self, layout, spare=None):
        B, L = self.B, self.L
        if layout == "sasrec":                             # items[:, 0] = inputs then targets shifted by one, items[:, 1, 1:] = negatives
            items = torch.zeros(B, 2, L + 1, dtype=torch.int64)
            items[:, 0, 0] = self.in_ids[:, 0]
            items[:, 0, 1:] = self.pos_ids
            items[:, 1, 0] = spare if spare is not None else 3
            items[:, 1, 1:] = self.neg_ids
            self.layout, self.idx_bstride = None, 2 * (L + 1)
        else:                                              # inputs | targets | negatives
            items = torch.stack([self.in_ids, self.pos_ids, self.neg_ids], 1).contiguous()
            self.layout, self.idx_bstride = (3 * L, L, 2 * L), 3 * L
        self.items = items
        self._gpu = {}

    def g(self, name):
        if name not in self._gpu:
            self._gpu[name] = getattr(self, name).cuda()
        return self._gpu[name]


def _scale(key):
    gs, dev = SCALES[key]
    return gs, (None if dev is None else torch.tensor([dev], dtype=torch.float32).cuda())


def _step():
    return torch.tensor([STEP], dtype=torch.int64).cuda()


def _some(**tensors):
    return _rec(**{k: v for k, v in tensors.items() if v is not None})


def _head_cases(x, tag, out, scales=tuple(SCALES), drops=DROPS):
    """every entry that reads the target / negative ids of x.items, into out[f"{entry}/.../{tag}"]"""
    from pixelrec_amd import ops

    D = x.D
    table, items, mask = x.g("table"), x.g("items"), x.g("mask")
    loss, pos, neg = ops.bpr_loss_fwd(x.g("out"), table, items, mask, layout=x.layout)
    out[f"bpr_loss_fwd/{tag}"] = _rec(loss=loss, pos=pos, neg=neg)
    d = (pos - neg).view(-1)
    assert float(d[0]) > 100.0 and (d.numel() == 1 or float(d[1]) < -100.0), tag
    for key in scales:
        gs, dev = _scale(key)
        dout, coef = ops.bpr_loss_bwd(x.g("pos"), x.g("neg"), table, items, mask, D, grad_scale=gs, grad_scale_dev=dev, layout=x.layout)
        out[f"bpr_loss_bwd/{key}/{tag}"] = _rec(dout=dout, coef=coef)
    for p in drops:
        y, xhat, rstd, loss, pos, neg = ops.ln_residual_bpr_fwd(x.g("x"), x.g("res"), x.g("gamma"), x.g("beta"), EPS, table, items, mask,
                                                                p_drop=p, seed=SEED, stream_id=STREAM, step_dev=_step(), layout=x.layout)
        out[f"ln_residual_bpr_fwd/p{p}/{tag}"] = _rec(y=y, xhat=xhat, rstd=rstd, loss=loss, pos=pos, neg=neg)
        for key in scales:
            gs, dev = _scale(key)
            dgamma, dbeta = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
            dz, dx, _, coef = ops.bpr_ln_bwd(x.g("pos"), x.g("neg"), table, items, mask, gs, dev, x.g("xhat"), x.g("rstd"), x.g("gamma"),
                                             dgamma, dbeta, p_drop=p, seed=SEED, stream_id=STREAM, need_dx=p > 0, step_dev=_step(),
                                             layout=x.layout)
            out[f"bpr_ln_bwd/p{p}/{key}/{tag}"] = _some(dz=dz, dx=dx, coef=coef, dgamma=dgamma, dbeta=dbeta)


def _input_cases(x, tag, out, drops=DROPS):
    """the entries that read the input ids of x.items"""
    from pixelrec_amd import ops

    for p in drops:
        y, xhat, rstd = ops.input_ln_fwd(x.g("table"), x.g("items"), x.idx_bstride, x.B, x.L, x.g("posemb"), x.g("gamma"), x.g("beta"),
                                         EPS, p_drop=p, seed=SEED, stream_id=STREAM, step_dev=_step())
        out[f"input_ln_fwd/p{p}/{tag}"] = _rec(y=y, xhat=xhat, rstd=rstd)
    out[f"embed_gather/{tag}"] = _rec(out=ops.embed_gather(x.g("table"), x.g("items")))


def _ln_cases(x, tag, out):
    """the LayerNorm sites and the stand-alone dropout: no ids"""
    from pixelrec_amd import ops

    D = x.D
    for p in DROPS:
        y, xhat, rstd = ops.ln_residual_fwd(x.g("x"), x.g("res"), x.g("gamma"), x.g("beta"), EPS, p_drop=p, seed=SEED, stream_id=STREAM,
                                            step_dev=_step())
        out[f"ln_residual_fwd/p{p}/{tag}"] = _rec(y=y, xhat=xhat, rstd=rstd)
        for mode in (0, 1):
            dgamma, dbeta = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
            dz, dx = ops.ln_bwd(mode, x.g("dy"), x.g("xhat"), x.g("rstd"), x.g("gamma"), dgamma, dbeta, p_drop=p, seed=SEED,
                                stream_id=STREAM, need_dx=(mode == 0 and p > 0), step_dev=_step())
            out[f"ln_bwd/gather{mode}/p{p}/{tag}"] = _some(dz=dz, dx=dx, dgamma=dgamma, dbeta=dbeta)
        out[f"dropout/p{p}/{tag}"] = _rec(y=ops.dropout(x.g("x"), p, SEED, STREAM, step_dev=_step()))


def _width_cases(D):
    out = {}
    for B, L in SHAPES:
        for layout in LAYOUTS:
            x, tag = Inputs(D, B, L, layout), f"{layout}/d{D}_b{B}_l{L}"
            _head_cases(x, tag, out)
            _input_cases(x, tag, out)
            if layout == LAYOUTS[0]:
                _ln_cases(x, f"d{D}_b{B}_l{L}", out)
            _clean()
    return out


HEAD_BATCHES = (1, 50, 300)
WD_ITEMS, WD_HL = 9, 70
DIN_L, DIN_D, DIN_HL = 3, 8, 6


def _wd_inputs(B):
    g = torch.Generator().manual_seed(7000 + B)
    alast = torch.randn(2 * B, WD_HL, generator=g) * 0.5
    dact = (torch.rand(2 * B, WD_HL, generator=g) < 0.5).float()
    wp = torch.randn(WD_HL, generator=g) * 0.1
    wide = torch.randn(WD_ITEMS, generator=g) * 0.1
    target = torch.randint(3, WD_ITEMS, (B, 2), generator=g)
    wide[1], wide[2] = 150.0, -150.0                       # x_0 near +150 and x_1 near -150: both saturated sides of the naive sigmoid
    target[0, 0] = 1
    if B > 1:
        target[1, 0], target[2, 1] = 2, 0
    return alast, dact, wp, wide, target


def _wd_run(B, target=None, scales=tuple(SCALES)):
    from pixelrec_amd import ops

    alast, dact, wp, wide, tgt = (t.cuda() for t in _wd_inputs(B))
    tgt = tgt if target is None else target.cuda()
    loss, head = ops.wd_head_fwd(alast, wp, wide, tgt)
    got = {"fwd": _rec(loss=loss, head=head)}
    for key in scales:
        gs, dev = _scale(key)
        dwp, dbp, dwb = torch.zeros(WD_HL, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
        dwide = torch.zeros(WD_ITEMS, device="cuda")
        dz = ops.wd_head_bwd(alast, dact, wp, tgt, head, dwp, dbp, dwide, dwb, grad_scale=gs, grad_scale_dev=dev)
        got[f"bwd/{key}"] = _rec(dz=dz, dwp=dwp, dbp=dbp, dwide=dwide, dwide_bias=dwb)
    return got


def _din_inputs(B):
    g = torch.Generator().manual_seed(9000 + B)
    R = 2 * B * DIN_L
    alast = torch.randn(R, DIN_HL, generator=g) * 0.5
    dact = (torch.rand(R, DIN_HL, generator=g) < 0.5).float()
    wd = torch.randn(DIN_HL, generator=g) * 0.3
    bd = torch.randn(1, generator=g) * 0.1
    emb = torch.randn(B * (DIN_L + 2), DIN_D, generator=g) * 0.5
    profile = torch.randint(0, 4, (B, DIN_L), generator=g)  # a quarter of the positions are padding
    return alast, dact, wd, bd, emb, profile


def _head_kernels_cases():
    from pixelrec_amd import ops

    out = {}
    for B in HEAD_BATCHES:
        for k, v in _wd_run(B).items():
            out[f"wd_head/{k}/b{B}"] = v
        alast, dact, wd, bd, emb, profile = (t.cuda() for t in _din_inputs(B))
        loss, s, kq, head = ops.din_head_fwd(alast, wd, bd, emb, profile)
        out[f"din_head/fwd/b{B}"] = _rec(loss=loss, s=s, kq=kq, head=head)
        for key in SCALES:
            gs, dev = _scale(key)
            dwd, dbd = torch.zeros(DIN_HL, device="cuda"), torch.zeros(1, device="cuda")
            dz, dsraw = ops.din_head_bwd(alast, dact, wd, profile, kq, head, DIN_D, dwd, dbd, grad_scale=gs, grad_scale_dev=dev)
            out[f"din_head/bwd/{key}/b{B}"] = _rec(dz=dz, dsraw=dsraw, dwd=dwd, dbd=dbd)
        _clean()
    return out


def _flagged(run):
    """run() with ids outside their range: the status bit must come up; the case clears it"""
    from pixelrec_amd import ops

    _clean()
    run()
    torch.cuda.synchronize()
    assert int(ops.device_status("cuda").item()) & BAD_INDEX, "a bad id did not flag the status word"
    ops.clear_status_bits("cuda", BAD_INDEX)
    _clean()


def _bad_inputs(x):
    """ids outside the table among the inputs (items[:, 0, t] in both layouts; embed_gather reads every id)"""
    x.items[1, 0, 2], x.items[2, 0, 3] = -1, N_TABLE
    x._gpu = {}
    return x


def _flagged_cases():
    D, (B, L) = 260, SHAPES[1]
    out = {}
    for layout in LAYOUTS:
        x = Inputs(D, B, L, layout)
        x.pos_ids[1, 2], x.pos_ids[2, 3], x.neg_ids[0, 4], x.neg_ids[1, 5] = -1, N_TABLE, -1, N_TABLE
        x.set_layout(layout)
        # (the backward entries clamp the same ids without flagging)
        _flagged(lambda: _head_cases(x, f"flagged/targets/{layout}", out, scales=("g0.3x0.7",), drops=(0.1,)))
        y = _bad_inputs(Inputs(D, B, L, layout))
        _flagged(lambda: _input_cases(y, f"flagged/inputs/{layout}", out, drops=(0.1,)))
    target = _wd_inputs(50)[4]
    target[5, 0], target[6, 0], target[7, 1], target[8, 1] = -1, WD_ITEMS, -1, WD_ITEMS
    got = {}
    _flagged(lambda: got.update(_wd_run(50, target=target, scales=("g0.3x0.7",))))
    out.update({f"wd_head/{k}/flagged": v for k, v in got.items()})
    return out


def _flags_one_by_one():
    """each id-checking entry alone on flagged ids raises the bit (the cases above run several entries between two checks)"""
    from pixelrec_amd import ops

    D, (B, L) = 260, SHAPES[1]
    for layout in LAYOUTS:
        x = Inputs(D, B, L, layout)
        x.pos_ids[1, 2], x.neg_ids[1, 5] = -1, N_TABLE
        x.set_layout(layout)
        table, items, mask = x.g("table"), x.g("items"), x.g("mask")
        _flagged(lambda: ops.bpr_loss_fwd(x.g("out"), table, items, mask, layout=x.layout))
        _flagged(lambda: ops.ln_residual_bpr_fwd(x.g("x"), x.g("res"), x.g("gamma"), x.g("beta"), EPS, table, items, mask, layout=x.layout))
        y = _bad_inputs(Inputs(D, B, L, layout))
        _flagged(lambda: ops.input_ln_fwd(y.g("table"), y.g("items"), y.idx_bstride, B, L, y.g("posemb"), y.g("gamma"), y.g("beta"), EPS))
        _flagged(lambda: ops.embed_gather(y.g("table"), y.g("items")))
    alast, _, wp, wide, target = _wd_inputs(50)
    target[5, 0], target[7, 1] = -1, WD_ITEMS
    _flagged(lambda: ops.wd_head_fwd(alast.cuda(), wp.cuda(), wide.cuda(), target.cuda()))


GROUPS = {**{f"d{D}": (lambda D=D: _width_cases(D)) for D in WIDTHS}, "heads": _head_kernels_cases, "flagged": _flagged_cases}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _group_of(name):
    if "flagged" in name:
        return "flagged"
    if name.startswith(("wd_head/", "din_head/")):
        return "heads"
    return name.rsplit("/", 1)[1].split("_")[0]               # ".../d260_b3_l13" -> "d260"


def test_inputs_reach_the_saturated_side_of_both_tails():
    for D in WIDTHS:
        for B, L in SHAPES:
            x = Inputs(D, B, L, "bert").x64
            assert bool(torch.isfinite(x).all())
            assert float(x[0]) > 100.0, (D, B, L)
            if B * L > 1:
                assert float(x[1]) < -100.0, (D, B, L)
    for B in HEAD_BATCHES:
        alast, _, wp, wide, target = (t.double() if t.is_floating_point() else t for t in _wd_inputs(B))
        xw = ((alast[0::2] - alast[1::2]) * wp).sum(1) + wide[target[:, 0]] - wide[target[:, 1]]
        assert float(xw[0]) > 100.0 and (B == 1 or float(xw[1]) < -100.0)


def test_every_id_checking_entry_flags_on_its_own():
    _flags_one_by_one()


@pytest.mark.parametrize("group", list(GROUPS))
def test_bits_of_the_separate_copies_are_kept(group, golden):
    got = GROUPS[group]()
    want = {k: v for k, v in golden.items() if _group_of(k) == group}
    assert sorted(got) == sorted(want) and want
    for name in sorted(want):
        assert got[name] == want[name], name


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: test_gpu_seq_head_bits.py --record FILE"
    cases = {}
    for make in GROUPS.values():
        cases.update(make())
    _flags_one_by_one()
    with open(sys.argv[2], "w") as f:                      # one case per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(cases[k], sort_keys=True)}" for k in sorted(cases)) + "\n}\n")
