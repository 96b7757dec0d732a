"""The bits of every entry point that runs on the shared pair-head core (csrc/pair_head.cuh: dot4, the id clamp with its status
flag, the two loss tails, the pair of wave dot products, the first-occurrence walk, the register row, the gradient scale, the CH
dispatch) against tests/golden/pair_head_bits.json, which was recorded with `python tests/test_gpu_pair_bits.py --record FILE` on
the build of the commit BEFORE the core was shared (six private float4 typedefs, five dot4s, three and two copies of the loss
tails, three occurrence scans).  Sharing the code changes no product, no order of a sum and no clamp, so per case every integer
output must be equal in full, and so must two u32 sums of every float output's bit patterns: the plain sum and the sum weighted by
(index + 1), which catches a permutation the first would miss.

Inputs (torch.Generator().manual_seed on the CPU, all finite), one set per (D, B):
  * D in 4, 64, 260, 772, 1028 (MF and VBPR also 2052): dv = 1, 16, 65, 193, 257, 513 float4s per row, CH = 1, 1, 2, 4, 8 (the <8>
    default branch of LightGCN's switch) and 16; 65, 193, 257 and 513 leave a ragged last lane group;
  * B = 50 and 1: with 50, a row's occurrences fall inside one 64-wide ballot window and across windows, and the last workgroup of
    four waves is ragged; ids come from pools of 7 users and 9 items, so every row recurs (each of VBPR's three segments too);
  * user and item rows drawn at scale 0.02.  Samples 0, 1, 2 (sample 0 alone when B = 1) use user s and positive item s: item row s
    is a copy of user row s, negated for s = 1, and user row s is then multiplied by 3000.  x_s = +-3000 |u_s|^2 +- ... ~ +-1.2 D,
    so for D >= 260 some |x| exceeds 100 in both signs (asserted below in fp64) and takes the saturated side of each loss tail;
    every result stays finite (-log(1e-8) on the inside form);
  * every backward entry runs with grad_scale 1 and no device scale, and with grad_scale 0.3 and a device scale of 0.7 (neither a
    power of two: a reordered product of coef, scale and device scale rounds differently and shows);
  * flagged ids, one case per id-checking entry (D 64, B 50): one id of -1 and one of n; PXR_STATUS_BAD_INDEX must be set, the
    clamped outputs must match the golden, and the case clears its bit.
ops.raise_on_bad_indices after every case shows that no status bit is left set, on the recording build as well."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pair_head_bits.json")
NU, NI = 7, 9
WIDTHS = (4, 64, 260, 772, 1028)
WIDE = 2052                                                # MF and VBPR only: CH 16
BATCHES = (50, 1)
SCALES = {"g1": (1.0, None), "g0.3x0.7": (0.3, 0.7)}
BAD_INDEX = 1                                              # PXR_STATUS_BAD_INDEX


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
from tests.golden_util import rec_bits as _rec  # noqa: E402   (shared with tests/test_gpu_seq_head_bits.py)


def _clean():
    from pixelrec_amd import ops

    ops.raise_on_bad_indices("cuda")


class Inputs:
    """the shared inputs of one (D, B), on the GPU"""

    def __init__(self, D, B):
        g = torch.Generator().manual_seed(1000 * D + B)
        self.D, self.B = D, B
        U = torch.randn(NU, D, generator=g) * 0.02
        I = torch.randn(NI, D, generator=g) * 0.02
        user = torch.randint(0, NU, (B,), generator=g)
        item = torch.randint(0, NI, (B, 2), generator=g)
        for s in range(min(3, B)):
            user[s], item[s, 0] = s, s
            item[s, 1] = 3 + s                             # a negative that is none of the copied rows
            I[s] = -U[s] if s == 1 else U[s]
            U[s] *= 3000.0
        self.x64 = ((U[user].double() * (I[item[:, 0]].double() - I[item[:, 1]].double())).sum(1))
        spare = torch.randn(1, D, generator=g) * 0.02      # row 0 of the tables: nothing reads it
        Um = torch.randn(NU, D, generator=g) * 0.02        # VBPR's user_modal_embedding
        self.e = (torch.randn(2 * B, D, generator=g) * 0.02).cuda()
        self.beta = (torch.randn(2 * B, generator=g) * 0.02).cuda()
        self.feat = (torch.randn(NI, D, generator=g) * 0.02).cuda()
        self.wb = (torch.randn(D, generator=g) * 0.02).cuda()
        self.occ = (torch.randn(3 * B, D, generator=g) * 0.02).cuda()
        self.pad = (torch.randn(B, D, generator=g) * 0.02)  # the second half of SRGNN's [B, 2D] query rows: never read
        self.user, self.item = user.cuda(), item.cuda()
        self.mf_table = torch.cat([spare, U, I]).cuda()
        self.vbpr_table = torch.cat([spare, U, I, Um]).cuda()
        self.emb = torch.cat([U, I]).cuda()
        self.items_table = I.cuda()
        self.ufeat = U[user].contiguous().cuda()
        self.ifeat = I[item.view(-1)].contiguous().cuda()
        self.srgnn_out = torch.cat([U[user], self.pad], 1).contiguous().cuda()


def _scale(key):
    gs, dev = SCALES[key]
    return gs, (None if dev is None else torch.tensor([dev], dtype=torch.float32).cuda())


def _mf_cases():
    from pixelrec_amd import ops

    out = {}
    for B in BATCHES:
        for D in WIDTHS + (WIDE,):
            x, tag = Inputs(D, B), f"d{D}_b{B}"
            rows = ops.mf_pair_rows(x.user, x.item, NU, NI)
            if D == WIDTHS[0]:                             # the row kernels do not see D
                out[f"mf/pair_rows/b{B}"] = _rec(rows=rows)
                out[f"mf/pair_rows/users_only/b{B}"] = _rec(rows=ops.mf_pair_rows(x.user, None, NU, NI))
            loss, coef = ops.mf_pair_fwd(x.mf_table, x.mf_table, B, rows=rows)
            out[f"mf/pair_fwd/rows/{tag}"] = _rec(loss=loss, coef=coef)
            loss_t, coef_t = ops.mf_pair_fwd(x.ufeat, x.ifeat, B)
            out[f"mf/pair_fwd/towers/{tag}"] = _rec(loss=loss_t, coef=coef_t)
            for key in SCALES:
                gs, dev = _scale(key)
                du, di = torch.zeros_like(x.ufeat), torch.zeros_like(x.ifeat)
                ops.mf_pair_bwd(x.ufeat, x.ifeat, coef_t, du, di, grad_scale=gs, grad_scale_dev=dev)
                out[f"mf/pair_bwd/{key}/{tag}"] = _rec(du=du, di=di)
                sp = ops.SparseRows(3 * B, D, "cuda")
                ops.mf_table_grad(rows, B, sp, table=x.mf_table, coef=coef, grad_scale=gs, grad_scale_dev=dev)
                out[f"mf/table_grad/head/{key}/{tag}"] = _rec(idx=sp.idx, rows=sp.rows, n=sp.n)
                sp = ops.SparseRows(3 * B, D, "cuda")
                ops.mf_table_grad(rows, B, sp, occ=x.occ, grad_scale=gs, grad_scale_dev=dev)
                out[f"mf/table_grad/occ/{key}/{tag}"] = _rec(idx=sp.idx, rows=sp.rows, n=sp.n)
            _clean()
    return out


def _vbpr_cases():
    from pixelrec_amd import ops

    out = {}
    for B in BATCHES:
        for D in WIDTHS + (WIDE,):
            x, tag = Inputs(D, B), f"d{D}_b{B}"
            rows = ops.vbpr_rows(x.user, x.item, NU, NI)
            if D == WIDTHS[0]:
                out[f"vbpr/rows/b{B}"] = _rec(rows=rows)
                out[f"vbpr/rows/users_only/b{B}"] = _rec(rows=ops.vbpr_rows(x.user, None, NU, NI))
            flat = x.item.view(-1)
            o, beta = ops.vbpr_gather(x.feat, flat, x.wb)
            out[f"vbpr/gather/item_out/{tag}"] = _rec(out=o, beta=beta)
            out[f"vbpr/gather/item_beta/{tag}"] = _rec(beta=ops.vbpr_gather(x.feat, flat, x.wb, copy=False)[1])
            o, beta = ops.vbpr_gather(x.feat, None, x.wb)
            out[f"vbpr/gather/all_out/{tag}"] = _rec(out=o, beta=beta)
            out[f"vbpr/gather/all_beta/{tag}"] = _rec(beta=ops.vbpr_gather(x.feat, None, x.wb, copy=False)[1])
            loss, coef = ops.vbpr_pair_fwd(x.vbpr_table, rows, x.e, x.beta, B)
            out[f"vbpr/pair_fwd/{tag}"] = _rec(loss=loss, coef=coef)
            for key in SCALES:
                gs, dev = _scale(key)
                de, csign = torch.zeros_like(x.e), torch.zeros(2 * B, device="cuda")
                sp = ops.SparseRows(4 * B, D, "cuda")
                ops.vbpr_pair_bwd(x.vbpr_table, rows, x.e, coef, B, de, csign, sp, grad_scale=gs, grad_scale_dev=dev)
                out[f"vbpr/pair_bwd/{key}/{tag}"] = _rec(de=de, csign=csign, idx=sp.idx, rows=sp.rows, n=sp.n)
            _clean()
    return out


def _lgcn_cases():
    from pixelrec_amd import ops

    out = {}
    for B in BATCHES:
        for D in WIDTHS:
            x, tag = Inputs(D, B), f"d{D}_b{B}"
            loss, diff, coef, nodes = ops.lgcn_pair_fwd(x.emb, NU, NI, x.user, x.item)
            out[f"lgcn/pair_fwd/{tag}"] = _rec(loss=loss, diff=diff, coef=coef, nodes=nodes)
            for key in SCALES:
                gs, dev = _scale(key)
                grad = torch.empty_like(x.emb)
                ops.lgcn_pair_bwd(x.emb, nodes, coef, grad, grad_scale=gs, grad_scale_dev=dev)
                out[f"lgcn/pair_bwd/{key}/{tag}"] = _rec(grad=grad)
            _clean()
    return out


def _srgnn_cases():
    from pixelrec_amd import ops

    out = {}
    for B in BATCHES:
        for D in WIDTHS:
            x, tag = Inputs(D, B), f"d{D}_b{B}"
            loss, coef = ops.srgnn_pair_fwd(x.srgnn_out, 2 * D, x.items_table, x.item, B)
            out[f"srgnn/pair_fwd/{tag}"] = _rec(loss=loss, coef=coef)
            for key in SCALES:
                gs, dev = _scale(key)
                dout, cout = torch.zeros(B, 2 * D, device="cuda"), torch.zeros(2 * B, device="cuda")
                ops.srgnn_pair_bwd(x.items_table, x.item, coef, dout, 2 * D, grad_scale=gs, grad_scale_dev=dev, coef_out=cout,
                                   coef_stride=2)
                out[f"srgnn/pair_bwd/coef_out/{key}/{tag}"] = _rec(dout=dout, coef_out=cout)
                dout = torch.zeros(B, 2 * D, device="cuda")
                ops.srgnn_pair_bwd(x.items_table, x.item, coef, dout, 2 * D, grad_scale=gs, grad_scale_dev=dev)
                out[f"srgnn/pair_bwd/plain/{key}/{tag}"] = _rec(dout=dout)
            _clean()
    return out


POOL = (3, 4, 8)                                           # B, L, E of the pooling case


def _pool_inputs():
    B, L, E = POOL
    g = torch.Generator().manual_seed(77)
    return (torch.randn(NI, E, generator=g) * 0.02).cuda(), torch.randint(0, NI, (B, L), generator=g)


def _curator_cases():
    from pixelrec_amd import ops

    out = {}
    for B in BATCHES:
        for D in WIDTHS:
            x = Inputs(D, B)
            loss, coef = ops.curator_pair_fwd(x.ufeat, x.ifeat, B)
            out[f"curator/pair_fwd/d{D}_b{B}"] = _rec(loss=loss, coef=coef)
            _clean()
    B, L, E = POOL
    h, ids = _pool_inputs()
    cat, argmax = ops.curator_pool(h, B, L, ids=ids.cuda())
    out["curator/pool/ids/b3_l4_e8"] = _rec(cat=cat, argmax=argmax)
    _clean()
    return out


ACF_P = 3


def _acf_inputs(B):
    g = torch.Generator().manual_seed(500 + B)
    profile = torch.randint(0, NI, (B, ACF_P), generator=g)
    items = torch.randint(0, NI, (B, 2), generator=g)
    profile[0, ACF_P - 1] = 0                              # a padding position
    items[B - 1, 1] = 0                                    # item 0 among the step's items: read, no gradient row
    return profile, items, torch.randint(0, NU, (B,), generator=g)


def _acf_cases():
    from pixelrec_amd import ops

    out = {}
    for B in BATCHES:
        profile, items, user = (t.cuda() for t in _acf_inputs(B))
        rows, gidx = ops.acf_rows(profile, items, user, NI, NU)
        out[f"acf/rows/gidx/b{B}"] = _rec(rows=rows, gidx=gidx)
        out[f"acf/rows/no_gidx/b{B}"] = _rec(rows=ops.acf_rows(profile, items, user, NI, NU, want_gidx=False)[0])
        out[f"acf/rows/no_items/b{B}"] = _rec(rows=ops.acf_rows(profile, None, user, NI, NU, want_gidx=False)[0])
        _clean()
    return out


def _flagged(run):
    """run() with ids outside their range: the status bit must come up; the case clears it"""
    from pixelrec_amd import ops

    _clean()
    got = run()
    torch.cuda.synchronize()
    assert int(ops.device_status("cuda").item()) & BAD_INDEX, "a bad id did not flag the status word"
    ops.clear_status_bits("cuda", BAD_INDEX)
    _clean()
    return got


def _flagged_cases():
    from pixelrec_amd import ops

    D, B = 64, 50
    x = Inputs(D, B)
    user, item = x.user.clone(), x.item.clone()
    user[5], user[6] = -1, NU
    item[7, 0], item[8, 1] = -1, NI
    out = {}
    out["flagged/mf/pair_rows"] = _flagged(lambda: _rec(rows=ops.mf_pair_rows(user, item, NU, NI)))
    out["flagged/vbpr/rows"] = _flagged(lambda: _rec(rows=ops.vbpr_rows(user, item, NU, NI)))

    def gather():
        o, beta = ops.vbpr_gather(x.feat, item.view(-1), x.wb)
        return _rec(out=o, beta=beta)
    out["flagged/vbpr/gather"] = _flagged(gather)

    def lgcn():
        loss, diff, coef, nodes = ops.lgcn_pair_fwd(x.emb, NU, NI, user, item)
        return _rec(loss=loss, diff=diff, coef=coef, nodes=nodes)
    out["flagged/lgcn/pair_fwd"] = _flagged(lgcn)

    def srgnn():                                           # the backward clamps the same ids without flagging
        loss, coef = ops.srgnn_pair_fwd(x.srgnn_out, 2 * D, x.items_table, item, B)
        dout = torch.zeros(B, 2 * D, device="cuda")
        ops.srgnn_pair_bwd(x.items_table, item, coef, dout, 2 * D)
        return _rec(loss=loss, coef=coef, dout=dout)
    out["flagged/srgnn/pair"] = _flagged(srgnn)

    def pool():
        Bp, L, _ = POOL
        h, ids = _pool_inputs()
        ids[0, 1], ids[2, 3] = -1, NI
        cat, argmax = ops.curator_pool(h, Bp, L, ids=ids.cuda())
        return _rec(cat=cat, argmax=argmax)
    out["flagged/curator/pool"] = _flagged(pool)

    def acf():
        profile, items, u = (t.cuda() for t in _acf_inputs(B))
        profile[1, 0], items[2, 1], u[3], u[4] = -1, NI, -1, NU
        rows, gidx = ops.acf_rows(profile, items, u, NI, NU)
        return _rec(rows=rows, gidx=gidx)
    out["flagged/acf/rows"] = _flagged(acf)
    return out


GROUPS = {"mf": _mf_cases, "vbpr": _vbpr_cases, "lgcn": _lgcn_cases, "srgnn": _srgnn_cases, "curator": _curator_cases,
          "acf": _acf_cases, "flagged": _flagged_cases}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_inputs_reach_the_saturated_side_of_both_tails():
    for D in WIDTHS + (WIDE,):
        x = Inputs(D, 50).x64
        assert bool(torch.isfinite(x).all())
        if D >= 260:
            assert float(x.max()) > 100.0 and float(x.min()) < -100.0, D


@pytest.mark.parametrize("group", list(GROUPS))
def test_bits_of_the_separate_copies_are_kept(group, golden):
    got = GROUPS[group]()
    want = {k: v for k, v in golden.items() if k.split("/")[0] == group}
    assert sorted(got) == sorted(want) and want
    for name in sorted(want):
        assert got[name] == want[name], name


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: test_gpu_pair_bits.py --record FILE"
    cases = {}
    for make in GROUPS.values():
        cases.update(make())
    with open(sys.argv[2], "w") as f:                      # one case per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(cases[k], sort_keys=True)}" for k in sorted(cases)) + "\n}\n")
