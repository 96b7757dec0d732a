"""The split-K hand-over of the grouped weight gradient (grouped_dw_p3_kernel<Cfg, EARLY, 2>, csrc/gemm_p3.hip): two workgroups
reduce half of the tokens of a 256x128 tile each, publish their partial of the PARTNER's 128-row block and finish their own block
as `first-half partial + second-half partial`.  Checked here, on both operand formats that take the split (three bf16 planes,
tile 425612822; two fp16 planes, tile 225612822):
  * determinism -- the same bits from launch to launch, back to back on the same flag words into NaN-filled outputs (a flag left
    raised would let the next launch read an unpublished block: NaN), alone or inside a group of 8 (tile_begin != 0) and with the
    group's order permuted;
  * values against fp64, with the bounds the existing split-K cases use (test_gpu_gemm_p3._tol for the bf16 planes,
    test_gpu_h2's 4e-6 sqrt(T) max|ref| for the fp16 planes);
  * the bits of the store-then-add hand-over this one replaced (tests/golden/dw_handover_bits.json, recorded from that kernel with
    `python tests/test_gpu_dw_handover.py --record FILE`): the sum order did not change, so the checksums must not.
Shapes: out features N of 32 / 160 / 256 / 288 (the upper row block wholly outside the matrix, partly outside, exactly full, and a
second tile row that holds 32 rows), in features K below, at and above one 128-column tile, tokens T whose 32-token panels split
unevenly between the halves (33: 32 + 32 of padding; 64: 32 + 32; 1600: 800 + 800).  The entry points take N and K in multiples
of 32 only: K = 24 and K = 136 (a row that is no multiple of 8 floats) are refused before any launch, which is asserted."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SPLIT = {"bf16x3": 425612822, "h2": 225612822}
NS, KS_OK, KS_REFUSED, TS = (32, 160, 256, 288), (32, 128, 160), (24, 136), (33, 64, 1600)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dw_handover_bits.json")
HEADLINE = [(1536, 512), (512, 512), (1024, 512), (512, 1024)] * 2          # (N, K) of a layer's four matrices, two layers


def _operands(fmt, T, N, K, seed):
    from pixelrec_amd import ops

    g = torch.Generator().manual_seed(seed)
    dy, x = (torch.randn(T, N, generator=g) * 1e-2).cuda(), torch.randn(T, K, generator=g).cuda()
    if fmt == "h2":
        dyp, xp = ops.split_h2_auto([dy])[0], ops.split_h2_auto([x])[0]
    else:
        dyp, xp = ops.split_planes(dy), ops.split_planes(x)
    return dy, x, dyp, xp


def _launch(fmt, ops_, with_db):
    """one split launch of the problems [(dyp, xp, N, K)] into NaN-filled outputs"""
    from pixelrec_amd import ops

    outs = [(torch.full((N, K), float("nan"), device="cuda"), torch.full((N,), float("nan"), device="cuda") if with_db else None)
            for _, _, N, K in ops_]
    ops.grouped_dw_planes([(dyp, xp, dW, db) for (dyp, xp, _, _), (dW, db) in zip(ops_, outs)], tile_hint=SPLIT[fmt])
    return outs


def _same(a, b):
    return all(torch.equal(x[0], y[0]) and (x[1] is None or torch.equal(x[1], y[1])) for x, y in zip(a, b))


@pytest.mark.parametrize("with_db", [True, False])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("fmt", ["bf16x3", "h2"])
def test_split_launch_bits_and_values(fmt, T, with_db):
    from pixelrec_amd import ops

    shapes = [(N, K) for N in NS for K in KS_OK]
    data = [_operands(fmt, T, N, K, 1000 * T + N + K) for N, K in shapes]
    probs = [(d[2], d[3], N, K) for d, (N, K) in zip(data, shapes)]
    solo = [_launch(fmt, [p], with_db)[0] for p in probs]                    # groups of one problem
    for (dy, x, _, _), (dW, db) in zip(data, solo):                          # values against fp64
        rW, rb = dy.double().t() @ x.double(), dy.double().sum(0)
        eW, eb = (dW.double() - rW).abs().max().item(), 0.0 if db is None else (db.double() - rb).abs().max().item()
        if fmt == "h2":
            assert eW <= 4e-6 * (T ** 0.5) * float(rW.abs().max()), (dW.shape, eW)
            assert eb <= 4e-6 * (T ** 0.5) * float(rb.abs().max()) + 1e-12, (dW.shape, eb)
        else:
            assert eW <= 2e-6 * (T ** 0.5) * float(rW.abs().max()) + 1e-6, (dW.shape, eW)
            assert eb <= 2e-6 * (T ** 0.5) * float(rb.abs().max()) + 1e-7, (dW.shape, eb)
    for p, s in zip(probs, solo):                                            # the same launch again, back to back on the same flags
        for _ in range(2):
            assert _same(_launch(fmt, [p], with_db), [s])
    perm = torch.randperm(8, generator=torch.Generator().manual_seed(T)).tolist()
    for lo in (0, 2, 4):                                                     # groups of 8: every shape at a tile_begin > 0 as well
        idx = list(range(lo, lo + 8))
        for order in (idx, [idx[i] for i in perm]):
            for _ in range(2):
                assert _same(_launch(fmt, [probs[i] for i in order], with_db), [solo[i] for i in order]), (lo, order)
    ops.raise_on_bad_indices("cuda")                                         # nobody timed out waiting for a flag


@pytest.mark.parametrize("fmt", ["bf16x3", "h2"])
def test_rows_that_are_no_multiple_of_32_floats_are_refused(fmt):
    from pixelrec_amd.lib import PxrError

    for K in KS_REFUSED:
        _, _, dyp, xp = _operands(fmt, 64, 32, 32, 3)
        xp.cols = K                                                          # (the shape check comes before anything is read)
        with pytest.raises(PxrError, match="multiples of 32"):
            _launch(fmt, [(dyp, xp, 32, K)], True)


def _u32_sum(t):
    return int((t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF).sum().item())


def _golden_cases():
    """name -> [[checksum of dW, checksum of db] per problem]: the headline group (T = 3200) and two small shapes, both formats"""
    out = {}
    for fmt in ("bf16x3", "h2"):
        for name, T, shapes in (("headline", 3200, HEADLINE), ("n160_k160_t33", 33, [(160, 160)]), ("n288_k128_t1600", 1600, [(288, 128)])):
            probs = []
            for i, (N, K) in enumerate(shapes):
                _, _, dyp, xp = _operands(fmt, T, N, K, 77 + i)
                probs.append((dyp, xp, N, K))
            out[f"{fmt}/{name}"] = [[_u32_sum(dW), _u32_sum(db)] for dW, db in _launch(fmt, probs, True)]
    return out


def test_bits_of_the_store_then_add_hand_over_are_kept():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = _golden_cases()
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


if __name__ == "__main__":
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: test_gpu_dw_handover.py --record FILE"
    with open(sys.argv[2], "w") as f:
        json.dump(_golden_cases(), f, indent=0, sort_keys=True)
        f.write("\n")
