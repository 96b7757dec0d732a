"""The figures behind the tolerances of tests/test_gpu_topk_walk.py, on the CPU: for every DIN and WideDeep walk case, the largest
error of the reference-form float32 predict (the literal [B, N, L + 1] form) against the float64 restatement, relative to the
largest |score| of the case.

    python tools/measure_topk_walk.py
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import din_restate, widedeep_restate  # noqa: E402


def main():
    for name, R in (("DIN", din_restate), ("WideDeep", widedeep_restate)):
        worst = (0.0, None)
        for case, args in R.WALK_CASES.items():
            t0 = time.time()
            P, win, _ = R.walk_case(*args)
            s64 = R.scores64(P, win)
            s32 = R.predict_literal(P, win)
            rel = float((s32.double() - s64).abs().max() / s64.abs().max())
            print(f"{name:9s} {case:26s} {args}: {rel:.3e} of the largest |score| {float(s64.abs().max()):.3e}  ({time.time() - t0:.1f} s)",
                  flush=True)
            worst = max(worst, (rel, case))
        print(f"{name}: largest {worst[0]:.4e} ({worst[1]})", flush=True)


if __name__ == "__main__":
    main()
