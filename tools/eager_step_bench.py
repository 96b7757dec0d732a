"""Host time of one eagerly issued training step, per model family, at the tiny shapes of tests/test_gpu_packed_bits.py.

    python tools/eager_step_bench.py --model widedeep [--steps 300] [--rounds 5] [--profile 25]

At these shapes the device finishes long before the host has issued the next launch, so ms per step of the loop `zero_grad /
forward / backward / step` IS the host time of the step: the models' own Python, the ops wrappers, the launches.  (The step the
other benches time is replayed from a hipGraph, where none of that runs.)  One model per process: a model timed after others in
the same process inherits their allocator and collector state.  Prints one JSON line: the rounds, their minimum and median.
--profile N adds cProfile's N most expensive functions (by own time) of one further round, on stderr.
"""
import argparse
import cProfile
import json
import os
import pstats
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def main():
    from tests import test_gpu_packed_bits as P

    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True, choices=sorted(P.MODELS))
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--profile", type=int, default=0, metavar="N")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        m = P.MODELS[args.model](tmp)
        opt, batches, _ = P._training(args.model, m)

        def steps(n):
            for i in range(n):
                opt.zero_grad()
                loss = m(batches[i % len(batches)])
                loss.backward()
                opt.step()

        steps(args.warmup)
        rounds = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t = time.perf_counter()
            steps(args.steps)
            torch.cuda.synchronize()
            rounds.append(round((time.perf_counter() - t) / args.steps * 1e3, 4))
        print(json.dumps({"model": args.model, "steps": args.steps, "host_ms_per_step_rounds": rounds, "min": min(rounds),
                          "median": statistics.median(rounds)}))
        if args.profile:
            prof = cProfile.Profile()
            prof.enable()
            steps(args.steps)
            prof.disable()
            pstats.Stats(prof, stream=sys.stderr).sort_stats("tottime").print_stats(args.profile)


if __name__ == "__main__":
    main()
