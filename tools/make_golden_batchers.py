"""Records what every batcher of pixelrec_amd/data/dataset.py yields into tests/golden/batcher_streams.json:
    python tools/make_golden_batchers.py
tests/test_batcher_streams_cpu.py runs collect() and compares it with that file, key by key.  The file is recorded BEFORE a change
to the data layer and must be reproduced byte for byte after it: checkpoint resumes, `estimate_exchange_rows` and every restatement
test depend on the batchers' streams being functions of (seed, epoch, rank) alone.

Inputs: tests/golden/TinyInter.csv through Data (88 items, 61 users) as SEQ, AUGSEQ or PAIR, whichever the batcher reads;
MAX_ITEM_LIST_LENGTH 5 and 50, train_batch_size 8, eval_batch_size 7, config seed 5, mask_ratio 0.4, sampler seed 3;
(world, rank) in {(1,0), (2,0), (2,1), (3,2)}; epochs 0 and 1 through set_epoch; drop_last False and True.  Only the public surface
is used: the constructors, set_epoch, len(), _indices(), make_batch(rows, rng), iteration, estimate_exchange_rows.

Per train case: len(batcher); per epoch a sha256 of _indices(), a sha256 over every yielded element in order (dtype, shape,
contiguity and raw bytes of each tensor; plain integers as text) and the number of rng.integers / rng.random calls make_batch makes
along _indices() on a generator seeded like the frame's, [config seed, epoch, rank].  That replay must yield what iteration yields
(the rng key is part of the contract), which collect() asserts.  Per eval case: len() and the sha256 of one pass, both phases.
Under "errors": the text of every constructor ValueError and of every exhaustion ValueError, the latter on a stub dataload of
item_num 3 with the one chunk [1, 2], whose every candidate negative lies in the chunk.

collect() refuses to record a vacuous file: every train batcher must redraw in some case (more integers calls than batches), and
SeqTrainBatcher must be recorded on both sides of its `item_num > 2 * W` guard.
"""
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pixelrec_amd.data import dataset as D  # noqa: E402
from pixelrec_amd.data.dataload import Data  # noqa: E402
from pixelrec_amd.utils.enum_type import InputType  # noqa: E402

GDIR = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GDIR, "batcher_streams.json")
SEED, SAMPLER_SEED = 5, 3
HEX = 24                             # hex digits kept of each sha256: 96 bits tell any change, and the file stays small
LENGTHS = (5, 50)
RANKS = ((1, 0), (2, 0), (2, 1), (3, 2))
# name -> (class, the input type its Data is built with, extra config)
TRAIN = {"SeqTrainBatcher": (D.SeqTrainBatcher, "SEQ", {}),
         "SeqTrainBatcher+device_sampler": (D.SeqTrainBatcher, "SEQ", {"device_sampler": True}),
         "BERT4RecTrainBatcher": (D.BERT4RecTrainBatcher, "SEQ", {}),
         "TwoTowerTrainBatcher": (D.TwoTowerTrainBatcher, "AUGSEQ", {}),
         "SampleAcfTrainBatcher": (D.SampleAcfTrainBatcher, "SEQ", {}),
         "DinTrainBatcher": (D.DinTrainBatcher, "SEQ", {}),
         "MoPoolTrainBatcher": (D.MoPoolTrainBatcher, "SEQ", {}),
         "CuratorTrainBatcher": (D.CuratorTrainBatcher, "SEQ", {}),
         "MoTowerTrainBatcher": (D.MoTowerTrainBatcher, "SEQ", {}),
         "MoBert4RecTrainBatcher": (D.MoBert4RecTrainBatcher, "SEQ", {}),
         "PairTrainBatcher": (D.PairTrainBatcher, "PAIR", {}),
         "GraphTrainBatcher": (D.GraphTrainBatcher, "AUGSEQ", {})}
EVAL = {"SeqEvalBatcher": (D.SeqEvalBatcher, {}),
        "PairEvalBatcher": (D.PairEvalBatcher, {}),
        "AcfEvalBatcher": (D.AcfEvalBatcher, {}),
        "GraphEvalBatcher": (D.GraphEvalBatcher, {}),
        "VisRankEvalBatcher": (D.VisRankEvalBatcher, {}),
        "VisRankEvalBatcher+history_window3": (D.VisRankEvalBatcher, {"history_window": 3})}


class CountingRng:
    """Forwards to a real Generator and counts the calls."""

    def __init__(self, key):
        self.rng = np.random.default_rng(key)
        self.n_integers = self.n_random = 0

    def integers(self, *a, **k):
        self.n_integers += 1
        return self.rng.integers(*a, **k)

    def random(self, *a, **k):
        self.n_random += 1
        return self.rng.random(*a, **k)


def _feed(h, x):
    if isinstance(x, (tuple, list)):
        h.update(b"(")
        for y in x:
            _feed(h, y)
        h.update(b")")
    elif isinstance(x, np.ndarray):
        _feed(h, torch.from_numpy(x))
    elif torch.is_tensor(x):
        h.update(f"{x.dtype}{tuple(x.shape)}{x.is_contiguous()}".encode())
        h.update(x.contiguous().numpy().tobytes())
    else:
        h.update(f"int:{int(x)};".encode())


def digest(batches):
    h = hashlib.sha256()
    for batch in batches:
        _feed(h, batch)
    return h.hexdigest()[:HEX]


def _config(L, kind, extra):
    cfg = {"data_path": GDIR, "dataset": "TinyInter", "MAX_ITEM_LIST_LENGTH": L, "MODEL_INPUT_TYPE": getattr(InputType, kind),
           "train_batch_size": 8, "eval_batch_size": 7, "seed": SEED, "mask_ratio": 0.4}
    cfg.update(extra)
    return cfg


def _data(L, kind):
    d = Data(_config(L, kind, {}))
    d.build()
    return d


def _replay(batcher, epoch, rank):
    """make_batch along _indices() on a counting generator seeded like the frame's -> (batches as numpy, integers, random)."""
    idx, bs = batcher._indices(), batcher.batch_size
    rng = CountingRng([SEED, epoch, rank])
    out = [batcher.make_batch(idx[b * bs:(b + 1) * bs], rng) for b in range(len(batcher))]
    return out, rng.n_integers, rng.n_random


def _train_case(cls, cfg, data, world, rank, drop_last):
    batcher = cls(cfg, data, rank=rank, world=world, seed=SAMPLER_SEED, drop_last=drop_last)
    rec = {"len": len(batcher), "indices": [], "stream": [], "integers": [], "random": []}
    for epoch in (0, 1):
        batcher.set_epoch(epoch)
        rec["indices"].append(digest([batcher._indices()]))
        rec["stream"].append(digest(iter(batcher)))
        batches, n_int, n_rand = _replay(batcher, epoch, rank)
        if not cfg.get("device_sampler"):
            assert digest(batches) == rec["stream"][-1], "iteration is not make_batch along _indices() under [seed, epoch, rank]"
        rec["integers"].append(n_int)
        rec["random"].append(n_rand)
    if (world, rank) == (2, 1) and hasattr(batcher, "estimate_exchange_rows") and cls is not D.MoBert4RecTrainBatcher:
        rec["exchange_rows"] = batcher.estimate_exchange_rows(n_batches=4)
    return rec


def _error(fn):
    try:
        fn()
    except ValueError as e:
        return str(e)
    return None


def _stub(item_num, chunk):
    """A dataload with the one chunk `chunk` of user 1, in all three forms (SEQ chunks, the AUGSEQ prefix that is the whole chunk,
    PAIR interactions)."""
    chunk = np.asarray(chunk, dtype=np.int64)
    return SimpleNamespace(item_num=item_num, _sorted_items=chunk,
                           train_feat={"item_seq": [chunk], "user_id": np.ones(len(chunk), dtype=np.int64), "item_id": chunk,
                                       "seq_start": np.zeros(1, dtype=np.int64), "seq_len": np.asarray([len(chunk)])})


def _errors():
    cfg = {"MAX_ITEM_LIST_LENGTH": 5, "train_batch_size": 8, "seed": SEED, "mask_ratio": 1.0}
    rows = np.zeros(1, dtype=np.int64)
    out = {"TwoTowerTrainBatcher/no_prefixes": _error(lambda: D.TwoTowerTrainBatcher(_config(5, "SEQ", {}), _data(5, "SEQ")))}
    for name, (cls, _, extra) in TRAIN.items():
        if extra:
            continue
        # Pair refuses item_num <= 1; the others that check refuse item_num <= 2 (one item and the padding)
        small = 1 if cls is D.PairTrainBatcher else 2
        out[f"{name}/item_num{small}"] = _error(lambda: cls(cfg, _stub(small, [1])))
        if cls is D.PairTrainBatcher:
            out[f"{name}/full_history"] = _error(lambda: cls(cfg, _stub(3, [1, 2])))
            continue
        batcher = cls(cfg, _stub(3, [1, 2]))
        rng = CountingRng(0)
        holder = []
        out[f"{name}/exhausted"] = _error(lambda: holder.append(batcher.make_batch(rows, rng)))
        # the sequence batchers end their redraws silently: what they then return, and after how many draws, is recorded instead
        out[f"{name}/exhausted_integers"] = rng.n_integers
        out[f"{name}/exhausted_batch"] = digest(holder) if holder else None
    return out


def collect():
    data = {(L, kind): _data(L, kind) for L in LENGTHS for kind in ("SEQ", "AUGSEQ", "PAIR")}
    train, evals = {}, {}
    for name, (cls, kind, extra) in TRAIN.items():
        for L in LENGTHS:
            cfg = _config(L, kind, extra)
            for world, rank in RANKS:
                for drop_last in (False, True):
                    train[f"{name}/L{L}/world{world}rank{rank}/drop_last{int(drop_last)}"] = _train_case(
                        cls, cfg, data[L, kind], world, rank, drop_last)
    for name, (cls, extra) in EVAL.items():
        for L in LENGTHS:
            cfg = _config(L, "SEQ", extra)
            for world, rank in RANKS:
                for phase in ("valid", "test"):
                    batcher = cls(cfg, data[L, "SEQ"], phase, rank, world)
                    evals[f"{name}/L{L}/world{world}rank{rank}/{phase}"] = {
                        "len": len(batcher), "users": digest([batcher.users]), "stream": digest(iter(batcher))}

    # not vacuous: every make_batch draws once and then once per redraw
    def extra_draws(key):
        return sum(n - train[key]["len"] for n in train[key]["integers"])
    for name in TRAIN:
        assert any(extra_draws(k) > 0 for k in train if k.startswith(name + "/")), f"{name} never redraws in the recorded cases"
    seq = {L: sum(extra_draws(k) for k in train if k.startswith(f"SeqTrainBatcher/L{L}/")) for L in LENGTHS}
    assert seq[5] > 0 and seq[50] == 0, "SeqTrainBatcher is not recorded on both sides of its item_num > 2 * W guard"
    return {"train": train, "eval": evals, "errors": _errors()}


def dumps(res):
    return json.dumps(res, indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    with open(OUT, "w") as f:
        f.write(dumps(collect()))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
