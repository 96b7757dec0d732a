"""The data layer's contract, pinned: what every train and eval batcher yields -- number of batches, DistributedSampler order, every
tensor's dtype, shape, contiguity and bytes, the number of draws make_batch takes from the epoch's rng, estimate_exchange_rows and
the text of every ValueError -- equals tests/golden/batcher_streams.json, which tools/make_golden_batchers.py recorded before the
batchers were moved onto one frame.  The recorder itself refuses a vacuous recording (every batcher redraws somewhere;
SeqTrainBatcher on both sides of its guard)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("make_golden_batchers", os.path.join(ROOT, "tools", "make_golden_batchers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def got(recorder):
    return recorder.collect()


@pytest.fixture(scope="module")
def want(recorder):
    with open(recorder.OUT) as f:
        return json.load(f)


@pytest.mark.parametrize("section", ["train", "eval", "errors"])
def test_every_case_equals_the_recording(got, want, section):
    assert sorted(got[section]) == sorted(want[section])
    wrong = {k: (got[section][k], want[section][k]) for k in want[section] if got[section][k] != want[section][k]}
    assert not wrong, "\n".join(f"{section}/{k}: got {g}, recorded {w}" for k, (g, w) in wrong.items())


def test_the_recording_is_reproduced_byte_for_byte(recorder, got):
    with open(recorder.OUT) as f:
        assert recorder.dumps(got) == f.read()
