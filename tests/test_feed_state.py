"""records.ShuffleBatcher.get_state / set_state: a new batcher given a saved
state yields the same picks to the same StopIteration as the one it was taken
from.  37 examples, batches of 5, a queue of 10 and 3 epochs: the smallest
case in which the buffer spans an epoch boundary (batch 6 is filled from rows
of two passes) and the stream runs dry while batches are still drawn (111
examples: 22 batches, the last two from the draining buffer)."""
import json

import numpy as np
import pytest

from mog_air.records import ShuffleBatcher

N, BATCH, QUEUE, EPOCHS = 37, 5, 10, 3
TOTAL = (N * EPOCHS) // BATCH  # 22 batches, then StopIteration


def _batcher(seed=77):
    images = np.arange(N, dtype=np.float32)[:, None] * np.ones((1, 3), np.float32)
    digits = (np.arange(N) % 4).astype(np.int32)
    return ShuffleBatcher(images, digits, BATCH, EPOCHS, min_after_dequeue=QUEUE, seed=seed)


def _drain(b):
    out = []
    while True:
        try:
            out.append(b.next_indices())
        except StopIteration:
            return out


@pytest.fixture(scope="module")
def reference():
    """The uninterrupted run's picks, computed once."""
    picks = _drain(_batcher())
    assert len(picks) == TOTAL
    return picks


def _advance(n):
    b = _batcher()
    for _ in range(n):
        b.next_indices()
    return b


# After batch k >= 1 the queue has taken 5 k + 10 examples from the stream and
# holds 10.  Batch 0; mid-epoch; 35 taken, so the next fill crosses from pass 0
# (rows 35, 36) into pass 1; the stream dry (111 taken) and the buffer
# draining; after the last batch.
SNAPSHOTS = [0, 3, 5, 21, TOTAL]


def test_snapshots_cover_the_cases():
    s = _advance(0).get_state()
    assert s["buf"].size == 0 and (s["epoch"], s["index"], s["exhausted"]) == (0, 0, False)
    s = _advance(3).get_state()
    assert s["buf"].size == QUEUE and (s["epoch"], s["index"], s["exhausted"]) == (0, 25, False)
    s = _advance(5).get_state()
    assert s["buf"].size == QUEUE and (s["epoch"], s["index"], s["exhausted"]) == (0, 35, False)
    s = _advance(6).get_state()
    assert (s["epoch"], s["index"]) == (1, 3)
    s = _advance(21).get_state()
    assert s["exhausted"] and s["buf"].size == 6 and s["epoch"] == EPOCHS
    s = _advance(TOTAL).get_state()
    assert s["exhausted"] and s["buf"].size == N * EPOCHS - TOTAL * BATCH == 1


@pytest.mark.parametrize("at", SNAPSHOTS)
def test_set_state_continues_the_picks(reference, at):
    state = _advance(at).get_state()
    fresh = _batcher(seed=5)  # another seed: everything must come from the state
    fresh.set_state(state)
    rest = _drain(fresh)
    assert len(rest) == TOTAL - at
    for got, want in zip(rest, reference[at:]):
        np.testing.assert_array_equal(got, want)
    with pytest.raises(StopIteration):
        fresh.next_indices()


@pytest.mark.parametrize("at", SNAPSHOTS)
def test_state_survives_npz_without_pickle(tmp_path, reference, at):
    state = _advance(at).get_state()
    buf = state.pop("buf")
    path = tmp_path / "feed.npz"
    np.savez(path, buf=buf, meta=np.array(json.dumps(state)))
    with np.load(path, allow_pickle=False) as z:
        loaded = dict(json.loads(str(z["meta"])), buf=z["buf"])
    assert loaded["rng"]["state"] == state["rng"]["state"]  # 128 bits, as a decimal string
    assert int(loaded["rng"]["state"]) >= 0
    fresh = _batcher(seed=5)
    fresh.set_state(loaded)
    for got, want in zip(_drain(fresh), reference[at:]):
        np.testing.assert_array_equal(got, want)
    again = fresh.get_state()
    assert again["exhausted"] and again["buf"].size == N * EPOCHS - TOTAL * BATCH


def test_next_batch_after_set_state_gathers_the_same_rows(reference):
    b = _advance(5)
    fresh = _batcher(seed=5)
    fresh.set_state(b.get_state())
    x, k = fresh.next_batch()
    np.testing.assert_array_equal(x[:, 0], reference[5].astype(np.float32))
    np.testing.assert_array_equal(k, (reference[5] % 4).astype(np.int32))


def test_set_state_refuses_a_state_of_another_dataset():
    state = _advance(6).get_state()
    images = np.zeros((8, 3), np.float32)
    small = ShuffleBatcher(images, np.zeros(8, np.int32), BATCH, EPOCHS, min_after_dequeue=QUEUE)
    before = small.get_state()
    with pytest.raises(ValueError, match="outside this dataset"):
        small.set_state(state)
    after = small.get_state()
    assert after["rng"] == before["rng"] and after["buf"].size == 0


def test_fingerprint_tells_datasets_apart():
    a, b = _batcher(), _batcher()
    assert a.fingerprint() == b.fingerprint() == {"examples": N,
                                                  "digits_crc32": a.fingerprint()["digits_crc32"]}
    b.digits = b.digits.copy()
    b.digits[3] += 1
    assert a.fingerprint() != b.fingerprint()
