"""records.ShuffleBatcher.next_indices: the picks behind next_batch, batch for
batch, from the same RNG draws, ending at the same call."""
import numpy as np
import pytest

from mog_air.records import ShuffleBatcher


def _set(n=150, width=7):
    rng = np.random.default_rng(3)
    images = rng.uniform(size=(n, width)).astype(np.float32)
    images[:, 0] = np.arange(n)  # every row identifies itself
    return images, rng.integers(0, 4, n).astype(np.int32)


def test_next_indices_are_the_picks_of_next_batch():
    images, digits = _set()
    a = ShuffleBatcher(images, digits, 64, 3, min_after_dequeue=100, seed=77)
    b = ShuffleBatcher(images, digits, 64, 3, min_after_dequeue=100, seed=77)
    calls = 0
    while True:
        try:
            x, k = a.next_batch()
        except StopIteration:
            with pytest.raises(StopIteration):
                b.next_indices()
            break
        idx = b.next_indices()
        calls += 1
        assert idx.shape == (64,) and idx.min() >= 0 and idx.max() < 150
        np.testing.assert_array_equal(x[:, 0], idx.astype(np.float32))
        np.testing.assert_array_equal(x, images[idx])
        np.testing.assert_array_equal(k, digits[idx])
        assert k.dtype == np.int32
    assert calls == (150 * 3) // 64  # 450 examples: 7 full batches, then the end


def test_next_batch_is_unchanged_by_the_split():
    """next_batch still draws from the RNG exactly as the single-method form
    did: a hand-rolled copy of the queue gives the same picks."""
    images, digits = _set()
    a = ShuffleBatcher(images, digits, 64, 3, min_after_dequeue=100, seed=5)
    rng = np.random.default_rng(5)
    src = iter([i for _ in range(3) for i in range(150)])
    buf = []
    for _ in range(3):
        while len(buf) < 164:
            try:
                buf.append(next(src))
            except StopIteration:
                break
        picks = []
        for _ in range(64):
            j = int(rng.integers(len(buf)))
            buf[j], buf[-1] = buf[-1], buf[j]
            picks.append(buf.pop())
        x, _ = a.next_batch()
        np.testing.assert_array_equal(x[:, 0], np.asarray(picks, np.float32))
