"""The device canvas stream without a device: the NumPy restatement
(tests/synth_stream_ref.py) makes well-formed images and exhausts no regular
case, datasets.glyph_bank holds the glyphs datasets.synthesize places,
records.StreamFeed's state round-trips, the trainers' new flags parse and
refuse what they must."""
import argparse
import functools

import numpy as np
import pytest

from mog_air import datasets, records, trainer

import synth_stream_ref as ref

N = 2000
SEED = 12345
# (kind, bbox, counts): the regular cases
CASES = [("mnist", False, (1, 3)), ("mnist", False, (0, 2)), ("mnist", False, (2, 4)),
         ("mnist", True, (3,)), ("dsprites", False, (2, 4)), ("dsprites", False, (1, 3))]


@functools.lru_cache(maxsize=None)
def _bank(kind, bbox):
    return datasets.glyph_bank(kind, bbox=bbox)


@functools.lru_cache(maxsize=None)
def _run(kind, bbox, counts):
    bank, sizes, _ = _bank(kind, bbox)
    return ref.synth_ref(bank, sizes, counts, 50 if kind == "mnist" else 64, SEED, 0, N)


def test_philox_words_match_the_published_vectors():
    """Random123's known answer for Philox4x32-10 with counter and key zero;
    the stream's tag takes it off the models' counters."""
    w = ref.philox_words(0, [0], tag=0)[0]
    assert [int(v) for v in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = (1 << 64) - 1
    assert ref.philox_words(ones, [ones, 2 ** 52 + 5]).max() < 2 ** 32
    assert ref.STREAM_TAG != 0
    assert not np.array_equal(ref.philox_words(7, [5], tag=0), ref.philox_words(7, [5]))


@pytest.mark.parametrize("kind,bbox,counts", [CASES[0], CASES[3], CASES[4]])
def test_restated_images_are_well_formed(kind, bbox, counts):
    bank, sizes, _ = _bank(kind, bbox)
    C = 50 if kind == "mnist" else 64
    images, digits, objects, status, _ = _run(kind, bbox, counts)
    assert images.shape == (N, C * C) and images.min() >= 0.0 and images.max() <= 1.0
    assert set(digits.tolist()) == set(counts)  # every count of -dn appears
    assert np.array_equal(digits, (objects[:, :, 0] >= 0).sum(axis=1))
    for i in range(N):
        total = np.zeros((C, C), np.float32)
        taken = np.zeros((C, C), bool)
        for g, x, y, w, h in objects[i, :digits[i]]:
            assert 0 <= g < len(bank) and (h, w) == tuple(sizes[g])
            assert 0 <= x and x + w <= C and 0 <= y and y + h <= C
            glyph = bank[g, :h, :w]
            assert not (taken[y:y + h, x:x + w] & (glyph > 0)).any()
            taken[y:y + h, x:x + w] |= glyph > 0
            total[y:y + h, x:x + w] += glyph
        assert np.all(objects[i, digits[i]:] == -1)
        assert np.array_equal(images[i], np.clip(total, 0, 1).ravel())


@pytest.mark.parametrize("kind,bbox,counts", CASES)
def test_no_regular_case_exhausts_its_restarts(kind, bbox, counts):
    _, digits, _, status, _ = _run(kind, bbox, counts)
    assert not status.any()
    assert set(digits.tolist()) == set(counts)


def test_stream_is_a_function_of_seed_and_image_number():
    bank, sizes, _ = _bank("mnist", False)
    whole = _run("mnist", False, (1, 3))
    part = ref.synth_ref(bank, sizes, (1, 3), 50, SEED, 37, 9)
    for a, b in zip(whole[:4], part[:4]):
        assert np.array_equal(a[37:46], b)
    other = ref.synth_ref(bank, sizes, (1, 3), 50, SEED + 1, 37, 9)
    assert not np.array_equal(other[0], part[0])


@pytest.mark.parametrize("kind,bbox", [("mnist", False), ("mnist", True), ("dsprites", False)])
def test_glyph_bank_holds_the_glyphs_synthesize_draws(kind, bbox):
    bank, sizes, labels = _bank(kind, bbox)
    rng = np.random.default_rng(0)
    if kind == "mnist":
        glyphs = datasets.stroke_glyphs(512, rng, *((11, 15) if bbox else (17, 23)))
        want_labels = rng.integers(0, 10, 512)
    else:
        import os
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data",
                            "multi_dsprites", "data.npz")
        glyphs, lab = datasets.dsprite_glyphs(path)
        want_labels = lab[:, 1] if lab.ndim == 2 else lab
    assert bank.shape == (len(glyphs), 32, 32) and bank.dtype == np.float32
    assert sizes.shape == (len(glyphs), 2) and sizes.dtype == np.int32
    assert np.array_equal(labels, want_labels)
    for i, glyph in enumerate(glyphs):
        # (the stroke glyphs are float64; a float32 canvas holds their rounding)
        g = datasets.crop_non_empty(glyph).astype(np.float32)
        assert tuple(sizes[i]) == g.shape
        assert np.array_equal(bank[i, :g.shape[0], :g.shape[1]], g)
        assert np.count_nonzero(bank[i]) == np.count_nonzero(g)  # zero padded
    assert sizes.max() <= {("mnist", False): 21, ("mnist", True): 15,
                           ("dsprites", False): 26}[(kind, bbox)]
    # the test set of the trainers is made of these glyphs
    sets = datasets.synthesize(kind, [1], 3, test_set_size=1, seed=0, bbox=bbox)
    row = sets["test"]
    g0, (x, y), (w, h) = row["indices"][0][0], row["positions"][0], row["boxes"][0]
    assert np.array_equal(row["images"][0][y:y + h, x:x + w], bank[g0, :h, :w])


def test_stream_feed_state_round_trips_without_a_device():
    bank, sizes, _ = _bank("mnist", True)
    feed = records.StreamFeed(bank, sizes, [1, 3], 50, 96, seed=7, rank=1, world=4)
    st = feed.get_state()
    assert st["kind"] == "stream" and st["next"] == 0
    assert st["buf"].dtype == np.int64 and st["buf"].size == 0
    assert feed._shard() == (24, 48)
    feed.set_state({"kind": "stream", "next": 960, "buf": np.zeros((0,), np.int64)})
    assert feed.get_state()["next"] == 960
    other = records.StreamFeed(bank, sizes, [1, 3], 50, 96, seed=7)
    other.set_state({k: v for k, v in feed.get_state().items()})
    assert other.get_state()["next"] == 960
    assert other.fingerprint() == feed.fingerprint()  # ranks do not enter
    import json
    assert json.loads(json.dumps(feed.fingerprint())) == feed.fingerprint()
    for changed in (records.StreamFeed(bank, sizes, [1, 3], 50, 96, seed=8),
                    records.StreamFeed(bank, sizes, [1, 2], 50, 96, seed=7),
                    records.StreamFeed(bank, sizes, [1, 3], 64, 96, seed=7),
                    records.StreamFeed(bank[:-1], sizes[:-1], [1, 3], 50, 96, seed=7),
                    records.StreamFeed(bank * 0.5, sizes, [1, 3], 50, 96, seed=7)):
        assert changed.fingerprint() != feed.fingerprint()
    with pytest.raises(ValueError):
        feed.set_state({"rng": {}, "buf": np.zeros((0,), np.int64), "epoch": 0, "index": 0})
    with pytest.raises(ValueError):
        feed.set_state({"kind": "stream", "next": -1, "buf": np.zeros((0,), np.int64)})


def _parse(argv):
    p = argparse.ArgumentParser()
    trainer.add_common_args(p, reader_threads=4)
    return p.parse_args(argv)


def test_new_flags_parse_and_default_to_today():
    args = _parse([])
    assert (args.batch_size, args.stream, args.stream_seed) == (64, 0, 12345)
    args = _parse(["--batch-size", "8192", "--stream", "1", "--stream-seed", "9",
                   "--iterations", "5"])
    assert (args.batch_size, args.stream, args.stream_seed) == (8192, 1, 9)
    with pytest.raises(SystemExit):
        _parse(["--stream", "2"])


def test_stream_refusals(tmp_path):
    absent = (str(tmp_path / "common13.tfrecords"), str(tmp_path / "test13.tfrecords"))
    trainer.check_feed_args(_parse([]), *absent)
    trainer.check_feed_args(_parse(["--stream", "1", "--iterations", "4"]), *absent)
    with pytest.raises(ValueError, match="needs --iterations"):
        trainer.check_feed_args(_parse(["--stream", "1"]), *absent)
    with pytest.raises(ValueError, match="--batch-size"):
        trainer.check_feed_args(_parse(["--batch-size", "0"]), *absent)
    open(absent[1], "wb").close()
    with pytest.raises(ValueError, match="exist"):
        trainer.check_feed_args(_parse(["--stream", "1", "--iterations", "4"]), *absent)
    trainer.check_feed_args(_parse(["--iterations", "4"]), *absent)  # --stream 0: as before


def test_make_feed_takes_the_batch_size():
    x = np.zeros((300, 4), np.float32)
    k = np.arange(300, dtype=np.int32) % 3
    args = _parse(["--batch-size", "128"])
    feed = trainer.make_feed(args, x, k, trainer.Dist(1, 2), resident=False)
    xb, kb, n = feed.next_batch()
    assert n == 128 and len(kb) == 64
    # a caller without the flag (an older argument namespace) keeps 64
    feed = trainer.make_feed(argparse.Namespace(), x, k, trainer.Dist(), resident=False)
    assert feed.next_batch()[2] == 64
