"""ops.synth_canvases (csrc/synth.hip) and records.StreamFeed against the NumPy
restatement of the stream (tests/synth_stream_ref.py): every output bit for
bit, for the regular banks, for a crafted bank that reaches the restart and
exhaust paths, for batch sizes that leave waves and workgroups partly empty,
across a split launch and across runs; the wrapper's refusals; the feed's
shards, state and fresh tensors."""
import functools

import numpy as np
import pytest
import torch

import synth_stream_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 12345
HIGH = 2 ** 40 + 5  # an image number whose counter has a high word


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


@functools.lru_cache(maxsize=None)
def _bank(kind, bbox=False):
    from mog_air import datasets
    return datasets.glyph_bank(kind, bbox=bbox)[:2]


def _square_bank():
    bank = np.zeros((1, 32, 32), np.float32)
    bank[0, :20, :20] = 1.0
    return bank, np.array([[20, 20]], np.int32)


@functools.lru_cache(maxsize=None)
def _want(kind, bbox, counts, canvas, seed, first, b):
    bank, sizes = _square_bank() if kind == "square" else _bank(kind, bbox)
    return ref.synth_ref(bank, sizes, counts, canvas, seed, first, b)


def _device(bank, sizes, counts, canvas, seed, first, b):
    from mog_air import ops
    sb = ops.SynthBank(bank, sizes, counts, canvas, DEV)
    x = torch.full((b, canvas * canvas), -7.0, device=DEV)
    k, o, s = (torch.full(shape, -7, dtype=torch.int32, device=DEV)
               for shape in ((b,), (b, 8, 5), (b,)))
    ops.synth_canvases(sb, seed, first, x, k, o, s)
    return tuple(t.cpu().numpy() for t in (x, k, o, s))


def _assert_equal(got, want):
    for g, w, name in zip(got, want, ("images", "digits", "objects", "status")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), (name, np.argwhere(g != w)[:5])


@pytest.mark.parametrize("first", [0, HIGH])
@pytest.mark.parametrize("kind,bbox,counts,canvas", [
    ("mnist", False, (1, 3), 50), ("mnist", False, (0, 2), 50), ("mnist", True, (3,), 50),
    ("dsprites", False, (2, 4), 64)])
def test_bit_exact_against_the_restatement(kind, bbox, counts, canvas, first):
    want = _want(kind, bbox, counts, canvas, SEED, first, 64)
    assert not want[3].any() and set(want[1].tolist()) == set(counts)
    _assert_equal(_device(*_bank(kind, bbox), counts, canvas, SEED, first, 64), want)


def test_restart_and_exhaust_paths_on_a_crowded_canvas():
    """Four solid 20 x 20 squares on 50 x 50 pixels: the only coverage of the
    restart and exhaust paths (at most 8 * 4 * 100 attempts per image)."""
    want = _want("square", False, (4,), 50, 1, 0, 64)
    status, restarts = want[3], want[4]["restarts"]
    assert ((status == 0) & (restarts == 0)).any()  # placed at once
    assert ((status == 0) & (restarts > 0)).any()   # placed after a restart
    assert (status == 1).any() and (want[1][status == 1] < 4).all()  # exhausted: fewer objects
    assert max(want[4]["attempts"]) >= 50           # a late attempt accepted
    _assert_equal(_device(*_square_bank(), (4,), 50, 1, 0, 64), want)


@pytest.mark.parametrize("b", [1, 5, 67])
def test_batches_that_fill_no_whole_workgroup(b):
    want = _want("mnist", False, (1, 3), 50, SEED, 3, 67)
    got = _device(*_bank("mnist"), (1, 3), 50, SEED, 3, b)
    _assert_equal(got, tuple(w[:b] for w in want[:4]))


def test_odd_canvas_takes_the_dword_stores():
    """C * C = 2601 is no multiple of 4: the kernel's other store path."""
    want = _want("mnist", True, (1, 3), 51, SEED, 0, 9)
    _assert_equal(_device(*_bank("mnist", True), (1, 3), 51, SEED, 0, 9), want)


def test_split_launch_and_repeat_give_the_same_bits():
    args = _bank("dsprites") + ((2, 4), 64, SEED)
    whole = _device(*args, HIGH, 67)
    again = _device(*args, HIGH, 67)
    head, tail = _device(*args, HIGH, 29), _device(*args, HIGH + 29, 38)
    for w, a, h, t in zip(whole, again, head, tail):
        assert w.tobytes() == a.tobytes()
        assert w.tobytes() == np.concatenate([h, t]).tobytes()


def test_refusals_leave_the_outputs_untouched():
    from mog_air import ops
    bank, sizes = _bank("mnist")
    for bad in (lambda: ops.SynthBank(bank[:, :31], sizes, [1], 50, DEV),        # bank side
                lambda: ops.SynthBank(bank, sizes * 0, [1], 50, DEV),            # h, w = 0
                lambda: ops.SynthBank(bank, sizes + 12, [1], 50, DEV),           # h, w > 32
                lambda: ops.SynthBank(np.zeros((1, 32, 32), np.float32),
                                      np.array([[32, 33]], np.int32), [1], 64, DEV),
                lambda: ops.SynthBank(bank, sizes, [1], 31, DEV),                # canvas
                lambda: ops.SynthBank(bank, sizes, [1], 65, DEV),
                lambda: ops.SynthBank(bank, sizes, [9], 50, DEV),                # count > GMAX
                lambda: ops.SynthBank(bank, sizes, [-1], 50, DEV),
                lambda: ops.SynthBank(bank, sizes, [], 50, DEV),
                lambda: ops.SynthBank(bank[:0], sizes[:0], [1], 50, DEV),        # G < 1
                lambda: ops.SynthBank(bank.astype(np.float64), sizes, [1], 50, DEV),
                lambda: ops.SynthBank(bank, sizes.astype(np.int64), [1], 50, DEV),
                lambda: ops.SynthBank(bank[:, :, ::-1], sizes, [1], 50, DEV),    # not contiguous
                lambda: ops.SynthBank(bank, sizes, [1.0], 50, DEV),
                lambda: ops.SynthBank(bank, sizes, [1], 50, "cpu")):
        with pytest.raises(ValueError):
            bad()
    sb = ops.SynthBank(bank, sizes, [1, 3], 50, DEV)

    def outputs():
        return [torch.full((6, 2500), -7.0, device=DEV)] + [
            torch.full(shape, -7, dtype=torch.int32, device=DEV)
            for shape in ((6,), (6, 8, 5), (6,))]

    x, k, o, s = outs = outputs()
    for call in (lambda: ops.synth_canvases(sb, 1, 0, x[:, :2499], k, o, s),
                 lambda: ops.synth_canvases(sb, 1, 0, x[:, ::2], k, o, s),
                 lambda: ops.synth_canvases(sb, 1, 0, x.double(), k, o, s),
                 lambda: ops.synth_canvases(sb, 1, 0, x, k.long(), o, s),
                 lambda: ops.synth_canvases(sb, 1, 0, x, k[:5], o, s),
                 lambda: ops.synth_canvases(sb, 1, 0, x, k, o[:, :7], s),
                 lambda: ops.synth_canvases(sb, 1, 0, x, k, o, s.cpu()),
                 lambda: ops.synth_canvases(sb, 1, 0, x.cpu(), k, o, s),
                 lambda: ops.synth_canvases(sb, 1, -1, x, k, o, s),
                 lambda: ops.synth_canvases(sb, 1, 2 ** 52 - 5, x, k, o, s),
                 lambda: ops.synth_canvases(sb, -1, 0, x, k, o, s),
                 lambda: ops.synth_canvases(sb, 2 ** 64, 0, x, k, o, s),
                 lambda: ops.synth_canvases((bank, sizes), 1, 0, x, k, o, s)):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == -7).all())
    # the operator itself refuses extents its launch would overrun
    with pytest.raises(RuntimeError):
        torch.ops.mog_air.synth_canvases_(sb.bank, sb.sizes, sb.G, sb.counts, 2, 50, 1, 0, 7,
                                          x, k, o, s)
    with pytest.raises(RuntimeError):
        torch.ops.mog_air.synth_canvases_(sb.bank, sb.sizes, sb.G + 1, sb.counts, 2, 50, 1, 0, 6,
                                          x, k, o, s)
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == -7).all())
    ops.synth_canvases(sb, 2 ** 64 - 1, 2 ** 52 - 6, x, k, o, s)  # the last images there are
    assert bool((k >= 1).all())


# ------------------------------------------------------------- StreamFeed ----
def _feed(batch, rank=0, world=1, seed=SEED):
    from mog_air import records
    bank, sizes = _bank("mnist")
    return records.StreamFeed(bank, sizes, [1, 3], 50, batch, seed=seed, device=DEV, rank=rank,
                              world=world)


def _host(feed):
    x, k, n = feed.next_batch()
    return x.cpu().numpy(), k.cpu().numpy(), feed.objects.cpu().numpy(), feed.status.cpu().numpy()


def test_feed_shards_concatenate_to_the_global_batch():
    want = _want("mnist", False, (1, 3), 50, SEED, 0, 26)  # two global batches of 13
    one, halves = _feed(13), [_feed(13, r, 2) for r in range(2)]
    for i in range(2):
        whole = _host(one)
        parts = [_host(f) for f in halves]
        assert [len(p[1]) for p in parts] == [7, 6]
        _assert_equal(whole, tuple(w[13 * i:13 * i + 13] for w in want[:4]))
        for w, a, b in zip(whole, *parts):
            assert w.tobytes() == np.concatenate([a, b]).tobytes()
    x, k, n = halves[1].next_batch()
    assert n == 13 and x.is_cuda and x.dtype == torch.float32 and k.dtype == torch.int32


def test_feed_state_continues_the_stream():
    straight = _feed(13)
    batches = [_host(straight) for _ in range(4)]
    first = _feed(13)
    for i in range(2):
        _host(first)
    state = first.get_state()
    assert state["next"] == 26
    resumed = _feed(13, 1, 2)  # another number of ranks: the same global batches
    resumed.set_state(state)
    other = _feed(13, 0, 2)
    other.set_state(state)
    for i in (2, 3):
        a, b = _host(other), _host(resumed)
        for w, p, q in zip(batches[i], a, b):
            assert w.tobytes() == np.concatenate([p, q]).tobytes()
    assert resumed.get_state()["next"] == straight.get_state()["next"] == 52


def test_feed_batches_are_fresh_tensors():
    feed = _feed(13)
    x0, k0, _ = feed.next_batch()
    keep_x, keep_k, keep_o = x0.clone(), k0.clone(), feed.objects.clone()
    o0 = feed.objects
    x1, k1, _ = feed.next_batch()
    torch.cuda.synchronize()
    assert x1.data_ptr() != x0.data_ptr() and k1.data_ptr() != k0.data_ptr()
    assert feed.objects.data_ptr() != o0.data_ptr()
    assert torch.equal(x0, keep_x) and torch.equal(k0, keep_k) and torch.equal(o0, keep_o)
    assert not torch.equal(x1, x0)
