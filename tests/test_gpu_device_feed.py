"""The device batch feed: ops.gather_rows (csrc/gather_rows.hip) against
index_select, records.DeviceFeed against records.ShuffleBatcher."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("rows,width", [(37, 2500), (5, 4096), (9, 30), (9, 31)])
@pytest.mark.parametrize("B", [1, 13, 64])
def test_gather_rows_matches_index_select(rows, width, B):
    """16-byte rows (2500, 4096 floats) and the dword path (30: rows not
    16-byte multiples; 31: odd); repeats, row 0 and the last row among the
    picks; rows of the output beyond B untouched."""
    from mog_air import ops
    g = torch.Generator().manual_seed(rows * 131 + B)
    src = torch.randn(rows, width, generator=g).to(DEV)
    ksrc = torch.randint(0, 9, (rows,), generator=g, dtype=torch.int32).to(DEV)
    idx = torch.randint(0, rows, (B,), generator=g)
    idx[0] = rows - 1
    if B > 2:
        idx[1], idx[2], idx[-1] = 0, 0, rows - 1
    out = torch.full((B + 3, width), float("nan"), device=DEV)
    kout = torch.full((B + 3,), -7, dtype=torch.int32, device=DEV)
    ops.gather_rows(src, idx.numpy(), out, ksrc=ksrc, kout=kout)
    want = src.index_select(0, idx.to(DEV))
    assert torch.equal(out[:B].view(torch.int32), want.view(torch.int32))
    assert torch.equal(kout[:B], ksrc.index_select(0, idx.to(DEV)))
    assert torch.isnan(out[B:]).all() and (kout[B:] == -7).all()
    # without the digit counts
    out2 = torch.empty(B, width, device=DEV)
    ops.gather_rows(src, idx, out2)
    assert torch.equal(out2, want)


def test_gather_rows_refusals():
    from mog_air import ops
    src = torch.zeros(5, 8, device=DEV)
    out = torch.full((4, 8), float("nan"), device=DEV)
    for bad in ([0, 5], [-1, 2]):
        with pytest.raises(ValueError):
            ops.gather_rows(src, bad, out)
    assert torch.isnan(out).all()  # nothing was launched
    with pytest.raises(ValueError):
        ops.gather_rows(src.cpu(), [0], out)
    with pytest.raises(ValueError):
        ops.gather_rows(src, [0, 1, 2, 3, 4], out)          # more picks than output rows
    with pytest.raises(ValueError):
        ops.gather_rows(src, [0], torch.zeros(4, 7, device=DEV))
    with pytest.raises(ValueError):
        ops.gather_rows(src.double(), [0], out)
    with pytest.raises(ValueError):
        ops.gather_rows(src, [0], out, ksrc=torch.zeros(5, dtype=torch.int32, device=DEV))


def _set(n=150, width=2500):
    rng = np.random.default_rng(11)
    return (rng.uniform(size=(n, width)).astype(np.float32),
            rng.integers(0, 4, n).astype(np.int32))


def test_device_feed_is_the_shuffle_batcher():
    from mog_air.records import DeviceFeed, ShuffleBatcher
    images, digits = _set()
    host = ShuffleBatcher(images, digits, 64, 3, min_after_dequeue=100, seed=9)
    feed = DeviceFeed(images, digits, 64, 3, min_after_dequeue=100, seed=9, device=DEV)
    prev = None
    calls = 0
    while True:
        try:
            hx, hk = host.next_batch()
        except StopIteration:
            with pytest.raises(StopIteration):
                feed.next_batch()
            break
        x, k, nglobal = feed.next_batch()
        calls += 1
        assert nglobal == 64 and x.is_cuda and x.dtype == torch.float32 and k.dtype == torch.int32
        assert x.cpu().numpy().tobytes() == hx.tobytes()
        assert k.cpu().numpy().tobytes() == hk.tobytes()
        if prev is not None:  # the previous batch is not overwritten by this one
            assert prev[0].cpu().numpy().tobytes() == prev[2].tobytes()
            assert prev[1].cpu().numpy().tobytes() == prev[3].tobytes()
            assert prev[0].data_ptr() != x.data_ptr()
        prev = (x, k, hx, hk)
    assert calls == 7


def test_device_feed_shards_like_dist():
    from mog_air.records import DeviceFeed, ShuffleBatcher
    from mog_air.trainer import Dist
    images, digits = _set()
    # 63: a global batch the two ranks do not split evenly
    for batch in (64, 63):
        host = ShuffleBatcher(images, digits, batch, 1, min_after_dequeue=100, seed=4)
        feeds = [DeviceFeed(images, digits, batch, 1, min_after_dequeue=100, seed=4, device=DEV,
                            rank=r, world=2) for r in range(2)]
        for _ in range(2):
            hx, hk = host.next_batch()
            for r, feed in enumerate(feeds):
                sx, sk = Dist(r, 2).shard(hx, hk)
                x, k, nglobal = feed.next_batch()
                assert nglobal == batch and x.shape[0] == len(sk)
                assert x.cpu().numpy().tobytes() == sx.tobytes()
                assert k.cpu().numpy().tobytes() == sk.tobytes()
