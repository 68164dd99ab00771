"""mog_air.checkpoint on the device: a run stopped at step N, saved, loaded
into fresh models and continued equals the uninterrupted run bit for bit
 -- AIR in every configuration, eager and through the
captured graph; AIR-ASR as far as its step is deterministic; and the
refusals, which leave the model untouched.

Every comparison is preceded by its control: two uninterrupted runs of the
configuration from one seed agree bit for bit.  A failing control is
nondeterminism of the step itself, not of the restore."""
import warnings

import numpy as np
import pytest
import torch

import ckpt_cases as cc

pytestmark = pytest.mark.gpu

N = 3  # steps before the save, and after it


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _steps(model, data):
    return [model.step(x, k)[:3] for x, k in data]


def _uninterrupted(pair, path, step=_steps):
    """N steps, one test-model infer (so that its Philox offset is not 0 at
    the save), [save], N steps; then the test model's outputs."""
    train, test = pair
    data = cc.batches(2 * N)
    losses = step(train, data[:N])
    test.infer(*cc.fixed_batch())
    if path is not None:
        from mog_air import checkpoint
        checkpoint.save_state(path, train, test)
    losses += step(train, data[N:])
    return losses, cc.snapshot(train, test), cc.infer_outputs(test)


@pytest.mark.parametrize("config", list(cc.AIR_CONFIGS))
def test_air_continuation_is_bitwise(tmp_path, config):
    from mog_air import checkpoint
    path = str(tmp_path / "air-state-3.npz")
    lx, sx, ox = _uninterrupted(cc.air_pair(config, "ck_x_" + config), path)
    # control: the same run again, without the save
    lc, sc, oc = _uninterrupted(cc.air_pair(config, "ck_c_" + config), None)
    assert lc == lx, "control: the step is not deterministic"
    cc.assert_same(sc, sx, "control")
    cc.assert_outputs_equal(oc, ox, "control")
    # a fresh pair under another scope and from another weight seed: all of
    # its state comes from the file
    train, test = cc.air_pair(config, "ck_r_" + config, seed=99)
    views = {n: train.params.view(n) for n, _ in train.params.specs[:2]}
    ptrs = [getattr(train.params, n).data_ptr() for n in ("flat", "m", "v")]
    version = train.params.version
    assert checkpoint.load_state(path, train, test) is None  # no loop was saved
    assert train.params.version > version
    assert ptrs == [getattr(train.params, n).data_ptr() for n in ("flat", "m", "v")]
    assert all(train.params.view(n) is v for n, v in views.items())  # loaded in place
    assert train.global_step == N and test.global_step == N
    # the annealed prior has moved with the restored global_step
    assert train.hyper("z_pres_prior_log_odds") < float(np.log(np.float32(10000.0))) - 1.0
    lr = _steps(train, cc.batches(2 * N)[N:])
    assert lr == lx[N:], (lr, lx[N:])
    cc.assert_same(cc.snapshot(train, test), sx, "resumed")
    cc.assert_outputs_equal(cc.infer_outputs(test), ox, "resumed")


def _graphed(model, data):
    out = []
    for x, k in data:
        model.train_step_graphed(x, k)
        out.append(tuple(model._ws.means[:3].cpu().tolist()))
    return out


def test_captured_graph_continuation_is_bitwise(tmp_path):
    """Capture, 2 graphed steps, save, 2 more: X.  Loading into the SAME
    model (its graph holds raw pointers into the buffers that are loaded in
    place) and into a fresh one, then 2 graphed steps, gives X."""
    from mog_air import checkpoint
    path = str(tmp_path / "air-state-2.npz")
    data = cc.batches(4)
    train, test = cc.air_pair("fp32", "ckg_x")
    lx = _graphed(train, data[:2])
    assert train._graph is not None
    checkpoint.save_state(path, train, test)
    lx += _graphed(train, data[2:])
    sx = cc.snapshot(train, test)
    # control
    ctrain, ctest = cc.air_pair("fp32", "ckg_c")
    assert _graphed(ctrain, data) == lx, "control: the graphed step is not deterministic"
    cc.assert_same(cc.snapshot(ctrain, ctest), sx, "control")
    # the same model, its graph kept
    graph = train._graph
    checkpoint.load_state(path, train, test)
    assert train.global_step == 2
    assert _graphed(train, data[2:]) == lx[2:]
    assert train._graph is graph  # replayed, not captured again
    cc.assert_same(cc.snapshot(train, test), sx, "same model")
    # a fresh model: its first graphed step is the eager one + capture
    ftrain, ftest = cc.air_pair("fp32", "ckg_f", seed=99)
    checkpoint.load_state(path, ftrain, ftest)
    assert _graphed(ftrain, data[2:]) == lx[2:]
    assert ftrain._graph is not None
    cc.assert_same(cc.snapshot(ftrain, ftest), sx, "fresh model")


def _files_equal(a, b):
    from mog_air import checkpoint
    (aa, am), (ba, bm) = checkpoint.read_file(a), checkpoint.read_file(b)
    assert am == bm
    assert sorted(aa) == sorted(ba)
    for k in aa:
        assert aa[k].dtype == ba[k].dtype and aa[k].tobytes() == ba[k].tobytes(), k


def test_asr_state_round_trip_and_deterministic_part(tmp_path):
    """AIR-ASR's per-step head gradients use float atomics, so
    the parameters after a step are not claimed bit-equal.  What is
    deterministic: the file round trip, the first resumed step's forward
    (log_variables) and the counters of every following step.  When the
    control finds the step bit-deterministic at this shape, the full bitwise
    check runs too."""
    from mog_air import checkpoint
    path, again = str(tmp_path / "air-state-3.npz"), str(tmp_path / "again" / "air-state-3.npz")
    (tmp_path / "again").mkdir()
    data = cc.batches(2 * N)

    def run(pair, save):
        train, test = pair
        _steps(train, data[:N])
        test.infer(*cc.fixed_batch())
        if save:
            checkpoint.save_state(path, train, test)
        logs, counters = [], []
        for x, k in data[N:]:
            train.step(x, k)
            logs.append(train.log_variables)
            counters.append((train.global_step, train.params.adam_t, train._noise_ctr))
        return logs, counters, cc.snapshot(train, test)

    lx, cx, sx = run(cc.asr_pair("cka_x"), True)
    lc, ccnt, sc = run(cc.asr_pair("cka_c"), False)
    assert ccnt == cx
    deterministic = lc == lx and all(np.array_equal(sc[n], sx[n]) for n in ("flat", "m", "v"))
    print("AIR-ASR control: the step is %sbit-deterministic at B = %d" % (
        "" if deterministic else "NOT ", cc.B))

    train, test = cc.asr_pair("cka_r", seed=99)
    checkpoint.load_state(path, train, test)
    checkpoint.save_state(again, train, test)
    _files_equal(path, again)
    logs, counters = [], []
    for x, k in data[N:]:
        train.step(x, k)
        logs.append(train.log_variables)
        counters.append((train.global_step, train.params.adam_t, train._noise_ctr))
    assert logs[0] == lx[0]  # computed in the forward, from the restored state alone
    assert counters == cx
    assert (np.float32(train.params.beta1_power).tobytes(), np.float32(
        train.params.beta2_power).tobytes()) == sx["scalars"][:2]
    assert test._noise_ctr == sx["scalars"][5]
    if deterministic:
        assert logs == lx
        cc.assert_same(cc.snapshot(train, test), sx, "resumed")


def _flat_bits(model):
    return {n: cc.bits(getattr(model.params, n)) for n in ("flat", "m", "v")}


def _assert_untouched(model, before, step, ctr):
    after = _flat_bits(model)
    for n in before:
        np.testing.assert_array_equal(before[n], after[n], err_msg=n)
    assert (model.global_step, model._noise_ctr) == (step, ctr)


@pytest.fixture(scope="module")
def air_state(tmp_path_factory):
    """A cnn=False AIR state after one step, written once."""
    from mog_air import checkpoint
    path = str(tmp_path_factory.mktemp("refusals") / "air-state-1.npz")
    train, test = cc.air_pair("fp32", "ckr_src")
    train.step(*cc.batches(1)[0])
    checkpoint.save_state(path, train, test)
    return path


def test_air_state_is_refused_by_an_asr_model(air_state):
    from mog_air import checkpoint
    train, test = cc.asr_pair("ckr_asr")
    train.step(*cc.batches(1)[0])
    before, step, ctr = _flat_bits(train), train.global_step, train._noise_ctr
    with pytest.raises(ValueError, match="air/air_model/infer_rnn_running/kernel"):
        checkpoint.load_state(air_state, train, test)
    with pytest.raises(ValueError, match="air/air_model/infer_rnn_running/kernel"):
        checkpoint.load_variables(air_state, train)
    _assert_untouched(train, before, step, ctr)


def test_cnn_false_state_is_refused_by_a_cnn_model(air_state):
    from mog_air import checkpoint
    train, test = cc.air_pair("cnn", "ckr_cnn")
    before, step, ctr = _flat_bits(train), train.global_step, train._noise_ctr
    # the LSTM kernel's rows are the encoder's features there, not the canvas
    with pytest.raises(ValueError, match="air/rnn/rnn/basic_lstm_cell/kernel with shape"):
        checkpoint.load_state(air_state, train, test)
    _assert_untouched(train, before, step, ctr)


def test_other_refusals_and_the_precision_warning(air_state, tmp_path):
    from mog_air import checkpoint
    train, test = cc.air_pair("fp32", "ckr_seed", noise_seed=23)
    before, step, ctr = _flat_bits(train), train.global_step, train._noise_ctr
    with pytest.raises(ValueError, match="noise_seed is 23"):
        checkpoint.load_state(air_state, train, test)

    class Two:
        rank, world = 0, 2
    train.noise_seed = test.noise_seed = 22
    with pytest.raises(ValueError, match="saved by 1 ranks, this run has 2"):
        checkpoint.load_state(air_state, train, test, ctx=Two())
    with pytest.raises(ValueError, match="no feed state"):
        from mog_air.records import ShuffleBatcher
        checkpoint.load_state(air_state, train, test, feed=ShuffleBatcher(
            np.zeros((4, 1), np.float32), np.zeros(4, np.int32), 2, 1, 2))
    _assert_untouched(train, before, step, ctr)
    # weights mode takes the variables alone, whatever the seeds
    train.noise_seed = 23
    checkpoint.load_state(air_state, train, test, mode="weights")
    assert train.global_step == 0 and train.params.adam_t == 0 and train._noise_ctr == ctr
    assert not np.array_equal(_flat_bits(train)["flat"], before["flat"])
    np.testing.assert_array_equal(_flat_bits(train)["m"], before["m"])
    # another precision only warns
    btrain, btest = cc.air_pair("bf16", "ckr_bf16")
    with pytest.warns(UserWarning, match="saved at precision fp32 and continues at bf16"):
        checkpoint.load_state(air_state, btrain, btest)
    assert btrain.global_step == 1
    ftrain, ftest = cc.air_pair("fp32", "ckr_same")
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the same precision: no warning
        checkpoint.load_state(air_state, ftrain, ftest)


def test_feed_and_loop_ride_along(tmp_path):
    """save_state with a feed and a loop state; load_state hands the loop
    back, continues the feed's picks and refuses another dataset."""
    from mog_air import checkpoint
    from mog_air.records import ShuffleBatcher

    def feed(n=37, seed=12345):
        return ShuffleBatcher(np.zeros((n, 1), np.float32), (np.arange(n) % 3).astype(np.int32),
                              5, 3, min_after_dequeue=10, seed=seed)
    train, test = cc.air_pair("fp32", "ckf_src")
    f = feed()
    for _ in range(6):
        f.next_indices()
    loop = {"step": 6, "rows": [[1.5, 0.25, float(np.float32(0.1))]], "best": [0.0] * 4}
    path = checkpoint.save_state(str(tmp_path / "air-state-6.npz"), train, test, feed=f, loop=loop)
    want = [f.next_indices() for _ in range(3)]
    g = feed(seed=1)
    assert checkpoint.load_state(path, train, test, feed=g) == loop
    for w in want:
        np.testing.assert_array_equal(g.next_indices(), w)
    with pytest.raises(ValueError, match="another dataset"):
        checkpoint.load_state(path, train, test, feed=feed(n=38))
    assert checkpoint.load_state(path, train, test, feed=None) == loop  # no fingerprint check
