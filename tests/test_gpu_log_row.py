"""The AIR-ASR log row on the device (ops.asr_log_row, csrc/log_row.hip), the
models' ``log_row_`` and ``trainer.LogRing``.

Kernel against tests/asr_log_row_ref.py on crafted tensors: bar (a) -- each
output within one fp32 spacing of the float64 value --, the copied entries bit
for bit, no NaN although every record row at t >= T_exec is NaN, two launches
equal, and every wrapper refusal before any launch.  ``log_row_`` against the
``log_variables`` property of the model bench.make_asr_model builds: bar (b),
the forward error of the property's own fp32 reductions, with sum|x| taken from
the workspace."""
import numpy as np
import pytest
import torch

import asr_log_row_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 6


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _dev(a):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in a.items()}


def _launch(d, out, **replace):
    from mog_air import ops
    args = dict(d, **replace)
    ops.asr_log_row(*[args[k] for k in ref.ARRAYS], out,
                    slots=[ref.SLOTS[n] for n in ("z_pres_kl", "scale_kl", "shift_kl", "pr_num")])


# ------------------------------------------------------------------ kernel ---
@pytest.mark.parametrize("B", [1, 5, 67, 1030])
@pytest.mark.parametrize("t_exec", [1, 3, 6])
def test_kernel_matches_float64_restatement(B, t_exec):
    a = ref.crafted(T, t_exec, B, seed=7000 + 10 * B + t_exec)
    want = ref.log_row(a)
    d = _dev(a)
    out = torch.full((16,), float("nan"), device=DEV)
    _launch(d, out)
    got = out.cpu().numpy()
    again = torch.full((16,), float("nan"), device=DEV)
    _launch(d, again)
    assert not np.isnan(got).any(), got
    for i, name in enumerate(ref.NAMES):
        print(name, repr(got[i]), repr(want[i]))
        if name in ref.COPIED:
            src = {"num_margin": a["margin"][0], "TotLoss": a["means"][0],
                   "accu": a["means"][1]}[name]
            assert got[i:i + 1].view(np.int32)[0] == np.float32(src).view(np.int32), name
        else:
            assert abs(float(got[i]) - want[i]) <= np.spacing(np.float32(abs(want[i]))), \
                (name, got[i], want[i])
    assert np.array_equal(got.view(np.int32), again.cpu().numpy().view(np.int32))


def test_wrapper_refusals_leave_out_untouched():
    B = 5
    a = ref.crafted(T, 3, B, seed=1)
    d = _dev(a)
    out = torch.full((16,), 123.0, device=DEV)
    f32 = lambda *s: torch.zeros(s, device=DEV)  # noqa: E731
    bad = [
        dict(vkl=d["vkl"].double()),                       # dtype
        dict(live=d["live"].float()),
        dict(bce=d["bce"].cpu()),                          # device
        dict(arec=d["arec"].cpu()),
        dict(bce=f32(B + 1)),                              # shapes
        dict(zmask=f32(T, B + 1)),
        dict(arec=f32(T, ref.NQ - 1, B)),
        dict(margin=f32(2)),
        dict(means=f32(3)),
        dict(live=torch.zeros(T + 2, device=DEV, dtype=torch.int32)),
        dict(vkl=f32(B, T).t()),                           # non-contiguous
        dict(klsum=f32(2 * B)[::2]),
        dict(arec=f32(ref.NQ, T, B).transpose(0, 1)),
    ]
    for replace in bad:
        with pytest.raises(ValueError):
            _launch(d, out, **replace)
    # T outside 1..8
    for t in (0, 9):
        steps = dict(arec=f32(t, ref.NQ, B), vkl=f32(t, B), zmask=f32(t, B),
                     live=torch.zeros(t + 1, device=DEV, dtype=torch.int32))
        with pytest.raises(ValueError, match="loop steps"):
            _launch(d, out, **steps)
    # the output itself
    for o in (torch.zeros(15, device=DEV), torch.zeros(16, device=DEV, dtype=torch.float64),
              torch.zeros(16), torch.zeros(32, device=DEV)[::2]):
        with pytest.raises(ValueError):
            _launch(d, o)
    with pytest.raises(ValueError, match="slots"):
        from mog_air import ops
        ops.asr_log_row(*[d[k] for k in ref.ARRAYS], out, slots=[23, 24, 25, 30])
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full((16,), 123.0, device=DEV))


# ------------------------------------------------------------- the models ---
def _workspace_arrays(m):
    return {k: getattr(m._ws, k).detach().cpu().numpy() for k in ref.ARRAYS}


def _check_against_property(m, what):
    out = torch.full((16,), float("nan"), device=DEV)
    m.log_row_(out)
    got = out.cpu().numpy()
    lv = m.log_variables
    assert tuple(lv) == tuple(m.log_names) == ref.NAMES
    bar = ref.bar_b(_workspace_arrays(m))
    for i, name in enumerate(ref.NAMES):
        want = np.float32(lv[name])
        print(what, name, repr(got[i]), repr(want), bar[i])
        if name in ref.COPIED:
            assert got[i:i + 1].view(np.int32)[0] == want.view(np.int32), (what, name)
        else:
            assert abs(float(got[i]) - float(lv[name])) <= bar[i], (what, name, got[i], lv[name])


@pytest.mark.parametrize("B", [8, 64])
def test_asr_log_row_matches_log_variables(B):
    import bench
    m = bench.make_asr_model("fp32", torch.device(DEV), "logrow%d" % B)
    data = []
    for i in range(3):
        x, k = bench.synthetic(B, 500 + i)
        data.append((torch.as_tensor(x).to(DEV), torch.as_tensor(k).to(DEV)))
    m.train_step_async(*data[0])
    _check_against_property(m, "async")
    for x, k in data:
        m.train_step_graphed(x, k)
    assert m._graph is not None and m._ws is m._graph_ws
    _check_against_property(m, "replay")
    m.infer(*data[1])
    _check_against_property(m, "infer")


def test_air_log_row_is_the_means_bits():
    import bench
    m = bench.make_model("fp32", torch.device(DEV), 1, 0, "logrow_air")
    assert m.log_names == ("loss", "accuracy", "mse")
    data = []
    for i in range(3):
        x, k = bench.synthetic(64, 600 + i)
        data.append((torch.as_tensor(x).to(DEV), torch.as_tensor(k).to(DEV)))

    def check(what):
        out = torch.full((3,), float("nan"), device=DEV)
        m.log_row_(out)
        assert torch.equal(out.view(torch.int32), m._ws.means[:3].view(torch.int32)), what
        assert (float(out[0]), float(out[1]), float(out[2])) == (m.loss, m.accuracy, m.mse_loss)

    loss, acc, mse, _ = m.step(*data[0])
    check("eager")
    out = torch.empty(3, device=DEV)
    m.log_row_(out)
    assert out.tolist() == [loss, acc, mse]
    for x, k in data:
        m.train_step_graphed(x, k)
    check("replay")
    m.infer(*data[1])
    check("infer")
    for bad in (torch.empty(4, device=DEV), torch.empty(3), torch.empty(3, device=DEV).double()):
        with pytest.raises(ValueError):
            m.log_row_(bad)


# ---------------------------------------------------------------- LogRing ---
def test_log_ring_push_drain(monkeypatch):
    import bench
    from mog_air import trainer
    from mog_air.asr_model import AIRModel as AsrModel
    from mog_air.model_base import ModelBase

    def boom(*a, **k):
        raise AssertionError("a per-step host read")
    monkeypatch.setattr(ModelBase, "step", boom)
    monkeypatch.setattr(AsrModel, "log_variables", property(boom))

    m = bench.make_model("fp32", torch.device(DEV), 1, 0, "logring_air")
    x, k = bench.synthetic(64, 700)
    x, k = torch.as_tensor(x).to(DEV), torch.as_tensor(k).to(DEV)
    ring = trainer.LogRing(m)
    assert tuple(ring.buf.shape) == (trainer.LOG_EACH_ITERATION, 3) and ring.drain() == []
    want = []
    for i in range(23):
        m.train_step_graphed(x, k)
        if i < 20:
            ring.push(m)
            want.append(m._ws.means[:3].clone())
        else:
            with pytest.raises(RuntimeError, match="full"):
                ring.push(m)
    rows = ring.drain()
    assert len(rows) == 20 and all(isinstance(v, float) for r in rows for v in r)
    assert rows == [w.tolist() for w in want]  # push order, the means' values
    assert ring.drain() == []
    m.train_step_graphed(x, k)
    ring.push(m)
    assert ring.drain() == [m._ws.means[:3].tolist()]

    a = bench.make_asr_model("fp32", torch.device(DEV), "logring_asr")
    ring = trainer.LogRing(a, rows=4)
    for _ in range(3):
        a.train_step_graphed(x, k)
        ring.push(a)
    rows = ring.drain()
    assert len(rows) == 3 and len(rows[0]) == 16 and np.isfinite(np.asarray(rows)).all()
    assert rows[2][ref.NAMES.index("TotLoss")] == float(a._ws.means[0])
