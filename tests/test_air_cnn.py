"""AIR cnn=True encoder, CPU side: the test helper (tests/air_cnn_ref.py) pinned
-- its numpy chain against conv2d / max_pool2d, its pooling convention, its
restated loop against oracle/air_torch.py -- its inputs shown not to be
degenerate, and the parameter table with the cnn block."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import air_oracle as ao
from oracle import air_torch as at

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import air_cnn_ref as ref  # noqa: E402

SEEDS = (300, 301, 302)


@pytest.mark.parametrize("seed", SEEDS)
def test_case_inputs_are_not_degenerate(seed):
    share, ties, margin = ref.check_case(ref.case(seed, 6))
    print(f"seed {seed}: nonzero features {share:.3f}, nonzero ties {ties}, margin {margin:.3g}")


def test_encoder_numpy_equals_torch_float64():
    c = ref.case(300, 6)
    x = np.concatenate([c["x"], ref.corner_canvas()[None]])
    got = ref.encoder_numpy(x, c["P"])
    want = ref.encoder_torch(x, c["P"], torch.float64).numpy()
    assert got.shape == want.shape == (7, ref.NFEAT) and got.dtype == np.float32
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert err < 1e-5, err
    # and every intermediate plane, so that a compensating error cannot hide
    c1, p1, c2, p2, c3 = ref.encoder_planes(x, c["P"])
    assert p1.shape == (7, 25, 25, 8) and p2.shape == (7, 12, 12, 8)
    np.testing.assert_array_equal(p2, ref.pool_first_max(c2)[0])
    np.testing.assert_array_equal(p2, c2[:, :24, :24].reshape(7, 12, 2, 12, 2, 8).max((2, 4)))


def test_pool_tie_goes_to_the_first_maximum():
    """A hand-built 2x2 window of four equal values: pool_first_max and
    max_pool2d's gradient both pick (0, 0); a later strict maximum wins."""
    a = np.full((1, 2, 2, 1), 0.25, np.float32)
    best, arg = ref.pool_first_max(a)
    assert best.item() == 0.25 and arg.item() == 0
    t = torch.tensor(a.reshape(1, 1, 2, 2), dtype=torch.float64, requires_grad=True)
    torch.nn.functional.max_pool2d(t, 2).sum().backward()
    np.testing.assert_array_equal(t.grad.numpy().reshape(2, 2), [[1, 0], [0, 0]])
    a[0, 1, 0, 0] = 0.5
    assert ref.pool_first_max(a)[1].item() == 2
    a[0, 0, 1, 0] = 0.5  # (0, 1) now ties with (1, 0): the first one wins
    assert ref.pool_first_max(a)[1].item() == 1


def test_conv2_row_and_column_24_get_no_gradient():
    """pool2 drops conv2's row / column 24: with the encoder cut at conv2's
    output, the gradient of the features there is exactly zero."""
    c = ref.case(300, 6)
    P = c["P"]
    t = lambda n: torch.tensor(P[ref.CNN + n], dtype=torch.float64)  # noqa: E731
    x = torch.tensor(c["x"][:2], dtype=torch.float64).reshape(-1, 1, 50, 50)
    Fn = torch.nn.functional
    a = Fn.max_pool2d(torch.relu(Fn.conv2d(x, t("conv1/kernel").permute(3, 2, 0, 1),
                                           t("conv1/bias"), padding=2)), 2)
    c2 = torch.relu(Fn.conv2d(a, t("conv2/kernel").permute(3, 2, 0, 1), t("conv2/bias"),
                              padding=2)).detach().requires_grad_(True)
    c3 = torch.relu(Fn.conv2d(Fn.max_pool2d(c2, 2), t("conv3/kernel").permute(3, 2, 0, 1),
                              t("conv3/bias"), padding=2))
    assert c2.shape[-2:] == (25, 25) and c3.shape[-2:] == (12, 12)
    (c3 * torch.tensor(np.random.default_rng(5).standard_normal(tuple(c3.shape)))).sum().backward()
    g = c2.grad.numpy()
    assert np.abs(g[:, :, :24, :24]).max() > 0
    assert not g[:, :, 24, :].any() and not g[:, :, :, 24].any()


def _grads(fn, P):
    Pt = {n: torch.tensor(v, dtype=torch.float64, requires_grad=True) for n, v in P.items()}
    out = fn(Pt)
    out["loss"].backward()
    return out, Pt


@pytest.mark.parametrize("fixed", [False, True])
def test_restated_loop_equals_air_forward_when_the_features_are_the_canvas(fixed):
    """The loop body both ways: with the canvas itself as the LSTM input (and
    the cnn=False kernel) the restated loop is oracle/air_torch.py's."""
    c = ref.case(300, 6)
    cfg, P0 = c["cfg"], c["P0"]
    nz = at.to_torch(c["nz"])
    x = torch.tensor(c["x"], dtype=torch.float64)
    Gc = torch.tensor(np.random.default_rng(31).standard_normal((cfg.batch, 2500)) * 0.01)
    want, Pw = _grads(lambda P: at.air_forward(cfg, P, nz, x, canvas_cotangent=Gc,
                                               fixed_steps=fixed), P0)
    got, Pg = _grads(lambda P: ref.air_cnn_forward_torch(cfg, P, nz, x, canvas_cotangent=Gc,
                                                         fixed_steps=fixed, features=x), P0)
    assert got["T"] == want["T"] >= 2
    np.testing.assert_array_equal(got["digits"].numpy(), want["digits"].numpy())
    assert float(got["loss"].detach()) == pytest.approx(float(want["loss"].detach()), rel=1e-12)
    for n in Pw:
        np.testing.assert_allclose(Pg[n].grad.numpy(), Pw[n].grad.numpy(), rtol=1e-12,
                                   atol=1e-12 * float(Pw[n].grad.abs().max()), err_msg=n)
    # and the train loss (BCE term) forward
    with torch.no_grad():
        Pt = at.to_torch(P0)
        a = at.air_forward(cfg, Pt, nz, x, fixed_steps=fixed)
        b = ref.air_cnn_forward_torch(cfg, Pt, nz, x, fixed_steps=fixed, features=x)
    np.testing.assert_allclose(b["loss_b"].numpy(), a["loss_b"].numpy(), rtol=1e-12)


def test_restated_loop_reaches_the_cnn_tensors():
    c = ref.case(300, 6)
    cfg = c["cfg"]
    x = torch.tensor(c["x"], dtype=torch.float64)
    _, Pt = _grads(lambda P: ref.air_cnn_forward_torch(cfg, P, at.to_torch(c["nz"]), x,
                                                       fixed_steps=True), c["P"])
    for n in ref.cnn_names():
        assert float(Pt[n].grad.abs().max()) > 0, n


def test_param_specs_append_the_cnn_block():
    from mog_air.params import ParamStore, cnn_param_specs, param_specs
    args = (256, 784, (512, 256), (256, 512), 50, 64, 64)
    plain = param_specs(2500, *args)
    assert plain == ao.param_specs(ao.AirConfig())  # cnn=False: today's table
    st = ParamStore(plain, torch.device("cpu"), seed=1235)
    # today's offsets: every tensor rounded up to 64 floats, in table order
    off = 0
    for name, shape in plain:
        assert st.offsets[name] == off, name
        off += (int(np.prod(shape)) + 63) // 64 * 64
    assert st.total == off
    cnn = param_specs(1152, *args) + cnn_param_specs(8)
    assert cnn[len(plain):] == ref.cnn_specs(8) == [
        ("air/cnn/conv1/kernel", (5, 5, 1, 8)), ("air/cnn/conv1/bias", (8,)),
        ("air/cnn/conv2/kernel", (5, 5, 8, 8)), ("air/cnn/conv2/bias", (8,)),
        ("air/cnn/conv3/kernel", (5, 5, 8, 8)), ("air/cnn/conv3/bias", (8,))]
    assert cnn[0] == (ref.KERNEL, (1152 + 256, 1024))
    assert cnn[1:len(plain)] == plain[1:]
    # the draws of the cnn=False table do not move when a 4-D block follows it
    both = ParamStore(plain + cnn_param_specs(8), torch.device("cpu"), seed=1235)
    assert torch.equal(both.flat[:st.total], st.flat)
    for name, _ in plain:
        assert both.offsets[name] == st.offsets[name]


def test_glorot_limit_of_conv_kernels():
    from mog_air.params import ParamStore, cnn_param_specs, glorot_limit
    assert glorot_limit((5, 5, 8, 8)) == pytest.approx(np.sqrt(6.0 / 400.0), rel=1e-12)
    assert glorot_limit((5, 5, 1, 8)) == pytest.approx(np.sqrt(6.0 / 225.0), rel=1e-12)
    assert glorot_limit((2500, 1024)) == pytest.approx(np.sqrt(6.0 / 3524.0), rel=1e-12)
    st = ParamStore(cnn_param_specs(8), torch.device("cpu"), seed=3)
    d = st.state_dict()
    for name, shape in cnn_param_specs(8):
        if len(shape) == 4:
            lim = glorot_limit(shape)
            assert 0.9 * lim < np.abs(d[name]).max() <= lim, name
        else:
            assert not d[name].any(), name
