"""The IMPALA residual network without a GPU: the NumPy restatements of the pooling kernels (tests/resnet_ref.py) against
PyTorch's own max_pool2d and its autograd in float64, the parameter layout of AtariResnetPolicy, and every refusal --
each raised before a device is touched."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_ref as rr

POOL_SHAPES = [(1, 1, 1, 4), (2, 2, 3, 4), (3, 5, 4, 8), (5, 7, 7, 36), (2, 13, 10, 32), (1, 104, 80, 16)]


def pool_input(shape, ties, seed=0):
    rs = np.random.RandomState(seed + sum(shape))
    if ties:                        # integers in -2 .. 2: most windows hold their maximum more than once
        return rs.randint(-2, 3, size=shape).astype(np.float32)
    return rs.randn(*shape).astype(np.float32)


@pytest.mark.parametrize("ties", [True, False], ids=["ties", "floats"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_numpy_pool_equals_torch_max_pool2d_and_its_autograd(shape, ties):
    b, h, w, c = shape
    z = pool_input(shape, ties)
    dy = pool_input((b,) + rr.out_hw(h, w) + (c,), ties, seed=1)
    y, y_relu, arg = rr.maxpool_fwd32(z)
    zt = torch.from_numpy(z.astype(np.float64)).permute(0, 3, 1, 2).requires_grad_()
    yt, it = F.max_pool2d(zt, 3, 2, 1, return_indices=True)
    np.testing.assert_array_equal(y.astype(np.float64), yt.detach().permute(0, 2, 3, 1).numpy())
    np.testing.assert_array_equal(y_relu, np.maximum(y, 0))
    assert not np.signbit(y_relu).any()
    # arg -> the flat input index PyTorch reports (the first maximum in row-major window order)
    oy, ox = np.arange(y.shape[1])[None, :, None, None], np.arange(y.shape[2])[None, None, :, None]
    flat = (2 * oy - 1 + arg // 3) * w + (2 * ox - 1 + arg % 3)
    np.testing.assert_array_equal(flat, it.permute(0, 2, 3, 1).numpy())
    if ties and h * w > 1:
        assert len(np.unique(arg)) > 1
    want, = torch.autograd.grad(yt, zt, torch.from_numpy(dy.astype(np.float64)).permute(0, 3, 1, 2))
    got = rr.maxpool_bwd32(dy, arg, h, w)
    if ties:                        # small integers: every float32 sum is exact
        np.testing.assert_array_equal(got.astype(np.float64), want.permute(0, 2, 3, 1).numpy())
    else:                           # at most four terms per element
        np.testing.assert_allclose(got, want.permute(0, 2, 3, 1).numpy(), rtol=0, atol=4 * 2.0 ** -24 * np.abs(dy).max() * 4)
    assert (got[rr.maxpool_bwd32(np.ones_like(dy), arg, h, w) == 0] == 0).all()


def test_add_relu_restatement():
    a, b = np.float32([1.5, -2.0, 0.0, -0.0]), np.float32([-1.5, 1.0, -0.0, -0.0])
    s, r = rr.add_relu32(a, b)
    np.testing.assert_array_equal(s, np.float32([0.0, -1.0, 0.0, -0.0]))
    np.testing.assert_array_equal(r, np.float32([0, 0, 0, 0]))
    assert not np.signbit(r).any()


def _policy(**kw):
    from accel_rl_amd.policies.atari_resnet_policy import AtariResnetPolicy
    return AtariResnetPolicy(**kw)


def test_parameter_count_and_names_of_the_default_network():
    policy = _policy()
    layout = policy.reference_layout((4, 104, 80), 6)
    names = [n for n, _ in layout]
    convs = []
    for s in range(3):
        convs += ["S%dConv" % s] + ["S%dB%dConv%d" % (s, b, k) for b in range(2) for k in range(2)]
    assert len(convs) == 15
    assert names == [n + t for n in convs for t in "Wb"] + ["FC0W", "FC0b", "OutputW", "Outputb", "OutputW", "Outputb"]
    shapes = dict(layout[:-4])
    assert shapes["S0ConvW"] == (16, 4, 3, 3) and shapes["S1ConvW"] == (32, 16, 3, 3) and shapes["S2B1Conv1W"] == (32, 32, 3, 3)
    assert shapes["FC0W"] == (13 * 10 * 32, 256)               # 104 x 80 -> 52 x 40 -> 26 x 20 -> 13 x 10
    want = (16 * 4 * 9 + 16) + 4 * (16 * 16 * 9 + 16) + (32 * 16 * 9 + 32) + 4 * (32 * 32 * 9 + 32) + \
        (32 * 32 * 9 + 32) + 4 * (32 * 32 * 9 + 32) + (4160 * 256 + 256) + (256 * 6 + 6) + (256 + 1)
    assert sum(int(np.prod(s)) for _, s in layout) == want == 1164759
    assert not policy.serve_supported() and not policy._u8_conv1


@pytest.mark.parametrize("kw", [dict(channels=(16, 30, 32)), dict(channels=(16, 2)), dict(channels=(16, 1028)),
                                dict(channels=()), dict(channels=(16,) * 5), dict(blocks_per_section=0),
                                dict(blocks_per_section=5), dict(blocks_per_section=1.5), dict(hidden_sizes=())],
                         ids=lambda kw: "%s=%s" % next(iter(kw.items())))
def test_constructor_refusals(kw):
    with pytest.raises(NotImplementedError):
        _policy(**kw)


def test_initialize_refusals_come_before_any_device(monkeypatch):
    """An empty pooled image, max_rows_per_pass = "auto" and hidden sizes the dense kernels do not take: raised by
    initialize() before it allocates (this machine has no device: anything later would fail otherwise)."""
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec

    def no_device(*a, **kw):
        raise AssertionError("a device tensor was asked for")
    monkeypatch.setattr(torch, "zeros", no_device)
    with pytest.raises(NotImplementedError, match="empty"):
        _policy().initialize(EnvSpec(UintBox((4, 0, 80)), Discrete(6)))
    policy = _policy()
    policy.max_rows_per_pass = "auto"
    with pytest.raises(NotImplementedError, match="max_rows_per_pass"):
        policy.rows_per_pass()
    with pytest.raises(NotImplementedError, match="max_rows_per_pass"):
        policy.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(6)))
    policy.max_rows_per_pass = 64
    assert policy.rows_per_pass() == 64
    with pytest.raises(NotImplementedError, match="multiples of 4"):
        _policy(hidden_sizes=(30,)).initialize(EnvSpec(UintBox((4, 12, 8)), Discrete(6)))
