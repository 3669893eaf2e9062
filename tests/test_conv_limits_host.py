"""CPU-only: pins tests/conv_ref.py -- the float64 reference of tests/test_conv_limits_gpu.py -- to a naive seven-loop numpy
convolution (tiny shapes: non-square kernels, asymmetric padding, stride 3, padding larger than the kernel, H < stride),
to F.conv2d + autograd in float64 (random geometries) and to the layout conventions of accel_rl_amd._lib."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref

#         b  H  W  C  K  kh kw st ph pw
TINY = [(2, 5, 4, 3, 2, 3, 2, 1, 1, 0),       # non-square kernel, asymmetric padding
        (1, 7, 8, 2, 3, 3, 3, 3, 0, 2),       # stride 3, a column the stride never reaches, padding on one axis only
        (2, 1, 5, 2, 2, 2, 2, 2, 1, 0),       # H < stride
        (1, 3, 3, 1, 2, 2, 2, 1, 2, 3)]       # padding at least as large as the kernel: whole windows in the border


def _operands(row, seed):
    b, H, W, C, K, kh, kw, st, ph, pw = row
    ho, wo = conv_ref.out_hw(row)
    rs = np.random.RandomState(seed)
    return (rs.randn(b, H, W, C), rs.randn(K, kh, kw, C), rs.randn(K), rs.randn(b, ho, wo, K), rs.randn(b, H, W, C))


def _naive(row, x, w, bias, dy):
    """y, dx, dw by seven nested loops over (b, oy, ox, k, ty, tx, c)."""
    b, H, W, C, K, kh, kw, st, ph, pw = row
    ho, wo = conv_ref.out_hw(row)
    y = np.zeros((b, ho, wo, K)) + bias
    dx, dw = np.zeros_like(x), np.zeros_like(w)
    for n in range(b):
        for oy in range(ho):
            for ox in range(wo):
                for k in range(K):
                    for ty in range(kh):
                        for tx in range(kw):
                            h, v = oy * st + ty - ph, ox * st + tx - pw
                            if not (0 <= h < H and 0 <= v < W):
                                continue
                            for c in range(C):
                                y[n, oy, ox, k] += x[n, h, v, c] * w[k, ty, tx, c]
                                dx[n, h, v, c] += dy[n, oy, ox, k] * w[k, ty, tx, c]
                                dw[k, ty, tx, c] += dy[n, oy, ox, k] * x[n, h, v, c]
    return y, dx, dw


@pytest.mark.parametrize("row", TINY)
def test_conv_ref_is_the_seven_loop_convolution(row):
    x, w, bias, dy, mask = _operands(row, seed=sum(row))
    y, dx, dw = _naive(row, x, w, bias, dy)
    t = torch.from_numpy
    close = lambda got, want: np.abs(got.numpy() - want).max() <= 1e-13 * max(np.abs(want).max(), 1.0)     # noqa: E731
    assert close(conv_ref.fwd(t(x), t(w), t(bias), row, False), y)
    assert close(conv_ref.fwd(t(x), t(w), t(bias), row, True), np.maximum(y, 0))
    assert close(conv_ref.fwd(t(x), t(w), None, row, False), y - bias)
    assert close(conv_ref.dgrad(t(dy), t(w), row), dx)
    assert close(conv_ref.dgrad(t(dy), t(w), row, t(mask)), np.where(mask > 0, dx, 0))
    assert close(conv_ref.wgrad(t(dy), t(x), row), dw)
    assert close(conv_ref.dbias(t(dy)), dy.reshape(-1, row[4]).sum(0))
    # pixels no window reads: the naive loops never touch them
    touched = np.zeros(x.shape[1:3], dtype=bool)
    b, H, W, C, K, kh, kw, st, ph, pw = row
    ho, wo = conv_ref.out_hw(row)
    for oy in range(ho):
        for ox in range(wo):
            for ty in range(kh):
                for tx in range(kw):
                    h, v = oy * st + ty - ph, ox * st + tx - pw
                    if 0 <= h < H and 0 <= v < W:
                        touched[h, v] = True
    assert np.array_equal(conv_ref.reads(row).numpy(), touched)


def test_the_tiny_shapes_hold_the_edges_they_are_meant_to():
    assert not conv_ref.reads(TINY[1]).all() and not conv_ref.reads(TINY[2]).all()       # unread columns exist
    assert conv_ref.out_hw(TINY[2]) == (1, 2) and TINY[2][1] < TINY[2][7]
    # a window wholly in the border: the bare convolution is exactly 0 there
    x, w, bias, dy, _ = _operands(TINY[3], seed=1)
    y = conv_ref.fwd(torch.from_numpy(x), torch.from_numpy(w), None, TINY[3], False)
    assert (y[:, 0, :, :] == 0).all() and (y[:, :, 0, :] == 0).all() and (y != 0).any()


def test_mask_rule_zeroes_both_signed_zeros_and_negatives():
    row = (1, 1, 4, 1, 1, 1, 1, 1, 0, 0)
    dy = torch.tensor([1.0, 2.0, 3.0, 4.0]).reshape(1, 1, 4, 1)
    w = torch.ones(1, 1, 1, 1)
    mask = torch.tensor([0.0, -0.0, -1.0, 1e-30]).reshape(1, 1, 4, 1)
    assert conv_ref.dgrad(dy, w, row, mask).reshape(-1).tolist() == [0.0, 0.0, 0.0, 4.0]


def _random_rows(n, seed):
    rs = np.random.RandomState(seed)
    rows = []
    while len(rows) < n:
        st = int(rs.randint(1, 4))
        kh, kw = int(rs.randint(1, 5)), int(rs.randint(1, 5))
        ph, pw = int(rs.randint(0, 4)), int(rs.randint(0, 4))
        H, W = int(rs.randint(1, 10)), int(rs.randint(1, 10))
        if H + 2 * ph < kh or W + 2 * pw < kw:
            continue
        rows.append((int(rs.randint(1, 4)), H, W, int(rs.randint(1, 6)), int(rs.randint(1, 6)), kh, kw, st, ph, pw))
    return rows


@pytest.mark.parametrize("row", _random_rows(12, seed=20261019))
def test_conv_ref_matches_float64_conv2d_and_its_autograd(row):
    b, H, W, C, K, kh, kw, st, ph, pw = row
    x, w, bias, dy, mask = (torch.from_numpy(a) for a in _operands(row, seed=7))
    nchw = lambda t: t.permute(0, 3, 1, 2)                          # noqa: E731
    xr, wr = nchw(x).detach().requires_grad_(), nchw(w).detach().requires_grad_()
    out = F.conv2d(xr, wr, bias, stride=st, padding=(ph, pw))
    gx, gw = torch.autograd.grad(out, (xr, wr), nchw(dy))
    close = lambda got, want: (got - want).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1.0)   # noqa: E731
    assert close(conv_ref.fwd(x, w, bias, row, True), F.relu(out.detach()).permute(0, 2, 3, 1))
    assert close(conv_ref.dgrad(dy, w, row), gx.permute(0, 2, 3, 1))
    assert close(conv_ref.wgrad(dy, x, row), gw.permute(0, 2, 3, 1))
    # fp32 inputs are widened, not computed in fp32
    y32 = conv_ref.fwd(x.float(), w.float(), bias.float(), row, False)
    assert y32.dtype == torch.float64
    assert torch.equal(y32, conv_ref.fwd(x.float().double(), w.float().double(), bias.float().double(), row, False))


def test_layout_conventions_of_the_binding():
    from accel_rl_amd import _lib
    for row in TINY + _random_rows(6, seed=3):
        g = _lib.conv_geom(*row)
        assert conv_ref.geom_row(g) == row
        assert _lib.conv_out_hw(g) == conv_ref.out_hw(row) == conv_ref.out_hw(g)
    # the u8 twins: planar [rows][C][H][W] observations through a row index, (K, C, kh, kw) weights
    rs = np.random.RandomState(5)
    obs = torch.from_numpy(rs.randint(0, 256, (5, 2, 8, 8)).astype(np.uint8))
    idx = torch.tensor([4, 0, 4], dtype=torch.int32)
    w = torch.from_numpy(rs.randn(4, 2, 4, 4))
    row = (3, 8, 8, 2, 4, 4, 4, 4, 0, 0)
    scale = float(np.float32(1.0 / 255.0))
    dy = torch.from_numpy(rs.randn(3, 2, 2, 4))
    x = obs[idx.long()].double() * scale
    xr, wr = x.clone(), w.clone().requires_grad_()
    out = F.conv2d(xr, wr, None, stride=4)
    gw, = torch.autograd.grad(out, wr, dy.permute(0, 3, 1, 2))
    assert torch.allclose(conv_ref.fwd_u8(obs, idx, scale, w, None, row, False), out.detach().permute(0, 2, 3, 1), rtol=0, atol=1e-12)
    got = conv_ref.wgrad_u8(dy, obs, idx, scale, row)
    assert got.shape == w.shape and torch.allclose(got, gw, rtol=0, atol=1e-12)
    assert torch.equal(conv_ref.fwd_u8(obs[idx.long()], None, scale, w, None, row, False), conv_ref.fwd_u8(obs, idx, scale, w, None, row, False))


def test_rounded_is_nearest_even_bf16():
    t = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.1415927, 0.0, -0.0,
                      1e-40, 3.0e38])
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.140625, 0.0, -0.0, 0.0, 0.0], dtype=torch.float64)
    got = conv_ref.rounded(t)
    assert torch.equal(got[:7], want[:7])                      # ties to even both ways, above a tie, a negative, the zeros
    rs = np.random.RandomState(0)
    r = torch.from_numpy((rs.randn(4096) * np.exp2(rs.randint(-30, 30, 4096))).astype(np.float32))
    assert torch.equal(conv_ref.rounded(r), r.bfloat16().double())
    assert torch.equal(conv_ref.rounded(t[7:]), t[7:].bfloat16().double())     # a subnormal, a value near the top
