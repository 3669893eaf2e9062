"""Plain float64 restatement of the contraction kernels' three operations (csrc/mfma_conv.hip), NHWC activations and
(K, kh, kw, C) weights as the library lays them out: explicit sums over the filter taps -- per tap (ty, tx) a strided slice
of the zero-padded input and an einsum over the channels.  No library convolution, no autograd; runs wherever its
operands live (CPU or device).  tests/test_conv_limits_host.py pins it to a seven-loop numpy convolution and to
F.conv2d + autograd in float64.

geom: an ArlConvGeom or a row (batch, H, W, C, K, kh, kw, stride, pad_h, pad_w)."""
import torch


def geom_row(geom):
    if hasattr(geom, "in_h"):
        return (geom.batch, geom.in_h, geom.in_w, geom.in_c, geom.out_c, geom.kh, geom.kw, geom.stride, geom.pad_h,
                geom.pad_w)
    return tuple(int(v) for v in geom)


def out_hw(geom):
    b, H, W, C, K, kh, kw, st, ph, pw = geom_row(geom)
    return (H + 2 * ph - kh) // st + 1, (W + 2 * pw - kw) // st + 1


def _padded(x, ph, pw):
    b, H, W, C = x.shape
    xp = x.new_zeros((b, H + 2 * ph, W + 2 * pw, C))
    xp[:, ph:ph + H, pw:pw + W, :] = x
    return xp


def _taps(geom):
    """(ty, tx, rows, columns): the padded-input pixels tap (ty, tx) meets, one per output pixel."""
    b, H, W, C, K, kh, kw, st, ph, pw = geom_row(geom)
    ho, wo = out_hw(geom)
    for ty in range(kh):
        for tx in range(kw):
            yield ty, tx, slice(ty, ty + (ho - 1) * st + 1, st), slice(tx, tx + (wo - 1) * st + 1, st)


def fwd(x, w, bias, geom, relu):
    """y[b, oy, ox, k] = act(bias[k] + sum_{ty, tx, c} xpad[b, oy st + ty, ox st + tx, c] w[k, ty, tx, c])"""
    b, H, W, C, K, kh, kw, st, ph, pw = geom_row(geom)
    ho, wo = out_hw(geom)
    x, w = x.double().reshape(b, H, W, C), w.double().reshape(K, kh, kw, C)
    xp = _padded(x, ph, pw)
    y = x.new_zeros((b, ho, wo, K))
    for ty, tx, rows, cols in _taps(geom):
        y += torch.einsum("bhwc,kc->bhwk", xp[:, rows, cols, :], w[:, ty, tx, :])
    if bias is not None:
        y += bias.double().reshape(1, 1, 1, K)
    return y.clamp(min=0) if relu else y


def dgrad(dy, w, geom, mask=None):
    """dx[b, h, w, c] = sum over the (oy, ox, ty, tx) with oy st + ty - pad_h = h, ox st + tx - pad_w = w of
    sum_k dy[b, oy, ox, k] w[k, ty, tx, c]; zero where mask is not > 0 (-0.0 and +0.0 both zero the element)."""
    b, H, W, C, K, kh, kw, st, ph, pw = geom_row(geom)
    ho, wo = out_hw(geom)
    dy, w = dy.double().reshape(b, ho, wo, K), w.double().reshape(K, kh, kw, C)
    dxp = dy.new_zeros((b, H + 2 * ph, W + 2 * pw, C))
    for ty, tx, rows, cols in _taps(geom):
        dxp[:, rows, cols, :] += torch.einsum("bhwk,kc->bhwc", dy, w[:, ty, tx, :])
    dx = dxp[:, ph:ph + H, pw:pw + W, :].contiguous()
    if mask is not None:
        dx = torch.where(mask.reshape(dx.shape) > 0, dx, torch.zeros_like(dx))
    return dx


def wgrad(dy, x, geom):
    """dw[k, ty, tx, c] = sum_{b, oy, ox} dy[b, oy, ox, k] xpad[b, oy st + ty, ox st + tx, c]"""
    b, H, W, C, K, kh, kw, st, ph, pw = geom_row(geom)
    ho, wo = out_hw(geom)
    dy, x = dy.double().reshape(b, ho, wo, K), x.double().reshape(b, H, W, C)
    xp = _padded(x, ph, pw)
    dw = x.new_zeros((K, kh, kw, C))
    for ty, tx, rows, cols in _taps(geom):
        dw[:, ty, tx, :] = torch.einsum("bhwk,bhwc->kc", dy, xp[:, rows, cols, :])
    return dw


def dbias(dy):
    """Column sums of dy[..., K]."""
    return dy.double().reshape(-1, dy.shape[-1]).sum(0)


def reads(geom):
    """bool [H, W]: input pixels that at least one window reads (the others get an exactly-zero data gradient)."""
    b, H, W, C, K, kh, kw, st, ph, pw = geom_row(geom)
    ho, wo = out_hw(geom)
    hit = torch.zeros(H + 2 * ph, W + 2 * pw, dtype=torch.bool)
    for ty, tx, rows, cols in _taps(geom):
        hit[rows, cols] = True
    return hit[ph:ph + H, pw:pw + W]


# ---- the u8 twins: planar observations u8 [rows][C][H][W] (optionally through a row-index list), pixel scale, weights /
# weight gradient in (K, C, kh, kw) order; no padding

def u8_rows(obs, idx, scale):
    """The NHWC float64 input the u8 kernels see: float(obs[idx]) * scale."""
    rows = obs if idx is None else obs[idx.long()]
    return rows.double().permute(0, 2, 3, 1) * float(scale)


def fwd_u8(obs, idx, scale, w, bias, geom, relu):
    return fwd(u8_rows(obs, idx, scale), w.double().permute(0, 2, 3, 1), bias, geom, relu)


def wgrad_u8(dy, obs, idx, scale, geom):
    return wgrad(dy, u8_rows(obs, idx, scale), geom).permute(0, 3, 1, 2).contiguous()


def rounded(t):
    """Nearest-even rounding of fp32 to bf16 (the BF16 route's operands), by integer arithmetic on the bit patterns; as float64."""
    bits = t.float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    bits = torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32)
    return bits.view(torch.float32).reshape(t.shape).double()
