"""TEST INFRASTRUCTURE for the IMPALA residual network (csrc/resnet.hip, policies/atari_resnet_policy.py).  The reference
has no such network: the yardsticks are NumPy restatements of the three streaming kernels in exactly the order
include/accel_rl_hip.h states (float32 arithmetic, so the GPU must give the same bits), and the whole network in float64
through PyTorch's own conv2d / max_pool2d on the CPU, differentiated by autograd."""
import numpy as np
import torch
import torch.nn.functional as F

import autograd_ref

TINY = 1e-8                 # the losses' epsilon (aac_base.py)
BRANCH_MARGIN = 1e-5        # a rectifier input / a pool window's lead, relative to max |.| of its layer


def out_hw(in_h, in_w):
    return (in_h - 1) // 2 + 1, (in_w - 1) // 2 + 1


# ---- the kernels, restated ---------------------------------------------------------------------------------------------

def maxpool_fwd32(z):
    """z f32[B][H][W][C] -> (y f32, y_relu f32, arg u8), each [B][Ho][Wo][C]: the window walked ky = 0, 1, 2 and inside
    kx = 0, 1, 2, a strictly larger value replacing the best so far; positions outside the image never take part."""
    assert z.dtype == np.float32
    b, h, w, c = z.shape
    oh, ow = out_hw(h, w)
    zp = np.pad(z, ((0, 0), (1, 1), (1, 1), (0, 0)), constant_values=-np.inf)       # (-inf > best is never true)
    best = np.full((b, oh, ow, c), -np.inf, np.float32)
    arg = np.zeros((b, oh, ow, c), np.uint8)
    for ky in range(3):
        for kx in range(3):
            v = zp[:, ky:ky + 2 * oh - 1:2, kx:kx + 2 * ow - 1:2, :]
            m = v > best
            best = np.where(m, v, best)
            arg = np.where(m, np.uint8(3 * ky + kx), arg)
    return best, np.where(best > 0, best, np.float32(0)), arg


def maxpool_bwd32(dy, arg, in_h, in_w):
    """dz f32[B][in_h][in_w][C]: per input element the terms dy[oy][ox] of the windows whose arg points at it, oy ascending
    and inside ox ascending; the first term as it is, the others added in float32; +0 without a term.  For an element
    (i, j) the window rows come as oy = i // 2 (ky = 1 or 2) and then (i + 1) // 2 (ky = 0), so walking ky = 1, 2, 0 and
    inside kx = 1, 2, 0 over all windows at once visits every element's terms in that order."""
    assert dy.dtype == np.float32 and arg.dtype == np.uint8 and dy.shape == arg.shape
    b, oh, ow, c = dy.shape
    assert (oh, ow) == out_hw(in_h, in_w)
    dz = np.zeros((b, in_h, in_w, c), np.float32)
    have = np.zeros((b, in_h, in_w, c), bool)
    for ky in (1, 2, 0):
        iy = 2 * np.arange(oh) - 1 + ky
        vy = (iy >= 0) & (iy < in_h)
        for kx in (1, 2, 0):
            ix = 2 * np.arange(ow) - 1 + kx
            vx = (ix >= 0) & (ix < in_w)
            rows, cols = iy[vy][:, None], ix[vx][None, :]
            d = dy[:, vy][:, :, vx]
            hit = arg[:, vy][:, :, vx] == 3 * ky + kx
            cur, seen = dz[:, rows, cols], have[:, rows, cols]
            dz[:, rows, cols] = np.where(hit, np.where(seen, cur + d, d), cur)
            have[:, rows, cols] = seen | hit
    return dz


def add_relu32(a, b):
    s = (a + b).astype(np.float32)
    return s, np.where(s > 0, s, np.float32(0))


# ---- the float64 network on the reference layout -----------------------------------------------------------------------

def ref_params(policy, flat_bucket, dtype=np.float64):
    """The reference-layout tensors of a bucket, requiring gradients (policy._ref_shapes' order)."""
    fl = policy.bucket_to_reference(flat_bucket)
    out, pos = [], 0
    for shape in policy._ref_shapes:
        m = int(np.prod(shape))
        out.append(torch.from_numpy(fl[pos:pos + m].reshape(shape).astype(dtype)).requires_grad_())
        pos += m
    return out


def ref_net(rp, channels, blocks, n_hidden, n_act, x):
    """x [B, C, H, W] scaled observations -> (prob [B, A], value [B], taps).  rp: conv (W, b) in network order, hidden
    (W, b).., policy (W, b), value (W, b); conv W (out, in, kh, kw) of a true convolution, dense W (in, out) on
    (c, h, w)-ordered inputs.  taps: [("relu" | "pool", tensor)] -- every tensor a rectifier reads and every pool input."""
    taps, k = [], 0

    def conv(a):
        nonlocal k
        y = F.conv2d(a, rp[k].flip(2, 3), rp[k + 1], padding=1)
        k += 2
        return y

    for _ in channels:
        z = conv(x)
        taps.append(("pool", z))
        x = F.max_pool2d(z, 3, 2, 1)
        for _ in range(blocks):
            taps.append(("relu", x))
            pre = conv(F.relu(x))
            taps.append(("relu", pre))
            x = x + conv(F.relu(pre))
        taps.append(("relu", x))
        x = F.relu(x)               # what the next section's conv (after the last section: the first dense layer) reads
    x = x.flatten(1)
    for _ in range(n_hidden):
        pre = x @ rp[k] + rp[k + 1]
        taps.append(("relu", pre))
        x = F.relu(pre)
        k += 2
    logits, value = x @ rp[k] + rp[k + 1], (x @ rp[k + 2] + rp[k + 3])[:, 0]
    assert k + 4 == len(rp) and logits.shape[1] == n_act
    return torch.softmax(logits, dim=1), value, taps


def branch_margin(taps):
    """The smallest relative margin by which any rectifier input stays away from 0 and any pool window's largest value
    leads its second: float32 takes the same branches as float64 where this is far above float32's rounding."""
    worst = np.inf
    for kind, t in taps:
        t = t.detach()
        scale = float(t.abs().max())
        if kind == "relu":
            worst = min(worst, float(t.abs().min()) / scale)
        else:
            win = F.unfold(F.pad(t, (1, 1, 1, 1), value=-np.inf), 3, stride=2)              # [B, C * 9, L]
            win = win.view(t.shape[0], t.shape[1], 9, -1)
            top = win.topk(2, dim=2).values
            worst = min(worst, float((top[:, :, 0] - top[:, :, 1]).min()) / scale)
    return worst


def pg_loss(prob, value, kind, actions, advantages, returns, old_prob, clip, v_coeff, ent_coeff):
    """The mean losses of aac_base.py / a2c.py / ppo.py over the rows (no valids): kind 0 A2C, kind 1 PPO (the
    reference's Theano surrogate gradient: autograd_ref.ppo_surrogate)."""
    n = prob.shape[0]
    ar = torch.arange(n)
    pa = prob[ar, actions]
    if kind == 1:
        ratio = (pa + TINY) / (old_prob[ar, actions] + TINY)
        pi = -autograd_ref.ppo_surrogate(ratio, advantages, clip, "theano").mean()
    else:
        pi = -(torch.log(pa + TINY) * advantages).mean()
    v = v_coeff * ((value - returns) ** 2).mean()
    ent = -ent_coeff * (-(prob * torch.log(prob + TINY)).sum(dim=1)).mean()
    return pi, v, ent
