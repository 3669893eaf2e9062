"""TEST INFRASTRUCTURE: V-MPO's device stages (csrc/vmpo.hip) restated in float64 -- the order-preserving key and the
stable top-half selection of arl_vmpo_weights with its softmax weights and the temperature's dual terms (NumPy, sums in
position order), and arl_vmpo_head_loss_parts' losses and closed-form gradients on torch tensors of any precision
(ppg_ref.head / ppg_ref.head_grads give the output layer around them).  tests/test_vmpo_host.py checks the closed forms
against float64 autograd; the GPU tests compare the kernels with them.  At the end: advantages built from chosen keys
(from_keys, radix_case, radix_trace, sign_and_range_cases) for tests/test_r2d2_vmpo_sacd_limits_*.py."""
import numpy as np
import torch

TINY = 1e-8
DUAL_FLOOR = 1e-8


def keys(adv):
    """uint32 keys of fp32 advantages: unsigned order of the keys = order of the values, +0.0 above -0.0."""
    bits = np.ascontiguousarray(adv, dtype=np.float32).view(np.uint32)
    return bits ^ np.where(bits >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def select(adv):
    """bool [n]: the n_top = (n + 1) // 2 positions first in (key descending, position ascending)."""
    k = keys(adv).astype(np.int64)
    n = k.size
    order = np.argsort(-k, kind="stable")               # stable: equal keys keep their position order
    sel = np.zeros(n, dtype=bool)
    sel[order[:(n + 1) // 2]] = True
    return sel


def weights(adv, eta, eps_eta):
    """-> dict(sel bool [n], psi f64 [n] (0 where not selected), temp_loss, d_eta, L, n_top, addends) from the fp32
    advantages of a minibatch in position order and the fp32 eta, both promoted to float64; sums run in position order.
    addends: the magnitudes whose ulp bounds the rounding of (temp_loss, d_eta, L) -- their terms may cancel."""
    a = np.asarray(adv, dtype=np.float32).astype(np.float64)
    eta, eps_eta = float(np.float32(eta)), float(eps_eta)
    sel = select(adv)
    n_top = int(sel.sum())
    m = a[sel].max()
    e = np.where(sel, np.exp((a - m) / eta), 0.0)
    s = np.cumsum(e)[-1]                                 # position order (e is exactly 0 where not selected)
    psi = e / s
    sa = np.cumsum(psi * a)[-1]
    log_term = np.log(s / n_top)
    big_l = m / eta + log_term
    temp_loss = eta * eps_eta + eta * big_l
    d_eta = (eps_eta + big_l) - sa / eta
    addends = (max(abs(eta * eps_eta), abs(m), abs(eta * log_term)),
               max(abs(eps_eta), abs(m / eta), abs(log_term), abs(sa / eta)),
               max(abs(m / eta), abs(log_term)))
    return dict(sel=sel, psi=psi, temp_loss=temp_loss, d_eta=d_eta, L=big_l, n_top=n_top, addends=addends)


def temp_loss_sym(adv_sel, eta, eps_eta):
    """The temperature's dual loss on the SELECTED advantages as a formula autograd differentiates (torch float64)."""
    return eta * eps_eta + eta * (torch.logsumexp(adv_sel / eta, dim=0) - np.log(adv_sel.numel()))


def losses(prob, value, act, psi, ret, old, alpha, c_v, wgt):
    """(pi_loss, v_loss, alpha-scaled KL term, mean KL): the network's loss is the sum of the first three; psi and alpha
    are constants of it."""
    pa = prob[torch.arange(prob.shape[0], device=prob.device), act]
    pi = -(psi * torch.log(pa + TINY)).sum()
    v = c_v * (wgt * (value - ret) ** 2).sum()
    kl = (wgt * (old * (torch.log(old + TINY) - torch.log(prob + TINY))).sum(dim=1)).sum()
    return pi, v, alpha * kl, kl


def dout(prob, value, act, psi, ret, old, alpha, c_v, wgt):
    """d (pi_loss + v_loss + alpha KL) / d out [B, A + 1] in closed form, the kernel's expressions."""
    n = prob.shape[0]
    rows = torch.arange(n, device=prob.device)
    pa = prob[rows, act]
    g = torch.zeros_like(prob)
    g[rows, act] = -psi / (pa + TINY)
    dot = (g * prob).sum(dim=1, keepdim=True)
    q = old * prob / (prob + TINY)
    dpi = prob * (g - dot) + (alpha * wgt)[:, None] * (prob * q.sum(dim=1, keepdim=True) - q)
    return torch.cat([dpi, (2. * c_v * wgt * (value - ret))[:, None]], dim=1)


def dual_grads(d_eta, mean_kl, eps_alpha):
    """(d temp_loss / d eta, d alpha_loss / d alpha) for alpha_loss = alpha (eps_alpha - sg[KL]) + sg[alpha] KL."""
    return d_eta, eps_alpha - mean_kl


# ---- cases built from keys (tests/test_r2d2_vmpo_sacd_limits_gpu.py / _host.py) --------------------------------------------

KEY_MIN, KEY_MAX = 0x00800000, 0xFF7FFFFF           # the finite values' keys: below lie -inf and the negative NaNs, above
LIMIT_SIZES = [1, 3, 1025, 65535, 65536]            # +inf and the positive ones
PREFIX = [0x00000000, 0xBF000000, 0xBF800000, 0xBF800000]       # the bytes above pass p: values in [0.5, 2) from pass 1 on
LANE_OF_PASS = [20, 7, 41, 62]                      # the lane whose four bins the cases of pass p walk through


def from_keys(k):
    """fp32 advantages whose keys() are k: the inverse of keys(), finite values only."""
    k = np.ascontiguousarray(k, dtype=np.uint32)
    assert k.size and int(k.min()) >= KEY_MIN and int(k.max()) <= KEY_MAX, "a key of a value that is not finite"
    bits = np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    adv = bits.view(np.float32)
    assert np.isfinite(adv).all() and np.array_equal(keys(adv), k)
    return adv


def radix_trace(k):
    """The four passes of the header's radix select on uint32 keys, as integers on the host.  Per pass: the candidates
    (keys that agree with the bins chosen so far), how many bins they fill, and -- for the lane l that owns bins
    255 - 4 l .. 252 - 4 l and holds the wanted rank -- want, above (candidates in higher lanes' bins), incl (above + the
    lane's own), the lane's counts c[0 .. 3] from its top bin down, the chosen bin and r = its place in the lane.
    -> (list of four dicts, the threshold key, the number of keys equal to it that are selected)."""
    k = np.ascontiguousarray(k, dtype=np.uint32).astype(np.int64)
    want, prefix, mask, out = (k.size + 1) // 2, 0, 0, []
    for p in range(4):
        shift = 24 - 8 * p
        cand = k[(k & mask) == prefix]
        hist = np.bincount((cand >> shift) & 255, minlength=256)
        above = 0
        for lane in range(64):
            top = 255 - 4 * lane
            c = [int(hist[top - j]) for j in range(4)]
            if above < want <= above + sum(c):
                break
            above += sum(c)
        incl, r, inner = above + sum(c), 0, above
        while want > inner + c[r]:
            inner += c[r]
            r += 1
        out.append(dict(candidates=int(cand.size), bins=int((hist > 0).sum()), lane=lane, want=want, above=above, incl=incl,
                        c=c, bin=top - r, r=r))
        prefix |= (top - r) << shift
        mask |= 255 << shift
        want -= inner
    return out, prefix, want


def first_deciding_pass(trace):
    """the first pass whose histogram has more than one bin filled; None if every key is the same."""
    for p, t in enumerate(trace):
        if t["bins"] > 1:
            return p
    return None


def _bin_counts(n, T, edge):
    """{bin: count} of byte p over n keys, so that the n_top-th largest key falls in bin T.  The lane that owns T owns
    bins top .. top - 3; `edge`:
      mid     keys on both sides of T, in every other bin of the lane too where n allows
      incl    the wanted rank is the count at and above the lane's bins: nothing in the lane below T
      above1  the wanted rank is one more than the count above the lane: nothing in the lane above T"""
    n_top = (n + 1) // 2
    top = 255 - 4 * ((255 - T) // 4)
    lane_hi, lane_lo = list(range(T + 1, top + 1)), list(range(top - 3, T))
    far_hi = sorted({b for b in (top + 1, 255) if top < b <= 255})
    far_lo = sorted({b for b in (top - 4, 0) if 0 <= b < top - 3})
    if edge == "mid":
        hi_bins, lo_bins = lane_hi + far_hi, lane_lo + far_lo
        hi = n_top // 2 if hi_bins else 0
        lo = (n - n_top + 1) // 2 if lo_bins else 0
    elif edge == "incl":
        hi_bins, lo_bins = lane_hi + far_hi, far_lo
        hi = n_top // 2 if hi_bins else 0
        lo = n - n_top
        assert lo_bins or lo == 0, "incl needs a lane below"
    else:
        hi_bins, lo_bins = far_hi, lane_lo + far_lo
        hi = n_top - 1
        lo = (n - n_top + 1) // 2 if lo_bins else 0
        assert hi_bins or hi == 0, "above1 needs a lane above"
    counts = {T: n - hi - lo}
    for total, bins in ((hi, hi_bins), (lo, lo_bins)):
        for j, b in enumerate(bins):
            share = total // len(bins) + (1 if j < total % len(bins) else 0)
            if share:
                counts[b] = share
    assert sum(counts.values()) == n and min(counts.values()) > 0
    return counts


def radix_case(rs, n, p, T, edge):
    """n keys that agree in the bytes above pass p (PREFIX), whose byte p follows _bin_counts(n, T, edge), with random
    lower bytes and positions in random order.  In pass 0 the two end bins hold finite values in half their range only
    (bin 0: byte 1 >= 0x80; bin 255: byte 1 < 0x80).  -> uint32 keys."""
    shift = 24 - 8 * p
    counts = _bin_counts(n, T, edge)
    byte = np.concatenate([np.full(c, b, dtype=np.int64) for b, c in sorted(counts.items())])
    low = rs.randint(0, 1 << shift, size=n).astype(np.int64) if shift else np.zeros(n, np.int64)
    k = (PREFIX[p] & ~((1 << (shift + 8)) - 1) & 0xFFFFFFFF) | (byte << shift) | low
    if p == 0:
        k = np.where(byte == 0, k | 0x00800000, np.where(byte == 255, k & ~0x00800000, k))
    return k[rs.permutation(n)].astype(np.uint32)


def radix_families(n):
    """[(name, p, T, edge)] for one size: per pass, the two end bins, the four bins of one lane, and the two edge counts."""
    fam = []
    for p in range(4):
        top = 255 - 4 * LANE_OF_PASS[p]
        fam += [("p%d-bin255" % p, p, 255, "mid"), ("p%d-bin0" % p, p, 0, "mid")]
        fam += [("p%d-lane%d-r%d" % (p, LANE_OF_PASS[p], r), p, top - r, "mid") for r in range(4)]
        fam += [("p%d-incl" % p, p, top - 1, "incl"), ("p%d-above1" % p, p, top - 2, "above1")]
    return fam


def eta_for(adv):
    """an fp32 temperature under which no selected weight underflows: (m - the smallest selected advantage) / eta <= 40,
    so psi >= e^-40 / 65536 ~ 6e-23, a normal fp32 number; between 2^-126 and 1e37."""
    a = np.asarray(adv, np.float32).astype(np.float64)
    sel = select(adv)
    spread = a[sel].max() - a[sel].min()
    return float(np.float32(min(max(spread / 40., 2.0 ** -126), 1e37))) if spread > 0 else 1.0


def sign_and_range_cases(rs, n):
    """[(name, advantages f32[n], eta)]: the inverted half of the key alone; the threshold on either side of the sign
    change (keys 0x80000000 = +0.0 and 0x7FFFFFFF = -0.0 are neighbours: pass 0 decides between bins 128 and 127, the last
    bin of lane 31 and the first of lane 32); denormals of both signs at eta = 1 and at the smallest normal eta (where the
    weights differ); values up to 0.9 FLT_MAX at eta = 1."""
    n_top = (n + 1) // 2
    neg = -np.abs(rs.randn(n)).astype(np.float32) - np.float32(1e-3)
    pos_n = np.abs(rs.randn(n)).astype(np.float32) + np.float32(1e-3)

    def around_zero(n_pos):
        a = neg.copy()
        a[:n_pos] = pos_n[:n_pos]
        if n_pos >= 1:
            a[n_pos - 1] = 0.0                      # the smallest key of the upper half of the key space
        if n_pos < n:
            a[n_pos] = -0.0                         # the largest key of the lower half
        return a[rs.permutation(n)]
    den = (rs.randint(1, 1 << 23, size=n).astype(np.uint32) | (rs.randint(0, 2, size=n).astype(np.uint32) << 31)).view(np.float32)
    big = ((rs.rand(n) * 2. - 1.) * 0.9 * float(np.finfo(np.float32).max)).astype(np.float32)
    out = [("all-negative", neg, 0.7), ("threshold-is-plus-zero", around_zero(n_top), 0.7),
           ("denormals-eta1", den, 1.0), ("denormals-eta-min", den, 2.0 ** -126), ("near-flt-max-eta1", big, 1.0)]
    if n_top >= 2 or n == 1:
        out.insert(2, ("threshold-is-minus-zero", around_zero(n_top - 1), 0.7))
    return out
