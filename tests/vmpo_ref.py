"""TEST INFRASTRUCTURE: V-MPO's device stages (csrc/vmpo.hip) restated in float64 -- the order-preserving key and the
stable top-half selection of arl_vmpo_weights with its softmax weights and the temperature's dual terms (NumPy, sums in
position order), and arl_vmpo_head_loss_parts' losses and closed-form gradients on torch tensors of any precision
(ppg_ref.head / ppg_ref.head_grads give the output layer around them).  tests/test_vmpo_host.py checks the closed forms
against float64 autograd; the GPU tests compare the kernels with them."""
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
