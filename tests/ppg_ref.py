"""TEST INFRASTRUCTURE: PPG's two output stages (csrc/ppg.hip: arl_ppg_head_loss_parts) restated on torch tensors of
any precision -- the losses as formulas autograd can differentiate, and the closed-form gradients the kernel evaluates.
tests/test_ppg_host.py checks the closed forms against float64 autograd; the GPU tests compare the kernel with both.

Rows carry a weight `wgt` (inv_n of the kernel: 1 / batch, or the caller's inv_count), so every loss is a weighted sum."""
import torch

import autograd_ref

TINY = 1e-8


def head(h, w, b, n_act, stop_value=False):
    """h [B, hid], w [A + 1, hid], b [A + 1] -> (prob [B, A], value [B], out [B, A + 1]); stop_value: the value row reads
    h.detach() -- the policy phase's stopped gradient (the value loss trains w[A], b[A] and nothing below)."""
    pi = h @ w[:n_act].t() + b[:n_act]
    v = (h.detach() if stop_value else h) @ w[n_act] + b[n_act]
    out = torch.cat([pi, v[:, None]], dim=1)
    return torch.softmax(out[:, :n_act], dim=1), out[:, n_act], out


def policy_losses(prob, value, act, adv, ret, old_pa, clip, c_v, c_e, wgt, tie_rule="theano"):
    """(pi_loss, v_loss, ent_loss): PPO's, as arl_pg_head_loss_parts kind 1 (ppo.py:42-51, aac_base.py:60-66)."""
    pa = prob[torch.arange(prob.shape[0], device=prob.device), act]
    ratio = (pa + TINY) / (old_pa + TINY)
    pi = -(wgt * autograd_ref.ppo_surrogate(ratio, adv, clip, tie_rule)).sum()
    v = c_v * (wgt * (value - ret) ** 2).sum()
    ent = -c_e * (wgt * -(prob * torch.log(prob + TINY)).sum(dim=1)).sum()
    return pi, v, ent


def aux_losses(prob, value, ret, old, beta_clone, c_v, wgt):
    """(clone, v_loss): beta_clone * mean KL(old || prob) with the distribution's TINY (Categorical.kl_sym) and the value
    regression."""
    kl = (old * (torch.log(old + TINY) - torch.log(prob + TINY))).sum(dim=1)
    return beta_clone * (wgt * kl).sum(), c_v * (wgt * (value - ret) ** 2).sum()


def policy_dout(prob, value, act, adv, ret, old_pa, clip, c_v, c_e, wgt, tie_rule="theano"):
    """d (pi + v + ent) / d out [B, A + 1] in closed form, the kernel's expressions."""
    n, a = prob.shape
    rows = torch.arange(n, device=prob.device)
    pa = prob[rows, act]
    ratio = (pa + TINY) / (old_pa + TINY)
    lo, hi = 1. - clip, 1. + clip
    s1, s2 = ratio * adv, torch.clamp(ratio, lo, hi) * adv
    surr = torch.minimum(s1, s2)
    inside = (ratio >= lo) & (ratio <= hi)
    zero = torch.zeros_like(adv)
    if tie_rule == "theano":
        g_ratio = torch.where((surr == s1) | inside, adv, zero)
    elif tie_rule == "both":
        g_ratio = torch.where(surr == s1, adv, zero) + torch.where((surr == s2) & inside, adv, zero)
    else:
        g_ratio = torch.where(inside | (s1 < s2), adv, zero)
    lg = torch.log(prob + TINY)
    gk = c_e * wgt[:, None] * (lg + prob / (prob + TINY))
    gk[rows, act] = gk[rows, act] - wgt * g_ratio / (old_pa + TINY)
    dot = (gk * prob).sum(dim=1, keepdim=True)
    dv = 2. * c_v * wgt * (value - ret)
    return torch.cat([prob * (gk - dot), dv[:, None]], dim=1)


def aux_dout(prob, value, ret, old, beta_clone, c_v, wgt):
    """d (clone + v) / d out [B, A + 1]: q_k = old_k p_k / (p_k + TINY); beta_clone wgt (p_j sum_k q_k - q_j); the value
    column 2 c_v wgt (V - R)."""
    q = old * prob / (prob + TINY)
    dpi = (beta_clone * wgt)[:, None] * (prob * q.sum(dim=1, keepdim=True) - q)
    return torch.cat([dpi, (2. * c_v * wgt * (value - ret))[:, None]], dim=1)


def head_grads(dout, h, w, n_act, stop_value):
    """(dh, dw, db) of the output layer from dout; stop_value: dh leaves the value row out (dw, db keep it)."""
    dh = dout[:, :n_act] @ w[:n_act] if stop_value else dout @ w
    return dh, dout.t() @ h, dout.sum(dim=0)
