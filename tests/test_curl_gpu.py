"""CURL on the device: arl_curl_loss_parts (csrc/curl.hip) through the C ABI, AtariCurlDqnPolicy.curl_loss_and_grads and
CurlOptimizer's momentum step, each against float64 torch autograd of the stated formulas.  The bars are the project's
whole-step ones: gradients rtol 2e-3, atol 2e-5 max|want|; losses 2e-3 relative; the accuracy exact."""
import functools

import numpy as np
import pytest
import torch

from munchausen_ref import GAMMA, huber64
from test_munchausen_gpu import _ref_convs, _ref_params, _ref_q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SPARE = 3                                       # rows past every output that must stay NaN


def _close(got, want, what):
    scale = np.abs(want).max()
    print("%-12s max |want| %.3g max err %.3g" % (what, scale, np.abs(got - want).max()))
    assert np.allclose(got, want, rtol=2e-3, atol=2e-5 * scale), what


def _infonce64(zq, zk, w, coef):
    """-> (loss, logits): coef * mean_i (logsumexp_j S_ij - S_ii), S = zq w zk^T, float64 torch."""
    s = zq @ w @ zk.T
    return coef * (torch.logsumexp(s, dim=1) - s.diag()).mean(), s


@functools.lru_cache(maxsize=None)
def _case(b, d, logit_scale, coef):
    """fp32 inputs whose logits are of order logit_scale, and the float64 reference (computed once per case)."""
    rs = np.random.RandomState(1000 * b + d)
    zq, zk = rs.randn(b, d).astype(np.float32), rs.randn(b, d).astype(np.float32)
    w = (rs.randn(d, d) * (logit_scale / d)).astype(np.float32)
    tq, tw = torch.from_numpy(zq).double().requires_grad_(), torch.from_numpy(w).double().requires_grad_()
    loss, s = _infonce64(tq, torch.from_numpy(zk).double(), tw, coef)
    loss.backward()
    s = s.detach()
    if b > 1:                                   # no row whose two largest logits are close: the arg-max is decided
        top = s.sort(dim=1, descending=True).values
        assert (top[:, 0] - top[:, 1]).min().item() > 1e-4
    hits = int((s.argmax(dim=1) == torch.arange(b)).sum())
    return zq, zk, w, loss.item(), hits, tq.grad.numpy(), tw.grad.numpy(), s.abs().max().item()


def _launch(c, b, d, coef):
    from accel_rl_amd import _lib
    lib = _lib.load()
    dev = lambda a: torch.from_numpy(a).to(DEV)                 # noqa: E731
    zq, zk, w = dev(c[0]), dev(c[1]), dev(c[2])
    dzq, dw, loss2 = (torch.full(s, NAN, device=DEV) for s in ((b + SPARE, d), (d + SPARE, d), (4,)))
    ws = _lib.curl_workspace(d, DEV)
    rc = lib.arl_curl_loss_parts(zq.data_ptr(), zk.data_ptr(), w.data_ptr(), b, d, coef, dzq.data_ptr(), dw.data_ptr(),
                                 loss2.data_ptr(), ws.data_ptr(), None, None)
    assert rc == 0, lib.arl_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(dzq[b:]).all() and torch.isnan(dw[d:]).all() and torch.isnan(loss2[2:]).all()
    return dzq[:b].cpu().numpy(), dw[:d].cpu().numpy(), loss2[:2].cpu().numpy()


@pytest.mark.parametrize("d", [4, 36, 128])
@pytest.mark.parametrize("b", [1, 2, 31, 32, 33, 65])
def test_kernel_matches_float64_autograd(b, d):
    """One row, below / at / over the 32-row tile, two tiles + 1 (the key tiles take the same ragged sizes); below one
    MFMA block, over one, the LDS maximum."""
    c = _case(b, d, 2.0, 0.7)
    assert 0.5 < c[7] < 30 or b == 1
    dzq, dw, loss2 = _launch(c, b, d, 0.7)
    if b > 1:
        _close(dzq, c[5], "dzq")
        _close(dw, c[6], "dw")
    else:                                       # one row is its own only key: loss 0, softmax - I = 0
        assert not dzq.any() and not dw.any()
    assert abs(loss2[0] - c[3]) <= 2e-3 * abs(c[3]) + 1e-7
    assert round(float(loss2[1]) * b) == c[4] and abs(loss2[1] - c[4] / b) < 1e-6


def test_large_logits_zero_coefficient_and_determinism():
    b, d = 33, 36
    c = _case(b, d, 15.0, 0.7)                  # logits of order 50: the row maximum has to come off before exp
    assert 50 < c[7] < 100
    got = _launch(c, b, d, 0.7)
    _close(got[0], c[5], "dzq")
    _close(got[1], c[6], "dw")
    assert abs(got[2][0] - c[3]) <= 2e-3 * abs(c[3]) and round(float(got[2][1]) * b) == c[4]
    again = _launch(c, b, d, 0.7)
    assert all(np.array_equal(x, y) for x, y in zip(got, again))
    dzq, dw, loss2 = _launch(c, b, d, 0.0)
    assert not dzq.any() and not dw.any() and loss2[0] == 0 and round(float(loss2[1]) * b) == c[4]


# ---- the policy and the optimizer ------------------------------------------------------------------------------------

N_ACT, LATENT, COEF = 6, 36, 0.5                # latent 36: stored at a stride of 64, the padding stays zero


@functools.lru_cache(maxsize=None)
def _policy(dueling):
    """The small network (2 conv layers, hidden 64, 6 actions), perturbed; target and momentum encoder differ from it."""
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn import AtariCurlDqnPolicy
    from accel_rl_amd.spaces import Discrete, EnvSpec, UintBox
    from accel_rl_amd.util.seed import set_seed
    set_seed(5)
    spec = dict(cnn_specs[0], hidden_sizes=[64])
    policy = AtariCurlDqnPolicy(epsilon=0.3, dueling=dueling, latent=LATENT, **spec)
    policy.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(N_ACT)), device=DEV)
    rs = np.random.RandomState(3)
    flat = policy.get_param_values()
    flat = flat + (rs.randn(flat.size) * 0.01).astype(np.float32)
    flat[-LATENT * LATENT:] = rs.randn(LATENT * LATENT) * 20. / LATENT         # logits of order 1 on these features
    policy.set_param_values(flat)
    np.testing.assert_array_equal(policy.get_param_values(), flat)              # round trip through the reference layout
    policy.flat_target.copy_(policy.flat_params * 0.9)
    policy.flat_momentum.mul_(0.95)
    return policy, spec


def _minibatch(b):
    rs = np.random.RandomState(b)
    dev = lambda a: torch.from_numpy(a).to(DEV)                 # noqa: E731
    u8 = lambda n: dev(rs.randint(0, 256, size=(n, 4, 104, 80), dtype=np.uint8))       # noqa: E731
    return (u8(2 * b), u8(b), dev(rs.randint(0, N_ACT, size=b).astype(np.uint8)), dev((rs.randn(b) * 0.05).astype(np.float32)),
            dev((rs.rand(b) < 0.3).astype(np.uint8)), dev((rs.rand(b) + 0.2).astype(np.float32)))


@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
@pytest.mark.parametrize("b", [3, 8])
def test_whole_update_matches_float64_autograd(b, dueling):
    policy, spec = _policy(dueling)
    mb = _minibatch(b)
    obs, nxt, act, ret, term, isw = mb
    policy.flat_grads.fill_(NAN)
    rows, td = policy.curl_loss_and_grads(*mb, GAMMA, 1.0, True, COEF)
    got = policy.bucket_to_reference(policy.flat_grads)
    diag = policy.curl_diag[:2].cpu().numpy()
    # float64: Q loss on view 0 + COEF * InfoNCE(view 0 online, view 1 through the momentum parameters, detached)
    rp, rt = _ref_params(policy, policy.flat_params), _ref_params(policy, policy.flat_target)
    bucket = policy.flat_params.clone()
    for om, op, n in policy._mom_ranges:
        bucket[op:op + n] = policy.flat_momentum[om:om + n]
    rm = _ref_params(policy, bucket)
    x0, x1, xn = (t.cpu().double() * float(np.float32(1. / 255)) for t in (obs[:b], obs[b:], nxt))
    q = _ref_q(rp, spec, x0, dueling)
    with torch.no_grad():
        sel = _ref_q(rp, spec, xn, dueling).argmax(dim=1)
        y = ret.cpu().double() + (1. - term.cpu().double()) * GAMMA * _ref_q(rt, spec, xn, dueling)[torch.arange(b), sel]
        zk = _ref_convs(rm, spec, x1)[0] @ rm[-3] + rm[-2]
    d = y - q[torch.arange(b), act.cpu().long()]
    want_rows = isw.cpu().double() / b * huber64(d, 1.0)
    closs, s = _infonce64(_ref_convs(rp, spec, x0)[0] @ rp[-3] + rp[-2], zk, rp[-1], COEF)
    top = s.detach().sort(dim=1, descending=True).values
    assert 0.3 < s.abs().max().item() < 30 and (top[:, 0] - top[:, 1]).min().item() > 1e-4
    grads = torch.autograd.grad(want_rows.sum() + closs, rp)
    want = np.concatenate([g.numpy().reshape(-1) for g in grads])
    for name, g in (("bilinear", grads[-1]), ("projection", grads[-3]), ("conv 1", grads[0])):
        assert g.abs().max().item() > 0, name
    _close(got, want, "gradients")
    _close(got[-LATENT * LATENT:], grads[-1].numpy().reshape(-1), "bilinear")
    assert np.allclose(rows.cpu().numpy(), want_rows.detach().numpy(), rtol=2e-3, atol=0)
    assert np.allclose(td.cpu().numpy(), d.detach().abs().clamp(max=1.0).numpy(), rtol=2e-3, atol=0)
    assert abs(diag[0] - closs.item()) <= 2e-3 * closs.item()
    assert round(float(diag[1]) * b) == int((s.argmax(dim=1) == torch.arange(b)).sum())
    # coef = 0: the tensors shared with AtariDqnPolicy take q_loss_and_grads' gradient on view 0, bit for bit
    shared = policy._offsets[policy._k_proj]
    policy.curl_loss_and_grads(*mb, GAMMA, 1.0, True, 0.0)
    with_zero = policy.flat_grads.clone()
    policy.q_loss_and_grads(obs[:b].contiguous(), *mb[1:], GAMMA, 1.0, double_dqn=True)
    assert torch.equal(with_zero[:shared], policy.flat_grads[:shared]) and not with_zero[shared:].any()


def test_momentum_step_and_graph_replay():
    from accel_rl_amd.algos.dqn import CURL
    policy, _ = _policy(True)
    keep = policy.flat_params.clone(), policy.flat_momentum.clone()
    tau, mb = 0.25, _minibatch(8)
    algo = CURL(latent=LATENT, momentum_tau=tau, prioritized_replay=True, curl_coef=COEF,
                optimizer_args=dict(learning_rate=1e-4))
    algo.optimizer.initialize(*algo.build_loss(None, policy), target=policy)
    try:
        for call in range(5):                   # two eager calls, the capture, two more replays
            old = policy.flat_momentum.clone()
            algo.optimizer.optimize(mb)
            torch.cuda.synchronize()
            new = torch.cat([policy.flat_params[op:op + n] for _, op, n in policy._mom_ranges])
            alpha = torch.tensor(1. - tau, dtype=torch.float32)         # arl_acer_avg_step: alpha avg + (1 - alpha) params
            want = (alpha * old.cpu()) + ((1. - alpha) * new.cpu())
            assert torch.equal(policy.flat_momentum.cpu(), want) and not torch.equal(old, policy.flat_momentum), call
        assert algo.optimizer._graph is not None
        assert torch.isfinite(policy.flat_params).all() and torch.isfinite(policy.curl_diag[:2]).all()
    finally:
        policy.flat_params.copy_(keep[0])
        policy.flat_momentum.copy_(keep[1])
