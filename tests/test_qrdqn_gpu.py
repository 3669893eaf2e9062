"""Quantile-regression DQN on the device (csrc/dqn.hip: arl_qrdqn_act / arl_qrdqn_loss, AtariQrDqnPolicy,
QuantileDQN).  The reference has no QR-DQN, so the yardstick is `ref_qr_loss` below: a float64 restatement of the
formulas of include/accel_rl_hip.h ("Quantile-regression DQN output stage"), gradient from autograd where kappa > 0 and
from the closed form where kappa == 0.

Tolerances.  loss_rows and priorities: the C51 bar, rtol 2e-4 (tests/test_catdqn_gpu.py).  Gradient: rtol 2e-4 plus
atol = (N + 8) * 2^-24 * (1 + max|T| / kappa) * max_b w_b -- the rounding of an N-term fp32 sum of terms bounded by
w_b / N (the kernel's chains are N / 4 + 3 additions long), plus the rounding of T passed through the clip's slope
1 / kappa.  On quantised inputs (every u exact in fp32) the second part is absent: atol = (N + 8) * 2^-24 * max_b w_b."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
POISON = 1e9                    # what the padding columns of every input hold: they must be ignored


def merge(t, n_act):
    """[B][A + 1][N] advantage rows then one value row -> [B][A][N]: val + (adv - mean_a adv)."""
    adv, val = t[:, :n_act], t[:, n_act:n_act + 1]
    return val + (adv - adv.mean(dim=1, keepdim=True))


def ref_qr_loss(pred, tgt, pol, act, ret, term, isw, gamma_n, kappa, n_act, dueling):
    """float64.  pred / tgt / pol: [B][A (+ 1)][N] without the padding (pol None: not double DQN); pred may require
    grad.  Returns a dict: rows (w_b loss_b), loss_b, grad (d sum(rows) / d pred), T, u, a_next, margin, w."""
    assert pred.dtype == torch.float64
    b, n = pred.shape[0], pred.shape[2]
    full = (lambda t: merge(t, n_act)) if dueling else (lambda t: t)        # noqa: E731
    ar = torch.arange(b)
    q = full(pol if pol is not None else tgt).mean(dim=2)
    a_next = q.argmax(dim=1)
    if n_act > 1:
        top2 = torch.topk(q, 2, dim=1).values
        margin = (top2[:, 0] - top2[:, 1]).min().item()
    else:
        margin = float("inf")
    keep = 1. - term.double()
    T = ret.double()[:, None] + keep[:, None] * (gamma_n * full(tgt)[ar, a_next])          # [B][j]
    th = full(pred)[ar, act.long()]                                                        # [B][i]
    u = T[:, None, :] - th[:, :, None]                                                     # [B][i][j]
    ind = (u < 0).double()                                                                 # u == 0: not negative
    tau = (torch.arange(n, dtype=torch.float64) + 0.5) / n
    wt = (tau[None, :, None] - ind).abs()
    if kappa > 0:
        au = u.abs()
        rho = wt * torch.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa)) / kappa
    else:
        rho = wt * u.abs()
    loss_b = rho.sum(dim=(1, 2)) / n
    w = (isw.double() if isw is not None else torch.ones(b, dtype=torch.float64)) / b
    rows = w * loss_b
    if kappa > 0:
        grad, = torch.autograd.grad(rows.sum(), pred)
    else:                                           # closed form, then back through the (linear) merge
        dth = -(w / n)[:, None] * (tau[None, :, None] - ind).sum(dim=2)
        dm = torch.zeros(b, n_act, n, dtype=torch.float64)
        dm[ar, act.long()] = dth
        grad = torch.cat([dm - dm.mean(dim=1, keepdim=True), dm.sum(dim=1, keepdim=True)], dim=1) if dueling else dm
    return dict(rows=rows.detach(), loss_b=loss_b.detach(), grad=grad, T=T.detach(), u=u.detach(), a_next=a_next,
                margin=margin, w=w)


def _block(rs, batch, n_act, n, stride, dueling, scale=2.):
    t = (rs.randn(batch, n_act + int(dueling), stride) * scale).astype(np.float32)
    t[:, :, n:] = POISON
    return t


def _selecting(rs, t, n_act, n):
    """Make the greedy action of block `t` unambiguous: the action rows (the advantage rows under dueling, where the
    merge adds the same to every action) are centred, given a mean in [-0.4, 0.4], and one randomly chosen row gets
    +1.0 on every quantile: the Q margin is at least 1 - 0.8."""
    batch = t.shape[0]
    t[:, :n_act, :n] -= t[:, :n_act, :n].mean(axis=2, keepdims=True)
    t[:, :n_act, :n] += rs.uniform(-0.4, 0.4, size=(batch, n_act, 1)).astype(np.float32)
    chosen = rs.randint(0, n_act, size=batch)
    t[np.arange(batch), chosen, :n] += np.float32(1.0)
    return chosen


def _case(seed, n_act, n, stride, batch, double, weighted, dueling):
    rs = np.random.RandomState(seed)
    pred, tgt = _block(rs, batch, n_act, n, stride, dueling), _block(rs, batch, n_act, n, stride, dueling)
    pol = _block(rs, batch, n_act, n, stride, dueling) if double else None
    chosen = _selecting(rs, pol if double else tgt, n_act, n)
    act = rs.randint(0, n_act, size=batch).astype(np.uint8)
    ret = (rs.randn(batch) * 3).astype(np.float32)
    term = (rs.rand(batch) < 0.3).astype(np.uint8)
    if batch > 1:
        term[0], term[1] = 1, 0                     # terminal and non-terminal rows in every case
    isw = (rs.rand(batch) + 0.1).astype(np.float32) if weighted else None
    return dict(pred=pred, tgt=tgt, pol=pol, act=act, ret=ret, term=term, isw=isw, chosen=chosen)


def _dev(x):
    return None if x is None else torch.from_numpy(x).to(DEV)


def _launch(c, n_act, n, gamma_n, kappa, dueling):
    from accel_rl_amd import _lib
    pred = _dev(c["pred"])
    batch = pred.shape[0]
    dth = torch.full_like(pred, float("nan"))
    rows = torch.full((batch,), float("nan"), device=DEV)
    pri = torch.full((batch,), float("nan"), device=DEV)
    _lib.qrdqn_loss(pred, _dev(c["tgt"]), _dev(c["pol"]), _dev(c["act"]), _dev(c["ret"]), _dev(c["term"]),
                    _dev(c["isw"]), n_act, n, gamma_n, kappa, dth, rows, pri, dueling=dueling)
    torch.cuda.synchronize()
    return dth.cpu(), rows.cpu(), pri.cpu()


def _reference(c, n_act, n, gamma_n, kappa, dueling):
    f64 = lambda x: None if x is None else torch.from_numpy(x[:, :, :n].astype(np.float64))       # noqa: E731
    t = lambda x: None if x is None else torch.from_numpy(x)                                      # noqa: E731
    pred = f64(c["pred"]).requires_grad_()
    return ref_qr_loss(pred, f64(c["tgt"]), f64(c["pol"]), t(c["act"]), t(c["ret"]), t(c["term"]), t(c["isw"]),
                       gamma_n, kappa, n_act, dueling)


def _check_against(ref, got, c, n_act, n, kappa_for_atol, exact_u=False):
    dth, rows, pri = got
    batch = rows.numel()
    assert ref["margin"] >= 0.1, ref["margin"]                              # every sample: no sample is skipped
    np.testing.assert_array_equal(ref["a_next"].numpy(), c["chosen"])
    w_max = ref["w"].max().item()
    if exact_u:
        atol = (n + 8) * EPS * w_max
        rtol = 0.
    else:
        atol = (n + 8) * EPS * (1 + ref["T"].abs().max().item() / kappa_for_atol) * w_max
        rtol = 2e-4
    print("margin %.3f  max|T| %.3f  atol %.3g  max grad err %.3g  max rel loss err %.3g" % (
        ref["margin"], ref["T"].abs().max().item(), atol, (dth[:, :, :n].double() - ref["grad"]).abs().max().item(),
        ((rows.double() - ref["rows"]).abs() / ref["rows"].abs()).max().item()))
    assert torch.isfinite(dth).all() and torch.isfinite(rows).all() and torch.isfinite(pri).all()
    np.testing.assert_allclose(rows.double().numpy(), ref["rows"].numpy(), rtol=2e-4, atol=0)
    np.testing.assert_allclose(pri.double().numpy(), ref["loss_b"].clamp(1e-6, 1e6).numpy(), rtol=2e-4, atol=0)
    err = (dth[:, :, :n].double() - ref["grad"]).abs()
    assert (err <= atol + rtol * ref["grad"].abs()).all(), err.max().item()
    assert not dth[:, :, n:].any()                                          # padding columns: exact zeros
    if dth.shape[1] == n_act:                                               # (not dueling) other actions' rows: exact zeros
        other = torch.ones(batch, n_act, dtype=torch.bool)
        other[torch.arange(batch), torch.from_numpy(c["act"]).long()] = False
        assert not dth[other].any()


SHAPES = [  # A, N, stride, batch, double, weighted, dueling
    (18, 64, 64, 32, False, True, False),           # a full wave, the flagship shape
    (3, 2, 4, 1, True, False, False),               # minimum N, fewer actions than waves, batch 1
    (64, 51, 52, 37, True, True, False),            # the maximum of actions, padding lanes, an odd batch
    (6, 5, 8, 5, False, False, True),               # dueling, padding columns
    (1, 64, 64, 3, True, True, True),               # a single action
]


@pytest.mark.parametrize("shape,kappa", [(s, 1.0) for s in SHAPES] + [(SHAPES[0], 0.25)])
def test_loss_priorities_and_gradient_vs_float64(shape, kappa):
    n_act, n, stride, batch, double, weighted, dueling = shape
    c = _case(100 * n_act + n + batch, n_act, n, stride, batch, double, weighted, dueling)
    gamma_n = float(np.float32(0.99 ** 3))
    ref = _reference(c, n_act, n, gamma_n, kappa, dueling)
    got = _launch(c, n_act, n, gamma_n, kappa, dueling)
    _check_against(ref, got, c, n_act, n, kappa)


@pytest.mark.parametrize("n_act,n,stride,batch", [(4, 7, 8, 5), (3, 64, 64, 3)])
def test_plain_quantile_regression_and_the_tie_rule_on_quantised_inputs(n_act, n, stride, batch):
    """gamma_n = 0.5, returns and target quantiles multiples of 1/4: every T_j is a multiple of 1/8; predicted quantiles
    multiples of 1/8 plus 1/16: every u is exact in fp32 and |u| >= 1/16.  Then some predicted quantiles of sample 0 are
    set equal to some T_j: u == 0 counts as not negative.  (Sample 0 is terminal, sample 1 is not: _case.)"""
    rs = np.random.RandomState(7 * n + n_act)
    c = _case(n + n_act, n_act, n, stride, batch, True, True, False)        # (the selecting net: pol, margin-built)
    c["tgt"][:, :, :n] = rs.randint(-32, 33, size=(batch, n_act, n)) / 4.
    c["ret"] = (rs.randint(-16, 17, size=batch) / 4.).astype(np.float32)
    c["pred"][:, :, :n] = rs.randint(-64, 64, size=(batch, n_act, n)) / 8. + 1. / 16
    gamma_n = 0.5
    ref0 = _reference(c, n_act, n, gamma_n, 0., False)
    T, u = ref0["T"], ref0["u"]
    assert torch.equal(T.float().double(), T) and torch.equal(T * 8, (T * 8).round())
    assert torch.equal(u.float().double(), u) and u.abs().min().item() >= 1. / 16
    _check_against(ref0, _launch(c, n_act, n, gamma_n, 0., False), c, n_act, n, None, exact_u=True)
    # ties: predicted quantiles i = 0, 2 (and the last) of sample 1 (not terminal) sit exactly on T_1, T_0 (and T_1)
    sb = 1
    a0 = int(c["act"][sb])
    tied = {0: 1, 2 % n: 0, n - 1: 1}
    for i, j in tied.items():
        c["pred"][sb, a0, i] = np.float32(T[sb, j].item())
    ref0, ref1 = _reference(c, n_act, n, gamma_n, 0., False), _reference(c, n_act, n, gamma_n, 1., False)
    assert all((ref0["u"][sb, i] == 0).any() for i in tied)
    got0, got1 = _launch(c, n_act, n, gamma_n, 0., False), _launch(c, n_act, n, gamma_n, 1., False)
    _check_against(ref0, got0, c, n_act, n, None, exact_u=True)
    _check_against(ref1, got1, c, n_act, n, 1.)
    # what the u == 0 pairs contribute: 0 at kappa = 1, -tau_i w_b / N each at kappa = 0
    w0 = ref0["w"][sb].item()
    for i in tied:
        zero = ref0["u"][sb, i] == 0
        tau = (i + 0.5) / n
        rest0 = -(w0 / n) * (tau - (ref0["u"][sb, i][~zero] < 0).double()).sum().item()
        assert abs(got0[0][sb, a0, i].item() - (rest0 - tau * w0 / n * int(zero.sum()))) <= (n + 8) * EPS * w0
        uu = ref1["u"][sb, i][~zero]
        rest1 = -(w0 / n) * ((tau - (uu < 0).double()).abs() * uu.clamp(-1, 1)).sum().item()
        assert abs(got1[0][sb, a0, i].item() - rest1) <= (n + 8) * EPS * (1 + T.abs().max().item()) * w0 + 2e-4 * abs(rest1)


@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
def test_action_kernel_greedy_ties_override_and_onehot(dueling):
    from accel_rl_amd import _lib
    b, a, n, s = 37, 18, 51, 52
    rs = np.random.RandomState(4 + int(dueling))
    theta = _block(rs, b, a, n, s, dueling)
    chosen = _selecting(rs, theta, a, n)
    theta[5, 9] = theta[5, 3]                       # two bit-identical rows, both the maximum: the lower index wins
    theta[5, 3, :n] += np.float32(2.0)
    theta[5, 9, :n] += np.float32(2.0)
    chosen[5] = 3
    t64 = torch.from_numpy(theta[:, :, :n].astype(np.float64))
    q = (merge(t64, a) if dueling else t64).mean(dim=2)
    top2 = torch.topk(q, 2, dim=1).values
    margin = top2[:, 0] - top2[:, 1]
    assert (margin[torch.arange(b) != 5] >= 0.1).all()
    q[5, 9] = -1e9                                  # (float64 rounding must not pick between the twins)
    np.testing.assert_array_equal(q.argmax(dim=1).numpy(), chosen)
    ov = np.full(b, -1, np.int32)
    ov[::5] = rs.randint(0, a, size=len(ov[::5]))
    onehot = torch.full((b, a), float("nan"), device=DEV)
    greedy = torch.full((b,), 255, dtype=torch.uint8, device=DEV)
    _lib.qrdqn_act(_dev(theta), _dev(ov), a, n, onehot, greedy, dueling=dueling)
    np.testing.assert_array_equal(greedy.cpu().numpy(), chosen)             # the argmax, override or not
    served = np.where(ov >= 0, ov, chosen)
    assert torch.equal(onehot.cpu(), F.one_hot(torch.from_numpy(served).long(), a).float())
    onehot2 = torch.full((b, a), float("nan"), device=DEV)
    _lib.qrdqn_act(_dev(theta), None, a, n, onehot2, None, dueling=dueling)   # no override table, no greedy output
    assert torch.equal(onehot2.cpu(), F.one_hot(torch.from_numpy(chosen).long(), a).float())


def test_refusals_launch_nothing():
    from accel_rl_amd import _lib
    lib = _lib.load()
    E_ARG, E_RANGE = -1, -2
    batch, rows, stride = 2, 66, 68                 # buffers large enough for every size named below
    theta = torch.zeros(batch, rows, stride, device=DEV)
    act = torch.zeros(batch, dtype=torch.uint8, device=DEV)
    ret = torch.zeros(batch, device=DEV)
    dth = torch.full_like(theta, 7.)
    rowsb, pri = torch.full((batch,), 7., device=DEV), torch.full((batch,), 7., device=DEV)
    onehot = torch.full((batch, rows), 7., device=DEV)
    greedy = torch.full((batch,), 7, dtype=torch.uint8, device=DEV)
    p = lambda t: t.data_ptr()                      # noqa: E731

    def loss(b=batch, a=6, n=8, s=8, kappa=1.0, pred=p(theta), out=p(dth), acts=p(act)):
        return lib.arl_qrdqn_loss(pred, p(theta), None, acts, p(ret), p(act), None, b, a, n, s, 0, 0.99, kappa, out,
                                  p(rowsb), p(pri), None)

    def serve(b=batch, a=6, n=8, s=8, th=p(theta), out=p(onehot)):
        return lib.arl_qrdqn_act(th, None, b, a, n, s, 0, out, p(greedy), None)

    for call in (loss, serve):
        assert call(n=1) == E_RANGE and b"qrdqn" in lib.arl_last_error()
        assert call(n=65, s=68) == E_RANGE
        assert call(a=65) == E_RANGE
        assert call(a=0) == E_RANGE
        assert call(s=10) == E_RANGE                # not a multiple of 4
        assert call(n=8, s=4) == E_RANGE            # below n_quantiles
        assert call(b=0) == E_RANGE
    assert loss(kappa=-1.0) == E_ARG and b"kappa" in lib.arl_last_error()
    assert loss(kappa=float("inf")) == E_ARG and loss(kappa=float("nan")) == E_ARG
    assert loss(pred=None) == E_ARG and b"null" in lib.arl_last_error()
    assert loss(out=None) == E_ARG and loss(acts=None) == E_ARG
    assert serve(th=None) == E_ARG and serve(out=None) == E_ARG
    torch.cuda.synchronize()
    for t in (dth, rowsb, pri, onehot):
        assert (t == 7.).all()
    assert (greedy == 7).all()
    assert loss() == 0 and serve() == 0             # the same calls inside the limits run
    torch.cuda.synchronize()
    assert not (dth.view(-1)[:batch * 6 * 8] == 7.).any() and not (onehot.view(-1)[:batch * 6] == 7.).any()


@pytest.mark.parametrize("shape,kappa", [(SHAPES[2], 1.0), (SHAPES[2], 0.0), (SHAPES[3], 1.0)])
def test_two_launches_are_bit_identical(shape, kappa):
    n_act, n, stride, batch, double, weighted, dueling = shape
    c = _case(11, n_act, n, stride, batch, double, weighted, dueling)
    gamma_n = float(np.float32(0.99 ** 3))
    one, two = _launch(c, n_act, n, gamma_n, kappa, dueling), _launch(c, n_act, n, gamma_n, kappa, dueling)
    assert torch.isfinite(one[0]).all()
    for x, y in zip(one, two):
        assert torch.equal(x, y)


# ---- policy and algorithm -----------------------------------------------------------------------------------------

def _make_policy(dueling, n_act=6, n_quantiles=8):
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_qr_dqn_policy import AtariQrDqnPolicy
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    set_seed(5)
    spec = dict(cnn_specs[0])
    policy = AtariQrDqnPolicy(epsilon=0.3, n_quantiles=n_quantiles, dueling=dueling, **spec)
    policy.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(n_act)), device=DEV)
    return policy, spec


def _ref_theta(rp, spec, x, n_act, n, dueling):
    """Plain torch on the reference layout: conv..., [hidden_Val (W, b), Val (W, b),] hidden (W, b), output (W, b)."""
    k = 0
    for i in range(len(spec["conv_filters"])):
        x = F.relu(F.conv2d(x, rp[k].flip(2, 3), rp[k + 1], stride=spec["conv_strides"][i],
                            padding=tuple(spec["conv_pads"][i])))
        k += 2
    x = x.flatten(1)
    if not dueling:
        return (F.relu(x @ rp[k] + rp[k + 1]) @ rp[k + 2] + rp[k + 3]).view(-1, n_act, n)
    val = F.relu(x @ rp[k] + rp[k + 1]) @ rp[k + 2] + rp[k + 3]
    adv = F.relu(x @ rp[k + 4] + rp[k + 5]) @ rp[k + 6] + rp[k + 7]
    return torch.cat([adv.view(-1, n_act, n), val.view(-1, 1, n)], dim=1)


def _torch_qr_loss(pred, tgt, pol, act, ret, term, isw, gamma_n, kappa, n_act, dueling):
    """The formulas once more in the tensors' own precision and device (for autograd through the whole network)."""
    b, n = pred.shape[0], pred.shape[2]
    full = (lambda t: merge(t, n_act)) if dueling else (lambda t: t)        # noqa: E731
    ar = torch.arange(b, device=pred.device)
    q = full(pol).mean(dim=2)
    top2 = torch.topk(q, 2, dim=1).values
    T = ret[:, None] + (1. - term.float())[:, None] * (gamma_n * full(tgt)[ar, q.argmax(dim=1)])
    u = T[:, None, :] - full(pred)[ar, act.long()][:, :, None]
    tau = (torch.arange(n, device=pred.device, dtype=pred.dtype) + 0.5) / n
    wt = (tau[None, :, None] - (u < 0).to(pred.dtype)).abs().detach()
    au = u.abs()
    rho = wt * torch.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa)) / kappa
    loss_b = rho.sum(dim=(1, 2)) / n
    return (isw * loss_b).mean(), loss_b.detach().clamp(1e-6, 1e6), (top2[:, 0] - top2[:, 1]).min().item()


@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
def test_training_step_matches_autograd_through_plain_torch(dueling):
    """One QuantileDQN minibatch (double DQN): gradients of every parameter in the reference's layout."""
    n_act, n, b = 6, 8, 6
    policy, spec = _make_policy(dueling)
    rows_, stride = n_act + int(dueling), policy._atom_stride
    # 8 quantiles, padded until rows x stride is a multiple of the MFMA k-tile (the categorical policy's rule)
    assert stride == (32 if dueling else 16) and (rows_ * stride) % 32 == 0 and policy._head_width == rows_ * stride
    assert policy._ref_shapes[-2] == (256, n_act * n) and policy.param_short_names[-2:] == ["OutputW", "Outputb"]
    if dueling:
        assert policy.param_short_names[-8:] == ["FCVal0W", "FCVal0b", "ValW", "Valb", "FC0W", "FC0b", "OutputW",
                                                 "Outputb"]
        assert policy._ref_shapes[-6] == (256, n)
    rs = np.random.RandomState(3)
    flat = policy.get_param_values()
    assert flat.size == policy.n_params == sum(int(np.prod(s)) for s in policy._ref_shapes)
    flat = flat + (rs.randn(flat.size) * 0.01).astype(np.float32)           # non-zero biases: layout errors would show
    policy.set_param_values(flat)
    np.testing.assert_array_equal(policy.get_param_values(), flat)          # round trip through the reference layout
    obs = torch.from_numpy(rs.randint(0, 256, size=(b, 4, 104, 80), dtype=np.uint8)).to(DEV)
    nxt = torch.from_numpy(rs.randint(0, 256, size=(b, 4, 104, 80), dtype=np.uint8)).to(DEV)
    act = torch.from_numpy(rs.randint(0, n_act, size=b).astype(np.uint8)).to(DEV)
    ret = torch.from_numpy(rs.randn(b).astype(np.float32)).to(DEV)
    term = torch.from_numpy((rs.rand(b) < 0.3).astype(np.uint8)).to(DEV)
    isw = torch.from_numpy((rs.rand(b) + 0.2).astype(np.float32)).to(DEV)
    policy.flat_target.copy_(policy.flat_params * 0.9)          # a target net that differs
    gamma_n = float(np.float32(0.99))
    policy.flat_grads.fill_(float("nan"))
    rows, pri = policy.qr_loss_and_grads(obs, nxt, act, ret, term, isw, gamma_n, 1.0, double_dqn=True)
    assert rows.data_ptr() + 4 * b == pri.data_ptr()            # the (2, b) buffer the optimizer's ring takes at once
    got = policy.bucket_to_reference(policy.flat_grads)

    def ref_params(flat_bucket):
        fl = policy.bucket_to_reference(flat_bucket)
        out, pos = [], 0
        for shape in policy._ref_shapes:
            m = int(np.prod(shape))
            out.append(torch.from_numpy(fl[pos:pos + m].reshape(shape).copy()).to(DEV).requires_grad_())
            pos += m
        return out
    rp, rt = ref_params(policy.flat_params), ref_params(policy.flat_target)
    scale = np.float32(1. / 255)
    pred = _ref_theta(rp, spec, obs.float() * scale, n_act, n, dueling)
    with torch.no_grad():
        tgt = _ref_theta(rt, spec, nxt.float() * scale, n_act, n, dueling)
        pol = _ref_theta(rp, spec, nxt.float() * scale, n_act, n, dueling)
    theta, _, _ = policy._logits(policy._scaled(obs))
    theta = theta.view(b, rows_, stride)
    assert torch.allclose(theta[:, :, :n], pred.detach(), rtol=1e-4, atol=1e-5) and not theta[:, :, n:].any()
    loss, pri_ref, margin = _torch_qr_loss(pred, tgt, pol, act, ret, term, isw, gamma_n, 1.0, n_act, dueling)
    assert margin > 1e-4, margin                                # the greedy next actions are away from fp32 ties
    grads = torch.autograd.grad(loss, rp)
    want = np.concatenate([g.detach().cpu().numpy().reshape(-1) for g in grads])
    assert abs(rows.sum().item() - loss.item()) <= 1e-4 * abs(loss.item())
    assert torch.allclose(pri, pri_ref, rtol=2e-3, atol=1e-5)
    assert np.allclose(got, want, rtol=2e-3, atol=2e-5 * max(np.abs(want).max(), 1e-3)), np.abs(got - want).max()
    greedy = policy.greedy_actions(nxt).cpu().numpy()           # served by arl_qrdqn_act
    qq = (merge(pol, n_act) if dueling else pol).mean(dim=2)
    np.testing.assert_array_equal(greedy, qq.argmax(dim=1).cpu().numpy())


def test_qr_dqn_trains_with_prioritized_replay_and_eval():
    """The categorical end-to-end configuration at toy size with QuantileDQN: GpuVecEvalSampler -> device replay
    (prioritized) -> quantile updates inside the captured graph -> target sync, epsilon / beta schedules; two seeded
    runs agree bit for bit."""
    from accel_rl_amd.algos.dqn.qr_dqn import QuantileDQN
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_qr_dqn_policy import AtariQrDqnPolicy
    from accel_rl_amd.runners.accel_rl import AccelRLEval
    from accel_rl_amd.sampler.gpu_sampler_with_eval import GpuVecEvalSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    finals = []
    for _ in range(2):
        sampler = GpuVecEvalSampler(eval_steps=8 * 40, eval_envs_per=1, EnvCls=SynthAtariEnv,
                                    env_args=dict(game="seaquest"), horizon=4, n_parallel=4, envs_per=2,
                                    max_path_length=25, max_decorrelation_steps=0, device=DEV)
        algo = QuantileDQN(batch_size=32, min_steps_learn=64 * 4, replay_size=64 * 60, training_intensity=8,
                           target_update_steps=64 * 3, reward_horizon=3, prioritized_replay=True,
                           double_dqn=True, eps_greedy_args=dict(anneal_steps=64 * 10))
        policy = AtariQrDqnPolicy(**cnn_specs[0], n_quantiles=16)
        runner = AccelRLEval(algo=algo, policy=policy, sampler=sampler, n_steps=64 * 24, seed=9,
                             eval_interval_steps=64 * 8)
        runner.train()
        tab = runner.last_tabular
        for key in ("StepsInEval", "TrajsInEval", "LossAverage", "PriorityAverage", "ReturnAverage", "ParamsNorm"):
            assert key in tab, key
        assert np.isfinite(tab["LossAverage"]) and tab["LossAverage"] > 0 and tab["TrajsInEval"] > 0
        assert algo._updates_per_optimize == 8 * 64 // 32 and abs(policy.get_epsilon() - 0.01) < 1e-9
        assert algo.replay_buffer.beta > 0.4
        finals.append(policy.get_param_values())
    assert np.isfinite(finals[0]).all()
    np.testing.assert_array_equal(finals[0], finals[1])
