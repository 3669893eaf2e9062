"""SAC-Discrete on the device (csrc/sac.hip: arl_sacd_act, arl_sacd_loss, arl_sacd_alpha_grad;
AtariSacDiscretePolicy, SacOptimizer, SacDiscrete).  The reference has none, so the yardsticks are the float64
restatements of tests/sacd_ref.py, whose docstring derives the tolerances used here.  Padding columns of every input
hold 1e9 and must be ignored; outputs are prefilled with NaN.  Every kernel test prints its largest error / bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sacd_ref as sr
from sacd_ref import EPS, GAMMA

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _launch_loss(c, gamma_n, delta_clip, log_alpha=None):
    from accel_rl_amd import _lib
    q1 = _dev(c["q1"])
    batch = q1.shape[0]
    dq1, dq2, dl = (torch.full_like(q1, NAN) for _ in range(3))
    stats = torch.full((4, batch), NAN, device=DEV)
    la = torch.tensor([c["log_alpha"] if log_alpha is None else log_alpha, NAN, NAN, NAN], dtype=torch.float32, device=DEV)
    _lib.sacd_loss(q1, _dev(c["q2"]), _dev(c["t1"]), _dev(c["t2"]), _dev(c["lo"]), _dev(c["ln"]), _dev(c["act"]),
                   _dev(c["ret"]), _dev(c["term"]), _dev(c["isw"]), la, c["n_act"], gamma_n, delta_clip, dq1, dq2, dl,
                   stats)
    torch.cuda.synchronize()
    return dq1.cpu(), dq2.cpu(), dl.cpu(), stats.cpu()


def _check_loss(c, gamma_n, delta_clip):
    """Bounds: tests/sacd_ref.py.  Returns the largest error / bound over td_abs, the three gradients and the rows."""
    A = c["n_act"]
    ref = sr.ref_loss(c, gamma_n, delta_clip)
    dq1, dq2, dl, stats = (t.double().numpy() for t in _launch_loss(c, gamma_n, delta_clip))
    for t in (dq1, dq2, dl, stats):
        assert np.isfinite(t).all()
    B = stats.shape[1]
    worst = 0.

    def within(got, want, atol, rtol=0.):
        nonlocal worst
        tol = atol + rtol * np.abs(want)
        ratio = np.where(np.abs(got - want) == 0, 0., np.abs(got - want) / np.maximum(tol, 1e-300)).max()
        worst = max(worst, ratio)
        assert ratio <= 1, ratio

    within(stats[1], ref["td"], ref["td_atol"])
    within(stats[0], ref["rows"], ref["rows_atol"])
    for got, key in ((dq1, "dq1"), (dq2, "dq2")):
        within(got[:, :A], ref[key], (ref["w"] * ref["td_atol"])[:, None], 2e-4)
        other = np.ones(got.shape, bool)
        other[np.arange(B), ref["act"]] = False
        assert not got[other].any()                             # exact zeros: the padding and every action not taken
    within(dl[:, :A], ref["dlogits"], ref["dl_atol"][:, None], 2e-4)
    assert not dl[:, A:].any()                                  # exact zeros in the padding
    assert (np.abs(dl[:, :A].sum(axis=1)) <= A * ref["dl_atol"]).all()
    within(stats[2], ref["pi_rows"], ref["pi_atol"], 2e-4)
    within(stats[3], ref["ent"], ref["ent_atol"], 2e-4)
    return worst


@pytest.mark.parametrize("delta_clip", [None, 1.0], ids=["squared", "huber"])
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("shape", sr.SHAPES, ids=lambda s: "A%d-S%d-B%d" % s)
def test_loss_statistics_and_three_gradients_vs_float64(shape, weighted, delta_clip):
    n_act, stride, batch = shape
    c = sr.case(sr.seed_of(shape, weighted), n_act, stride, batch, weighted,
                shift=sr.SHAPES.index(shape) + 3 * int(weighted))
    worst = _check_loss(c, GAMMA, delta_clip)
    print("SAC-D A%d S%d B%d %s %s: largest error / bound %.3f" % (n_act, stride, batch, "weighted" if weighted else "uniform",
                                                                  "huber" if delta_clip else "squared", worst))


def test_cases_hold_every_special_row():
    seen, ents, hot = set(), [], []
    orders = set()
    terminal = set()
    for k, shape in enumerate(sr.SHAPES):
        n_act, stride, batch = shape
        for weighted in (False, True):
            c = sr.case(sr.seed_of(shape, weighted), n_act, stride, batch, weighted, shift=k + 3 * int(weighted))
            ref = sr.ref_loss(c, GAMMA, 1.0)
            seen.update(c["kinds"].tolist())
            terminal.update(c["term"].tolist())
            act = ref["act"]
            assert (act < n_act).all() and ((c["act"] >= n_act) == (c["kinds"] == sr.ACT_OUTSIDE)).all()
            for b, kind in enumerate(c["kinds"]):
                q1a, q2a = c["q1"][b, act[b]], c["q2"][b, act[b]]
                orders.add(("taken", int(np.sign(q1a - q2a))))
                for key1, key2 in (("q1", "q2"), ("t1", "t2")):
                    orders.update((key1, int(s)) for s in np.sign(c[key1][b, :n_act] - c[key2][b, :n_act]))
                if n_act > 1 and kind == sr.ALL_EQUAL:
                    ents.append(abs(ref["ent"][b] - np.log(n_act)))
                if n_act > 1 and kind == sr.ONE_HOT:
                    z = np.sort(c["lo"][b, :n_act].astype(np.float64))
                    zn = np.sort(c["ln"][b, :n_act].astype(np.float64))
                    hot.append((z[-1] - z[-2], zn[-1] - zn[-2], ref["pi"][b].max()))
    assert seen == set(range(sr.N_KINDS)) and terminal == {0, 1}
    assert orders >= {(k, s) for k in ("taken", "q1", "t1") for s in (-1, 0, 1)}
    assert ents and max(ents) < 1e-12
    assert hot and all(g > 88 and gn > 88 and p == 1.0 for g, gn, p in hot)


def test_values_of_magnitude_1e4_stay_finite_and_within_the_bound():
    c = sr.case(77, 18, 32, 65, True, scale=1e4, shift=1)
    assert np.abs(c["t1"][:, :18]).max() > 1e4 and np.abs(c["q1"][:, :18]).max() > 1e4
    worst = max(_check_loss(c, GAMMA, clip) for clip in (None, 1.0))
    print("SAC-D |q| ~ 1e4: largest error / bound %.3f" % worst)


@pytest.mark.parametrize("n_act,stride,batch", [(1, 4, 1), (6, 32, 33), (18, 32, 65)])
def test_reduces_to_dqn_bit_for_bit(n_act, stride, batch):
    """log_alpha = -inf (alpha == 0), q2t_next == q1t_next, integer-valued inputs, logits_next ahead by 100 at the unique
    maximum of q1t_next: soft == that maximum, and dq1 / td_abs equal arl_dqn_loss's on (q1, q1t_next), pol_next NULL."""
    from accel_rl_amd import _lib
    rs = np.random.RandomState(5 + n_act)
    c = sr.case(9 + n_act, n_act, stride, batch, True)
    c["act"] = rs.randint(0, n_act, size=batch).astype(np.uint8)
    for key in ("q1", "q2", "t1", "lo", "ln"):
        c[key][:, :n_act] = rs.randint(-8, 9, size=(batch, n_act))
    best = rs.randint(0, n_act, size=batch)
    c["t1"][np.arange(batch), best] = 12
    c["ln"][np.arange(batch), best] = 120
    c["t2"] = c["t1"].copy()
    c["q2"] = c["q1"].copy()                                    # (then td_abs = (p + p) / 2 = p)
    c["ret"] = rs.randint(-4, 5, size=batch).astype(np.float32)
    for delta_clip in (1.0, None):
        dq1, dq2, _, stats = _launch_loss(c, GAMMA, delta_clip, log_alpha=float("-inf"))
        q = _dev(c["q1"])
        dq = torch.full_like(q, NAN)
        rows, td = torch.full((batch,), NAN, device=DEV), torch.full((batch,), NAN, device=DEV)
        _lib.dqn_loss(q, _dev(c["t1"]), None, _dev(c["act"]), _dev(c["ret"]), _dev(c["term"]), _dev(c["isw"]), n_act,
                      GAMMA, delta_clip, dq, rows, td)
        torch.cuda.synchronize()
        assert torch.isfinite(dq).all() and (batch == 1 or dq.abs().sum() > 0)
        assert torch.equal(dq1, dq.cpu()) and torch.equal(dq2, dq.cpu()) and torch.equal(stats[1], td.cpu())
        assert torch.isfinite(stats).all()


# ---- arl_sacd_act ---------------------------------------------------------------------------------------------------

def _launch_act(logits, n_act, override=None, deterministic=False):
    from accel_rl_amd import _lib
    batch = logits.shape[0]
    prob = torch.full((batch, n_act), NAN, device=DEV)
    greedy = torch.full((batch,), 255, dtype=torch.uint8, device=DEV)
    _lib.sacd_act(_dev(logits), _dev(override), n_act, prob, greedy, deterministic=deterministic)
    torch.cuda.synchronize()
    return prob.cpu().double().numpy(), greedy.cpu().numpy()


@pytest.mark.parametrize("shape", sr.SHAPES + [(6, 32, 257)], ids=lambda s: "A%d-S%d-B%d" % s)
def test_act_softmax_rows_ties_override_and_deterministic_mode(shape):
    n_act, stride, batch = shape
    c = sr.case(31 + n_act, n_act, stride, batch, False, shift=n_act)
    z = c["lo"]
    if n_act > 1:                                               # ties: two equal maxima, the first one is the greedy action
        z[0, :n_act] = -1.0
        z[0, n_act - 1] = z[0, n_act // 2] = 3.0
    want, greedy, atol = sr.ref_act(z, n_act)
    got, g = _launch_act(z, n_act)
    assert np.isfinite(got).all() and (np.abs(got - want) <= atol).all()
    print("act A%d B%d: largest soft-max error / bound %.3f" % (n_act, batch, (np.abs(got - want) / atol).max()))
    assert (np.abs(got.sum(axis=1) - 1.0) <= 4 * 2.0 ** -23 * n_act).all()
    assert (g == greedy).all() and (n_act == 1 or g[0] == n_act // 2)
    # deterministic mode: one-hot at the first maximum
    got_d, g_d = _launch_act(z, n_act, deterministic=True)
    assert (g_d == greedy).all() and (got_d == np.eye(n_act)[greedy]).all()
    # an override forces its action in either mode; -1 forces nothing; greedy stays the first maximum
    rs = np.random.RandomState(n_act)
    ov = np.where(rs.rand(batch) < 0.5, rs.randint(0, n_act, size=batch), -1).astype(np.int32)
    ov[0] = n_act - 1
    for det in (False, True):
        want_o, _, _ = sr.ref_act(z, n_act, override=ov, deterministic=det)
        got_o, g_o = _launch_act(z, n_act, override=ov, deterministic=det)
        forced = ov >= 0
        assert (got_o[forced] == want_o[forced]).all() and (g_o == greedy).all()
        assert (got_o[~forced] == (got_d if det else got)[~forced]).all()


# ---- arl_sacd_alpha_grad --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch", [1, 3, 65, 700])
def test_alpha_grad_vs_float64_and_its_sign(batch):
    from accel_rl_amd import _lib
    rs = np.random.RandomState(batch)
    ent = (rs.rand(batch) * 1.5 + 0.1).astype(np.float32)
    mean = float(ent.astype(np.float64).mean())
    for log_alpha in (-1.3, 0.0, 0.8):
        for target in (mean - 0.4, mean + 0.4):
            la = torch.tensor([log_alpha, NAN, NAN, NAN], dtype=torch.float32, device=DEV)
            out = torch.full((4,), NAN, device=DEV)
            _lib.sacd_alpha_grad(_dev(ent), la, target, out)
            torch.cuda.synchronize()
            got = out.cpu().double().numpy()
            want, atol = sr.ref_alpha_grad(ent, np.float32(log_alpha), float(np.float32(target)))
            assert abs(got[0] - want) <= atol, (got[0], want, atol)
            assert (got[0] > 0) == (target < mean)              # entropy above the target: the gradient lowers alpha
            assert (got[1:] == 0).all() and not np.signbit(got[1:]).any()


# ---- refusals and determinism ---------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    from accel_rl_amd import _lib
    lib = _lib.load()
    batch = 2
    rows = torch.zeros(batch, 260, device=DEV)                              # large enough for every size named below
    act = torch.zeros(batch, dtype=torch.uint8, device=DEV)
    ret = torch.zeros(batch, device=DEV)
    la = torch.zeros(4, device=DEV)
    nans = lambda *shape: torch.full(shape, NAN, device=DEV)                # noqa: E731
    dq1, dq2, dl, stats, prob, grad = nans(batch, 260), nans(batch, 260), nans(batch, 260), nans(4, batch), nans(batch, 256), nans(4)
    greedy = torch.full((batch,), 255, dtype=torch.uint8, device=DEV)
    p = lambda t: t.data_ptr()                                              # noqa: E731
    r = p(rows)

    def loss(q1=r, q2=r, t1=r, t2=r, lo=r, ln=r, acts=p(act), rets=p(ret), terms=p(act), log_alpha=p(la), o1=p(dq1),
             o2=p(dq2), o3=p(dl), st=p(stats), b=batch, a=6, s=8, gamma=0.99, clip=1.0):
        return lib.arl_sacd_loss(q1, q2, t1, t2, lo, ln, acts, rets, terms, None, log_alpha, b, a, s, gamma, clip, o1, o2,
                                 o3, st, None)

    def serve(lo=r, out=p(prob), b=batch, a=6, s=8):
        return lib.arl_sacd_act(lo, None, b, a, s, 0, out, p(greedy), None)

    def agrad(ent=r, log_alpha=p(la), out=p(grad), b=batch, target=0.5):
        return lib.arl_sacd_alpha_grad(ent, b, log_alpha, target, out, None)

    for name in ("q1", "q2", "t1", "t2", "lo", "ln", "acts", "rets", "terms", "log_alpha", "o1", "o2", "o3", "st"):
        assert loss(**{name: None}) == -1 and b"null" in lib.arl_last_error(), name
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert loss(gamma=bad) == -1 and b"gamma_n" in lib.arl_last_error()
        assert loss(clip=bad) == -1 and b"delta_clip" in lib.arl_last_error()
        assert agrad(target=bad) == -1 and b"target_entropy" in lib.arl_last_error()
    for kw in (dict(b=0), dict(b=-1), dict(b=2 ** 31), dict(a=0), dict(a=256, s=256), dict(s=10), dict(a=6, s=4)):
        assert loss(**kw) == -2, kw                                         # the sizes of arl_dqn_loss: ARL_E_RANGE
        assert serve(**kw) == -2, kw
    assert serve(lo=None) == -1 and serve(out=None) == -1
    assert agrad(ent=None) == -1 and agrad(log_alpha=None) == -1 and agrad(out=None) == -1
    assert agrad(b=0) == -2 and agrad(b=2 ** 31) == -2
    torch.cuda.synchronize()
    for t in (dq1, dq2, dl, stats, prob, grad):
        assert torch.isnan(t).all()
    assert (greedy == 255).all()
    assert loss() == 0 and serve() == 0 and agrad() == 0 and loss(a=255, s=256) == 0 and serve(a=255, s=256) == 0
    torch.cuda.synchronize()                                                # inside the limits they run
    for t in (dq1, dq2, dl):
        assert torch.isfinite(t.view(-1)[:batch * 256]).all()
    assert torch.isfinite(stats).all() and torch.isfinite(grad).all() and (greedy == 0).all()


def test_two_launches_are_bit_identical():
    c = sr.case(21, 18, 32, 257, True)
    one, two = _launch_loss(c, GAMMA, 1.0), _launch_loss(c, GAMMA, 1.0)
    assert torch.isfinite(one[3]).all() and all(torch.equal(x, y) for x, y in zip(one, two))
    from accel_rl_amd import _lib
    ent, la = one[3][3].to(DEV).contiguous(), torch.tensor([0.3, 0, 0, 0], dtype=torch.float32, device=DEV)
    outs = []
    for _ in range(2):
        out = torch.full((4,), NAN, device=DEV)
        _lib.sacd_alpha_grad(ent, la, 1.0, out)
        outs.append(out.cpu())
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


# ---- policy, optimizer, algorithm -----------------------------------------------------------------------------------

N_ACT, BATCH = 6, 8


def _make_policy(seed=5, **kw):
    """The small network (2 conv layers, hidden 64, 6 actions) three times over, with perturbed parameters and critic
    targets that differ from the online critics."""
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_sac_discrete_policy import AtariSacDiscretePolicy
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    set_seed(seed)
    spec = dict(cnn_specs[0], hidden_sizes=[64])
    policy = AtariSacDiscretePolicy(initial_alpha=0.6, **spec, **kw)
    policy.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(N_ACT)), device=DEV)
    rs = np.random.RandomState(3)
    flat = policy.get_param_values()
    policy.set_param_values(flat + (rs.randn(flat.size) * 0.01).astype(np.float32))
    policy.log_alpha[0] = float(np.log(0.6))                    # (the perturbation moved it too)
    for critic in (policy.q1, policy.q2):
        critic.flat_target.copy_(critic.flat_params * 0.9)
    return policy, spec


def _minibatch(seed, b=BATCH, ret_scale=0.05):
    rs = np.random.RandomState(seed)
    return dict(obs=_dev(rs.randint(0, 256, size=(b, 4, 104, 80), dtype=np.uint8)),
                nxt=_dev(rs.randint(0, 256, size=(b, 4, 104, 80), dtype=np.uint8)),
                act=_dev(rs.randint(0, N_ACT, size=b).astype(np.uint8)),
                ret=_dev((rs.randn(b) * ret_scale).astype(np.float32)),
                term=_dev((rs.rand(b) < 0.3).astype(np.uint8)), isw=_dev((rs.rand(b) + 0.2).astype(np.float32)))


def _ref_params(net, flat_bucket):
    fl = net.bucket_to_reference(flat_bucket)
    out, pos = [], 0
    for shape in net._ref_shapes:
        m = int(np.prod(shape))
        out.append(torch.from_numpy(fl[pos:pos + m].reshape(shape).astype(np.float64)).requires_grad_())
        pos += m
    return out


def _ref_net(rp, spec, x):
    """float64 plain torch on the reference layout: conv stack, one hidden layer, the output layer."""
    k = 0
    for i in range(len(spec["conv_filters"])):
        x = F.relu(F.conv2d(x, rp[k].flip(2, 3), rp[k + 1], stride=spec["conv_strides"][i],
                            padding=tuple(spec["conv_pads"][i])))
        k += 2
    return F.relu(x.flatten(1) @ rp[k] + rp[k + 1]) @ rp[k + 2] + rp[k + 3]


def test_sac_training_step_matches_autograd_through_plain_torch():
    """One eager SacOptimizer step.  The gradients of all three networks and of log_alpha and the four statistics rows
    against float64 autograd over the same three networks, at the bars of
    test_mdqn_training_step_matches_autograd_through_plain_torch; then the updated parameters of the three networks and
    log_alpha against a float64 Adam step from the parameters before (adam is not linear in the gradient, so the bars
    on the gradient do not carry over to the step: it is taken from the device's own gradients, to 1e-5 of the step)."""
    from accel_rl_amd.optimizers import update_methods
    from accel_rl_amd.optimizers.dqn import SacOptimizer
    policy, spec = _make_policy()
    mb = _minibatch(4)
    mb["term"][0], mb["term"][1] = 1, 0                       # a terminal row (|d| small) and one that bootstraps
    clip, target_entropy = 0.5, 0.5
    nets = (policy, policy.q1, policy.q2)
    targets_before = [c.flat_target.clone() for c in nets[1:]]
    before = [n.flat_params.clone() for n in nets] + [policy.log_alpha.clone()]
    lr, a_lr, eps = 3e-4, 1e-3, 1e-4
    opt = SacOptimizer(lr, update_methods.adam, update_method_args=dict(epsilon=eps), use_graph=False,
                       alpha_args=dict(learning_rate=a_lr))
    seen = {}

    def loss(inputs):
        for n in nets:
            n.flat_grads.fill_(NAN)
        stats = policy.sac_loss_and_grads(*inputs, GAMMA, clip, target_entropy)
        seen["stats"] = stats.clone()
        seen["grads"] = [n.flat_grads.clone() for n in nets] + [policy.log_alpha_grad.clone()]
        return stats[1], stats[0]
    opt.initialize(inputs=["obs", "next_obs", "act", "disc_n_return", "terminal", "importance_sample_weights"], loss=loss,
                   target=policy)
    opt.optimize((mb["obs"], mb["nxt"], mb["act"], mb["ret"], mb["term"], mb["isw"]))
    torch.cuda.synchronize()
    stats = seen["stats"].cpu().double()
    # ---- float64 plain torch over the same three networks
    rp = [_ref_params(n, b) for n, b in zip(nets, before)]
    rt = [_ref_params(n, t) for n, t in zip(nets[1:], targets_before)]
    scale = float(np.float32(1. / 255))
    obs, nxt = mb["obs"].cpu().double() * scale, mb["nxt"].cpu().double() * scale
    log_alpha = before[3][:1].cpu().double().requires_grad_()
    alpha = log_alpha.exp().detach()
    logits, q1, q2 = (_ref_net(p, spec, obs) for p in rp)
    with torch.no_grad():
        lpn = torch.log_softmax(_ref_net(rp[0], spec, nxt), dim=1)
        soft = (lpn.exp() * (torch.minimum(_ref_net(rt[0], spec, nxt), _ref_net(rt[1], spec, nxt)) - alpha * lpn)).sum(dim=1)
        y = mb["ret"].cpu().double() + (1. - mb["term"].cpu().double()) * GAMMA * soft
    ar, act = torch.arange(BATCH), mb["act"].cpu().long()
    w = mb["isw"].cpu().double() / BATCH
    d1, d2 = y - q1[ar, act], y - q2[ar, act]
    huber = lambda d: torch.where(d.abs() <= clip, 0.5 * d * d, clip * (d.abs() - clip / 2.))     # noqa: E731
    want_rows = w * huber(d1) + w * huber(d2)
    both = torch.cat([d1, d2]).abs()
    assert (both < clip).any() and (both > clip).any()          # both branches of the Huber loss in play
    want_td = (d1.abs().clamp(max=clip) + d2.abs().clamp(max=clip)) / 2
    lp = torch.log_softmax(logits, dim=1)
    want_pi = (lp.exp() * (alpha * lp - torch.minimum(q1, q2).detach())).sum(dim=1) / BATCH
    want_ent = -(lp.exp() * lp).sum(dim=1)
    alpha_loss = log_alpha.exp() * (want_ent.detach().mean() - target_entropy)
    for got, want in zip(stats, (want_rows, want_td, want_pi, want_ent)):
        assert np.allclose(got.numpy(), want.detach().numpy(), rtol=2e-3, atol=0)
    want_grads = [torch.autograd.grad(want_pi.sum(), rp[0]), torch.autograd.grad(want_rows.sum(), rp[1] + rp[2])]
    want_grads = [want_grads[0], want_grads[1][:len(rp[1])], want_grads[1][len(rp[1]):]]
    for net, got_flat, want in zip(nets, seen["grads"], want_grads):
        got = net.bucket_to_reference(got_flat)
        want = np.concatenate([g.detach().numpy().reshape(-1) for g in want])
        print("max grad err %.3g of max |grad| %.3g" % (np.abs(got - want).max(), np.abs(want).max()))
        assert np.abs(want).max() > 0
        assert np.allclose(got, want, rtol=2e-3, atol=2e-5 * max(np.abs(want).max(), 1e-3)), np.abs(got - want).max()
    want_ga, = torch.autograd.grad(alpha_loss, log_alpha)
    got_ga = seen["grads"][3].cpu().double()
    assert abs(got_ga[0].item() - want_ga.item()) <= 2e-3 * abs(want_ga.item()) and not got_ga[1:].any()
    # ---- the four updates: one float64 Adam step each, from the device's own gradients, every range its own
    after = [n.flat_params for n in nets] + [policy.log_alpha]
    moved = []
    for p0, p1, g, rate in zip(before, after, seen["grads"], (lr, lr, lr, a_lr)):
        p0, p1, g = p0.cpu().double(), p1.cpu().double(), g.cpu().double()
        m, v = 0.1 * g, 0.001 * g * g
        step = rate * np.sqrt(1 - 0.999) / (1 - 0.9) * m / (v.sqrt() + eps)
        err = (p1 - (p0 - step)).abs()
        assert (err <= 4 * EPS * p0.abs() + 1e-5 * step.abs() + 1e-12).all(), err.max().item()
        moved.append(step.abs().max().item())
    assert all(s > 1e-6 for s in moved)                         # every range moved, log_alpha too
    assert not after[3][1:].any()                               # entries 1 .. 3 of the log_alpha bucket stay 0
    for critic, t in zip(nets[1:], targets_before):
        assert torch.equal(critic.flat_target, t)               # the target critics are read, never written


def _algo(use_graph, **kw):
    from accel_rl_amd.algos.dqn.sac_discrete import SacDiscrete
    return SacDiscrete(batch_size=BATCH, prioritized_replay=True, delta_clip=1.0, optimizer_args=dict(use_graph=use_graph),
                       **kw)


def test_captured_updates_equal_eager_updates_bit_for_bit():
    """SacOptimizer(use_graph=True): two eager warm-up calls, the capture, then replays -- five updates in all --
    against five eager updates from the same start: the three networks, log_alpha (read inside the kernels, so every
    replay sees the last update of it) and the priorities."""
    batches = [_minibatch(30 + i) for i in range(5)]
    runs = []
    for use_graph in (True, False):
        policy, _ = _make_policy()
        algo = _algo(use_graph)
        inputs, loss = algo.build_loss(None, policy)
        assert len(inputs) == 6
        algo.optimizer.initialize(inputs=inputs, loss=loss, target=policy)
        steps = []
        for mb in batches:
            priority, _ = algo.optimizer.optimize((mb["obs"], mb["nxt"], mb["act"], mb["ret"], mb["term"], mb["isw"]))
            torch.cuda.synchronize()
            steps.append((priority.clone(), policy.flat_params.clone(), policy.q1.flat_params.clone(),
                          policy.q2.flat_params.clone(), policy.log_alpha.clone()))
        assert (algo.optimizer._graph is not None) == use_graph
        runs.append(steps)
        del algo
    for graph_step, eager_step in zip(*runs):
        for x, y in zip(graph_step, eager_step):
            assert torch.isfinite(x).all() and torch.equal(x, y)
    for k in range(1, 5):                                       # every range moved in every update
        assert all(not torch.equal(runs[0][k - 1][i], runs[0][k][i]) for i in (1, 2, 3, 4))


@pytest.mark.parametrize("scale,rises", [(1.5, True), (0.2, False)], ids=["target-above", "target-below"])
def test_sac_discrete_trains_with_prioritized_replay_eval_and_resume(scale, rises):
    """End to end at toy size: GpuVecEvalSampler -> device replay (prioritized) -> SAC updates inside the captured graph
    -> target copies, the beta schedule, one evaluation in deterministic mode, snapshot and resume.  The actor starts
    near uniform (entropy ~ log A): a target above it must raise log_alpha, a target below it lower it."""
    from accel_rl_amd.algos.dqn.sac_discrete import SacDiscrete
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_sac_discrete_policy import AtariSacDiscretePolicy
    from accel_rl_amd.runners.accel_rl import AccelRLEval
    from accel_rl_amd.sampler.gpu_sampler_with_eval import GpuVecEvalSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecEvalSampler(eval_steps=8 * 40, eval_envs_per=1, EnvCls=SynthAtariEnv,
                                env_args=dict(game="seaquest"), horizon=4, n_parallel=4, envs_per=2,
                                max_path_length=25, max_decorrelation_steps=0, device=DEV)
    algo = SacDiscrete(batch_size=32, min_steps_learn=64 * 4, replay_size=64 * 60, training_intensity=8,
                       target_update_steps=64 * 3, prioritized_replay=True, target_entropy_scale=scale)
    policy = AtariSacDiscretePolicy(**cnn_specs[0])
    first, modes = {}, []
    initialize, set_deterministic = policy.initialize, policy.set_deterministic

    def recording_initialize(*a, **kw):
        initialize(*a, **kw)
        first["params"] = policy.get_param_values()
        first["targets"] = [c.flat_target.clone() for c in (policy.q1, policy.q2)]

    def recording_set_deterministic(flag):
        modes.append(bool(flag))
        set_deterministic(flag)
    policy.initialize, policy.set_deterministic = recording_initialize, recording_set_deterministic
    runner = AccelRLEval(algo=algo, policy=policy, sampler=sampler, n_steps=64 * 24, seed=9, eval_interval_steps=64 * 8)
    runner.train()
    tab = runner.last_tabular
    for key in ("StepsInEval", "TrajsInEval", "LossAverage", "PriorityAverage", "PiLossAverage", "EntropyAverage",
                "AlphaAverage", "ReturnAverage"):
        assert key in tab and np.isfinite(tab[key]), key
    assert tab["LossAverage"] > 0 and tab["PriorityAverage"] > 0 and tab["TrajsInEval"] > 0
    assert 0 < tab["EntropyAverage"] <= np.log(policy.n_act) * (1 + 1e-6) and tab["AlphaAverage"] > 0
    assert algo._updates_per_optimize == 8 * 64 // 32 and algo.replay_buffer.beta > 0.4
    assert abs(algo.target_entropy - scale * np.log(policy.n_act)) < 1e-6
    log_alpha = policy.log_alpha.cpu().numpy()
    assert np.isfinite(log_alpha).all() and not log_alpha[1:].any()
    assert (log_alpha[0] > 1e-3) if rises else (log_alpha[0] < -1e-3)       # initial_alpha = 1: it started at 0
    final = policy.get_param_values()
    sizes = policy._param_sizes()
    assert np.isfinite(final).all() and final.size == sum(sizes) == policy.n_params
    ends = np.cumsum(sizes)
    for lo, hi in zip(ends - sizes, ends):                      # every part moved: actor, q1, q2, log_alpha
        assert not np.array_equal(final[lo:hi], first["params"][lo:hi])
    for critic, t0 in zip((policy.q1, policy.q2), first["targets"]):
        assert torch.isfinite(critic.flat_target).all() and not torch.equal(critic.flat_target, t0)     # copied
    assert modes and modes[0] is True and modes[-1] is False and not policy.get_deterministic()         # the evaluation
    # deterministic mode serves only greedy actions
    obs = torch.randint(0, 256, (16,) + tuple(policy._obs_shape), dtype=torch.uint8, device=DEV)
    soft_rows, _ = policy.prob_value(obs)
    assert ((soft_rows > 0) & (soft_rows < 1)).all()
    policy.set_deterministic(True)
    onehot, _ = policy.prob_value(obs)
    greedy = policy.greedy_actions(obs).long()
    assert torch.equal(onehot, torch.eye(policy.n_act, device=DEV)[greedy])
    policy.set_deterministic(False)
    # snapshot and resume: actor | q1 | q2 | log_alpha survive
    snap = runner.get_itr_snapshot(0)["policy_param_values"]
    np.testing.assert_array_equal(snap, final)
    resumed = AtariSacDiscretePolicy(initial_param_values=snap, **cnn_specs[0])
    resumed.initialize(policy.env_spec, device=DEV)
    np.testing.assert_array_equal(resumed.get_param_values(), final)
    assert torch.equal(resumed.flat_params, policy.flat_params) and torch.equal(resumed.q2.flat_params, policy.q2.flat_params)
    assert torch.equal(resumed.log_alpha, policy.log_alpha)


def test_host_draws_and_serve_group_draw_from_the_softmax_row():
    """The samplers' two serving paths: prob_value hands out the soft-max row and host_draws the uniforms to draw from it;
    serve_group (a sampler that feeds its categorical kernel 0.5) draws the group's actions itself, from its slice of
    the same uniforms, and serves them as one-hot rows."""
    from accel_rl_amd import _lib
    policy, _ = _make_policy()
    horizon, n_envs, row0, b = 3, 8, 4, 4
    state = np.random.get_state()
    u = policy.host_draws(horizon, n_envs)
    np.random.set_state(state)
    np.testing.assert_array_equal(u, np.random.rand(horizon * n_envs))      # the reference-order uniforms, nothing else drawn
    assert (policy._overrides[n_envs][1] == -1).all() and tuple(policy._overrides[n_envs][1].shape) == (horizon, n_envs)
    obs = _minibatch(8, b=n_envs)["obs"]
    policy.set_step(1)
    soft_rows, value = policy.prob_value(obs)
    assert ((soft_rows > 0) & (soft_rows < 1)).all() and not value.any()
    want = torch.empty(b, dtype=torch.uint8, device=DEV)
    _lib.sample_categorical(soft_rows[row0:row0 + b].contiguous(), _dev(u.reshape(horizon, n_envs)[1, row0:row0 + b].copy()), want)
    onehot, _ = policy.serve_group(obs[row0:row0 + b], row0, n_envs)
    assert torch.equal(onehot, torch.eye(N_ACT, device=DEV)[want.long()])
    policy.set_deterministic(True)
    onehot, _ = policy.serve_group(obs[row0:row0 + b], row0, n_envs)
    assert torch.equal(onehot, torch.eye(N_ACT, device=DEV)[policy.greedy_actions(obs[row0:row0 + b]).long()])
    policy.set_step(horizon)
    with pytest.raises(IndexError):
        policy.serve_group(obs[row0:row0 + b], row0, n_envs)
