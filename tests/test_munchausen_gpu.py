"""Munchausen DQN / IQN on the device (csrc/dqn.hip: arl_mdqn_loss, csrc/iqn.hip: arl_miqn_loss,
AtariDqnPolicy / AtariIqnPolicy.munchausen_loss_and_grads, MunchausenDQN, MunchausenIQN).  The reference has neither, so
the yardsticks are the float64 restatements of tests/munchausen_ref.py, whose docstring derives the tolerances used
here (the same cases run through an fp32 emulation in tests/test_munchausen_host.py).  Padding columns of every input
hold 1e9 and must be ignored; outputs are prefilled with NaN.  Every kernel test prints its largest error / bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import munchausen_ref as mr
from munchausen_ref import ALPHA, EPS, GAMMA, L0

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ---- M-DQN kernel ---------------------------------------------------------------------------------------------------

def _launch_mdqn(c, gamma_n, delta_clip, tau_e, alpha=ALPHA, l0=L0, baseline=False):
    """baseline: arl_dqn_loss with pol_next_q NULL on the same rows."""
    from accel_rl_amd import _lib
    q = _dev(c["q"])
    batch = q.shape[0]
    dq = torch.full_like(q, NAN)
    rows, td = torch.full((batch,), NAN, device=DEV), torch.full((batch,), NAN, device=DEV)
    args = (_dev(c["act"]), _dev(c["ret"]), _dev(c["term"]), _dev(c["isw"]), c["n_act"], gamma_n, delta_clip)
    if baseline:
        _lib.dqn_loss(q, _dev(c["nxt"]), None, *args, dq, rows, td, dueling=c["dueling"])
    else:
        _lib.mdqn_loss(q, _dev(c["nxt"]), _dev(c["cur"]), *args, tau_e, alpha, l0, dq, rows, td, dueling=c["dueling"])
    torch.cuda.synchronize()
    return dq.cpu(), rows.cpu(), td.cpu()


def _check_mdqn(c, gamma_n, delta_clip, tau_e):
    """Bounds: tests/munchausen_ref.py (M-DQN).  Returns the largest td_abs error / bound."""
    ref = mr.ref_mdqn(c, gamma_n, delta_clip, tau_e)
    dq, rows, td = _launch_mdqn(c, gamma_n, delta_clip, tau_e)
    cols = c["n_act"] + int(c["dueling"])
    assert torch.isfinite(dq).all() and torch.isfinite(rows).all() and torch.isfinite(td).all()
    atol = ref["atol"]
    td_err = (td.double() - ref["td"]).abs()
    ratio = (td_err / atol).max().item()
    assert (td_err <= atol).all(), ratio
    rows_tol = ref["w"] * (ref["slope"].abs() * atol + 0.5 * atol * atol) + 4 * EPS * ref["rows"].abs()
    assert ((rows.double() - ref["rows"]).abs() <= rows_tol).all()
    g_err = (dq[:, :cols].double() - ref["grad"]).abs()
    assert (g_err <= ref["w"].max() * atol[:, None] + 1e-5 * ref["grad"].abs()).all(), g_err.max().item()
    assert not dq[:, cols:].any()                               # exact zeros in the padding
    return ratio


@pytest.mark.parametrize("tau_e", mr.TAUS_E)
@pytest.mark.parametrize("batch", mr.MDQN_BATCHES)
@pytest.mark.parametrize("n_act,dueling", [(a, d) for a in mr.MDQN_ACTIONS for d in (False, True) if a <= 18 or not d],
                         ids=lambda v: ("dueling" if v else "plain") if isinstance(v, bool) else "A%d" % v)
def test_mdqn_loss_priorities_and_gradient_vs_float64(n_act, dueling, batch, tau_e):
    worst = 0.
    for weighted in (False, True):
        c = mr.mdqn_case(mr.mdqn_seed(n_act, batch, dueling, weighted), n_act, batch, dueling, weighted,
                         shift=n_act + int(dueling) + 3 * int(weighted))
        lp = mr.ref_mdqn(c, GAMMA, 1.0, tau_e)["lp_act"].numpy()
        if batch >= mr.N_KINDS:                                 # every special row is there, and does what it is there for
            assert set(c["kinds"].tolist()) == set(range(mr.N_KINDS)) and c["term"].any() and not c["term"].all()
            assert (lp[c["kinds"] == mr.LP_ZERO] == 0).all()
            if n_act > 1:
                assert (lp[c["kinds"] == mr.CLIPPED] < L0).all()
                assert np.allclose(lp[c["kinds"] == mr.ALL_EQUAL], -tau_e * np.log(n_act), rtol=1e-9)
                two = c["nxt"][c["kinds"] == mr.TWO_MAXIMA][:, :n_act]
                assert ((two == two.max(axis=1, keepdims=True)).sum(axis=1) == 2).all()
                close = lp[c["kinds"] == mr.CLOSE]
                assert (close < 0).all() and ((close > L0).all() or tau_e * np.log(n_act) + 0.05 > -L0)
        for delta_clip in (1.0, 0.0):
            worst = max(worst, _check_mdqn(c, GAMMA, delta_clip, tau_e))
    print("M-DQN A%d B%d %s tau_e %g: largest |td_abs error| / bound %.3f" % (n_act, batch, "dueling" if dueling else "plain",
                                                                            tau_e, worst))


@pytest.mark.parametrize("n_act,batch", [(6, 33), (255, 257)])
def test_mdqn_large_values_stay_finite_and_within_the_bound(n_act, batch):
    c = mr.mdqn_case(77 + n_act, n_act, batch, False, True, scale=1e4, shift=1)
    assert np.abs(c["nxt"][:, :n_act]).max() > 1e4
    worst = max(_check_mdqn(c, GAMMA, delta_clip, 0.03) for delta_clip in (1.0, 0.0))
    print("M-DQN A%d B%d |q| ~ 1e4: largest |td_abs error| / bound %.3f" % (n_act, batch, worst))


@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
@pytest.mark.parametrize("n_act,batch", [(1, 1), (6, 33), (18, 257)])
def test_mdqn_reduces_to_dqn_bit_for_bit(n_act, batch, dueling):
    """alpha = 0, tau_e = 2^-10, integer-valued inputs, the maximum of tgt_next unique by a gap of 4: every other e_a is
    exactly 0, soft_b == the maximum, the bonus is +-0 -- the three outputs equal arl_dqn_loss's (pol_next NULL)."""
    rs = np.random.RandomState(5 + n_act)
    c = mr.mdqn_case(9 + n_act, n_act, batch, dueling, True)
    cols = n_act + int(dueling)
    for key in ("q", "nxt", "cur"):
        c[key][:, :cols] = rs.randint(-8, 9, size=(batch, cols))
    c["nxt"][np.arange(batch), rs.randint(0, n_act, size=batch)] = 12
    c["ret"] = rs.randint(-4, 5, size=batch).astype(np.float32)
    for delta_clip in (1.0, 0.0):
        got = _launch_mdqn(c, GAMMA, delta_clip, 2.0 ** -10, alpha=0.)
        want = _launch_mdqn(c, GAMMA, delta_clip, None, baseline=True)
        assert torch.isfinite(want[0]).all()
        for x, y in zip(got, want):
            assert torch.equal(x, y)


# ---- M-IQN kernel ---------------------------------------------------------------------------------------------------

def _launch_miqn(c, gamma_n, kappa, tau_e, alpha=ALPHA, l0=L0, state=None, advance=0, baseline=False):
    """baseline: arl_iqn_loss with pol_next NULL on the same blocks."""
    from accel_rl_amd import _lib
    pred = _dev(c["pred"])
    batch, n, _ = pred.shape
    m = c["nxt"].shape[1]
    dth = torch.full_like(pred, NAN)
    rows, pri = torch.full((batch,), NAN, device=DEV), torch.full((batch,), NAN, device=DEV)
    tail = (_dev(c["act"]), _dev(c["ret"]), _dev(c["term"]), _dev(c["isw"]), c["n_act"], n, m, gamma_n, kappa)
    if baseline:
        _lib.iqn_loss(pred, _dev(c["tau"]), _dev(c["nxt"]), None, *tail, dth, rows, pri, state=state, advance=advance)
    else:
        _lib.miqn_loss(pred, _dev(c["tau"]), _dev(c["nxt"]), _dev(c["cur"]), *tail, tau_e, alpha, l0, dth, rows, pri,
                       state=state, advance=advance)
    torch.cuda.synchronize()
    return dth.cpu(), rows.cpu(), pri.cpu()


def _check_miqn(c, gamma_n, kappa, tau_e):
    """Bounds: tests/munchausen_ref.py (M-IQN).  Returns the largest gradient error / bound."""
    n_act = c["n_act"]
    if kappa == 0:
        mr.place_pred_away_from_targets(c, mr.ref_miqn_targets(c, gamma_n, tau_e))
    ref = mr.ref_miqn(c, gamma_n, kappa, tau_e)
    batch, n, _ = c["pred"].shape
    m = c["nxt"].shape[1]
    a_max = ref["atol"].max(dim=1).values                       # max_j atol_bj
    if kappa == 0:                                              # the indicator is pinned: no sign of u is in doubt
        margin = (ref["u"].abs().amin(dim=(1, 2)) / (16 * a_max)).min().item()
        print("kappa 0: min |u| / (16 x the bound on T) = %.3g" % margin)
        assert margin > 1, margin                               # every sample: no case is skipped
        assert n == 1 or ((ref["u"] < 0).any() and (ref["u"] > 0).any())
    dth, rows, pri = _launch_miqn(c, gamma_n, kappa, tau_e)
    assert torch.isfinite(dth).all() and torch.isfinite(rows).all() and torch.isfinite(pri).all()
    w_max = ref["w"].max()
    g_atol = (m + 8) * EPS * w_max + (a_max * w_max / kappa if kappa > 0 else torch.zeros_like(a_max))
    g_err = (dth[:, :, :n_act].double() - ref["grad"]).abs()
    g_tol = g_atol[:, None, None] + 2e-4 * ref["grad"].abs()
    ratio = (g_err / g_tol).max().item()
    print("    largest gradient error / the bound's atol part alone: %.3f" % (g_err / g_atol[:, None, None]).max().item())
    assert (g_err <= g_tol).all(), ratio
    loss_atol = n * a_max
    assert ((rows.double() - ref["rows"]).abs() <= 2e-4 * ref["rows"].abs() + ref["w"] * loss_atol).all()
    want_pri = ref["loss_b"].clamp(1e-6, 1e6)
    assert ((pri.double() - want_pri).abs() <= 2e-4 * want_pri + loss_atol).all()
    other = torch.ones(dth.shape, dtype=torch.bool)             # exact zeros outside the taken action's column
    other[torch.arange(batch), :, torch.from_numpy(c["act"]).long()] = False
    assert not dth[other].any()
    return ratio


@pytest.mark.parametrize("tau_e", mr.TAUS_E)
@pytest.mark.parametrize("kappa", [1.0, 0.0])
@pytest.mark.parametrize("batch", mr.MIQN_BATCHES)
@pytest.mark.parametrize("shape", mr.MIQN_SHAPES, ids=lambda s: "N%d-M%d-A%d-S%d" % s)
def test_miqn_loss_priorities_and_gradient_vs_float64(shape, batch, kappa, tau_e):
    n, m, n_act, stride = shape
    worst = 0.
    for weighted in (False, True):
        c = mr.miqn_case(mr.miqn_seed(shape, batch, weighted), n, m, n_act, stride, batch, weighted,
                         shift=mr.MIQN_SHAPES.index(shape) + 3 * int(weighted))
        worst = max(worst, _check_miqn(c, GAMMA, kappa, tau_e))
    print("M-IQN N%d M%d A%d B%d kappa %g tau_e %g: largest gradient error / bound %.3f" % (n, m, n_act, batch, kappa, tau_e,
                                                                                         worst))


def test_miqn_cases_hold_every_special_row():
    seen, lps = set(), {}
    for k, shape in enumerate(mr.MIQN_SHAPES[1:], 1):           # (one action: every row is all of them at once)
        for weighted in (False, True):
            c = mr.miqn_case(mr.miqn_seed(shape, 3, weighted), *shape, 3, weighted, shift=k + 3 * int(weighted))
            lp = mr.ref_miqn_targets(c, GAMMA, 0.03)["lp_act"].numpy()
            seen.update(c["kinds"].tolist())
            for kind, v in zip(c["kinds"], lp):
                lps.setdefault(int(kind), []).append((v, shape[2]))
    assert seen == set(range(mr.N_KINDS))
    assert all(v == 0 for v, _ in lps[mr.LP_ZERO]) and all(v < L0 for v, _ in lps[mr.CLIPPED])
    assert all(abs(v + 0.03 * np.log(a)) < 1e-9 for v, a in lps[mr.ALL_EQUAL])
    assert all(L0 < v < 0 for v, _ in lps[mr.CLOSE])


@pytest.mark.parametrize("kappa", [1.0, 0.0])
def test_miqn_large_values_stay_finite_and_within_the_bound(kappa):
    shape = (32, 64, 18, 32)
    c = mr.miqn_case(123, *shape, 3, True, scale=1e4, shift=1)
    assert np.abs(c["nxt"][:, :, :18]).max() > 1e4
    print("M-IQN |theta| ~ 1e4, kappa %g: largest gradient error / bound %.3f" % (kappa, _check_miqn(c, GAMMA, kappa, 0.03)))


@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (5, 7, 3, 32), (32, 64, 64, 64)], ids=lambda s: "N%d-M%d-A%d-S%d" % s)
def test_miqn_reduces_to_iqn_bit_for_bit(shape):
    """alpha = 0, tau_e = 2^-10, integer-valued inputs; every row j of tgt_next carries the gap (the chosen column holds
    12 .. 15, the others at most 8), so Q^next has it too: soft_j == tgt_next(j, a*) and the outputs are arl_iqn_loss's."""
    n, m, n_act, stride = shape
    batch = 3
    rs = np.random.RandomState(11 + n_act)
    c = mr.miqn_case(13 + n_act, n, m, n_act, stride, batch, True)
    for key, r in (("pred", n), ("nxt", m), ("cur", m)):
        c[key][:, :, :n_act] = rs.randint(-8, 9, size=(batch, r, n_act))
    c["nxt"][np.arange(batch), :, rs.randint(0, n_act, size=batch)] = rs.randint(12, 16, size=(batch, m))
    c["ret"] = rs.randint(-4, 5, size=batch).astype(np.float32)
    for kappa in (1.0, 0.0):
        got = _launch_miqn(c, GAMMA, kappa, 2.0 ** -10, alpha=0.)
        want = _launch_miqn(c, GAMMA, kappa, None, baseline=True)
        assert torch.isfinite(want[0]).all()
        for x, y in zip(got, want):
            assert torch.equal(x, y)


# ---- refusals and determinism ---------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    from accel_rl_amd import _lib
    lib = _lib.load()
    batch = 2
    theta = torch.zeros(batch, 66, 260, device=DEV)                         # large enough for every size named below
    act = torch.zeros(batch, dtype=torch.uint8, device=DEV)
    ret = torch.zeros(batch, device=DEV)
    state = torch.tensor([1, 5], dtype=torch.int64, device=DEV)
    nans = lambda *shape: torch.full(shape, NAN, device=DEV)                # noqa: E731
    dq, dth, rows, pri = nans(batch, 260), nans(batch, 66, 68), nans(batch), nans(batch)
    p = lambda t: t.data_ptr()                                              # noqa: E731
    th = p(theta)

    def mdqn(q=th, nxt=th, cur=th, acts=p(act), out=p(dq), r=p(rows), b=batch, a=6, s=8, duel=0, te=0.03, al=0.9, l0=-1.0):
        return lib.arl_mdqn_loss(q, nxt, cur, acts, p(ret), p(act), None, b, a, s, duel, 0.99, 1.0, te, al, l0, out, r,
                                 p(pri), None)

    def miqn(pred=th, nxt=th, cur=th, tp=th, out=p(dth), r=p(rows), b=batch, a=6, n=8, m=8, s=8, kappa=1.0, te=0.03,
             al=0.9, l0=-1.0):
        return lib.arl_miqn_loss(pred, tp, nxt, cur, p(act), p(ret), p(act), None, b, a, n, m, s, 0.99, kappa, te, al, l0,
                                 out, r, p(pri), p(state), 3, None)

    for call in (mdqn, miqn):
        for kw in (dict(nxt=None), dict(cur=None), dict(out=None), dict(r=None)):
            assert call(**kw) == -1 and b"null" in lib.arl_last_error(), kw
        for te in (0., -0.03, float("inf"), float("nan")):
            assert call(te=te) == -1 and b"tau_e" in lib.arl_last_error()
        for al in (-0.1, float("inf"), float("nan")):
            assert call(al=al) == -1 and b"alpha" in lib.arl_last_error()
        for l0 in (1e-3, float("-inf"), float("nan")):
            assert call(l0=l0) == -1 and b"l0" in lib.arl_last_error()
    assert mdqn(q=None) == -1 and mdqn(acts=None) == -1 and miqn(pred=None) == -1 and miqn(tp=None) == -1
    for kw in (dict(b=0), dict(a=0), dict(a=256, s=256), dict(s=10), dict(a=6, s=4), dict(a=8, s=8, duel=1)):
        assert mdqn(**kw) == -2, kw                                         # check_q: ARL_E_RANGE, as arl_dqn_loss
    for kw in (dict(b=0), dict(a=0), dict(a=65, s=68), dict(s=10), dict(a=6, s=4), dict(n=0), dict(n=65), dict(m=0),
               dict(m=65), dict(kappa=-1.0), dict(kappa=float("inf")), dict(kappa=float("nan"))):
        assert miqn(**kw) == -1, kw
    torch.cuda.synchronize()
    for t in (dq, dth, rows, pri):
        assert torch.isnan(t).all()
    assert state.cpu().tolist() == [1, 5]
    assert mdqn() == 0 and miqn() == 0 and mdqn(a=255, s=256) == 0 and mdqn(a=7, s=8, duel=1) == 0    # inside the limits they run
    torch.cuda.synchronize()
    assert torch.isfinite(dq.view(-1)[:batch * 256]).all() and torch.isfinite(dth.view(-1)[:batch * 8 * 8]).all()
    assert torch.isfinite(rows).all() and torch.isfinite(pri).all() and state.cpu().tolist() == [1, 8]


def test_two_launches_are_bit_identical_and_the_counter_advances_by_advance():
    c = mr.mdqn_case(21, 18, 257, True, True)
    one, two = _launch_mdqn(c, GAMMA, 1.0, 0.03), _launch_mdqn(c, GAMMA, 1.0, 0.03)
    assert torch.isfinite(one[0]).all() and all(torch.equal(x, y) for x, y in zip(one, two))
    for kappa in (1.0, 0.0):
        c = mr.miqn_case(22, 51, 64, 18, 20, 37, True)
        state = torch.tensor([3, 2 ** 40], dtype=torch.int64, device=DEV)
        one = _launch_miqn(c, GAMMA, kappa, 0.03, state=state, advance=3)
        assert state.cpu().tolist() == [3, 2 ** 40 + 3]
        two = _launch_miqn(c, GAMMA, kappa, 0.03)
        assert state.cpu().tolist() == [3, 2 ** 40 + 3]
        assert torch.isfinite(one[0]).all() and all(torch.equal(x, y) for x, y in zip(one, two))


# ---- policies -------------------------------------------------------------------------------------------------------

N_ACT, BATCH, N_Q = 6, 8, 4


def _make_policy(kind, seed=5, **kw):
    """The small network (2 conv layers, hidden 64, 6 actions) with perturbed parameters and a target net that differs."""
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
    from accel_rl_amd.policies.dqn.atari_iqn_policy import AtariIqnPolicy
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    set_seed(seed)
    spec = dict(cnn_specs[0], hidden_sizes=[64])
    if kind == "iqn":
        policy = AtariIqnPolicy(epsilon=0.3, n_quantiles=N_Q, n_target_quantiles=N_Q, n_policy_quantiles=8, **spec)
    else:
        policy = AtariDqnPolicy(epsilon=0.3, **spec, **kw)
    policy.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(N_ACT)), device=DEV)
    rs = np.random.RandomState(3)
    flat = policy.get_param_values()
    policy.set_param_values(flat + (rs.randn(flat.size) * 0.01).astype(np.float32))
    policy.flat_target.copy_(policy.flat_params * 0.9)
    return policy, spec


def _minibatch(seed, b=BATCH, ret_scale=0.05):
    rs = np.random.RandomState(seed)
    return dict(obs=_dev(rs.randint(0, 256, size=(b, 4, 104, 80), dtype=np.uint8)),
                nxt=_dev(rs.randint(0, 256, size=(b, 4, 104, 80), dtype=np.uint8)),
                act=_dev(rs.randint(0, N_ACT, size=b).astype(np.uint8)),
                ret=_dev((rs.randn(b) * ret_scale).astype(np.float32)),
                term=_dev((rs.rand(b) < 0.3).astype(np.uint8)), isw=_dev((rs.rand(b) + 0.2).astype(np.float32)),
                taus=tuple(_dev(rs.uniform(0.02, 0.98, size=b * N_Q).astype(np.float32)) for _ in range(3)))


def _ref_params(policy, flat_bucket):
    fl = policy.bucket_to_reference(flat_bucket)
    out, pos = [], 0
    for shape in policy._ref_shapes:
        m = int(np.prod(shape))
        out.append(torch.from_numpy(fl[pos:pos + m].reshape(shape).astype(np.float64)).requires_grad_())
        pos += m
    return out


def _ref_convs(rp, spec, x):
    k = 0
    for i in range(len(spec["conv_filters"])):
        x = F.relu(F.conv2d(x, rp[k].flip(2, 3), rp[k + 1], stride=spec["conv_strides"][i],
                            padding=tuple(spec["conv_pads"][i])))
        k += 2
    return x.flatten(1), k


def _ref_q(rp, spec, x, dueling):
    """float64 plain torch on the reference layout; dueling: flat order hidden_Val, Val, hidden, output; merged."""
    x, k = _ref_convs(rp, spec, x)
    if dueling:
        val = F.relu(x @ rp[k] + rp[k + 1]) @ rp[k + 2] + rp[k + 3]
        adv = F.relu(x @ rp[k + 4] + rp[k + 5]) @ rp[k + 6] + rp[k + 7]
        return val + (adv - adv.mean(dim=1, keepdim=True))
    return F.relu(x @ rp[k] + rp[k + 1]) @ rp[k + 2] + rp[k + 3]


def _ref_theta(rp, spec, x, tau):
    """tau [B][R] -> theta [B][R][A] (as tests/test_iqn_gpu.py:_ref_theta)."""
    psi, k = _ref_convs(rp, spec, x)
    c = torch.cos(np.pi * torch.arange(64, dtype=torch.float64) * tau[:, :, None])
    phi = F.relu(c @ rp[k] + rp[k + 1])
    h = F.relu((psi[:, None, :] * phi) @ rp[k + 2] + rp[k + 3])
    return h @ rp[k + 4] + rp[k + 5]


def _compare_step(policy, got_rows, got_pri, want_rows, want_pri, loss, rp, target_before):
    b = got_rows.numel()
    assert got_rows.data_ptr() + 4 * b == got_pri.data_ptr()    # the (2, b) buffer the optimizer's ring takes at once
    got = policy.bucket_to_reference(policy.flat_grads)
    want = np.concatenate([g.detach().numpy().reshape(-1) for g in torch.autograd.grad(loss, rp)])
    print("loss %.6g vs %.6g; max grad err %.3g of max |grad| %.3g" % (got_rows.sum().item(), loss.item(),
                                                                       np.abs(got - want).max(), np.abs(want).max()))
    assert np.abs(want).max() > 0
    assert np.allclose(got_rows.cpu().numpy(), want_rows.detach().numpy(), rtol=2e-3, atol=0)
    assert np.allclose(got_pri.cpu().numpy(), want_pri.detach().numpy(), rtol=2e-3, atol=0)
    assert np.allclose(got, want, rtol=2e-3, atol=2e-5 * max(np.abs(want).max(), 1e-3)), np.abs(got - want).max()
    assert torch.equal(policy.flat_target, target_before)       # the target network is read, never written


@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
def test_mdqn_training_step_matches_autograd_through_plain_torch(dueling):
    policy, spec = _make_policy("dqn", dueling=dueling)
    mb = _minibatch(4)
    clip, tau_e = 0.05, 0.03
    target_before = policy.flat_target.clone()
    policy.flat_grads.fill_(NAN)
    rows, td = policy.munchausen_loss_and_grads(mb["obs"], mb["nxt"], mb["act"], mb["ret"], mb["term"], mb["isw"], GAMMA,
                                                clip, tau_e, ALPHA, L0)
    rp, rt = _ref_params(policy, policy.flat_params), _ref_params(policy, policy.flat_target)
    scale = float(np.float32(1. / 255))
    obs, nxt = mb["obs"].cpu().double() * scale, mb["nxt"].cpu().double() * scale
    q = _ref_q(rp, spec, obs, dueling)
    with torch.no_grad():
        qn, qc = _ref_q(rt, spec, nxt, dueling), _ref_q(rt, spec, obs, dueling)
    ar, act = torch.arange(BATCH), mb["act"].cpu().long()
    lpn, pin = mr.soft64(qn, tau_e)
    bonus = ALPHA * mr.soft64(qc, tau_e)[0][ar, act].clamp(L0, 0.)
    y = (mb["ret"].cpu().double() + bonus) + (1. - mb["term"].cpu().double()) * GAMMA * (pin * (qn - lpn)).sum(dim=1)
    d = y - q[ar, act]
    want_rows = mb["isw"].cpu().double() / BATCH * mr.huber64(d, clip)
    assert (d.abs() < clip).any() and (d.abs() > clip).any()    # both branches of the Huber loss in play
    assert (bonus < 0).all()
    _compare_step(policy, rows, td, want_rows, d.abs().clamp(max=clip), want_rows.sum(), rp, target_before)


def test_miqn_training_step_matches_autograd_through_plain_torch():
    policy, spec = _make_policy("iqn")
    mb = _minibatch(6, ret_scale=1.0)
    tau_e, kappa = 0.03, 1.0
    target_before = policy.flat_target.clone()
    counter = policy._iqn_state.cpu().tolist()
    policy.flat_grads.fill_(NAN)
    rows, pri = policy.munchausen_loss_and_grads(mb["obs"], mb["nxt"], mb["act"], mb["ret"], mb["term"], mb["isw"], GAMMA,
                                                 kappa, tau_e, ALPHA, L0, taus=mb["taus"])
    assert policy._iqn_state.cpu().tolist() == counter          # given fractions leave the counter alone
    rp, rt = _ref_params(policy, policy.flat_params), _ref_params(policy, policy.flat_target)
    scale = float(np.float32(1. / 255))
    obs, nxt = mb["obs"].cpu().double() * scale, mb["nxt"].cpu().double() * scale
    t_pred, t_next, t_cur = (t.cpu().double().view(BATCH, N_Q) for t in mb["taus"])
    pred = _ref_theta(rp, spec, obs, t_pred)
    with torch.no_grad():
        th_n, th_c = _ref_theta(rt, spec, nxt, t_next), _ref_theta(rt, spec, obs, t_cur)
    ar, act = torch.arange(BATCH), mb["act"].cpu().long()
    lpn, pin = mr.soft64(th_n.mean(dim=1), tau_e)
    bonus = ALPHA * mr.soft64(th_c.mean(dim=1), tau_e)[0][ar, act].clamp(L0, 0.)
    soft = (pin[:, None, :] * (th_n - lpn[:, None, :])).sum(dim=2)
    T = (mb["ret"].cpu().double() + bonus)[:, None] + (1. - mb["term"].cpu().double())[:, None] * (GAMMA * soft)
    u = T[:, None, :] - pred[ar, :, act][:, :, None]
    wt = (t_pred[:, :, None] - (u < 0).double()).abs().detach()
    au = u.abs()
    loss_b = (wt * torch.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa)) / kappa).sum(dim=(1, 2)) / N_Q
    want_rows = mb["isw"].cpu().double() / BATCH * loss_b
    _compare_step(policy, rows, pri, want_rows, loss_b.clamp(1e-6, 1e6), want_rows.sum(), rp, target_before)


def _algo(kind, use_graph):
    from accel_rl_amd.algos.dqn.munchausen import MunchausenDQN, MunchausenIQN
    cls = MunchausenIQN if kind == "iqn" else MunchausenDQN
    return cls(batch_size=BATCH, prioritized_replay=True, optimizer_args=dict(use_graph=use_graph))


@pytest.mark.parametrize("kind", ["dqn", "iqn"])
def test_captured_updates_equal_eager_updates_bit_for_bit(kind):
    """DqnOptimizer(use_graph=True): two eager warm-up calls, the capture, then replays -- four updates in all -- against
    four eager updates from the same start (parameters, target net, optimiser state and, for IQN, the call counter)."""
    batches = [_minibatch(30 + i) for i in range(4)]
    runs = []
    for use_graph in (True, False):
        policy, _ = _make_policy(kind)
        if kind == "iqn":
            policy._iqn_state[1] = 17
        algo = _algo(kind, use_graph)
        inputs, loss = algo.build_loss(None, policy)
        assert len(inputs) == 6
        algo.optimizer.initialize(inputs=inputs, loss=loss, target=policy)
        steps = []
        for mb in batches:
            priority, _ = algo.optimizer.optimize((mb["obs"], mb["nxt"], mb["act"], mb["ret"], mb["term"], mb["isw"]))
            torch.cuda.synchronize()
            steps.append((priority.clone(), policy.flat_params.clone()))
        assert (algo.optimizer._graph is not None) == use_graph
        if kind == "iqn":
            assert policy._iqn_state.cpu().tolist()[1] == 17 + 3 * 4
        runs.append(steps)
        del algo
    for (pri_g, par_g), (pri_e, par_e) in zip(*runs):
        assert torch.isfinite(par_g).all() and torch.equal(pri_g, pri_e) and torch.equal(par_g, par_e)
    assert not torch.equal(runs[0][0][1], runs[0][3][1])        # the parameters moved


@pytest.mark.parametrize("kind", ["dqn", "iqn"])
def test_munchausen_trains_with_prioritized_replay_and_eval(kind):
    """test_iqn_gpu.py's end-to-end configuration at toy size (one-step returns, no double DQN): GpuVecEvalSampler ->
    device replay (prioritized) -> Munchausen updates inside the captured graph -> target sync, schedules, evaluation."""
    from accel_rl_amd.algos.dqn.munchausen import MunchausenDQN, MunchausenIQN
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
    from accel_rl_amd.policies.dqn.atari_iqn_policy import AtariIqnPolicy
    from accel_rl_amd.runners.accel_rl import AccelRLEval
    from accel_rl_amd.sampler.gpu_sampler_with_eval import GpuVecEvalSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecEvalSampler(eval_steps=8 * 40, eval_envs_per=1, EnvCls=SynthAtariEnv,
                                env_args=dict(game="seaquest"), horizon=4, n_parallel=4, envs_per=2,
                                max_path_length=25, max_decorrelation_steps=0, device=DEV)
    args = dict(batch_size=32, min_steps_learn=64 * 4, replay_size=64 * 60, training_intensity=8,
                target_update_steps=64 * 3, prioritized_replay=True, eps_greedy_args=dict(anneal_steps=64 * 10))
    if kind == "iqn":
        algo = MunchausenIQN(**args)
        policy = AtariIqnPolicy(**cnn_specs[0], n_quantiles=8, n_target_quantiles=8, n_policy_quantiles=16)
    else:
        algo = MunchausenDQN(**args)
        policy = AtariDqnPolicy(**cnn_specs[0])
    first = {}
    initialize = policy.initialize

    def recording_initialize(*a, **kw):
        initialize(*a, **kw)
        first["params"] = policy.get_param_values()
    policy.initialize = recording_initialize
    runner = AccelRLEval(algo=algo, policy=policy, sampler=sampler, n_steps=64 * 24, seed=9, eval_interval_steps=64 * 8)
    runner.train()
    tab = runner.last_tabular
    for key in ("StepsInEval", "TrajsInEval", "LossAverage", "PriorityAverage", "ReturnAverage", "ParamsNorm"):
        assert key in tab, key
    assert np.isfinite(tab["LossAverage"]) and tab["LossAverage"] > 0 and tab["TrajsInEval"] > 0
    assert np.isfinite(tab["PriorityAverage"]) and tab["PriorityAverage"] > 0
    assert algo._updates_per_optimize == 8 * 64 // 32 and abs(policy.get_epsilon() - 0.01) < 1e-9
    assert algo.replay_buffer.beta > 0.4
    final = policy.get_param_values()
    assert np.isfinite(final).all() and not np.array_equal(final, first["params"])      # the parameters moved
    target = policy.bucket_to_reference(policy.flat_target)
    assert np.isfinite(target).all() and not np.array_equal(target, first["params"])    # the target net was synced
    policy.update_target()
    assert torch.equal(policy.flat_target, policy.flat_params)
    if kind == "iqn":
        assert policy._iqn_state.cpu().tolist()[1] > 3 * algo._updates_per_optimize
