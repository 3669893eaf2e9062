"""PopArt on the device: the two entry points of csrc/popart.hip against the restatements of tests/popart_ref.py (bit for
bit, inside NaN guard bands; refusals leave the fill), the preservation step through the real head kernel within a derived
bound, one whole update of PopArtA2C / PopArtPPO / PopArtVMPO against float64 autograd of the restated pipeline, and the
four learners on the synthetic env -- beta 0 against plain PPO, a power-of-two reward scale against its statistics,
replayed against eager."""
import numpy as np
import pytest
import torch

import autograd_ref
import popart_ref
import test_resnet_gpu as trg
import vmpo_ref
from test_head_limits_gpu import _nan, _untouched
from test_ppg_gpu import _Float64Net, _assert_same_run, _cnn_setup, _whole_step_close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan64(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), got[bad][:4], want[bad][:4])


ROWS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4099]
HIDS = [1, 3, 64, 512, 1025]


# ---- arl_popart_denorm ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", ROWS)
def test_denorm_bit_for_bit(L, rows):
    rs = np.random.RandomState(rows)
    for n_last, stats in ((1, (0.75, 9.5625, 3., 4.)), (rows, (-1e3, 1e6 + 1e-2, 0.1, 1.)), (max(rows // 5, 1), (0., 1., 1., 0.))):
        value_n, last_n = rs.randn(rows).astype(F32), rs.randn(n_last).astype(F32)
        value_n[0] = F32(0.)
        # inputs and outputs one float past a 16-byte boundary: 4-byte alignment is all that is asked
        vin, lin = _nan(rows + 1), _nan(n_last + 1)
        vin[1:], lin[1:] = _dev(value_n), _dev(last_n)
        st = _nan64(6)
        st[1:5] = _dev(np.array(stats))
        out, last = _nan(rows + 3), _nan(n_last + 3)
        L.popart_denorm(vin[1:], lin[1:], st[1:5], out[1:rows + 1], last[1:n_last + 1])
        torch.cuda.synchronize()
        want, want_last = popart_ref.denorm(value_n, last_n, stats)
        _same_bits(out[1:rows + 1].cpu().numpy(), want, "value rows %d" % rows)
        _same_bits(last[1:n_last + 1].cpu().numpy(), want_last, "last_value rows %d" % rows)
        assert all(_untouched(x[:1]) and _untouched(x[-2:]) for x in (out, last))
        _same_bits(vin[1:].cpu().numpy(), value_n, "the recorded values")
        _same_bits(st[1:5].cpu().numpy(), np.array(stats), "the statistics")
        if stats == (0., 1., 1., 0.):
            _same_bits(out[1:rows + 1].cpu().numpy(), value_n, "the initial statistics are the identity")


# ---- arl_popart_step -----------------------------------------------------------------------------------------------------

class _Rig(object):
    """Every array arl_popart_step touches, inside NaN guards; the head as W_head[(A + 1), hid] with an ODD number of
    actions (the value row is then 4-byte aligned and no more for odd hid)."""

    def __init__(self, rs, rows, hid, n_act, stats=popart_ref.INIT_STATS, lead=1):
        assert n_act % 2 == 1
        self.rows, self.hid, self.n_act = rows, hid, n_act
        k = (n_act + 1) * hid
        # lead = 1: W_head and b_head start one float past a 16-byte boundary; lead = 4: on one, as in a policy's bucket
        self.w_all, self.b_all = _nan(lead + k + 1), _nan(lead + n_act + 2)
        self.w_host = (rs.randn(n_act + 1, hid) / np.sqrt(hid)).astype(F32)
        self.b_host = (rs.randn(n_act + 1) * 0.1).astype(F32)
        self.w_head, self.b_head = self.w_all[lead:lead + k], self.b_all[lead:lead + n_act + 1]
        self.w_head.copy_(_dev(self.w_host.reshape(-1)))
        self.b_head.copy_(_dev(self.b_host))
        self.w_value, self.b_value = self.w_head[n_act * hid:], self.b_head[n_act:]
        self.stats = _nan64(6)
        self.stats[1:5] = _dev(np.array(stats, dtype=F64))
        self.stats_host = np.array(stats, dtype=F64)
        self.ret, self.adv, self.diag = _nan(rows + 2), _nan(rows + 2), _nan(4)

    def step(self, L, ret, adv, valids, beta, sigma_min=1e-4, sigma_max=1e6):
        """One launch and the restatement's step; asserts every bit and every guard.  Returns the restatement's tuple."""
        rows = self.rows
        self.ret[1:rows + 1] = _dev(ret)
        self.adv[1:rows + 1] = _dev(adv if adv is not None else np.full(rows, np.nan, F32))
        L.popart_step(self.ret[1:rows + 1], None if adv is None else self.adv[1:rows + 1],
                      None if valids is None else _dev(valids), beta, sigma_min, sigma_max, self.stats[1:5],
                      self.w_value, self.b_value, self.diag[1:3])
        torch.cuda.synchronize()
        a = self.n_act
        want = popart_ref.step(ret, adv, valids, beta, sigma_min, sigma_max, self.stats_host, self.w_host[a], self.b_host[a:])
        ret_n, adv_n, stats_n, w_n, b_n, diag = want
        _same_bits(self.ret[1:rows + 1].cpu().numpy(), ret_n, "returns")
        if adv is None:
            assert _untouched(self.adv)
        else:
            _same_bits(self.adv[1:rows + 1].cpu().numpy(), adv_n, "advantages")
        _same_bits(self.stats[1:5].cpu().numpy(), stats_n, "stats")
        _same_bits(self.w_value.cpu().numpy(), w_n, "value row")
        _same_bits(self.b_value.cpu().numpy(), b_n, "value bias")
        _same_bits(self.diag[1:3].cpu().numpy(), diag, "diag2")
        # the policy rows keep their bits; nothing outside the arrays is written
        _same_bits(self.w_head[:a * self.hid].cpu().numpy(), self.w_host[:a].reshape(-1), "policy rows")
        _same_bits(self.b_head[:a].cpu().numpy(), self.b_host[:a], "policy biases")
        assert all(_untouched(x[:1]) and _untouched(x[-1:]) for x in (self.ret, self.adv, self.stats, self.diag, self.w_all,
                                                                     self.b_all))
        self.stats_host, self.w_host[a], self.b_host[a] = stats_n, w_n, b_n[0]
        return want


@pytest.mark.parametrize("with_adv", [True, False], ids=["adv", "noadv"])
@pytest.mark.parametrize("with_valids", [True, False], ids=["valids", "all"])
@pytest.mark.parametrize("rows", ROWS)
def test_step_two_calls_bit_for_bit(L, rows, with_valids, with_adv):
    case = ROWS.index(rows) + 2 * with_valids + with_adv
    hid, n_act = HIDS[case % len(HIDS)], (1, 5, 17)[case % 3]
    rs = np.random.RandomState(1000 * rows + case)
    rig = _Rig(rs, rows, hid, n_act)
    for call, (beta, scale, shift) in enumerate(((0.3, 40., 7.), (3e-4, 1e3, -50.))):
        ret = (rs.randn(rows) * scale + shift).astype(F32)
        adv = (rs.randn(rows) * scale).astype(F32) if with_adv else None
        valids = None
        if with_valids:
            valids = (rs.rand(rows) < 0.7).astype(np.int8)
            valids[rs.randint(rows)] = 1                                 # at least one row counts
            ret[valids == 0] = F32(np.inf) if call else F32(1e30)        # what a masked row holds does not matter
        ret_n, _, stats, _, _, _ = rig.step(L, ret, adv, valids, beta)
        assert stats[3] == call + 1 and np.isfinite(ret_n).all()
        if with_valids:
            assert (ret_n[valids == 0] == 0).all()


@pytest.mark.parametrize("hid", HIDS)
def test_step_every_width_bit_for_bit(L, hid):
    rs = np.random.RandomState(hid)
    rig = _Rig(rs, 70, hid, 3, stats=(0.5, 4.25, 2., 9.))
    for beta in (0.5, 0.01):
        rig.step(L, (rs.randn(70) * 5 + 1).astype(F32), rs.randn(70).astype(F32), None, beta)


def test_step_edge_inputs_bit_for_bit(L):
    rs = np.random.RandomState(77)
    rows, hid = 1030, 67
    rnd = lambda s=1.: (rs.randn(rows) * s).astype(F32)                                         # noqa: E731
    # all returns equal: the variance is exactly 0 and sigma_min decides
    rig = _Rig(rs, rows, hid, 5)
    _, _, stats, _, _, diag = rig.step(L, np.full(rows, 3.5, F32), rnd(), None, 1.0)
    assert stats.tolist() == [3.5, 12.25, 1e-4, 1.] and diag[1] == F32(1e-4)
    # returns of 1e6 one float32 step apart: nu' - mu'^2 cancels at 1e12
    rig = _Rig(rs, rows, hid, 5)
    ret = np.where(rs.rand(rows) < 0.5, F32(1e6), np.nextafter(F32(1e6), F32(2e6))).astype(F32)
    _, _, stats, _, _, _ = rig.step(L, ret, rnd(), None, 1.0)
    assert 1e-4 <= stats[2] <= 0.1
    _, _, stats, _, _, _ = rig.step(L, ret, None, None, 0.5)
    assert 1e-4 <= stats[2] <= 0.1
    # sigma_max decides
    rig = _Rig(rs, rows, hid, 5)
    _, _, stats, _, _, _ = rig.step(L, rnd(1e4), rnd(), None, 1.0, sigma_max=100.)
    assert stats[2] == 100.
    # beta 0 from the initial statistics: every array keeps its bits; beta 1: the batch's own moments
    rig = _Rig(rs, rows, hid, 5)
    ret, adv = rnd(30.), rnd()
    w_before, b_before = rig.w_host.copy(), rig.b_host.copy()
    ret_n, adv_n, stats, _, _, _ = rig.step(L, ret, adv, None, 0.)
    _same_bits(ret_n, ret, "beta 0: returns")
    _same_bits(adv_n, adv, "beta 0: advantages")
    _same_bits(rig.w_host, w_before, "beta 0: head")
    _same_bits(rig.b_host, b_before, "beta 0: biases")
    assert stats.tolist() == [0., 1., 1., 1.]
    ret_n, _, stats, _, _, _ = rig.step(L, ret, adv, None, 1.)
    assert abs(stats[0] - ret.astype(F64).mean()) < 1e-9 and abs(ret_n.astype(F64).mean()) < 1e-6
    assert abs(ret_n.astype(F64).std() - 1.) < 1e-5
    # all valids 0, and one infinite return among valid rows: statistics and head keep their bits
    rig = _Rig(rs, rows, hid, 5, stats=(2., 13., 3., 7.))
    w_before, b_before = rig.w_host.copy(), rig.b_host.copy()
    ret_n, adv_n, stats, _, _, diag = rig.step(L, rnd(30.), rnd(), np.zeros(rows, np.int8), 0.5)
    assert (ret_n == 0).all() and (adv_n == 0).all() and not np.signbit(ret_n).any()
    assert stats.tolist() == [2., 13., 3., 7.] and diag.tolist() == [2., 3.]
    ret = rnd(30.)
    ret[rows // 2] = F32(np.inf)
    ret_n, _, stats, _, _, _ = rig.step(L, ret, rnd(), None, 0.5)
    assert stats.tolist() == [2., 13., 3., 7.] and np.isinf(ret_n[rows // 2]) and np.isfinite(np.delete(ret_n, rows // 2)).all()
    _same_bits(rig.w_host, w_before, "skipped update: head")
    _same_bits(rig.b_host, b_before, "skipped update: biases")
    _same_bits(rig.w_head.cpu().numpy(), w_before.reshape(-1), "skipped update: head on the device")


def test_refusals_on_the_device_leave_the_fill(L):
    lib = L.load()
    s = L.stream_ptr()
    a = lambda x: x.data_ptr()                                                                  # noqa: E731
    vn, ln = torch.randn(8, device=DEV), torch.randn(2, device=DEV)
    stats, v, lv = _nan64(4), _nan(8), _nan(2)
    den = lib.arl_popart_denorm
    assert den(a(vn), 8, a(ln), 2, None, a(v), a(lv), s) == -1
    assert den(a(vn), 0, a(ln), 2, a(stats), a(v), a(lv), s) == -2
    assert den(a(vn), 8, a(ln), 9, a(stats), a(v), a(lv), s) == -2
    assert den(a(v), 8, a(ln), 2, a(stats), a(v), a(lv), s) == -1            # aliased
    assert den(a(vn), 8, a(lv), 2, a(stats), a(v), a(lv), s) == -1
    assert den(a(vn), 8, a(ln), 2, a(stats) + 4, a(v), a(lv), s) == -3
    ret, adv, w, b, diag = _nan(8), _nan(8), _nan(4), _nan(1), _nan(2)
    step = lib.arl_popart_step
    nan = float("nan")
    assert step(a(ret), a(adv), None, 8, 0.1, 1e-4, 1e6, a(stats), None, a(b), 4, a(diag), s) == -1
    assert step(a(ret), a(adv), None, 8, 1.1, 1e-4, 1e6, a(stats), a(w), a(b), 4, a(diag), s) == -1
    assert step(a(ret), a(adv), None, 8, nan, 1e-4, 1e6, a(stats), a(w), a(b), 4, a(diag), s) == -1
    assert step(a(ret), a(adv), None, 8, 0.1, 0., 1e6, a(stats), a(w), a(b), 4, a(diag), s) == -1
    assert step(a(ret), a(adv), None, 8, 0.1, 2., 1., a(stats), a(w), a(b), 4, a(diag), s) == -1
    assert step(a(ret), a(ret), None, 8, 0.1, 1e-4, 1e6, a(stats), a(w), a(b), 4, a(diag), s) == -1
    assert step(a(ret), a(adv), None, 0, 0.1, 1e-4, 1e6, a(stats), a(w), a(b), 4, a(diag), s) == -2
    assert step(a(ret), a(adv), None, (1 << 22) + 1, 0.1, 1e-4, 1e6, a(stats), a(w), a(b), 4, a(diag), s) == -2
    assert step(a(ret), a(adv), None, 8, 0.1, 1e-4, 1e6, a(stats), a(w), a(b), 0, a(diag), s) == -2
    assert step(a(ret), a(adv), None, 8, 0.1, 1e-4, 1e6, a(stats), a(w), a(b), 65537, a(diag), s) == -2
    assert step(a(ret), a(adv), None, 8, 0.1, 1e-4, 1e6, a(stats) + 4, a(w), a(b), 4, a(diag), s) == -3
    assert step(a(ret), a(adv), None, 8, 0.1, 1e-4, 1e6, a(stats), a(w) + 2, a(b), 4, a(diag), s) == -3
    assert b"arl_popart_step" in lib.arl_last_error()
    torch.cuda.synchronize()
    assert all(_untouched(x) for x in (stats, v, lv, ret, adv, w, b, diag))


# ---- preservation through the real head ------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(5, 63, 33), (3, 64, 17), (17, 512, 40), (1, 1000, 9)], ids=lambda c: "A%d-hid%d-B%d" % c)
def test_preservation_through_the_head_kernel(L, case):
    """sigma n + mu of every row, as arl_pg_head_infer computes n, before and after two steps.  In real arithmetic the
    step changes nothing; on the device w'_j and b' are each rounded to float32 once (at most 2^-24 relative, stated as
    2^-23 to cover the float64 roundings of the step itself): 2^-23 sigma' (sum_j |w'_j h_j| + |b'|).  To that comes the
    head kernel's own float32 accumulation error on either side, taken as its distance to a float64 evaluation of the
    same float32 weights, each in its own units (sigma before, sigma' after)."""
    n_act, hid, batch = case
    rs = np.random.RandomState(sum(case))
    rig = _Rig(rs, 300, hid, n_act, stats=(1.5, 2.25 + 16., 4., 3.), lead=4)
    h = np.maximum(rs.randn(batch, hid), 0).astype(F32)
    hd = _dev(h)

    def unnormalized():
        prob, n = _nan(batch, n_act), _nan(batch)
        L.pg_head_infer(hd, rig.w_head, rig.b_head, prob, n)
        torch.cuda.synchronize()
        mu, sigma = rig.stats_host[0], rig.stats_host[2]
        n32 = n.cpu().numpy().astype(F64)
        w, b = rig.w_host[n_act].astype(F64), F64(rig.b_host[n_act])
        n64 = h.astype(F64) @ w + b
        return sigma * n32 + mu, sigma * np.abs(n32 - n64), sigma * (np.abs(h.astype(F64) * w).sum(axis=1) + abs(b)), prob

    before, head_err, _, prob_before = unnormalized()
    for beta, scale, shift in ((0.5, 300., -40.), (0.2, 2., 1e3)):
        rig.step(L, (rs.randn(300) * scale + shift).astype(F32), None, None, beta)
        after, head_err_after, magnitude, prob = unnormalized()
        bound = 2. ** -23 * magnitude + head_err + head_err_after
        err = np.abs(after - before)
        print("A %d hid %d: sigma' %.4g max err %.3g, bound at that row %.3g" %
              (n_act, hid, rig.stats_host[2], err.max(), bound[err.argmax()]))
        assert (err <= bound).all(), (err.max(), bound[err.argmax()])
        _same_bits(prob.cpu().numpy(), prob_before.cpu().numpy(), "the policy's probabilities")
        before, head_err = after, head_err_after
    assert rig.stats_host[2] > 100.           # (the second step's shift: a scale far from where the head started)


def test_value_head_views_the_flat_parameters():
    from accel_rl_amd.policies.atari_resnet_policy import AtariResnetPolicy
    policy, _, _ = _cnn_setup()
    w, b = policy.value_head()
    a, k = policy.n_act, policy._k_head
    assert tuple(w.shape) == (64,) and tuple(b.shape) == (1,)
    assert w.data_ptr() == policy.params[k][a].data_ptr() and b.data_ptr() == policy.params[k + 1][a:].data_ptr()
    base, itemsize = policy.flat_params.data_ptr(), 4
    assert base <= w.data_ptr() < base + policy.flat_params.numel() * itemsize
    assert torch.equal(w, policy.params[k].detach()[a]) and torch.equal(b, policy.params[k + 1].detach()[a:])
    assert AtariResnetPolicy._head_internal_shapes is type(policy)._head_internal_shapes


# ---- one whole update against float64 autograd -----------------------------------------------------------------------------

def _gae64(values, last_values, rewards, dones, discount, lam):
    """float64 (advantages, returns) [n_env, T], nothing rounded: delta_t = r_t + g_t V_{t+1} - V_t, A_t = delta_t + g_t
    lam A_{t+1}, g_t = 0 at a done; returns = A + V (lam = 1: the discounted n-step return)."""
    n_env, horizon = rewards.shape
    adv = np.zeros((n_env, horizon), F64)
    a_next, v_next = np.zeros(n_env, F64), last_values
    for t in range(horizon - 1, -1, -1):
        g = np.where(dones[:, t] != 0, 0.0, discount)
        a_next = rewards[:, t] + g * v_next - values[:, t] + g * lam * a_next
        adv[:, t] = a_next
        v_next = values[:, t]
    return adv, adv + values


WHOLE = dict(a2c=dict(), ppo=dict(optimizer_args=dict(epochs=1, minibatch_size=24)),
             vmpo=dict(optimizer_args=dict(epochs=1, minibatch_size=24)))


@pytest.mark.parametrize("name", sorted(WHOLE))
def test_one_whole_update_matches_float64_autograd(name):
    """denorm -> scan -> moments -> preserved head -> normalised loss, restated in float64 on host copies of the
    parameters as they were before the step; against process_samples + _losses of the learner (40 rows of 8 envs)."""
    policy, data, idx = _cnn_setup()
    saved = policy.flat_params.clone()
    try:
        _whole_update(name, policy, data, None if name == "a2c" else idx)
    finally:
        policy.flat_params.copy_(saved)
        policy.note_params_changed()


def _whole_update(name, policy, data, idx):
    from accel_rl_amd.algos.pg import PopArtA2C, PopArtPPO, PopArtVMPO
    from accel_rl_amd.spaces import Discrete, EnvSpec, UintBox
    n_env, horizon, beta = 8, 5, 0.25
    algo = dict(a2c=PopArtA2C, ppo=PopArtPPO, vmpo=PopArtVMPO)[name](use_graph=False, beta=beta, popart_init=(1.5, 3.0),
                                                                    **WHOLE[name])
    algo.initialize(policy, EnvSpec(UintBox((4, 104, 80)), Discrete(6)), n_env * horizon, horizon, True)
    w_row, b_val = policy.value_head()
    b_val.fill_(0.4)                            # (a bias the preservation step has something to do with)
    rs = np.random.RandomState(5)
    extra = _dev(rs.randint(0, 256, size=(n_env, 4, 104, 80), dtype=np.uint8))
    rewards = (rs.randn(n_env * horizon) * 50.).astype(F32)             # far from the unit scale of clipped rewards
    dones = (rs.rand(n_env * horizon) < 0.15).astype(np.uint8)
    obs = data["observations"]
    value_n = policy.prob_value(obs)[1].clone()
    last_n = policy.value(extra).clone()
    samples = dict(observations=obs, extra_observations=extra, rewards=_dev(rewards), dones=_dev(dones),
                   actions=data["actions"], agent_infos=dict(value=value_n, prob=data["old_prob"]), env_infos=dict())
    net = _Float64Net(policy)                   # the parameters before the step
    state = algo.popart_state()
    assert state == dict(mu=1.5, nu=9. + 2.25, sigma=3., n_updates=0.)
    # ---- the device
    opt = algo.process_samples(0, samples)
    mb = dict(zip(algo.optimizer._input_names, algo.prep_opt_inputs(0, samples, opt)), idx=idx)
    policy.flat_grads.fill_(float("nan"))
    loss4 = algo._losses(mb).cpu().numpy()
    got = [g.detach().cpu().numpy().copy() for g in policy.grads]
    torch.cuda.synchronize()
    after = algo.popart_state()
    _same_bits(samples["agent_infos"]["value"].cpu().numpy(), value_n.cpu().numpy(), "the sampler's record")
    # ---- float64
    mu, sigma, nu = F64(state["mu"]), F64(state["sigma"]), F64(state["nu"])
    v = (sigma * value_n.cpu().numpy().astype(F64) + mu).reshape(n_env, horizon)
    lv = sigma * last_n.cpu().numpy().astype(F64) + mu
    adv, ret = _gae64(v, lv, rewards.astype(F64).reshape(n_env, horizon), dones.reshape(n_env, horizon), algo.discount,
                      float(algo.gae_lambda))
    adv, ret = adv.reshape(-1), ret.reshape(-1)
    mu_n = (1 - beta) * mu + beta * ret.mean()
    nu_n = (1 - beta) * nu + beta * (ret * ret).mean()
    sigma_n = np.sqrt(nu_n - mu_n * mu_n)
    assert 1e-4 < sigma_n < 1e6 and sigma_n > 2 * sigma        # the rewards' scale has moved the statistics
    _whole_step_close(np.array([after["mu"], after["nu"], after["sigma"]]), np.array([mu_n, nu_n, sigma_n]), 0., "stats")
    assert after["n_updates"] == 1
    ret_n, adv_n = (ret - mu_n) / sigma_n, adv / sigma_n
    _whole_step_close(opt["returns"].cpu().numpy().reshape(-1), ret_n, np.abs(ret_n).max(), "normalised returns")
    _whole_step_close(opt["advantages"].cpu().numpy().reshape(-1), adv_n, np.abs(adv_n).max(), "scaled advantages")
    a, k_head = policy.n_act, len(net.params) - 2
    with torch.no_grad():
        b_old = float(net.params[k_head + 1][a])
        net.params[k_head][a] *= float(sigma / sigma_n)
        net.params[k_head + 1][a] = (sigma * b_old + mu - mu_n) / sigma_n
    _whole_step_close(w_row.cpu().numpy(), net.params[k_head][a].detach().numpy(), 0., "preserved value row")
    _whole_step_close(b_val.cpu().numpy(), net.params[k_head + 1][a:].detach().numpy(), 0., "preserved value bias")
    sel = torch.arange(40) if idx is None else idx.cpu().long()
    n = sel.numel()
    x = policy._scaled_f32(obs, idx)[:, :policy._c_in].cpu().double()
    prob, value = autograd_ref.forward(net, x)
    act = data["actions"].cpu()[sel].long()
    old = data["old_prob"].cpu()[sel].double()
    ret_t, adv_t = torch.from_numpy(ret_n)[sel], torch.from_numpy(adv_n)[sel]
    dist = policy.distribution
    c_v = algo.v_loss_coeff
    v_loss = c_v * ((value - ret_t) ** 2).mean()
    if name == "vmpo":
        psi = vmpo_ref.weights(adv_n[sel.numpy()].astype(F32), algo.eta_init, algo.eps_eta)["psi"]
        wgt = torch.full((n,), 1. / n, dtype=torch.float64)
        pi, v_loss, akl, third = vmpo_ref.losses(prob, value, act, torch.from_numpy(psi), ret_t, old,
                                                 float(F32(algo.alpha_init)), c_v, wgt)
        total = pi + v_loss + akl
    else:
        if name == "a2c":
            pi = -(dist.log_likelihood_sym(act, dict(prob=prob)) * adv_t).mean()
        else:
            ratio = dist.likelihood_ratio_sym(act, dict(prob=old), dict(prob=prob))
            assert bool(((ratio.detach() - 1).abs() - algo.clip_param).abs().min() > 1e-3)      # no row on a kink
            pi = -autograd_ref.ppo_surrogate(ratio, adv_t, algo.clip_param).mean()
        third = -algo.ent_loss_coeff * dist.entropy_sym(dict(prob=prob)).mean()
        total = pi + v_loss + third
    want = [g.numpy() for g in torch.autograd.grad(total, net.params)]
    terms = np.array([float(t.detach()) for t in (pi, v_loss, third)])
    _whole_step_close(loss4[:3], terms, np.abs(terms).max(), "%s losses" % name)
    scale = max(max(np.abs(g).max() for g in want), 1e-3)
    assert all(np.isfinite(g).all() for g in got)
    for k, (g, wv) in enumerate(zip(got, want)):
        assert np.abs(wv).max() > 0, k
        _whole_step_close(g, wv, scale, "%s param %d" % (name, k))
    # what callers of policy.value see: the unnormalised value of the bootstrap rows is what it was before the step
    now = algo.unnormalize(policy.value(extra)).cpu().numpy()
    _whole_step_close(now, lv, np.abs(lv).max(), "unnormalize(policy.value)")


# ---- the algorithms ----------------------------------------------------------------------------------------------------------

def _train(cls, use_graph, n_itr, reward_scale=None, wrap=None, mid_batch_reset=True, max_path_length=25, **kwargs):
    """`cls` on the synthetic pong with unclipped rewards, 8 envs x horizon 5, spec 0 with a 64-wide hidden layer.
    reward_scale: the learner sees the rollout's rewards times this (a copy: the sampler's buffer keeps its own).
    wrap(algo): called once initialize has run."""
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game="pong", clip_reward=False), horizon=5, n_parallel=2,
                            envs_per=2, max_path_length=max_path_length, mid_batch_reset=mid_batch_reset,
                            max_decorrelation_steps=0, device=DEV)
    algo = cls(use_graph=use_graph, **kwargs)
    policy = AtariCnnPolicy(**dict(cnn_specs[0], hidden_sizes=[64]))
    log = dict(infos=[], rewards=[])
    initialize, optimize = algo.initialize, algo.optimize_policy

    def watching_initialize(*a, **kw):
        initialize(*a, **kw)
        log["first"] = policy.get_param_values()
        if wrap is not None:
            wrap(algo)

    def recording_optimize(itr, samples):
        log["rewards"].append(samples["rewards"].clone())
        if reward_scale is not None:
            if "scaled" not in log:             # (one dict, one tensor: the captured update keeps reading them)
                log["source"] = samples
                log["scaled"] = dict(samples, rewards=torch.empty_like(samples["rewards"]))
            assert samples is log["source"]
            torch.mul(samples["rewards"], reward_scale, out=log["scaled"]["rewards"])
            samples = log["scaled"]
        out = optimize(itr, samples)
        log["infos"].append(out[1])
        return out
    algo.initialize, algo.optimize_policy = watching_initialize, recording_optimize
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=40 * (n_itr - 1), seed=9, log_interval_steps=40)
    runner.train()
    torch.cuda.synchronize()
    log["infos"] = [{k: trg._host(v).copy() for k, v in info.items()} for info in log["infos"]]
    log["rewards"] = [trg._host(r) for r in log["rewards"]]
    return algo, policy, log


def _classes():
    from accel_rl_amd.algos.pg import PopArtA2C, PopArtIMPALA, PopArtPPO, PopArtVMPO
    return dict(a2c=PopArtA2C, ppo=PopArtPPO, vmpo=PopArtVMPO, impala=PopArtIMPALA)


MB = dict(optimizer_args=dict(epochs=2, minibatch_size=20))
RUN_ARGS = dict(a2c=dict(), ppo=MB, vmpo=dict(), impala=dict(rows_per_pass=16, vtrace_lambda=0.95, **MB))
PARENT_KEYS = dict(a2c=["GradNorm"], ppo=["GradNorm"], vmpo=["GradNorm", "Eta", "Alpha", "MeanKL"],
                   impala=["GradNorm", "RhoMean", "RhoClipFrac"])


def test_popart_ppo_at_beta_zero_is_plain_ppo(monkeypatch):
    """beta 0 from (mu, sigma) = (0, 1): the statistics stay, ratio = 1, every PopArt operation is an exact identity.
    Plain PPO runs with the rollout's stored activations switched off, so both take the full forward."""
    from accel_rl_amd.algos.pg.ppo import PPO
    algo, policy, log = _train(_classes()["ppo"], True, 3, beta=0., **MB)
    monkeypatch.setenv("ARL_REUSE_ACTS", "0")
    algo_p, policy_p, log_p = _train(PPO, True, 3, **MB)
    assert np.array_equal(log["first"], log_p["first"])
    _same_bits(policy.get_param_values(), policy_p.get_param_values(), "policy parameters")
    for x, y in zip(log["infos"], log_p["infos"]):
        _same_bits(x["GradNorm"], y["GradNorm"], "GradNorm")
        assert x["PopArtMu"][0] == 0 and x["PopArtSigma"][0] == 1
    assert not np.array_equal(policy.get_param_values(), log["first"])
    assert algo.popart_state() == dict(mu=0., nu=1., sigma=1., n_updates=3.)


@pytest.mark.parametrize("name", ["a2c", "impala"])
def test_a_power_of_two_reward_scale_moves_the_statistics_and_nothing_else(name):
    """Rewards r from (mu, sigma) = (0, 1) against 1024 r from (0, 1024): every unnormalised quantity is 1024 times the
    other run's, exactly (a power of two commutes with every rounding, no clamp engages), and every normalised one --
    the targets, the head, the gradients, the parameters -- is the same bits."""
    cls = _classes()[name]
    kw = dict(beta=0.25, **RUN_ARGS[name])
    algo, policy, log = _train(cls, True, 3, **kw)
    algo_s, policy_s, log_s = _train(cls, True, 3, reward_scale=1024., popart_init=(0., 1024.), **kw)
    assert np.array_equal(log["first"], log_s["first"])
    for r, r_s in zip(log["rewards"], log_s["rewards"]):
        _same_bits(r, r_s, "the rollouts' rewards")
    assert any(np.abs(r).max() > 0 for r in log["rewards"])
    _same_bits(policy.get_param_values(), policy_s.get_param_values(), "policy parameters")
    assert not np.array_equal(policy.get_param_values(), log["first"])
    for x, y in zip(log["infos"], log_s["infos"]):
        _same_bits(x["GradNorm"], y["GradNorm"], "GradNorm")
        _same_bits(x["PopArtSigma"] * F32(1024.), y["PopArtSigma"], "PopArtSigma")
        _same_bits(x["PopArtMu"] * F32(1024.), y["PopArtMu"], "PopArtMu")
    st, st_s = algo.popart_state(), algo_s.popart_state()
    assert st_s["sigma"] == 1024. * st["sigma"] and st_s["mu"] == 1024. * st["mu"] and st_s["nu"] == 1024. ** 2 * st["nu"]
    assert st["sigma"] != 1. and st["n_updates"] == st_s["n_updates"] == (3 if name == "a2c" else 6)


@pytest.mark.parametrize("name", ["a2c", "ppo", "vmpo", "impala"])
def test_replayed_iterations_equal_eager_ones(name):
    """Five iterations: two eager, one captured, two replayed; the same seeded run made eagerly ends in the same
    parameters and statistics and returned the same diagnostics, bit for bit."""
    cls = _classes()[name]
    kw = dict(beta=0.1, **RUN_ARGS[name])
    algo, policy, log = _train(cls, True, 5, **kw)
    assert algo._graph is not None and len(log["infos"]) == 5 and list(algo._graphs) == [False]
    final = policy.get_param_values()
    assert np.isfinite(final).all() and not np.array_equal(final, log["first"])
    assert algo.opt_info_keys == PARENT_KEYS[name] + ["PopArtMu", "PopArtSigma"]
    sigmas = [info["PopArtSigma"][0] for info in log["infos"]]
    for info in log["infos"]:
        assert sorted(info) == sorted(algo.opt_info_keys)
        assert all(np.isfinite(v).all() for v in info.values()) and info["PopArtSigma"][0] > 0
    assert all(s != t for s, t in zip(sigmas, sigmas[1:])), sigmas
    algo_e, policy_e, log_e = _train(cls, False, 5, **kw)
    assert algo_e._graph is None
    _assert_same_run(log, policy, log_e, policy_e)
    state, state_e = algo.popart_state(), algo_e.popart_state()
    assert state == state_e and state["n_updates"] == (10 if name == "impala" else 5)
    assert np.float32(state["sigma"]) == sigmas[-1]
    # the snapshot accessors: a round trip through the host, then unnormalize under the state put back
    algo.set_popart_state(2., 29., 5., 7.)
    assert algo.popart_state() == dict(mu=2., nu=29., sigma=5., n_updates=7.)
    out = algo.unnormalize(torch.tensor([0., 1., -0.5], device=DEV)).cpu().numpy()
    assert out.dtype == F32 and out.tolist() == [2., 7., -0.5]


@pytest.mark.parametrize("name", ["a2c", "ppo"])
def test_valids_reach_the_step_under_mid_batch_reset_false(name):
    """Episodes of at most 7 steps in batches of 5 without mid-batch resets: rows after an episode's end are masked.  The
    step's inputs and outputs of three eager iterations against the restatement, bit for bit -- the moments run over the
    valid rows, the masked rows come out 0 --, and the replayed run against the eager one."""
    cls = _classes()[name]
    kw = dict(beta=0.25, mid_batch_reset=False, max_path_length=7, **RUN_ARGS[name])
    seen = []

    def wrap(algo):
        inner = algo._popart_step

        def watched(opt):
            w, b = algo._pa_head
            before = dict(ret=opt["returns"].clone(), adv=opt["advantages"].clone(), valids=opt["valids"].clone(),
                          stats=algo._pa_stats.clone(), w=w.clone(), b=b.clone())
            inner(opt)
            seen.append(dict(before, ret_n=opt["returns"].clone(), adv_n=opt["advantages"].clone(),
                             stats_n=algo._pa_stats.clone(), w_n=w.clone(), b_n=b.clone(), diag=algo._pa_diag.clone()))
        algo._popart_step = watched
    algo_e, policy_e, log_e = _train(cls, False, 5, wrap=wrap, **kw)
    assert algo_e._use_valids and len(seen) == 5
    masked = 0
    for rec in seen:
        h = {k: v.cpu().numpy().reshape(-1) for k, v in rec.items()}
        assert h["valids"].dtype == np.int8 and h["valids"].any()
        masked += int((h["valids"] == 0).sum())
        ret_n, adv_n, stats_n, w_n, b_n, diag = popart_ref.step(h["ret"], h["adv"], h["valids"], 0.25, 1e-4, 1e6, h["stats"],
                                                                h["w"], h["b"])
        for got, want, what in ((h["ret_n"], ret_n, "returns"), (h["adv_n"], adv_n, "advantages"), (h["w_n"], w_n, "row"),
                                (h["stats_n"], stats_n, "stats"), (h["b_n"], b_n, "bias"), (h["diag"], diag, "diag2")):
            _same_bits(got, want, what)
        assert (h["ret_n"][h["valids"] == 0] == 0).all() and stats_n[3] == h["stats"][3] + 1
    assert masked > 0
    algo, policy, log = _train(cls, True, 5, **kw)
    assert algo._graph is not None
    _assert_same_run(log, policy, log_e, policy_e)
    assert algo.popart_state() == algo_e.popart_state()
