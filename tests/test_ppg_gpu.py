"""PPG on the GPU: arl_ppg_head_loss_parts (csrc/ppg.hip) against the float64 restatement tests/ppg_ref.py at the sizes
where its kernels change arm, the policies' loss kinds 2 and 3 against float64 autograd, and the learner -- both graphs,
the rollout memory, the auxiliary phase's own optimizer state, replayed iterations equal to eager ones bit for bit.

Kernel tolerances are the head tests' own (test_head_limits_gpu._tol: 2e-5 sqrt(k_red) max|want|), the whole-step ones
the project's (rtol 2e-3, atol 2e-5 max |.|).  As there, every PPO ratio sits a clear margin inside or outside the clip
range or is exactly 1, so that no decision depends on fp32 rounding."""
import functools

import numpy as np
import pytest
import torch

import autograd_ref
import ppg_ref
import resnet_ref as rr
import test_resnet_gpu as trg
from test_head_limits_gpu import _close, _head_inputs, _nan, _tol, _untouched

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")

# (n_actions, hid, batch): HEAD_CASES' arms -- the generic and the specialised widths, the head gradient summed inside
# the launch ((A + 1) hid <= 3 072) and by the row-split kernel, empty and long splits, LDS past 64 KiB
CASES = [(1, 1, 1), (2, 4, 3), (17, 60, 15), (18, 128, 1025), (2, 1000, 1025), (17, 1000, 4097), (6, 512, 4097),
         (18, 1024, 1), (18, 1024, 12288), (6, 64, 5), (6, 256, 5)]
VARIANTS = [(i, m, c) for i in (True, False) for m in (True, False) for c in (True, False)]     # idx, relu mask, inv_count
_case_id = lambda c: "A%d-hid%d-B%d" % c                                                       # noqa: E731
_var_id = lambda v: "%s-%s-%s" % (("idx" if v[0] else "rows"), ("mask" if v[1] else "nomask"),  # noqa: E731
                                  ("inv" if v[2] else "mean"))


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _launch(L, phase, h, w, b, act, adv, ret, old, idx, lr_mult, inv, clip, c_v, c_e, beta, mask_dh,
            tie_rule=0):
    """One arl_ppg_head_loss_parts + the fold, every output inside a larger NaN-filled buffer."""
    batch, hid = h.shape
    K = w.shape[0]
    o = dict(dout=_nan(batch + 1, K), dh=_nan(batch + 1, hid), dw=_nan(K + 1, hid), db=_nan(K + 4), loss4=_nan(5))
    folds = L.FoldList()
    folds.ppg_head_loss(h, w, b, act, adv, ret, old, idx, lr_mult, inv, K - 1, phase, clip, c_v, c_e, beta,
                        o["dout"][:batch], o["dh"][:batch], o["dw"][:K], o["db"][:K], o["loss4"][:4],
                        L.pg_head_workspace(DEV), relu_mask_dh=mask_dh, tie_rule=tie_rule)
    folds.run()
    torch.cuda.synchronize()
    assert _untouched(o["dout"][batch]) and _untouched(o["dh"][batch]) and _untouched(o["dw"][K])
    assert _untouched(o["db"][K:]) and _untouched(o["loss4"][4:])
    return dict(dout=o["dout"][:batch], dh=o["dh"][:batch], dw=o["dw"][:K], db=o["db"][:K], loss4=o["loss4"][:4])


def _policy_setup(L, case, with_idx, seed_salt=0):
    """_head_inputs plus PPO's old probabilities as test_head_limits_gpu builds them: the kernel's own fp32 probability
    of the taken action divided by a ratio a clear margin inside / outside [0.88, 1.12], or exactly it."""
    n_act, hid, batch = case
    gen, h, w, b, act, adv, ret, idx = _head_inputs(n_act, hid, batch, 7 * hid + n_act + batch + 1 + seed_salt)
    n_rows = adv.numel()
    if not with_idx:
        idx = None
    sel = torch.arange(batch, device=DEV) if idx is None else idx.long()
    rows = torch.arange(batch, device=DEV)
    a = act[sel].long()
    old = torch.softmax(torch.randn(n_rows, n_act, device=DEV, generator=gen), 1)
    p_k, v_k = torch.empty(batch, n_act, device=DEV), torch.empty(batch, device=DEV)
    L.pg_head_infer(h, w, b, p_k, v_k)
    pa_k = p_k[rows, a]
    r = torch.tensor([0.5, 0.95, 1.05, 2.0, 1.0], device=DEV)[rows % 5]
    old[sel, a] = torch.where(r == 1., pa_k, pa_k / r)
    c_eff = float(np.float32(0.2) * np.float32(0.6))
    rk = (pa_k + np.float32(1e-8)) / (old[sel, a] + np.float32(1e-8))
    assert bool((((rk - (1. - c_eff)).abs() > 0.02) & ((rk - (1. + c_eff)).abs() > 0.02)).all())
    assert bool((rk[r == 1.] == 1.).all())
    return dict(h=h, w=w, b=b, act=act, adv=adv, ret=ret, idx=idx, sel=sel, a=a, old=old, c_eff=c_eff, gen=gen,
                lr_mult=torch.full((1,), 0.6, device=DEV), p_k=p_k)


def _weights(batch, with_inv):
    """(inv_count tensor or None, float64 row weights): a caller's count that is not 1 / batch, or the mean."""
    if not with_inv:
        return None, torch.full((batch,), 1. / batch, dtype=torch.float64, device=DEV)
    inv = torch.full((1,), 1. / (batch + 3), device=DEV)
    return inv, inv.double().expand(batch)


def _check_losses(loss4, rows3):
    """Each loss is a sum over the batch: its error relative to the sum of its terms' magnitudes (the head tests' rule)."""
    want = [r.sum() for r in rows3]
    scale = [r.abs().sum() for r in rows3]
    want.append(sum(want))
    scale.append(sum(scale))
    for i in range(4):
        err = abs(loss4[i].item() - want[i].item())
        assert err <= 1e-5 * (scale[i].item() + 1.), (i, err, scale[i].item())


@pytest.mark.parametrize("variant", VARIANTS, ids=_var_id)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_policy_phase_vs_float64(L, case, variant):
    n_act, hid, batch = case
    with_idx, mask_dh, with_inv = variant
    s = _policy_setup(L, case, with_idx)
    inv, wgt = _weights(batch, with_inv)
    clip, c_v, c_e = 0.2, 0.5, 0.01
    got = _launch(L, L.PPG_POLICY, s["h"], s["w"], s["b"], s["act"], s["adv"], s["ret"], s["old"], s["idx"],
                  s["lr_mult"], inv, clip, c_v, c_e, 1.0, mask_dh)
    h64, w64, b64 = s["h"].double(), s["w"].double(), s["b"].double()
    prob, value, _ = ppg_ref.head(h64, w64, b64, n_act)
    sel, a = s["sel"], s["a"]
    adv, ret, old_pa = s["adv"][sel].double(), s["ret"][sel].double(), s["old"][sel, a].double()
    dout = ppg_ref.policy_dout(prob, value, a, adv, ret, old_pa, s["c_eff"], c_v, c_e, wgt)
    dh, dw, db = ppg_ref.head_grads(dout, h64, w64, n_act, stop_value=True)
    if mask_dh:
        dh = dh * (s["h"] > 0)
    K = n_act + 1
    _close(got["dout"], dout, K, "dout")
    _close(got["dh"], dh, K, "dh")
    _close(got["dw"], dw, batch, "dw")
    _close(got["db"], db, batch, "db")
    ratio = (prob[torch.arange(batch, device=DEV), a] + 1e-8) / (old_pa + 1e-8)
    _check_losses(got["loss4"], [-wgt * autograd_ref.ppo_surrogate(ratio, adv, s["c_eff"], "theano"),
                                 c_v * wgt * (value - ret) ** 2,
                                 c_e * wgt * (prob * torch.log(prob + 1e-8)).sum(dim=1)])


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_policy_phase_stops_the_value_gradient_and_equals_ppo_without_it(L, case):
    """dh carries nothing of the value loss: the same bits at v_loss_coeff 0 and at 1 with other returns.  At 0 the whole
    launch is arl_pg_head_loss_parts kind 1, output for output: both run head_kernel_dev.h's kernel with pg_row's
    expressions, a weight of 1.f * inv_n is inv_n, and the value row the policy phase leaves out of dh adds 0 * W."""
    n_act, hid, batch = case
    s = _policy_setup(L, case, True, seed_salt=3)
    args = (s["h"], s["w"], s["b"], s["act"], s["adv"])
    tail = (s["old"], s["idx"], s["lr_mult"], None, 0.2)
    zero = _launch(L, L.PPG_POLICY, *args, s["ret"], *tail, 0.0, 0.01, 1.0, True)
    one = _launch(L, L.PPG_POLICY, *args, s["ret"] * 3. + 1., *tail, 1.0, 0.01, 1.0, True)
    assert torch.equal(zero["dh"], one["dh"])
    assert torch.equal(zero["dout"][:, :n_act], one["dout"][:, :n_act]) and not zero["dout"][:, n_act].any()
    assert bool((one["dout"][:, n_act] != 0).any()) and not torch.equal(zero["dw"][n_act], one["dw"][n_act])
    K = n_act + 1
    ppo = dict(dout=_nan(batch, K), dh=_nan(batch, hid), dw=_nan(K, hid), db=_nan(K), loss4=_nan(4))
    L.pg_head_loss(s["h"], s["w"], s["b"], s["act"], s["adv"], s["ret"], s["old"], None, s["idx"], s["lr_mult"], None,
                   n_act, 1, 0.2, 0.0, 0.01, ppo["dout"], ppo["dh"], ppo["dw"], ppo["db"], ppo["loss4"],
                   L.pg_head_workspace(DEV), relu_mask_dh=True, tie_rule=L.PPO_TIE_THEANO)
    torch.cuda.synchronize()
    for name in ("dout", "dh", "dw", "db", "loss4"):
        assert torch.equal(zero[name], ppo[name]), name


def _aux_old(gen, n_rows, n_act):
    """Stored probabilities with exact zeros: every third row loses its first action (rows stay distributions where
    another action is left; with one action the row is all zero, which the formulas take as they take any other)."""
    old = torch.softmax(torch.randn(n_rows, n_act, device=DEV, generator=gen), 1)
    old[::3, 0] = 0.
    if n_act > 1:
        old = old / old.sum(dim=1, keepdim=True)
    assert bool((old == 0).any())
    return old


@pytest.mark.parametrize("variant", VARIANTS, ids=_var_id)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_auxiliary_phase_vs_float64(L, case, variant):
    n_act, hid, batch = case
    with_idx, mask_dh, with_inv = variant
    gen, h, w, b, _, _, ret, idx = _head_inputs(n_act, hid, batch, 5 * hid + n_act + batch + 2)
    if not with_idx:
        idx = None
    sel = torch.arange(batch, device=DEV) if idx is None else idx.long()
    old = _aux_old(gen, ret.numel(), n_act)
    inv, wgt = _weights(batch, with_inv)
    beta, c_v = 0.7, 0.5
    # (actions, advantages, lr_mult NULL; clip_param, ent_loss_coeff, tie_rule ignored, even where they are nonsense)
    got = _launch(L, L.PPG_AUX, h, w, b, None, None, ret, old, idx, None, inv, NAN, c_v, NAN, beta, mask_dh, tie_rule=77)
    h64, w64, b64 = h.double(), w.double(), b.double()
    prob, value, _ = ppg_ref.head(h64, w64, b64, n_act)
    old64, ret64 = old[sel].double(), ret[sel].double()
    dout = ppg_ref.aux_dout(prob, value, ret64, old64, beta, c_v, wgt)
    dh, dw, db = ppg_ref.head_grads(dout, h64, w64, n_act, stop_value=False)
    if mask_dh:
        dh = dh * (h > 0)
    K = n_act + 1
    _close(got["dout"], dout, K, "dout")
    _close(got["dh"], dh, K, "dh")
    _close(got["dw"], dw, batch, "dw")
    _close(got["db"], db, batch, "db")
    kl_terms = old64 * (torch.log(old64 + 1e-8) - torch.log(prob + 1e-8))
    want_clone, want_v = ppg_ref.aux_losses(prob, value, ret64, old64, beta, c_v, wgt)
    scale_clone = (beta * wgt[:, None] * kl_terms.abs()).sum().item()
    assert abs(got["loss4"][0].item() - want_clone.item()) <= 1e-5 * (scale_clone + 1.)
    assert abs(got["loss4"][1].item() - want_v.item()) <= 1e-5 * (want_v.item() + 1.)
    assert got["loss4"][2].item() == 0.
    assert abs(got["loss4"][3].item() - (want_clone + want_v).item()) <= 1e-5 * (scale_clone + want_v.item() + 1.)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_auxiliary_phase_at_its_own_probabilities_and_at_beta_zero(L, case):
    n_act, hid, batch = case
    gen, h, w, b, _, _, ret, _ = _head_inputs(n_act, hid, batch, 3 * hid + n_act + batch + 4)
    own, v_k = torch.empty(batch, n_act, device=DEV), torch.empty(batch, device=DEV)
    L.pg_head_infer(h, w, b, own, v_k)
    beta = 0.7
    got = _launch(L, L.PPG_AUX, h, w, b, None, None, ret[:batch].contiguous(), own, None, None, None, 0., 0.5, 0., beta,
                  False)
    zeros = torch.zeros(batch, n_act, dtype=torch.float64, device=DEV)
    _close(got["dout"][:, :n_act], zeros, n_act + 1, "dout at old == p", scale=beta / batch)
    assert abs(got["loss4"][0].item()) <= _tol(zeros, n_act + 1, scale=beta)
    old = _aux_old(gen, batch, n_act)
    got = _launch(L, L.PPG_AUX, h, w, b, None, None, ret[:batch].contiguous(), old, None, None, None, 0., 0.5, 0., 0.0,
                  False)
    assert not got["dout"][:, :n_act].any() and got["loss4"][0].item() == 0.
    assert bool((got["dout"][:, n_act] != 0).any())


@pytest.mark.parametrize("phase", [0, 1], ids=["policy", "aux"])
def test_two_launches_give_the_same_bits(L, phase):
    for case in ((6, 512, 4097), (2, 1000, 1025), (17, 60, 15)):
        s = _policy_setup(L, case, True, seed_salt=9)
        run = lambda: _launch(L, phase, s["h"], s["w"], s["b"], s["act"], s["adv"], s["ret"], s["old"], s["idx"],   # noqa: E731
                              s["lr_mult"], None, 0.2, 0.5, 0.01, 0.7, True)
        first, second = run(), run()
        for k in first:
            assert torch.equal(first[k], second[k]), (case, k)


def test_refusals_launch_nothing_and_the_limits_run(L):
    batch = 8
    lib = L.load()
    h = torch.rand(batch, 1025, device=DEV)
    w, b = torch.rand(20, 1025, device=DEV), torch.rand(20, device=DEV)
    act = torch.zeros(batch, dtype=torch.uint8, device=DEV)
    adv, ret = torch.rand(batch, device=DEV), torch.rand(batch, device=DEV)
    old, lr_mult = torch.rand(batch, 19, device=DEV), torch.ones(1, device=DEV)
    ws = L.pg_head_workspace(DEV)
    o = dict(dout=_nan(batch, 20), dh=_nan(batch, 1025), dw=_nan(20, 1025), db=_nan(20), loss4=_nan(4))
    items = (L.ArlFoldItem * 3)()
    import ctypes
    base = dict(h=h.data_ptr(), w=w.data_ptr(), b=b.data_ptr(), act=act.data_ptr(), adv=adv.data_ptr(),
                ret=ret.data_ptr(), old=old.data_ptr(), idx=None, lr=lr_mult.data_ptr(), inv=None, n=batch, hid=64,
                n_act=4, phase=0, tie=0, clip=0.2, c_v=0.5, c_e=0.01, beta=1.0, mask=0, dout=o["dout"].data_ptr(),
                dh=o["dh"].data_ptr(), dw=o["dw"].data_ptr(), db=o["db"].data_ptr(), loss4=o["loss4"].data_ptr(),
                ws=ws.data_ptr(), items=ctypes.cast(items, ctypes.c_void_p))

    def call(**kw):
        a = dict(base, **kw)
        return lib.arl_ppg_head_loss_parts(
            a["h"], a["w"], a["b"], a["act"], a["adv"], a["ret"], a["old"], a["idx"], a["lr"], a["inv"], a["n"], a["hid"],
            a["n_act"], a["phase"], a["tie"], a["clip"], a["c_v"], a["c_e"], a["beta"], a["mask"], a["dout"], a["dh"],
            a["dw"], a["db"], a["loss4"], a["ws"], a["items"], L.stream_ptr())

    for phase in (0, 1):
        # ARL_E_RANGE (-2): the first value past each limit
        for kw in (dict(n_act=0), dict(n_act=19), dict(hid=0), dict(hid=1025), dict(n=0), dict(n=1 << 31)):
            assert call(phase=phase, **kw) == -2, (phase, kw)
        # ARL_E_ARG (-1): mandatory pointers, coefficients the phase reads
        for name in ("h", "w", "b", "ret", "old", "dout", "dh", "dw", "db", "loss4", "ws", "items"):
            assert call(phase=phase, **{name: None}) == -1, (phase, name)
        for bad in (NAN, float("inf"), -float("inf")):
            assert call(phase=phase, c_v=bad) == -1
    for phase in (-1, 2):
        assert call(phase=phase) == -1 and b"phase" in lib.arl_last_error()
    for name in ("act", "adv", "lr"):                        # the policy phase reads them; the auxiliary phase does not
        assert call(phase=0, **{name: None}) == -1, name
    for tie in (-1, 3):
        assert call(phase=0, tie=tie) == -1 and b"tie_rule" in lib.arl_last_error()
    for bad in (NAN, float("inf")):
        assert call(phase=0, clip=bad) == -1 and call(phase=0, c_e=bad) == -1 and call(phase=1, beta=bad) == -1
    torch.cuda.synchronize()
    for name, t in o.items():
        assert _untouched(t), name
    assert all(it.part is None and it.out is None for it in items)
    # the limits themselves run: 18 actions x 1024 hidden units
    for phase in (0, 1):
        assert call(phase=phase, n_act=18, hid=1024, act=None if phase else act.data_ptr(),
                    adv=None if phase else adv.data_ptr(), lr=None if phase else lr_mult.data_ptr()) == 0
        L._check(lib.arl_fold_many(items, 3, L.stream_ptr()), "arl_fold_many")
        torch.cuda.synchronize()
        assert torch.isfinite(o["dout"].view(-1)[:batch * 19]).all() and torch.isfinite(o["loss4"]).all()


# ---- policies -----------------------------------------------------------------------------------------------------------

def _whole_step_close(got, want, scale, what):
    err = np.abs(got - want).max()
    print("%-24s max |want| %.3g max err %.3g" % (what, np.abs(want).max(), err))
    assert np.allclose(got, want, rtol=2e-3, atol=2e-5 * scale), (what, err, scale)


class _Float64Net(object):
    """What autograd_ref.forward reads of a policy, with float64 host copies of its internal parameter views."""

    def __init__(self, policy):
        self.params = [p.detach().cpu().double().requires_grad_() for p in policy.params]
        self._conv_geom, self._hid_geom, self._n_conv, self.n_act = (policy._conv_geom, policy._hid_geom, policy._n_conv,
                                                                     policy.n_act)


@functools.lru_cache(maxsize=None)
def _cnn_setup():
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    set_seed(3)
    policy = AtariCnnPolicy(**dict(cnn_specs[0], hidden_sizes=[64]))
    policy.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(6)), device=DEV)
    rs = np.random.RandomState(11)
    n = 40
    obs = torch.from_numpy(rs.randint(0, 256, size=(n, 4, 104, 80), dtype=np.uint8)).to(DEV)
    prob, _ = (t.clone() for t in policy.prob_value(obs))
    data = dict(observations=obs, actions=torch.from_numpy(rs.randint(0, 6, n).astype(np.uint8)).to(DEV),
                advantages=torch.from_numpy(rs.randn(n).astype(np.float32)).to(DEV),
                returns=torch.from_numpy(rs.randn(n).astype(np.float32)).to(DEV),
                old_prob=(prob * 0.9 + 0.1 / 6).contiguous())
    idx = torch.from_numpy(rs.permutation(n)[:24].astype(np.int32)).to(DEV)
    return policy, data, idx


@pytest.mark.parametrize("gather", [True, False], ids=["idx", "rows"])
@pytest.mark.parametrize("kind", [2, 3], ids=["policy", "aux"])
def test_cnn_policy_kinds_match_float64_autograd(kind, gather):
    policy, data, idx = _cnn_setup()
    idx = idx if gather else None
    mb = dict(data, idx=idx)
    lr_mult = torch.full((1,), 0.7, device=DEV)
    clip, c_v, c_e, beta = 0.2, 0.5, 0.01, 0.7
    policy.flat_grads.fill_(NAN)
    loss4 = policy.loss_and_grads(mb, kind, clip, c_v, c_e, lr_mult, beta_clone=beta).cpu().numpy()
    got = [g.detach().cpu().numpy().copy() for g in policy.grads]
    # float64 autograd on host copies of the same internal parameters
    net = _Float64Net(policy)
    x = policy._scaled_f32(data["observations"], idx)[:, :policy._c_in].cpu().double()
    sel = (torch.arange(40) if idx is None else idx.cpu().long())
    n = sel.numel()
    pick = lambda k: data[k].cpu()[sel]                                                      # noqa: E731
    wgt = torch.full((n,), 1. / n, dtype=torch.float64)
    prob, value = autograd_ref.forward(net, x)
    k_head = len(net.params) - 2
    if kind == 2:
        act = pick("actions").long()
        old_pa = pick("old_prob").double()[torch.arange(n), act]
        c_eff = float(np.float32(clip) * np.float32(0.7))
        pi, v, ent = ppg_ref.policy_losses(prob, value, act, pick("advantages").double(), pick("returns").double(),
                                           old_pa, c_eff, c_v, c_e, wgt)
        ratio = ((prob[torch.arange(n), act] + 1e-8) / (old_pa + 1e-8)).detach()
        assert bool(((ratio - 1).abs() - c_eff).abs().min() > 1e-3)      # no row on the surrogate's kinks
        want = list(torch.autograd.grad(pi + ent, net.params, retain_graph=True))
        for k, g in zip((k_head, k_head + 1), torch.autograd.grad(v, net.params[k_head:])):
            want[k] = want[k] + g                                         # the value loss reaches the head alone
        terms = [pi, v, ent]
    else:
        clone, v = ppg_ref.aux_losses(prob, value, pick("returns").double(), pick("old_prob").double(), beta, c_v, wgt)
        want = list(torch.autograd.grad(clone + v, net.params))
        terms = [clone, v, torch.zeros((), dtype=torch.float64)]
    terms = np.array([float(t.detach()) for t in terms])
    _whole_step_close(loss4[:3], terms, np.abs(terms).max(), "losses")
    assert abs(loss4[3] - terms.sum()) <= 2e-3 * np.abs(terms).sum()
    want = [g.numpy() for g in want]
    scale = max(max(np.abs(g).max() for g in want), 1e-3)
    assert all(np.isfinite(g).all() for g in got)
    for k, (g, wv) in enumerate(zip(got, want)):
        assert np.abs(wv).max() > 0, k
        _whole_step_close(g, wv, scale, "kind %d param %d" % (kind, k))


def _assert_value_loss_stays_in_the_head(policy, mb):
    """Kind 2 at v_loss_coeff 0 and 1: every gradient tensor keeps its bits but the head's value row and value bias."""
    lr_mult = torch.ones(1, device=DEV)
    policy.loss_and_grads(mb, 2, 0.2, 0.0, 0.01, lr_mult)
    zero = [g.clone() for g in policy.grads]
    policy.loss_and_grads(mb, 2, 0.2, 1.0, 0.01, lr_mult)
    one = [g.clone() for g in policy.grads]
    k, a = policy._k_head, policy.n_act
    assert tuple(zero[k].shape) == (a + 1, policy._hid_geom[-1][0]) and tuple(zero[k + 1].shape) == (a + 1,)
    for i, (g0, g1) in enumerate(zip(zero, one)):
        if i in (k, k + 1):
            assert torch.equal(g0[:a], g1[:a]) and not g0[a].any() and bool(g1[a].any()), i
        else:
            assert torch.equal(g0, g1) and bool(g0.any()), i


def test_cnn_policy_value_loss_reaches_the_value_row_alone():
    policy, data, idx = _cnn_setup()
    _assert_value_loss_stays_in_the_head(policy, dict(data, idx=idx))


@pytest.mark.parametrize("kind", [2, 3], ids=["policy", "aux"])
def test_cnn_policy_kinds_walked_in_passes_give_the_one_pass_gradient(kind):
    """24 rows in passes of 8 (AtariCnnPolicy.rows_per_pass): the same mean gradient as one pass, beta_clone passed on."""
    policy, data, idx = _cnn_setup()
    mb = dict(data, idx=idx)
    lr_mult = torch.ones(1, device=DEV)
    try:
        policy.max_rows_per_pass = None
        loss_one = policy.loss_and_grads(mb, kind, 0.2, 0.5, 0.01, lr_mult, beta_clone=0.7).clone()
        one = [g.clone() for g in policy.grads]
        policy.max_rows_per_pass = 8
        loss_p = policy.loss_and_grads(mb, kind, 0.2, 0.5, 0.01, lr_mult, beta_clone=0.7).clone()
        passes = [g.clone() for g in policy.grads]
    finally:
        policy.max_rows_per_pass = None
    assert torch.allclose(loss_p, loss_one, rtol=1e-5, atol=1e-6), (loss_p, loss_one)
    scale = max(max(g.abs().max().item() for g in one), 1e-3)
    for g1, gp in zip(one, passes):
        assert torch.allclose(gp, g1, rtol=1e-4, atol=1e-6 * scale), (gp - g1).abs().max().item()


@functools.lru_cache(maxsize=None)
def _resnet_reference(name, kind, gather):
    """The float64 step of test_resnet_gpu.reference_step for PPG's kinds: same parameters, observations, targets and
    behaviour probabilities; kind 2's gradient composed from grad(pi + ent) and the head's own grad(v)."""
    cfg, arr = trg.CASES[name], trg.case_arrays(name)
    ppo = trg.reference_step(name, 1, gather)
    rp, pos = [], 0
    for _, shape in trg._layout(name):
        m = int(np.prod(shape))
        rp.append(torch.from_numpy(arr["flat"][pos:pos + m].reshape(shape).astype(np.float64)).requires_grad_())
        pos += m
    rows = arr["idx"].astype(np.int64) if gather else np.arange(cfg["batch"])
    x = torch.from_numpy(arr["obs"][rows].astype(np.float64)) * np.float64(np.float32(1. / 255))
    prob, value, taps = rr.ref_net(rp, cfg["channels"], cfg["blocks"], len(cfg["hidden"]), cfg["n_act"], x)
    pick = lambda a: torch.from_numpy(a[rows].astype(np.float64))                              # noqa: E731
    old = pick(ppo["old_prob"])
    n = len(rows)
    wgt = torch.full((n,), 1. / n, dtype=torch.float64)
    if kind == 2:
        act = torch.from_numpy(arr["actions"][rows].astype(np.int64))
        pi, v, ent = ppg_ref.policy_losses(prob, value, act, pick(arr["advantages"]), pick(arr["returns"]),
                                           old[torch.arange(n), act], trg.CLIP, trg.V_COEFF, trg.ENT_COEFF, wgt)
        # reference layout: ..., policy (W, b), value (W, b) -- the last two are the head's value row and bias, the only
        # tensors the value loss reaches (and pi + ent does not)
        grads = list(torch.autograd.grad(pi + ent, rp[:-2], retain_graph=True)) + list(torch.autograd.grad(v, rp[-2:]))
        losses = [pi, v, ent]
    else:
        clone, v = ppg_ref.aux_losses(prob, value, pick(arr["returns"]), old, BETA, trg.V_COEFF, wgt)
        grads = list(torch.autograd.grad(clone + v, rp))
        losses = [clone, v, torch.zeros((), dtype=torch.float64)]
    return dict(losses=np.array([float(t.detach()) for t in losses]), grads=[g.numpy() for g in grads],
                margin=rr.branch_margin(taps), old_prob=ppo["old_prob"], names=[n_ for n_, _ in trg._layout(name)])


BETA = 0.7


@pytest.mark.parametrize("gather", [True, False], ids=["idx", "rows"])
@pytest.mark.parametrize("kind", [2, 3], ids=["policy", "aux"])
@pytest.mark.parametrize("name", sorted(trg.CASES))
def test_resnet_policy_kinds_match_float64_autograd(name, kind, gather):
    cfg, arr = trg.CASES[name], trg.case_arrays(name)
    ref = _resnet_reference(name, kind, gather)
    assert ref["margin"] > rr.BRANCH_MARGIN, ref["margin"]
    policy = trg._make_policy(name)
    policy.set_param_values(arr["flat"])
    batch = cfg["batch"]
    cut = (lambda a: a) if gather else (lambda a: a[:batch])
    dev = trg._dev
    mb = dict(observations=dev(cut(arr["obs"])), idx=dev(arr["idx"]) if gather else None,
              actions=dev(cut(arr["actions"])), advantages=dev(cut(arr["advantages"])),
              returns=dev(cut(arr["returns"])), old_prob=dev(cut(ref["old_prob"])))
    policy.flat_grads.fill_(NAN)
    loss4 = trg._host(policy.loss_and_grads(mb, kind, trg.CLIP, trg.V_COEFF, trg.ENT_COEFF, torch.ones(1, device=DEV),
                                            beta_clone=BETA))
    got_flat = policy.bucket_to_reference(policy.flat_grads)
    _whole_step_close(loss4[:3], ref["losses"], np.abs(ref["losses"]).max(), "losses")
    assert abs(float(loss4[3]) - ref["losses"].sum()) <= 2e-3 * np.abs(ref["losses"]).sum()
    want_flat = np.concatenate([g.reshape(-1) for g in ref["grads"]])
    assert np.isfinite(got_flat).all() and got_flat.size == want_flat.size
    scale, pos = max(np.abs(want_flat).max(), 1e-3), 0
    for gname, want in zip(ref["names"], ref["grads"]):
        got = got_flat[pos:pos + want.size].reshape(want.shape)
        pos += want.size
        assert np.abs(want).max() > 0, gname
        _whole_step_close(got, want, scale, "%s kind %d %s" % (name, kind, gname))
    if kind == 2 and gather:
        _assert_value_loss_stays_in_the_head(policy, mb)


# ---- learner ------------------------------------------------------------------------------------------------------------

def _train(use_graph, n_itr, resnet=False, wrap=None):
    """PPG on the synthetic pong, 8 envs x horizon 5: n_pi 2, two auxiliary epochs of four minibatches of 20 over the 80
    stored rows, pi_old computed in passes of 16.  wrap(algo, policy): called once initialize has run."""
    from accel_rl_amd.algos.pg import PPG
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.atari_resnet_policy import AtariResnetPolicy
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game="pong"), horizon=5, n_parallel=2, envs_per=2,
                            max_path_length=25, max_decorrelation_steps=0, device=DEV)
    algo = PPG(n_pi=2, e_aux=2, aux_minibatch_size=20, rows_per_pass=16, optimizer_args=dict(minibatch_size=20),
               use_graph=use_graph)
    policy = AtariResnetPolicy() if resnet else AtariCnnPolicy(**dict(cnn_specs[0], hidden_sizes=[64]))
    log = dict(infos=[])
    initialize, optimize = algo.initialize, algo.optimize_policy

    def watching_initialize(*a, **kw):
        initialize(*a, **kw)
        log["first"] = policy.get_param_values()
        if wrap is not None:
            wrap(algo, policy)

    def recording_optimize(itr, samples):
        out = optimize(itr, samples)
        log["infos"].append(out[1])
        return out
    algo.initialize, algo.optimize_policy = watching_initialize, recording_optimize
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=40 * (n_itr - 1), seed=9, log_interval_steps=40)
    runner.train()
    torch.cuda.synchronize()
    log["infos"] = [{k: trg._host(v).copy() for k, v in info.items()} for info in log["infos"]]
    return algo, policy, log


def _assert_same_run(log, policy, log_e, policy_e):
    assert np.array_equal(log["first"], log_e["first"])
    np.testing.assert_array_equal(policy_e.get_param_values(), policy.get_param_values())
    assert len(log["infos"]) == len(log_e["infos"])
    for a, b in zip(log["infos"], log_e["infos"]):
        assert sorted(a) == sorted(b)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_ppg_trains_and_replayed_phases_equal_eager_ones():
    """Nine iterations: the policy phase is captured at the third; auxiliary phases follow iterations 2, 4, 6, 8 -- two
    eager, one captured, one replayed.  The same seeded run made eagerly ends in the same parameters and returned the same
    diagnostics, bit for bit."""
    algo, policy, log = _train(True, 9)
    assert algo._graph is not None and algo._aux_graph is not None
    assert (algo._calls, algo._aux_phases, algo._mem_rows) == (9, 4, 80)
    assert algo._aux_opt._n_minibatches == 8 and algo.optimizer._n_minibatches == 2
    final = policy.get_param_values()
    assert np.isfinite(final).all() and not np.array_equal(final, log["first"]) and len(log["infos"]) == 9
    for i, info in enumerate(log["infos"]):
        assert sorted(info) == ["AuxCloneLoss", "AuxVLoss", "GradNorm"]
        assert info["GradNorm"].shape == (2,) and info["AuxVLoss"].shape == (1,) and info["AuxCloneLoss"].shape == (1,)
        assert all(np.isfinite(v).all() for v in info.values()) and (info["GradNorm"] > 0).all()
        if i < 2:                        # before the first auxiliary phase has completed
            assert info["AuxVLoss"][0] == 0 and info["AuxCloneLoss"][0] == 0
        else:
            assert info["AuxVLoss"][0] > 0 and info["AuxCloneLoss"][0] >= 0
    vs = [info["AuxVLoss"][0] for info in log["infos"]]
    assert vs[2] == vs[3] and vs[4] == vs[5] and len(set(vs[2::2])) == 4      # one value per completed phase
    algo_e, policy_e, log_e = _train(False, 9)
    assert algo_e._graph is None and algo_e._aux_graph is None and algo_e._aux_phases == 4
    _assert_same_run(log, policy, log_e, policy_e)


def test_ppg_trains_the_residual_network():
    algo, policy, log = _train(True, 5, resnet=True)
    assert algo._graph is not None and algo._aux_phases == 2 and policy.n_params == 1164759
    final = policy.get_param_values()
    assert np.isfinite(final).all() and not np.array_equal(final, log["first"])
    assert log["infos"][1]["AuxVLoss"][0] == 0 and log["infos"][2]["AuxVLoss"][0] > 0
    algo_e, policy_e, log_e = _train(False, 5, resnet=True)
    assert algo_e._graph is None
    _assert_same_run(log, policy, log_e, policy_e)


def test_auxiliary_phase_sees_the_last_rollouts_and_keeps_the_policy_optimizer_state():
    """One eager run, watched: at the start of an auxiliary phase the memory holds the last two rollouts in slot order;
    pi_old is prob_value_rows under the parameters of that moment; the phase moves the parameters and leaves the
    policy-phase optimizer's moments and step count alone."""
    rollouts, phases = [], []

    def wrap(algo, policy):
        process, device_aux = algo.process_samples, algo._device_aux

        def watched_process(itr, samples):
            opt = process(itr, samples)
            rollouts.append((samples["observations"].clone(), opt["returns"].clone()))
            return opt

        def watched_aux():
            o = algo.optimizer
            before = dict(obs=algo._mem_obs.clone(), ret=algo._mem_ret.clone(), params=policy.flat_params.clone(),
                          m=o._slot0.clone(), v=o._slot1.clone(), t=o._step_count.clone(),
                          aux_t=algo._aux_opt._step_count.clone(), n_rollouts=len(rollouts))
            before["want_old"] = policy.prob_value_rows(algo._mem_obs, 16, tag="ppg_check")[0].clone()
            device_aux()
            before["got_old"] = policy._scratch[("pv_prob" + "ppg_aux", 80)].clone()
            before["after"] = dict(params=policy.flat_params.clone(), m=o._slot0.clone(), v=o._slot1.clone(),
                                   t=o._step_count.clone(), aux_t=algo._aux_opt._step_count.clone())
            phases.append(before)
        algo.process_samples, algo._device_aux = watched_process, watched_aux
    algo, policy, log = _train(False, 4, wrap=wrap)
    assert len(rollouts) == 4 and len(phases) == 2
    for p, ph in enumerate(phases):
        assert ph["n_rollouts"] == 2 * (p + 1)
        for slot in range(2):
            obs, ret = rollouts[2 * p + slot]
            assert torch.equal(ph["obs"][40 * slot:40 * (slot + 1)], obs)
            assert torch.equal(ph["ret"][40 * slot:40 * (slot + 1)], ret)
        assert torch.equal(ph["got_old"], ph["want_old"]) and float(ph["got_old"].std()) > 0
        after = ph["after"]
        assert torch.equal(after["m"], ph["m"]) and torch.equal(after["v"], ph["v"]) and torch.equal(after["t"], ph["t"])
        assert bool(ph["m"].any()) and float(ph["t"]) > 0
        assert not torch.equal(after["params"], ph["params"])
        assert float(after["aux_t"]) > float(ph["aux_t"])               # its own step count moved instead
    assert not torch.equal(phases[0]["obs"], phases[1]["obs"])
