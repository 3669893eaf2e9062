"""ACER on the GPU: the four kernels of csrc/acer.hip against tests/acer_ref.py (bit for bit where the header says so,
under the derived bound elsewhere), their refusals, and the learner: one update against the float64 reference network,
the tie to the A2C head kernel (launched), the replay memory and its staging, and the two captured graphs against eager runs."""
import functools

import numpy as np
import pytest
import torch

import acer_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
E_ARG, E_RANGE, E_ALIGN = -1, -2, -3
F32 = np.float32


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


# ---- the scan ---------------------------------------------------------------------------------------------------------

def _scan(L, c, lam, stats=True, v_out=True, discount=0.99):
    n_env, T = c["n_env"], c["horizon"]
    d = {k: _dev(c[k]) for k in ("prob", "prob_last", "q", "q_last", "old_prob", "actions", "rewards", "dones")}
    A = c["prob"].shape[1]
    qret = torch.full((n_env * T,), NAN, device=DEV)
    v = torch.full((n_env * T,), NAN, device=DEV) if v_out else None
    st = torch.full((n_env, 2), NAN, device=DEV) if stats else None
    L.acer_retrace_scan(d["prob"], d["prob_last"], d["q"][:, :A], d["q_last"][:, :A], d["old_prob"], d["actions"],
                        d["rewards"], d["dones"], discount, lam, n_env, T, qret, v_out=v, stats=st)
    return _host(qret), None if v is None else _host(v), None if st is None else _host(st)


@pytest.mark.parametrize("done_at", [0, -1, None], ids=["done_first", "done_last", "no_done"])
@pytest.mark.parametrize("n_env,horizon,n_act", [(1, 1, 1), (2, 2, 2), (65, 5, 18), (3, 4096, 6)])
def test_retrace_scan_equals_the_float64_restatement_bit_for_bit(L, n_env, horizon, n_act, done_at):
    """(3, 4096, 6) walks four staging chunks; planted: behaviour probabilities of 0 and action bytes of 255."""
    c = ar.scan_case(100 * n_env + n_act, n_env, horizon, n_act, 64, done_at=done_at, mu_zero=True, act255=True)
    for lam in (0.0, 1.0):
        got = _scan(L, c, lam)
        want = ar.retrace(c["prob"], c["prob_last"], c["q"], c["q_last"], c["old_prob"], c["actions"], c["rewards"],
                          c["dones"], 0.99, lam, n_env, horizon)
        for g, w, name in zip(got, want, ("qret", "v", "stats")):
            np.testing.assert_array_equal(g, w, err_msg="%s lambda %g" % (name, lam))
        assert np.isfinite(got[0]).all() and got[2][:, 0].max() > 1e3


def test_retrace_scan_at_the_stride_limit_is_deterministic_and_its_outputs_are_optional(L):
    c = ar.scan_case(7, 2, 2, 2, 1 << 20, done_at=0)
    first, again, bare = _scan(L, c, 1.0), _scan(L, c, 1.0), _scan(L, c, 1.0, stats=False, v_out=False)
    want = ar.retrace(c["prob"], c["prob_last"], c["q"], c["q_last"], c["old_prob"], c["actions"], c["rewards"],
                      c["dones"], 0.99, 1.0, 2, 2)
    for g, a, w in zip(first, again, want):
        np.testing.assert_array_equal(g, w)
        np.testing.assert_array_equal(g, a)
    np.testing.assert_array_equal(bare[0], want[0])
    assert bare[1] is None and bare[2] is None


def test_retrace_scan_refusals_launch_nothing(L):
    lib = L.load()
    n_env, T, A, S = 3, 4, 6, 8
    steps = n_env * T
    prob, old = (torch.full((steps + 1, A), 1.0 / A, device=DEV) for _ in range(2))
    pl = torch.full((n_env + 1, A), 1.0 / A, device=DEV)
    q, ql = torch.zeros((steps + 1, S), device=DEV), torch.zeros((n_env + 1, S), device=DEV)
    rew = torch.zeros(steps + 1, device=DEV)
    act, done = (torch.zeros(steps, dtype=torch.uint8, device=DEV) for _ in range(2))
    qret, v = (torch.full((steps + 1,), NAN, device=DEV) for _ in range(2))
    stats = torch.full((n_env + 1, 2), NAN, device=DEV)
    p = lambda t: t.data_ptr()                                  # noqa: E731

    def scan(pr=p(prob), pL=p(pl), qq=p(q), qL=p(ql), s=S, ol=p(old), ac=p(act), re=p(rew), do=p(done), g=0.99, lam=1.0,
             n=n_env, t=T, a=A, out=p(qret), vo=p(v), st=p(stats)):
        return lib.arl_acer_retrace_scan(pr, pL, qq, qL, s, ol, ac, re, do, g, lam, n, t, a, out, vo, st, None)

    for k in ("pr", "pL", "qq", "qL", "ol", "ac", "re", "do", "out"):
        assert scan(**{k: None}) == E_ARG and b"null" in lib.arl_last_error(), k
    for kw in (dict(n=0), dict(n=2 ** 31), dict(t=0), dict(t=4097), dict(a=0), dict(a=19), dict(s=4), dict(s=10),
               dict(s=(1 << 20) + 4)):
        assert scan(**kw) == E_RANGE, kw
    for kw in (dict(g=-0.01), dict(g=1.01), dict(g=NAN), dict(lam=-0.01), dict(lam=INF), dict(lam=NAN)):
        assert scan(**kw) == E_ARG, kw
    for kw in (dict(out=p(rew)), dict(vo=p(prob) + 16), dict(st=p(ql)), dict(vo=p(qret)), dict(st=p(v) + 8),
               dict(out=p(q) + 4)):
        assert scan(**kw) == E_ARG and b"overlap" in lib.arl_last_error(), kw
    for k, t in (("pr", prob), ("pL", pl), ("qq", q), ("qL", ql), ("ol", old), ("re", rew), ("out", qret), ("vo", v),
                 ("st", stats)):
        assert scan(**{k: p(t) + 2}) == E_ALIGN, k
    torch.cuda.synchronize()
    assert all(torch.isnan(x).all() for x in (qret, v, stats))
    assert scan(vo=None, st=None) == 0
    torch.cuda.synchronize()
    assert (qret[:steps] == 0).all() and torch.isnan(qret[steps:]).all() and torch.isnan(v).all()


# ---- the loss ---------------------------------------------------------------------------------------------------------

def _loss(L, c, cc, delta, q_coeff=0.5, ent=0.01):
    B, S = c["out"].shape[0], c["half"]
    dout = torch.full((B, 2 * S), NAN, device=DEV)
    stats = torch.full((5, B), NAN, device=DEV)
    L.acer_loss(_dev(c["out"]), _dev(c["out_avg"]), _dev(c["old_prob"]), _dev(c["actions"]), _dev(c["qret"]),
                None if c["idx"] is None else _dev(c["idx"]), c["n_act"], cc, delta, q_coeff, ent, dout, stats)
    return _host(dout), _host(stats)


WORST = dict(ratio=0.0)


@pytest.mark.parametrize("with_idx", [False, True], ids=["rows", "idx"])
@pytest.mark.parametrize("n_act", [1, 2, 18])
@pytest.mark.parametrize("batch", [1, 63, 64, 65, 257])
def test_acer_loss_against_the_restatement(L, batch, n_act, with_idx):
    """c below and above every rho of the case, 1, +inf, and exactly one exact row's rho(a_t) (rho_t < c at equality); delta 0 (projection active wherever k . g > 0), a delta that
    leaves it active on some rows and inactive on others, and +inf.  One-hot rows and rows whose average policy is disjoint
    from the live one are planted (acer_ref.loss_case); one-action rows and one-hot rows are bit for bit."""
    c = ar.loss_case(17 * batch + n_act + int(with_idx), batch, n_act, with_idx)
    lo, hi = ar.rho_range(c)
    exact = ar.soft_exact(c["out"][:, :n_act]) & ar.soft_exact(c["out_avg"][:, :n_act])
    assert exact.all() if n_act == 1 else (batch < 4 or (exact.any() and not exact.all()))
    rho_t = ar.loss(c, 1.0, INF, 0.5, 0.01, exact_soft=True)[1][4]              # float64, exact on the exact rows
    at = [float(r) for r in rho_t[exact] if r > 0][:1]                             # c AT one row's rho(a_t): the tie
    for cc in [0.5 * lo if lo > 0 else 1e-3, float(F32(1.0)), 2.0 * hi + 1.0, INF] + at:
        for delta in (0.0, 0.5, INF):
            dout, stats = _loss(L, c, cc, delta)
            S = c["half"]
            assert (dout[:, n_act:S] == 0).all() and np.isfinite(dout).all() and np.isfinite(stats).all()
            q_cols = dout[:, S:].copy()
            src = c["idx"] if with_idx else np.arange(batch)
            act = np.minimum(c["actions"][src].astype(np.int64), n_act - 1)
            q_cols[np.arange(batch), act] = 0
            assert (q_cols == 0).all()
            w32, s32, core = ar.loss(c, cc, delta, 0.5, 0.01, exact_soft=True)
            np.testing.assert_array_equal(dout[exact], w32[exact].astype(F32), err_msg=str((cc, delta)))
            np.testing.assert_array_equal(stats[:, exact], s32[:, exact].astype(F32), err_msg=str((cc, delta)))
            if delta == INF:
                assert (stats[3] == 0).all()
            w64, s64, _ = ar.loss(c, cc, delta, 0.5, 0.01, exact_soft=False)
            d_atol, s_atol = ar.loss_bound(c, cc, delta, 0.5, 0.01)
            r = max(float((np.abs(dout - w64) / d_atol)[~exact].max(initial=0)),
                    float((np.abs(stats - s64) / s_atol)[:, ~exact].max(initial=0)))
            WORST["ratio"] = max(WORST["ratio"], r)
            assert r <= 1.0, (cc, delta, r)
    print("largest observed error over bound so far: %.3g" % WORST["ratio"])


def test_acer_loss_refusals_launch_nothing(L):
    """(The kk == 0 guard cannot be reached from soft-max rows; tests/test_acer_host.py shows it on the restatement.)"""
    lib = L.load()
    B, A, S = 5, 6, 32
    out, avg, dout = (torch.zeros((B + 1, 2 * S), device=DEV) for _ in range(3))
    dout.fill_(NAN)
    mu = torch.full((B + 1, A), 1.0 / A, device=DEV)
    act = torch.zeros(B, dtype=torch.uint8, device=DEV)
    qret = torch.zeros(B + 1, device=DEV)
    stats = torch.full((5 * B + 5,), NAN, device=DEV)
    p = lambda t: t.data_ptr()                                  # noqa: E731

    def loss(o=p(out), oa=p(avg), m=p(mu), ac=p(act), qr=p(qret), ix=None, b=B, a=A, s=S, c=10.0, dl=1.0, qc=0.5, ec=0.01,
             do=p(dout), st=p(stats)):
        return lib.arl_acer_loss(o, oa, m, ac, qr, ix, b, a, s, c, dl, qc, ec, do, st, None)
    for k in ("o", "oa", "m", "ac", "qr", "do", "st"):
        assert loss(**{k: None}) == E_ARG, k
    for kw in (dict(c=0.0), dict(c=-1.0), dict(c=NAN), dict(dl=-0.1), dict(dl=NAN), dict(qc=INF), dict(ec=NAN),
               dict(do=p(out)), dict(st=p(out) + 64), dict(st=p(dout))):
        assert loss(**kw) == E_ARG, kw
    for kw in (dict(b=0), dict(b=2 ** 31), dict(a=0), dict(a=19), dict(s=4), dict(s=30), dict(s=(1 << 19) + 4)):
        assert loss(**kw) == E_RANGE, kw
    for k, t in (("o", out), ("oa", avg), ("m", mu), ("qr", qret), ("do", dout), ("st", stats)):
        assert loss(**{k: p(t) + 2}) == E_ALIGN, k
    torch.cuda.synchronize()
    assert torch.isnan(dout).all() and torch.isnan(stats).all()
    assert loss(c=INF, dl=INF) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(dout[:B]).all() and torch.isnan(dout[B:]).all() and torch.isnan(stats[5 * B:]).all()


# ---- the average step and the gather --------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 686000])
def test_avg_step_bit_for_bit(L, n, offset):
    """686000: a spec-0 bucket's size.  The inputs hold elements where an fma would give other bits (acer_ref.fma_differs,
    checked on the first 1027)."""
    rs = np.random.RandomState(n)
    avg, params = rs.randn(n).astype(F32), rs.randn(n).astype(F32)
    if n == 1027:
        assert ar.fma_differs(avg, params, 0.99).any()
    a, p = torch.full((n + 8,), NAN, device=DEV), torch.full((n + 8,), NAN, device=DEV)
    a[offset:offset + n], p[offset:offset + n] = _dev(avg), _dev(params)
    L.acer_avg_step(a[offset:offset + n], p[offset:offset + n], 0.99)
    np.testing.assert_array_equal(_host(a[offset:offset + n]), ar.avg_step(avg, params, 0.99))
    assert torch.isnan(a[offset + n:]).all() and torch.isnan(a[:offset]).all()
    lib = L.load()
    assert lib.arl_acer_avg_step(None, p.data_ptr(), n, 0.5, None) == E_ARG
    assert lib.arl_acer_avg_step(a.data_ptr(), p.data_ptr(), n, 1.5, None) == E_ARG
    assert lib.arl_acer_avg_step(a.data_ptr(), p.data_ptr(), n, NAN, None) == E_ARG
    assert lib.arl_acer_avg_step(a.data_ptr(), a.data_ptr() + 4, n + 1, 0.5, None) == E_ARG
    assert lib.arl_acer_avg_step(a.data_ptr(), p.data_ptr(), 0, 0.5, None) == E_RANGE
    assert lib.arl_acer_avg_step(a.data_ptr() + 2, p.data_ptr(), n, 0.5, None) == E_ALIGN


@pytest.mark.parametrize("offset", [0, 3], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("seg_bytes", [1, 15, 16, 17, 5 * 4 * 104 * 80])
def test_gather_segments_byte_exact(L, seg_bytes, offset):
    """5 * 4 * 104 * 80: one trajectory of the feature tests' observations.  Repeated, first, last and out-of-range
    indices (clamped), bases off the 16-byte grid."""
    rs = np.random.RandomState(seg_bytes)
    n_src = 7
    src = rs.randint(0, 256, size=(n_src, seg_bytes), dtype=np.uint8)
    index = np.array([0, 6, 3, 3, -1, 7, 2 ** 31 - 1, -2 ** 31, 5], np.int32)
    sbuf = torch.zeros(n_src * seg_bytes + 16, dtype=torch.uint8, device=DEV)
    dbuf = torch.full((len(index) * seg_bytes + 16,), 255, dtype=torch.uint8, device=DEV)
    s = sbuf[offset:offset + n_src * seg_bytes].view(n_src, seg_bytes)
    d = dbuf[offset:offset + len(index) * seg_bytes].view(len(index), seg_bytes)
    s.copy_(_dev(src))
    L.gather_segments(s, _dev(index), d)
    np.testing.assert_array_equal(_host(d), ar.gather(src, index))
    assert (dbuf[:offset] == 255).all() and (dbuf[offset + len(index) * seg_bytes:] == 255).all()
    lib, ix = L.load(), _dev(index)
    assert lib.arl_gather_segments(None, ix.data_ptr(), 9, 7, seg_bytes, d.data_ptr(), None) == E_ARG
    assert lib.arl_gather_segments(s.data_ptr(), ix.data_ptr(), 9, 7, seg_bytes, s.data_ptr(), None) == E_ARG
    assert lib.arl_gather_segments(s.data_ptr(), ix.data_ptr(), 0, 7, seg_bytes, d.data_ptr(), None) == E_RANGE
    assert lib.arl_gather_segments(s.data_ptr(), ix.data_ptr(), 9, 7, 0, d.data_ptr(), None) == E_RANGE
    assert lib.arl_gather_segments(s.data_ptr(), ix.data_ptr() + 2, 8, 7, seg_bytes, d.data_ptr(), None) == E_ALIGN


# ---- policy -----------------------------------------------------------------------------------------------------------

N_ACT = 6


@functools.lru_cache(maxsize=None)
def _setup():
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_acer_policy import AtariAcerPolicy
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    set_seed(3)
    policy = AtariAcerPolicy(**dict(cnn_specs[0], hidden_sizes=[64]))
    policy.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(N_ACT)), device=DEV)
    with torch.no_grad():                                       # an output layer sharp enough for rows away from 1 / A
        policy.flat_params[policy._offsets[policy._k_head]:].mul_(20.0)
        policy.update_target()
        policy.flat_target.add_(0.002 * torch.randn_like(policy.flat_target) * (policy.flat_target != 0))
    rs = np.random.RandomState(11)
    n = 40
    obs = _dev(rs.randint(0, 256, size=(n, 4, 104, 80), dtype=np.uint8))
    prob = policy.prob_value(obs)[0].clone()
    data = dict(observations=obs, actions=_dev(rs.randint(0, N_ACT, n).astype(np.uint8)),
                returns=_dev(rs.randn(n).astype(F32)), old_prob=(prob * 0.9 + 0.1 / N_ACT).contiguous())
    idx = _dev(rs.permutation(n)[:24].astype(np.int32))
    return policy, data, idx


class _Float64Net(object):
    """What autograd_ref.forward reads of a policy, with float64 host copies of the given flat bucket's views."""

    def __init__(self, policy, flat):
        views = [flat[o:o + int(np.prod(s))].view(s) for o, s in zip(policy._offsets, policy._shapes)]
        views = [v.permute(0, 3, 1, 2) if (len(s) == 4 and not (k == 0 and policy._u8)) else v
                 for k, (v, s) in enumerate(zip(views, policy._shapes))]
        self.params = [v.detach().cpu().double().contiguous().requires_grad_() for v in views]
        self._conv_geom, self._hid_geom, self._n_conv = policy._conv_geom, policy._hid_geom, policy._n_conv


def _out64(net, policy, x):
    """The float64 network's raw output rows [B][2S]."""
    import torch.nn.functional as F
    p = net.params
    for i, (nf, ci, sz, st, pad, ho, wo) in enumerate(net._conv_geom):
        x = F.relu(F.conv2d(x, p[2 * i], p[2 * i + 1], stride=st, padding=pad))
    x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    k = 2 * net._n_conv
    for _ in net._hid_geom:
        x = F.relu(F.linear(x, p[k], p[k + 1]))
        k += 2
    return F.linear(x, p[k], p[k + 1])


def _whole_step_close(got, want, scale, what):
    """The bar the V-MPO, PPG and IMPALA tests apply to a whole step's gradient (tests/test_ppg_gpu.py)."""
    err = np.abs(got - want).max()
    print("%-24s max |want| %.3g max err %.3g" % (what, np.abs(want).max(), err))
    assert np.allclose(got, want, rtol=2e-3, atol=2e-5 * scale), (what, err, scale)


def _reference_grads(policy, data, idx, c, delta, q_coeff, ent):
    """d loss / d parameters of the float64 network (autograd through its layers) from acer_ref's dout on ITS output rows."""
    sel = np.arange(data["observations"].shape[0]) if idx is None else _host(idx).astype(np.int64)
    net, avg_net = _Float64Net(policy, policy.flat_params), _Float64Net(policy, policy.flat_target)
    x = policy._scaled_f32(data["observations"], idx)[:, :policy._c_in].cpu().double()
    out = _out64(net, policy, x)
    with torch.no_grad():
        out_avg = _out64(avg_net, policy, x)
    case = dict(out=out.detach().numpy(), out_avg=out_avg.numpy(), old_prob=_host(data["old_prob"]),
                actions=_host(data["actions"]), qret=_host(data["returns"]),
                idx=None if idx is None else sel.astype(np.int32), n_act=policy.n_act, half=policy.half_stride)
    dout, stats, _ = ar.loss(case, c, delta, q_coeff, ent, exact_soft=False)
    grads = torch.autograd.grad(out, net.params, grad_outputs=torch.from_numpy(dout))
    return [g.numpy() for g in grads], stats


@pytest.mark.parametrize("gather", [True, False], ids=["idx", "rows"])
def test_acer_loss_and_grads_matches_the_float64_reference_network(gather):
    policy, data, idx = _setup()
    idx = idx if gather else None
    policy.flat_grads.fill_(NAN)
    stats = _host(policy.acer_loss_and_grads(dict(data, idx=idx), 10.0, 0.05, 0.5, 0.01))
    got = [_host(g).copy() for g in policy.grads]
    want, want_stats = _reference_grads(policy, data, idx, 10.0, 0.05, 0.5, 0.01)
    assert (want_stats[3] > 0).any(), "the projection must be active on some rows"
    for i in range(5):
        _whole_step_close(stats[i], want_stats[i], np.abs(want_stats[i]).max(), "stats row %d" % i)
    scale = max(max(np.abs(g).max() for g in want), 1e-3)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.isfinite(g).all() and np.abs(w).max() > 0, k
        _whole_step_close(g, w, scale, "param %d" % k)
    k = policy._k_head
    assert (got[k][N_ACT:32] == 0).all() and (got[k][32 + N_ACT:] == 0).all() and (got[k + 1][N_ACT:32] == 0).all()


def test_flat_q_without_truncation_is_the_head_kernels_a2c_policy_gradient(L):
    """delta = c = +inf, ent_coeff = q_coeff = 0, Q rows constant (V == Q(a): the correction term has nothing to weigh),
    mu = pi: dout's logit half is  -(1 / B) adv (onehot - pi) rho pi / (pi + 1e-6).  The fused head kernel's kind 0
    (arl_pg_head_loss, pinned by tests/test_kernels_gpu.py) is launched on the SAME logits -- hid = A, an identity policy
    block in w_head, zero bias, zero value and entropy coefficients -- and the same advantages; its gradient is
    -(1 / B) adv (onehot - pi) pi / (pi + 1e-8).  The two differ by the factors rho = pi / (pi + 1e-6) and
    (pi + 1e-8) / (pi + 1e-6), each within 1e-6 / pi of 1, by the rounding of adv to fp32 and by the head kernel's fp32
    arithmetic (64 EPS): the bar."""
    rs = np.random.RandomState(4)
    B, A, S = 65, N_ACT, 32
    out = np.zeros((B, 2 * S), F32)
    out[:, :A] = rs.randn(B, A).astype(F32)
    out[:, S:S + A] = rs.randn(B, 1).astype(F32)
    pi64, _, _ = ar.soft64(out[:, :A])
    c = dict(out=out, out_avg=out.copy(), old_prob=pi64.astype(F32), actions=rs.randint(0, A, B).astype(np.uint8),
             qret=rs.randn(B).astype(F32), idx=None, n_act=A, half=S)
    dout, stats = _loss(L, c, INF, INF, q_coeff=0.0, ent=0.0)
    adv = c["qret"].astype(np.float64) - out[:, S].astype(np.float64)
    w_head = np.zeros((A + 1, A), F32)
    w_head[:A] = np.eye(A, dtype=F32)
    d_head, dh = torch.full((B, A + 1), NAN, device=DEV), torch.zeros((B, A), device=DEV)
    dw, db, loss4 = torch.zeros((A + 1, A), device=DEV), torch.zeros(A + 1, device=DEV), torch.zeros(4, device=DEV)
    L.pg_head_loss(_dev(out[:, :A]), _dev(w_head), torch.zeros(A + 1, device=DEV), _dev(c["actions"]),
                   _dev(adv.astype(F32)), torch.zeros(B, device=DEV), _dev(c["old_prob"]), None, None,
                   torch.ones(1, device=DEV), None, A, 0, 0., 0., 0., d_head, dh, dw, db, loss4, L.pg_head_workspace(DEV))
    want = _host(d_head)[:, :A].astype(np.float64)
    assert np.isfinite(want).all() and np.abs(want).max() > 0 and (_host(d_head)[:, A] == 0).all()
    slack = 2 * ar.AC_EPS / pi64.min() + 64 * ar.EPS
    err = np.abs(dout[:, :A] - want)
    print("A2C tie: max err %.3g, bar %.3g" % (err.max(), slack * np.abs(want).max()))
    assert (err <= slack * (np.abs(want) + np.abs(adv)[:, None] / B)).all()
    assert (dout[:, A:] == 0).all() and (stats[3] == 0).all()


def test_parameter_vector_round_trip_and_served_rows():
    policy, data, _ = _setup()
    flat = policy.get_param_values()
    assert flat.size == policy.n_params and policy.param_short_names[-4:] == ["OutputW", "Outputb", "QW", "Qb"]
    before = policy.flat_params.clone()
    policy.set_param_values(flat)
    assert torch.equal(policy.flat_params, before)
    prob, out = policy.pi_q_rows(data["observations"], rows_per_pass=16, tag="t_rows")
    served = policy.prob_value(data["observations"])[0]
    assert torch.equal(prob, served) and out.shape == (40, 64) and (out[:, N_ACT:32] == 0).all()
    np.testing.assert_allclose(_host(prob), ar.soft64(_host(out)[:, :N_ACT])[0], rtol=1e-5, atol=1e-7)
    policy.set_deterministic(True)
    hot = policy.prob_value(data["observations"])[0]
    policy.set_deterministic(False)
    assert ((hot == 1).sum(dim=1) == 1).all() and torch.equal(hot.argmax(dim=1), out[:, :N_ACT].argmax(dim=1))


# ---- learner ----------------------------------------------------------------------------------------------------------

def _train(use_graph, n_itr, wrap=None, **algo_args):
    """ACER on the synthetic pong, 8 envs x horizon 5, spec-0 convs, through the sampler and the runner."""
    from accel_rl_amd.algos.pg import ACER
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_acer_policy import AtariAcerPolicy
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game="pong"), horizon=5, n_parallel=2, envs_per=2,
                            max_path_length=25, max_decorrelation_steps=0, device=DEV)
    algo = ACER(use_graph=use_graph, rows_per_pass=16, **algo_args)
    policy = AtariAcerPolicy(**dict(cnn_specs[0], hidden_sizes=[64]))
    log = dict(infos=[], samples=[], steps=[], avg=[])
    initialize, optimize = algo.initialize, algo.optimize_policy

    def watching_initialize(*a, **kw):
        initialize(*a, **kw)
        log["first"] = policy.get_param_values()
        if wrap is not None:
            wrap(algo, policy, log)

    def recording_optimize(itr, samples):
        log["samples"].append({k: v.clone() for k, v in algo._fields_of(samples).items()})
        avg_before = policy.flat_avg.clone()
        state = log["pre"](algo, policy, log["samples"][-1]) if "pre" in log else None
        out = optimize(itr, samples)
        if "post" in log:
            log["post"](algo, policy, log["samples"][-1], state)
        log["avg"].append((avg_before, policy.flat_params.clone(), policy.flat_avg.clone()))
        log["infos"].append(out[1])
        log["steps"].append(algo.optimizer._step_count.clone())
        return out
    algo.initialize, algo.optimize_policy = watching_initialize, recording_optimize
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=40 * (n_itr - 1), seed=9, log_interval_steps=40)
    runner.train()
    torch.cuda.synchronize()
    log["infos"] = [{k: _host(v).copy() for k, v in info.items()} for info in log["infos"]]
    log["steps"] = [float(s.item()) for s in log["steps"]]
    return algo, policy, log


def _same_run(a, b):
    (_, pol, log), (_, pol_e, log_e) = a, b
    assert np.array_equal(log["first"], log_e["first"])
    np.testing.assert_array_equal(pol_e.get_param_values(), pol.get_param_values())
    assert torch.equal(pol_e.flat_avg, pol.flat_avg) and len(log["infos"]) == len(log_e["infos"])
    for x, y in zip(log["infos"], log_e["infos"]):
        assert sorted(x) == sorted(y)
        for k in x:
            np.testing.assert_array_equal(x[k], y[k], err_msg=k)


def test_one_acer_update_through_the_runner_matches_the_references():
    """Six eager iterations (30 steps: past the 25-step episode limit, so an update sees `done` rows) with replay_ratio 0 and a discount, lambda, c and delta of their own (a swap would show).
    Before each update: the rows the sampler recorded as the behaviour policy are the rows the policy serves on the same
    observations, step by step, and the rows pi_q_rows computes on the whole batch, bit for bit.  After each update: opt["returns"] equals acer_ref.retrace on
    pi_q_rows' outputs under the parameters of before the update, bit for bit (process_samples, the Q views, the extra
    rows as bootstrap, dones, discount and lambda); the gradient the update left in flat_grads equals the float64 reference
    network's from those targets under the whole-step bar (the returns reach the loss; the average network is the second
    bucket)."""
    n, t, disc, lam, cc, delta = 8, 5, 0.97, 0.9, 1.5, 0.02
    seen = []

    def pre(algo, policy, s):
        obs, prob = s["observations"].view((n, t) + tuple(s["observations"].shape[1:])), s["prob"].view(n, t, -1)
        for step in range(t):
            assert torch.equal(policy.prob_value(obs[:, step].contiguous())[0], prob[:, step]), step
        assert torch.equal(policy.pi_q_rows(s["observations"], 16, tag="chk_served")[0], s["prob"])
        return dict(params=policy.flat_params.clone(), avg=policy.flat_avg.clone())

    def post(algo, policy, s, before):
        torch.cuda.synchronize()
        returns = algo._opt_buf["returns"].clone()
        got = [_host(g).copy() for g in policy.grads]
        now = policy.flat_params.clone(), policy.flat_avg.clone()
        policy.flat_params.copy_(before["params"])
        policy.flat_avg.copy_(before["avg"])
        try:
            half = policy.half_stride
            prob, out = (_host(x).copy() for x in policy.pi_q_rows(s["observations"], 16, tag="chk_rows"))
            prob_l, out_l = (_host(x).copy() for x in policy.pi_q_rows(s["extra_observations"], 16, tag="chk_last"))
            want = ar.retrace(prob, prob_l, out[:, half:], out_l[:, half:], _host(s["prob"]), _host(s["actions"]).reshape(-1),
                              _host(s["rewards"]).reshape(-1), _host(s["dones"]).reshape(-1), disc, lam, n, t)
            np.testing.assert_array_equal(_host(returns), want[0])
            data = dict(observations=s["observations"], actions=s["actions"].reshape(-1), returns=returns,
                        old_prob=s["prob"])
            ref, ref_stats = _reference_grads(policy, data, None, cc, delta, 0.5, 0.01)
        finally:
            policy.flat_params.copy_(now[0])
            policy.flat_avg.copy_(now[1])
        scale = max(max(np.abs(g).max() for g in ref), 1e-3)
        for k, (g, w) in enumerate(zip(got, ref)):
            assert np.isfinite(g).all() and np.abs(w).max() > 0, k
            _whole_step_close(g, w, scale, "update %d param %d" % (len(seen), k))
        seen.append(dict(active=int((ref_stats[3] > 0).sum()), done=int(_host(s["dones"]).astype(bool).sum()),
                         same_avg=bool(torch.equal(before["params"], before["avg"]))))

    def wrap(algo, policy, log):
        log["pre"], log["post"] = pre, post
    algo, policy, log = _train(False, 6, wrap=wrap, replay_ratio=0, discount=disc, retrace_lambda=lam, c=cc, delta=delta)
    print(seen)
    assert len(seen) == 6 and seen[0]["same_avg"] and not seen[1]["same_avg"]
    assert sum(d["done"] for d in seen) > 0 and sum(d["active"] for d in seen) > 0
    for before, params, after in log["avg"]:
        np.testing.assert_array_equal(_host(after), ar.avg_step(_host(before), _host(params), 0.99))


def test_on_policy_acer_replayed_iterations_equal_eager_ones_and_record_the_served_rows():
    """replay_ratio 0, five iterations: the third is captured, the rest replayed; the eager twin ends in the same
    parameters, average network and diagnostics, bit for bit.  The recorded behaviour rows are soft-max rows of the
    network that served them: rho's mean over the first on-policy batch is within 1e-4 of 1."""
    run = _train(True, 5, replay_ratio=0)
    algo, policy, log = run
    assert algo._graph is not None and algo._mem is None and len(log["infos"]) == 5
    final = policy.get_param_values()
    assert np.isfinite(final).all() and not np.array_equal(final, log["first"])
    assert not torch.equal(policy.flat_avg, policy.flat_params)
    for info in log["infos"]:
        assert sorted(info) == sorted(algo.opt_info_keys) and all(np.isfinite(v).all() for v in info.values())
        assert info["GradNorm"][0] > 0 and info["ReplayUpdates"][0] == 0 and info["Entropy"][0] > 0
        assert abs(info["RhoMean"][0] - 1) <= 1e-4 + 2e-5
    prob = log["samples"][0]["prob"]
    assert torch.allclose(prob.sum(dim=1), torch.ones_like(prob[:, 0]), atol=1e-5) and float(prob.min()) > 0
    assert log["steps"] == [1., 2., 3., 4., 5.]
    for before, params, after in log["avg"]:                     # one update per iteration: one average step, bit for bit
        np.testing.assert_array_equal(_host(after), ar.avg_step(_host(before), _host(params), 0.99))
    _same_run(run, _train(False, 5, replay_ratio=0))


def test_acer_with_replay_stages_stored_rows_and_its_graphs_equal_eager_runs():
    """A memory of 3 rollouts, replay from the second on, seven iterations (the slots wrap twice).  Every staged batch
    equals the stored trajectories its index row names, byte for byte; the index rows are the table's successive rows;
    the optimizer's step count advances by 1 + r per iteration; the run with both graphs equals the eager run bit for bit."""
    def wrap(algo, policy, log):
        log["staged"], replay = [], algo._device_replay

        def watched():
            replay()
            if not torch.cuda.is_current_stream_capturing():
                k = sum(1 for e in log["staged"] if e[3] == algo._calls)
                assert torch.equal(algo._idx_now.cpu(), algo._idx_host[k]), "replay update k reads the table's row k"
                log["staged"].append((algo._idx_now.clone(), {k: v.clone() for k, v in algo._staged.items()},
                                      {k: v.clone() for k, v in algo._mem.items()}, algo._calls))
        algo._device_replay = watched
    args = dict(replay_ratio=2, replay_steps=120, replay_start_steps=80, r_max=3)
    eager = _train(False, 7, wrap=wrap, **args)
    algo_e, _, log_e = eager
    rs = [int(i["ReplayUpdates"][0]) for i in log_e["infos"]]
    assert rs[0] == 0 and sum(rs) >= 3 and max(rs) <= 3 and algo_e.replay_rollouts == 3 and algo_e.replay_start == 2
    assert len(log_e["staged"]) == sum(rs) == algo_e._replays
    steps = np.cumsum([1 + r for r in rs]).astype(np.float64).tolist()
    assert log_e["steps"] == steps
    for idx, staged, mem, _ in log_e["staged"]:
        for name in staged:
            assert torch.equal(staged[name], mem[name][idx.long()]), name
    stored = algo_e._mem
    for back, slot in ((1, 6 % 3), (2, 5 % 3), (3, 4 % 3)):            # the last three rollouts, after two wraps
        for name, t in log_e["samples"][-back].items():
            assert torch.equal(stored[name][slot * 8:(slot + 1) * 8].reshape(t.shape).to(t.dtype), t), (name, slot)
    graphed = _train(True, 7, **args)
    assert graphed[0]._graph is not None and (graphed[0]._replay_graph is not None) == (sum(rs) >= 3)
    assert graphed[2]["steps"] == steps
    _same_run(graphed, eager)
