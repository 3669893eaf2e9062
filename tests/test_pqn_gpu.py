"""PQN on the GPU: the LayerNorm + rectifier kernels against float64 within the bound of DESIGN.md 22, the Q(lambda) scan
bit for bit against its float64 restatement, the regression loss within arl_dqn_loss's bound, every refusal, one whole
training step of AtariPqnPolicy against float64 autograd, and the learner replayed from its graph against an eager run.
Yardsticks: tests/pqn_ref.py."""
import numpy as np
import pytest
import torch

import pqn_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
E_ARG, E_RANGE, E_ALIGN = -1, -2, -3
EPS = 1e-5


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


# ---- LayerNorm + rectifier --------------------------------------------------------------------------------------------

LN_WIDTHS, LN_ROWS = (4, 32, 64, 100, 512, 1024), (1, 3, 64, 65, 1031)


def _ln_case(rows, width):
    """Inputs with gamma / beta away from 1 / 0, a row with one large entry (row 0) and, from three rows on, a constant
    last row (0.75: every partial sum of the row is exact, so var = 0 exactly)."""
    rs = np.random.RandomState(rows * 7919 + width)
    z = rs.randn(rows, width).astype(np.float32)
    z[0, width // 3] = 50.0
    if rows >= 3:
        z[-1] = 0.75
    gamma = (1.0 + 0.5 * rs.randn(width)).astype(np.float32)
    beta = (0.3 * rs.randn(width)).astype(np.float32)
    dy = rs.randn(rows, width).astype(np.float32)
    return z, gamma, beta, dy


def _ln_fwd(L, z, gamma, beta):
    y = torch.full(z.shape, NAN, device=DEV)
    stats = torch.full((z.shape[0], 2), NAN, device=DEV)
    L.ln_relu_fwd(_dev(z), _dev(gamma), _dev(beta), EPS, y, stats)
    return y, stats


def _ln_bwd(L, dy, y, z, stats, gamma, masked, in_place=False):
    dy = dy.clone()
    dz = dy if in_place else torch.full(tuple(dy.shape), NAN, device=DEV)
    dg, db = (torch.full((dy.shape[1],), NAN, device=DEV) for _ in range(2))
    L.ln_relu_bwd(dy, y, z, stats, gamma, masked, dz, dg, db, L.ln_bwd_workspace(DEV))
    return dz, dg, db


@pytest.mark.parametrize("width", LN_WIDTHS)
def test_ln_forward_and_backward_within_the_derived_bound(L, width):
    """Error <= the first-order bound of DESIGN.md 22 at every (rows, width); no element excluded (the float64 backward
    takes the GPU's own mask).  The constant row: finite, xhat = 0 exactly (y = max(0, beta)), and dz as float64 gives it:
    rstd (h - mean h) -- not 0 for a general dy, see test_ln_constant_row_with_constant_h_has_zero_dz.
    Largest error / bound measured on an MI355X, per width: DESIGN.md 22."""
    worst = dict(y=0., mean=0., rstd=0., dz=0., dgamma=0., dbeta=0.)
    for rows in LN_ROWS:
        z, gamma, beta, dy = _ln_case(rows, width)
        y, stats = _ln_fwd(L, z, gamma, beta)
        y64, mean64, rstd64 = pr.ln_relu_fwd64(z, gamma, beta, EPS)
        e_y, e_mean, e_rstd = pr.ln_fwd_bound(z, gamma, beta, EPS)
        yh, sh = _host(y).astype(np.float64), _host(stats).astype(np.float64)
        assert np.isfinite(yh).all() and np.isfinite(sh).all()
        ratios = dict(y=(np.abs(yh - y64) / e_y).max(), mean=(np.abs(sh[:, 0] - mean64) / e_mean).max(),
                      rstd=(np.abs(sh[:, 1] - rstd64) / e_rstd).max())
        if rows >= 3:
            np.testing.assert_array_equal(_host(y)[-1], np.maximum(beta, 0))
            assert sh[-1, 0] == 0.75 and sh[-1, 1] == np.float32(1) / np.sqrt(np.float32(0) + np.float32(EPS))
        mask = _host(y) > 0
        assert mask.any() and not mask.all()
        dz, dg, db = _ln_bwd(L, _dev(dy), y, _dev(z), stats, _dev(gamma), False)
        dz64, dg64, db64 = pr.ln_relu_bwd64(dy, mask, z, gamma, EPS)
        e_dz, e_dg, e_db = pr.ln_bwd_bound(dy, mask, z, gamma, EPS)
        ratios.update(dz=(np.abs(_host(dz) - dz64) / np.maximum(e_dz, 1e-300)).max(),
                      dgamma=(np.abs(_host(dg) - dg64) / np.maximum(e_dg, 1e-300)).max(),
                      dbeta=(np.abs(_host(db) - db64) / np.maximum(e_db, 1e-300)).max())
        print("ln width %4d rows %4d error / bound: %s" % (width, rows, " ".join("%s %.3f" % kv for kv in ratios.items())))
        for k, v in ratios.items():
            assert v <= 1.0, (k, rows, width, v)
            worst[k] = max(worst[k], v)
        dz2, dg2, db2 = _ln_bwd(L, _dev(dy), y, _dev(z), stats, _dev(gamma), False, in_place=True)
        assert torch.equal(dz, dz2) and torch.equal(dg, dg2) and torch.equal(db, db2)       # dz over dy: the same bits
    print("ln width %4d largest error / bound: %s" % (width, " ".join("%s %.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("width", [4, 64, 100, 1024])
def test_ln_constant_row_with_constant_h_has_zero_dz(L, width):
    """var = 0 and g_j gamma_j the same for every j: dz = rstd (h - mean h) = 0 exactly."""
    z = np.full((3, width), -1.25, np.float32)
    gamma, beta = np.full(width, 2.0, np.float32), np.full(width, 0.5, np.float32)
    y, stats = _ln_fwd(L, z, gamma, beta)
    assert (_host(y) == 0.5).all()
    dz, dg, db = _ln_bwd(L, torch.full((3, width), 3.0, device=DEV), y, _dev(z), stats, _dev(gamma), False)
    assert (_host(dz) == 0).all() and (_host(dg) == 0).all() and (_host(db) == 9.0).all()


@pytest.mark.parametrize("rows,width", [(65, 32), (1031, 64), (3, 100), (64, 512), (65, 1024)])
def test_ln_backward_masked_flag_is_bit_identical(L, rows, width):
    z, gamma, beta, dy = _ln_case(rows, width)
    y, stats = _ln_fwd(L, z, gamma, beta)
    dy_d = _dev(dy)
    want = _ln_bwd(L, dy_d, y, _dev(z), stats, _dev(gamma), False)
    masked = torch.where(y > 0, dy_d, torch.zeros_like(dy_d))
    assert not torch.equal(masked, dy_d)
    for flag in (True, False):                                  # the mask applied twice changes nothing either
        got = _ln_bwd(L, masked, y, _dev(z), stats, _dev(gamma), flag)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), flag


@pytest.mark.parametrize("rows,width", [(1031, 64), (1031, 100), (9000, 32)])
def test_ln_is_deterministic(L, rows, width):
    """Two launches, the same bits; (1031, 100) and (9000, 32) take 256 workgroups of two row walks each, (1031, 64) 65."""
    assert pr.ln_shape(rows, width)[2] > 1
    z, gamma, beta, dy = _ln_case(rows, width)
    runs = []
    for _ in range(2):
        y, stats = _ln_fwd(L, z, gamma, beta)
        runs.append((y, stats) + _ln_bwd(L, _dev(dy), y, _dev(z), stats, _dev(gamma), False))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert all(torch.isfinite(a).all() for a in runs[0])


# ---- Q(lambda) scan ---------------------------------------------------------------------------------------------------

def _scan_case(n_env, horizon, n_act, seed, stride=32, ties=False):
    rs = np.random.RandomState(seed)
    q = rs.randn(n_env, horizon, stride).astype(np.float32)
    q[:, :, n_act:] = 1e6                                       # the padding columns are never read
    q_last = rs.randn(n_env, stride).astype(np.float32)
    q_last[:, n_act:] = 1e6
    if ties and n_act > 1:
        q[:, :, 1] = q[:, :, :n_act].max(axis=2) + 0.5          # two equal row maxima
        q[:, :, 0] = q[:, :, 1]
        q_last[:, 0] = q_last[:, :n_act].max(axis=1)
    r = rs.randn(n_env, horizon).astype(np.float32)
    d = (rs.rand(n_env, horizon) < 0.15).astype(np.uint8)
    d[0, 0] = 1                                                 # a done at the first step,
    d[-1, -1] = 1                                               # at the last step
    if horizon >= 4:
        d[n_env // 2, 1:3] = 1                                  # and on consecutive steps
    return q, q_last, r, d


@pytest.mark.parametrize("n_env,horizon", [(1, 1), (3, 2), (64, 5), (65, 33), (256, 128)])
def test_qlambda_scan_equals_the_float64_restatement_bit_for_bit(L, n_env, horizon):
    for n_act in (1, 4, 18):
        q, q_last, r, d = _scan_case(n_env, horizon, n_act, seed=n_env + horizon + n_act, ties=(n_act == 4))
        qd, qld, rd, dd = _dev(q.reshape(-1, 32)), _dev(q_last), _dev(r.reshape(-1)), _dev(d.reshape(-1))
        for lam in (0.0, 0.65, 1.0):
            out = torch.full((n_env * horizon,), NAN, device=DEV)
            L.qlambda_scan(qd, qld, rd, dd, 0.99, lam, n_env, horizon, n_act, out)
            want = pr.qlambda_scan64(q, q_last, n_act, r, d, 0.99, lam)
            np.testing.assert_array_equal(_host(out).reshape(n_env, horizon), want, err_msg=str((n_act, lam)))


# ---- regression loss --------------------------------------------------------------------------------------------------

def _regress(L, q, idx, act, ret, n_act, clip):
    bsz = q.shape[0]
    dq = torch.full(q.shape, NAN, device=DEV)
    pack = torch.full((2, bsz), NAN, device=DEV)
    L.q_regress_loss(_dev(q), _dev(idx), _dev(act), _dev(ret), n_act, clip, dq, pack[0], pack[1])
    return _host(dq), _host(pack[0]), _host(pack[1])


@pytest.mark.parametrize("n_act,bsz", [(4, 33), (18, 300)])
@pytest.mark.parametrize("clip", [None, 1.0, 0.25])
@pytest.mark.parametrize("gather", [False, True], ids=["rows", "idx"])
def test_q_regress_loss_within_the_dqn_bound(L, n_act, bsz, clip, gather):
    rs = np.random.RandomState(n_act * bsz)
    n = bsz + 50 if gather else bsz
    q = rs.randn(bsz, 32).astype(np.float32)
    act, ret = rs.randint(0, n_act, n).astype(np.uint8), rs.randn(n).astype(np.float32)
    idx = rs.permutation(n)[:bsz].astype(np.int32) if gather else None
    dq, rows, td = _regress(L, q, idx, act, ret, n_act, clip)
    ref = pr.q_regress64(q, idx, act, ret, n_act, clip)
    ok = ref["ok"]
    assert ok.sum() >= 0.95 * bsz and np.isfinite(dq).all()
    assert (np.abs(rows - ref["rows"])[ok] <= ref["rows_tol"][ok]).all()
    assert (np.abs(td - ref["td"])[ok] <= ref["td_tol"][ok]).all()
    assert (np.abs(dq[:, :n_act] - ref["dq"]).max(axis=1)[ok] <= ref["dq_tol"][ok]).all()
    assert (dq[:, n_act:] == 0).all() and (np.count_nonzero(dq, axis=1) <= 1).all()
    emu = pr.q_regress32(q, idx, act, ret, n_act, clip)        # no transcendental, no contraction: the same bits
    for a, b in zip((dq, rows, td), emu):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("clip", [1.0, 0.25])
def test_q_regress_loss_at_the_huber_threshold(L, clip):
    """|d| == delta_clip exactly takes the squared branch (ad > c is false): compared with the fp32 emulation."""
    q = np.zeros((8, 32), np.float32)
    q[:, 2] = [0.5, -0.5, 0.25, 2.0, -2.0, 1.0, 0.0, 0.75]
    act = np.full(8, 2, np.uint8)
    ret = (q[:, 2] + np.float32(clip) * np.array([1, -1, 1, -1, 1, -1, 1, -1], np.float32)).astype(np.float32)
    assert (np.abs(ret - q[:, 2]) == np.float32(clip)).all()
    dq, rows, td = _regress(L, q, None, act, ret, 4, clip)
    for a, b in zip((dq, rows, td), pr.q_regress32(q, None, act, ret, 4, clip)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(rows, np.float32(0.5) * np.float32(clip) ** 2 / np.float32(8))
    np.testing.assert_array_equal(td, np.float32(clip))


# ---- refusals ---------------------------------------------------------------------------------------------------------

def test_ln_refusals_launch_nothing(L):
    lib = L.load()
    rows, width = 5, 8
    z, y, dy, dz = (torch.full((rows + 1, width), NAN, device=DEV) for _ in range(4))
    stats = torch.full((rows + 1, 2), NAN, device=DEV)
    gamma, beta, dg, db = (torch.full((width + 4,), NAN, device=DEV) for _ in range(4))
    ws = L.ln_bwd_workspace(DEV)
    p = lambda t: t.data_ptr()                                  # noqa: E731

    def fwd(z_=p(z), g=p(gamma), b=p(beta), y_=p(y), s=p(stats), r=rows, w=width, eps=1e-5):
        return lib.arl_ln_relu_fwd(z_, g, b, r, w, eps, y_, s, None)

    def bwd(dy_=p(dy), y_=p(y), z_=p(z), s=p(stats), g=p(gamma), dz_=p(dz), dg_=p(dg), db_=p(db), ws_=p(ws), r=rows,
            w=width, m=0):
        return lib.arl_ln_relu_bwd(dy_, y_, z_, s, g, r, w, m, dz_, dg_, db_, ws_, None, None)

    for kw in (dict(z_=None), dict(g=None), dict(b=None), dict(y_=None), dict(s=None)):
        assert fwd(**kw) == E_ARG and b"null" in lib.arl_last_error(), kw
    for kw in (dict(dy_=None), dict(y_=None), dict(z_=None), dict(s=None), dict(g=None), dict(dz_=None), dict(dg_=None),
               dict(db_=None), dict(ws_=None)):
        assert bwd(**kw) == E_ARG and b"null" in lib.arl_last_error(), kw
    for kw in (dict(r=0), dict(r=-1), dict(r=2 ** 31), dict(w=0), dict(w=2), dict(w=6), dict(w=1028), dict(w=1032)):
        assert fwd(**kw) == E_RANGE and bwd(**kw) == E_RANGE, kw
    for eps in (0.0, -1e-5, NAN, float("inf")):
        assert fwd(eps=eps) == E_ARG, eps
    assert fwd(y_=p(z)) == E_ARG                                # z is kept: no in-place forward
    assert bwd(m=2) == E_ARG and bwd(m=-1) == E_ARG
    for kw in (dict(z_=p(z) + 4), dict(g=p(gamma) + 4), dict(b=p(beta) + 8), dict(y_=p(y) + 4), dict(s=p(stats) + 8)):
        assert fwd(**kw) == E_ALIGN, kw
    for kw in (dict(dy_=p(dy) + 4), dict(y_=p(y) + 4), dict(z_=p(z) + 8), dict(s=p(stats) + 8), dict(g=p(gamma) + 4),
               dict(dz_=p(dz) + 4), dict(dg_=p(dg) + 4), dict(db_=p(db) + 12), dict(ws_=p(ws) + 4)):
        assert bwd(**kw) == E_ALIGN, kw
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in (y, stats, dz, dg, db))
    z.normal_(), dy.normal_(), gamma.fill_(1.5), beta.fill_(0.1)
    assert fwd() == 0 and bwd() == 0 and bwd(m=1, dz_=p(dy)) == 0                           # accepted, it runs
    torch.cuda.synchronize()
    assert torch.isfinite(y[:rows]).all() and torch.isfinite(dz[:rows]).all() and torch.isfinite(dg[:width]).all()
    assert torch.isnan(y[rows:]).all() and torch.isnan(dz[rows:]).all() and torch.isnan(dg[width:]).all()


def test_scan_and_regress_refusals_launch_nothing(L):
    lib = L.load()
    n_env, horizon, stride = 3, 4, 8
    q = torch.zeros(n_env * horizon + 1, stride, device=DEV)
    q_last, r = torch.zeros(n_env + 1, stride, device=DEV), torch.zeros(n_env * horizon, device=DEV)
    d = torch.zeros(n_env * horizon, dtype=torch.uint8, device=DEV)
    out = torch.full((n_env * horizon,), NAN, device=DEV)
    p = lambda t: t.data_ptr()                                  # noqa: E731

    def scan(q_=p(q), ql=p(q_last), r_=p(r), d_=p(d), o=p(out), g=0.99, lam=0.65, n=n_env, t=horizon, a=6, s=stride):
        return lib.arl_qlambda_scan(q_, ql, r_, d_, g, lam, n, t, a, s, o, None)

    for kw in (dict(q_=None), dict(ql=None), dict(r_=None), dict(d_=None), dict(o=None)):
        assert scan(**kw) == E_ARG and b"null" in lib.arl_last_error(), kw
    for kw in (dict(n=0), dict(n=2 ** 31), dict(t=0), dict(t=4097), dict(a=0), dict(a=65, s=68), dict(a=6, s=4),
               dict(a=5, s=6)):
        assert scan(**kw) == E_RANGE, kw
    for kw in (dict(g=-0.01), dict(g=1.01), dict(g=NAN), dict(g=float("inf")), dict(lam=-0.01), dict(lam=1.01),
               dict(lam=NAN), dict(o=p(r)), dict(o=p(q) + 16), dict(o=p(q_last)), dict(r_=p(out) + 8)):
        assert scan(**kw) == E_ARG, kw
    assert scan(q_=p(q) + 4) == E_ALIGN and scan(ql=p(q_last) + 8) == E_ALIGN
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and (q == 0).all() and (r == 0).all()
    assert scan(g=1.0, lam=1.0) == 0 and scan(g=0.0, lam=0.0, a=8) == 0                    # at the limits it runs
    torch.cuda.synchronize()
    assert (out == 0).all()

    batch = 4
    qq, act, ret = torch.zeros(batch, stride, device=DEV), torch.zeros(batch, dtype=torch.uint8, device=DEV), \
        torch.zeros(batch, device=DEV)
    dq, rows, td = (torch.full(s, NAN, device=DEV) for s in ((batch, stride), (batch,), (batch,)))

    def reg(q_=p(qq), a_=p(act), r_=p(ret), dq_=p(dq), ro=p(rows), t_=p(td), b=batch, a=6, s=stride):
        return lib.arl_q_regress_loss(q_, None, a_, r_, b, a, s, 1.0, dq_, ro, t_, None)

    for kw in (dict(q_=None), dict(a_=None), dict(r_=None), dict(dq_=None), dict(ro=None), dict(t_=None)):
        assert reg(**kw) == E_ARG and b"null" in lib.arl_last_error(), kw
    for kw in (dict(b=0), dict(b=2 ** 31), dict(a=0), dict(a=256, s=256), dict(s=10), dict(a=6, s=4)):       # as arl_dqn_loss
        assert reg(**kw) == E_RANGE, kw
    torch.cuda.synchronize()
    assert all(torch.isnan(x).all() for x in (dq, rows, td))
    act.fill_(200)                                              # an action past the row is read as the last one
    assert reg() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(dq).all() and (dq[:, 6:] == 0).all() and torch.isfinite(rows).all()


# ---- policy -----------------------------------------------------------------------------------------------------------

def _make_policy(n_act, seed=5):
    """Spec-0 convs, one hidden layer of 64; parameters perturbed, gamma / beta away from 1 / 0."""
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_pqn_policy import AtariPqnPolicy
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    set_seed(seed)
    spec = dict(cnn_specs[0], hidden_sizes=[64])
    policy = AtariPqnPolicy(epsilon=0.3, **spec)
    policy.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(n_act)), device=DEV)
    rs = np.random.RandomState(3)
    flat = policy.get_param_values()
    n_ln = 2 * (16 + 32 + 64)
    flat = flat + (rs.randn(flat.size) * 0.01).astype(np.float32)
    flat[-n_ln:] += (rs.randn(n_ln) * 0.2).astype(np.float32)
    policy.set_param_values(flat)
    return policy, spec


def test_parameters_round_trip_and_lead_with_the_conv_stack():
    policy, _ = _make_policy(6)
    names = policy.param_short_names
    assert names[-6:] == ["Conv0LNg", "Conv0LNb", "Conv1LNg", "Conv1LNb", "FC0LNg", "FC0LNb"]
    flat = policy.get_param_values()
    assert flat.size == policy.n_params == sum(int(np.prod(s)) for s in policy._ref_shapes)
    rs = np.random.RandomState(1)
    new = rs.randn(flat.size).astype(np.float32)
    policy.set_param_values(new)
    np.testing.assert_array_equal(policy.get_param_values(), new)
    # the conv layers' gamma / beta sit before grad_split_offset, the dense layer's behind the output layer
    k_ln = policy._k_ln
    assert all(policy._offsets[k] < policy.grad_split_offset for k in range(k_ln, k_ln + 4))
    assert all(policy._offsets[k] > policy._offsets[policy._k_head] for k in (k_ln + 4, k_ln + 5))
    assert policy.grad_split_offset == policy._offsets[4] and sorted(policy._offsets) == sorted(set(policy._offsets))
    from accel_rl_amd.policies.dqn.atari_pqn_policy import AtariPqnPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    init = AtariPqnPolicy(**dict(cnn_specs[0], hidden_sizes=[64]))
    init.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(6)), device=DEV)
    tail = init.get_param_values()[-2 * (16 + 32 + 64):]
    want = np.concatenate([np.r_[np.ones(w), np.zeros(w)] for w in (16, 32, 64)]).astype(np.float32)
    np.testing.assert_array_equal(tail, want)                  # gamma = 1, beta = 0 at initialisation
    assert not init.serve_supported()


@pytest.mark.parametrize("n_act", [4, 18])
@pytest.mark.parametrize("clip,gather", [(None, True), (0.05, False)], ids=["squared-idx", "huber-rows"])
def test_training_step_matches_autograd_through_plain_torch(n_act, clip, gather):
    """pqn_loss_and_grads at batch 8 against float64 autograd of tests/pqn_ref.py:ref_q on the reference layout; the bars
    of the other policies' whole-step tests (rtol 2e-3, atol 2e-5 max |grad|): the contractions are the same kernels."""
    batch = 8
    policy, spec = _make_policy(n_act)
    rs = np.random.RandomState(11)
    n = 13 if gather else batch
    obs = _dev(rs.randint(0, 256, size=(n, 4, 104, 80), dtype=np.uint8))
    act = _dev(rs.randint(0, n_act, size=n).astype(np.uint8))
    ret = _dev((rs.randn(n) * 0.5).astype(np.float32))
    idx = _dev(rs.permutation(n)[:batch].astype(np.int32)) if gather else None
    policy.flat_grads.fill_(NAN)
    rows, td = policy.pqn_loss_and_grads(obs, idx, act, ret, clip)
    assert rows.data_ptr() + 4 * batch == td.data_ptr()
    got = policy.bucket_to_reference(policy.flat_grads)
    rp = pr.ref_params(policy, policy.flat_params)
    src = torch.arange(batch) if idx is None else idx.cpu().long()
    x = obs.cpu()[src].double() * float(np.float32(1. / 255))
    q = pr.ref_q(rp, spec, x, policy._ln_eps)
    q_gpu = policy.q(obs)[src.to(DEV)] if gather else policy.q(obs)
    assert torch.allclose(q_gpu.cpu().double(), q.detach(), rtol=2e-3, atol=2e-5 * float(q.detach().abs().max()))
    d = ret.cpu().double()[src] - q[torch.arange(batch), act.cpu().long()[src]]
    ad = d.abs()
    loss_rows = 0.5 * d * d if clip is None else torch.where(ad <= clip, 0.5 * d * d, clip * (ad - clip / 2))
    if clip is not None:
        assert (ad < clip).any() and (ad > clip).any()
    want_rows = loss_rows / batch
    want = np.concatenate([g.detach().numpy().reshape(-1) for g in torch.autograd.grad(want_rows.sum(), rp)])
    print("loss %.6g vs %.6g; max grad err %.3g of max |grad| %.3g" % (rows.sum().item(), want_rows.sum().item(),
                                                                       np.abs(got - want).max(), np.abs(want).max()))
    assert np.isfinite(got).all() and np.abs(want).max() > 0
    n_ln = 2 * (16 + 32 + 64)
    assert np.abs(want[-n_ln:]).max() > 0                       # gamma / beta take part
    assert np.allclose(_host(rows), want_rows.detach().numpy(), rtol=2e-3, atol=0)
    assert np.allclose(_host(td), (ad if clip is None else ad.clamp(max=clip)).detach().numpy(), rtol=2e-3, atol=1e-6)
    assert np.allclose(got, want, rtol=2e-3, atol=2e-5 * max(np.abs(want).max(), 1e-3)), np.abs(got - want).max()


# ---- learner ----------------------------------------------------------------------------------------------------------

def _train_pqn(use_graph):
    from accel_rl_amd.algos.dqn.pqn import PQN
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_pqn_policy import AtariPqnPolicy
    from accel_rl_amd.runners.accel_rl import AccelRLEval
    from accel_rl_amd.sampler.gpu_sampler_with_eval import GpuVecEvalSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecEvalSampler(eval_steps=8 * 20, eval_envs_per=1, EnvCls=SynthAtariEnv, env_args=dict(game="pong"),
                                horizon=8, n_parallel=4, envs_per=2, max_path_length=25, max_decorrelation_steps=0,
                                device=DEV)
    algo = PQN(optimizer_args=dict(minibatch_size=32, epochs=2), eps_greedy_args=dict(anneal_steps=128 * 3),
               rows_per_pass=48, use_graph=use_graph)
    policy = AtariPqnPolicy(**dict(cnn_specs[0], hidden_sizes=[64]))
    log = dict(infos=[], eps=[], evals=0)
    initialize, optimize, evaluate = policy.initialize, algo.optimize_policy, sampler.evaluate_policy

    def recording_initialize(*a, **kw):
        initialize(*a, **kw)
        log["first"] = policy.get_param_values()

    def recording_optimize(itr, samples):
        out = optimize(itr, samples)
        log["infos"].append(out[1])
        log["eps"].append(policy.get_epsilon())
        return out

    def recording_evaluate(itr):
        log["evals"] += 1
        log["eval_eps"] = policy.get_epsilon()
        return evaluate(itr)
    policy.initialize, algo.optimize_policy, sampler.evaluate_policy = recording_initialize, recording_optimize, \
        recording_evaluate
    runner = AccelRLEval(algo=algo, policy=policy, sampler=sampler, n_steps=128 * 4, seed=9, eval_interval_steps=128 * 2)
    runner.train()
    torch.cuda.synchronize()
    log["infos"] = [{k: _host(v).copy() for k, v in info.items()} for info in log["infos"]]
    return algo, policy, log


def test_pqn_trains_and_replayed_iterations_equal_eager_ones():
    """PQN on the synthetic pong, 16 envs x horizon 8, 2 epochs of 4 minibatches of 32, five iterations: the third is
    captured, the rest replayed; the same seeded run made eagerly ends in the same parameters and returned the same
    diagnostics, bit for bit.  The rollout's forward runs in passes of 48 rows (128 = 48 + 48 + 32)."""
    algo, policy, log = _train_pqn(True)
    assert algo._graph is not None and algo.optimizer._n_minibatches == 8 and len(log["infos"]) == 5
    final = policy.get_param_values()
    assert np.isfinite(final).all() and not np.array_equal(final, log["first"])
    for info in log["infos"]:
        assert sorted(info) == ["GradNorm", "Loss", "TdAbs"]
        assert all(v.shape == (8,) and np.isfinite(v).all() for v in info.values())
        assert (info["Loss"] > 0).all() and (info["TdAbs"] > 0).all() and (info["GradNorm"] > 0).all()
    want_eps = [min(1, k / 3) * 0.001 + (1 - min(1, k / 3)) * 1.0 for k in range(5)]
    assert log["eps"] == want_eps
    assert log["evals"] >= 2 and log["eval_eps"] == 0.0        # greedy evaluation, the schedule's value restored after it
    algo_e, policy_e, log_e = _train_pqn(False)
    assert algo_e._graph is None and np.array_equal(log["first"], log_e["first"])
    np.testing.assert_array_equal(policy_e.get_param_values(), final)
    for a, b in zip(log["infos"], log_e["infos"]):
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
