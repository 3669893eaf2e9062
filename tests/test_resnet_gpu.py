"""The IMPALA residual network on the GPU: the pooling and residual-sum kernels bit for bit against their NumPy
restatements, their determinism and refusals, the three forward paths of AtariResnetPolicy against one another, one whole
training step against float64 autograd, and A2C / IMPALA replayed from their graphs against eager runs.
Yardsticks: tests/resnet_ref.py."""
import functools

import numpy as np
import pytest
import torch

import resnet_ref as rr
from test_resnet_host import POOL_SHAPES, pool_input

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
E_ARG, E_RANGE, E_ALIGN = -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


# ---- the kernels --------------------------------------------------------------------------------------------------------

def _pool(L, z, with_relu=True, with_arg=True):
    b, h, w, c = z.shape
    shape = (b,) + rr.out_hw(h, w) + (c,)
    y = torch.full(shape, NAN, device=DEV)
    y_relu = torch.full(shape, NAN, device=DEV) if with_relu else None
    arg = torch.full(shape, 255, dtype=torch.uint8, device=DEV) if with_arg else None
    L.maxpool3s2_fwd(_dev(z), y, y_relu, arg)
    return y, y_relu, arg


def _pool_bwd(L, dy, arg, h, w):
    dz = torch.full((dy.shape[0], h, w, dy.shape[3]), NAN, device=DEV)
    L.maxpool3s2_bwd(_dev(dy), _dev(arg), dz)
    return dz


@pytest.mark.parametrize("ties", [True, False], ids=["ties", "floats"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_forward_and_backward_equal_the_restatement_bit_for_bit(L, shape, ties):
    b, h, w, c = shape
    z = pool_input(shape, ties)
    dy = pool_input((b,) + rr.out_hw(h, w) + (c,), ties, seed=1)
    want_y, want_relu, want_arg = rr.maxpool_fwd32(z)
    y, y_relu, arg = _pool(L, z)
    np.testing.assert_array_equal(_host(y), want_y)
    np.testing.assert_array_equal(_host(y_relu), want_relu)
    assert not np.signbit(_host(y_relu)).any()
    np.testing.assert_array_equal(_host(arg), want_arg)
    y_only, none_relu, none_arg = _pool(L, z, with_relu=False, with_arg=False)                 # the optional outputs left out
    assert none_relu is None and none_arg is None and torch.equal(y_only, y)
    assert torch.equal(_pool(L, z, with_arg=False)[1], y_relu) and torch.equal(_pool(L, z, with_relu=False)[2], arg)
    dz = _pool_bwd(L, dy, want_arg, h, w)
    want_dz = rr.maxpool_bwd32(dy, want_arg, h, w)
    np.testing.assert_array_equal(_host(dz), want_dz)
    np.testing.assert_array_equal(np.signbit(_host(dz)), np.signbit(want_dz))
    # determinism: a second run of each, the same bits
    again = _pool(L, z)
    assert all(torch.equal(a, b_) for a, b_ in zip(again, (y, y_relu, arg)))
    assert torch.equal(_pool_bwd(L, dy, want_arg, h, w), dz)


@pytest.mark.parametrize("n", [4, 8, 260, 400012])
def test_add_relu_equals_the_restatement_bit_for_bit(L, n):
    rs = np.random.RandomState(n)
    a, b = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    b[::7] = -a[::7]                                            # exact zeros among the sums
    want_s, want_r = rr.add_relu32(a, b)
    assert (want_s == 0).any() and (want_s > 0).any() and (want_s < 0).any()
    for alias in (None, "a", "b"):
        for with_relu in (True, False):
            ad, bd = _dev(a), _dev(b)
            out = dict(a=ad, b=bd).get(alias)
            if out is None:
                out = torch.full((n,), NAN, device=DEV)
            relu = torch.full((n,), NAN, device=DEV) if with_relu else None
            L.add_relu(ad, bd, out, relu)
            np.testing.assert_array_equal(_host(out), want_s, err_msg=str((alias, with_relu)))
            if with_relu:
                np.testing.assert_array_equal(_host(relu), want_r)
                assert not np.signbit(_host(relu)).any()
            if alias != "a":
                np.testing.assert_array_equal(_host(ad), a)     # an input that is not the output is left alone
            if alias != "b":
                np.testing.assert_array_equal(_host(bd), b)
    ad, bd = _dev(a), _dev(b)
    runs = []
    for _ in range(2):
        out, relu = torch.full((n,), NAN, device=DEV), torch.full((n,), NAN, device=DEV)
        L.add_relu(ad, bd, out, relu)
        runs.append((out, relu))
    assert all(torch.equal(x, y) for x, y in zip(*runs))


@pytest.mark.parametrize("n,c,h,w", [(1, 1, 1, 1), (5, 4, 9, 7), (4, 3, 5, 3), (3, 6, 2, 9), (2, 4, 104, 80)])
def test_gather_of_any_plane_equals_the_restatement_bit_for_bit(L, n, c, h, w):
    rs = np.random.RandomState(n + c + h + w)
    obs = rs.randint(0, 256, size=(n, c, h, w), dtype=np.uint8)
    scale = np.float32(1. / 255)
    cp = (c + 3) // 4 * 4
    for idx in (None, rs.randint(0, n, size=n + 2).astype(np.int32)):
        rows = np.arange(n) if idx is None else idx
        want = np.zeros((len(rows), h, w, cp), np.float32)
        want[..., :c] = obs[rows].transpose(0, 2, 3, 1).astype(np.float32) * scale
        out = torch.full((len(rows), h, w, cp), NAN, device=DEV)
        L.gather_scale_obs_nhwc_any(_dev(obs), _dev(idx), out, float(scale))
        np.testing.assert_array_equal(_host(out), want)
        assert not np.signbit(_host(out)).any()
    if c == 4 and (h * w) % 16 == 0:                            # where both apply, the vectorised gather gives the same bits
        fast = torch.full((n, h, w, 4), NAN, device=DEV)
        L.gather_scale_obs_nhwc(_dev(obs), None, fast, float(scale))
        slow = torch.full((n, h, w, 4), NAN, device=DEV)
        L.gather_scale_obs_nhwc_any(_dev(obs), None, slow, float(scale))
        assert torch.equal(fast, slow)


def test_refusals_launch_nothing(L):
    lib = L.load()
    b, h, w, c = 2, 5, 4, 8
    oh, ow = rr.out_hw(h, w)
    z, dz = torch.zeros(b * h * w * c + 8, device=DEV), torch.full((b * h * w * c + 8,), NAN, device=DEV)
    y, y_relu, dy = (torch.full((b * oh * ow * c + 8,), NAN, device=DEV) for _ in range(3))
    arg = torch.full((b * oh * ow * c + 8,), 255, dtype=torch.uint8, device=DEV)
    p = lambda t: t.data_ptr()                                  # noqa: E731

    def fwd(z_=p(z), y_=p(y), r_=p(y_relu), a_=p(arg), b_=b, h_=h, w_=w, c_=c):
        return lib.arl_maxpool3s2_fwd(z_, b_, h_, w_, c_, y_, r_, a_, None)

    def bwd(dy_=p(dy), a_=p(arg), dz_=p(dz), b_=b, h_=h, w_=w, c_=c):
        return lib.arl_maxpool3s2_bwd(dy_, a_, b_, h_, w_, c_, dz_, None)

    for kw in (dict(z_=None), dict(y_=None)):
        assert fwd(**kw) == E_ARG and b"null" in lib.arl_last_error(), kw
    for kw in (dict(dy_=None), dict(a_=None), dict(dz_=None)):
        assert bwd(**kw) == E_ARG and b"null" in lib.arl_last_error(), kw
    for kw in (dict(c_=0), dict(c_=6), dict(c_=1028), dict(c_=-4), dict(h_=0), dict(w_=0), dict(h_=-1), dict(b_=0),
               dict(b_=2 ** 20 + 1), dict(h_=2 ** 16 + 1)):
        assert fwd(**kw) == E_RANGE and bwd(**kw) == E_RANGE, kw
    assert fwd(y_=p(z)) == E_ARG and fwd(r_=p(z)) == E_ARG and fwd(r_=p(y)) == E_ARG and bwd(dz_=p(dy)) == E_ARG
    for kw in (dict(z_=p(z) + 4), dict(y_=p(y) + 8), dict(r_=p(y_relu) + 4), dict(a_=p(arg) + 2)):
        assert fwd(**kw) == E_ALIGN, kw
    for kw in (dict(dy_=p(dy) + 4), dict(a_=p(arg) + 1), dict(dz_=p(dz) + 12)):
        assert bwd(**kw) == E_ALIGN, kw

    n = 16
    a_t, b_t = torch.zeros(n + 4, device=DEV), torch.zeros(n + 4, device=DEV)
    s_t, r_t = torch.full((n + 4,), NAN, device=DEV), torch.full((n + 4,), NAN, device=DEV)

    def add(a_=p(a_t), b_=p(b_t), s_=p(s_t), r_=p(r_t), n_=n):
        return lib.arl_add_relu(a_, b_, n_, s_, r_, None)

    for kw in (dict(a_=None), dict(b_=None), dict(s_=None)):
        assert add(**kw) == E_ARG and b"null" in lib.arl_last_error(), kw
    for kw in (dict(n_=6), dict(n_=0), dict(n_=-4), dict(n_=2), dict(n_=2 ** 40 + 4)):
        assert add(**kw) == E_RANGE, kw
    assert add(r_=p(a_t)) == E_ARG and add(r_=p(b_t)) == E_ARG and add(r_=p(s_t)) == E_ARG
    for kw in (dict(a_=p(a_t) + 4), dict(b_=p(b_t) + 8), dict(s_=p(s_t) + 4), dict(r_=p(r_t) + 12)):
        assert add(**kw) == E_ALIGN, kw
    obs = torch.zeros((3, 3, 5, 3), dtype=torch.uint8, device=DEV)
    x_t = torch.full((3 * 15 * 4 + 4,), NAN, device=DEV)
    rows_t = torch.zeros(4, dtype=torch.int32, device=DEV)

    def gather(o_=p(obs), i_=None, x_=p(x_t), b_=3, c_=3, pl=15):
        return lib.arl_gather_scale_obs_nhwc_any(o_, i_, b_, c_, pl, 1.0, x_, None)

    assert gather(o_=None) == E_ARG and gather(x_=None) == E_ARG
    for kw in (dict(b_=0), dict(b_=2 ** 24 + 1), dict(c_=0), dict(c_=1025), dict(pl=0), dict(pl=2 ** 24 + 1)):
        assert gather(**kw) == E_RANGE, kw
    assert gather(x_=p(x_t) + 4) == E_ALIGN and gather(i_=p(rows_t) + 2) == E_ALIGN
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in (y, y_relu, dz, s_t, r_t, x_t)) and (arg == 255).all()
    assert gather() == 0 and gather(i_=p(rows_t)) == 0
    torch.cuda.synchronize()
    assert (x_t[:180] == 0).all() and torch.isnan(x_t[180:]).all()
    dy.fill_(1.0)
    assert fwd() == 0 and fwd(r_=None, a_=None) == 0 and bwd() == 0 and add() == 0 and add(r_=None, s_=p(a_t)) == 0
    torch.cuda.synchronize()                                    # accepted calls run, and stay inside their arrays
    n_out, n_in = b * oh * ow * c, b * h * w * c
    assert (y[:n_out] == 0).all() and torch.isnan(y[n_out:]).all() and torch.isnan(y_relu[n_out:]).all()
    assert torch.isfinite(dz[:n_in]).all() and torch.isnan(dz[n_in:]).all()
    assert (arg[:n_out] <= 8).all() and (arg[n_out:] == 255).all()
    assert (s_t[:n] == 0).all() and torch.isnan(s_t[n:]).all() and torch.isnan(r_t[n:]).all()


# ---- policy -------------------------------------------------------------------------------------------------------------

CASES = dict(
    # the paper's channel counts: the <= 16-column fp32 arm and the 17 .. 64-column split arms both run
    paper=dict(obs=(4, 12, 8), batch=2, channels=(16, 32, 32), blocks=2, hidden=(64,), n_act=6, seed=3),
    # odd images, channel counts off the tiles: the generic arms (bias gradients by the all-ones contraction)
    odd=dict(obs=(4, 9, 7), batch=3, channels=(4, 20, 8), blocks=1, hidden=(64,), n_act=6, seed=5))


def case_arrays(name):
    """Everything random of a whole-step case, from its seed alone (host arrays): parameters of realistic scale in the
    reference layout (Glorot-uniform convs, unit-variance-preserving dense layers, small non-zero biases), u8 observations
    (three rows more than the batch, for the gathered variant) and the minibatch's targets."""
    from accel_rl_amd.policies.atari_resnet_policy import AtariResnetPolicy
    cfg = CASES[name]
    rs = np.random.RandomState(1000 + cfg["seed"])
    policy = AtariResnetPolicy(channels=cfg["channels"], blocks_per_section=cfg["blocks"], hidden_sizes=cfg["hidden"])
    flat = []
    for pname, shape in policy.reference_layout(cfg["obs"], cfg["n_act"]):
        if len(shape) == 4:
            a = np.sqrt(6. / ((shape[0] + shape[1]) * 9))
            t = rs.uniform(-a, a, size=shape)
        elif len(shape) == 2:
            t = rs.randn(*shape) / np.sqrt(shape[0])
        else:
            t = 0.05 * rs.randn(*shape)
        flat.append(t.astype(np.float32).reshape(-1))
    n = cfg["batch"] + 3
    return dict(flat=np.concatenate(flat), obs=rs.randint(0, 256, size=(n,) + cfg["obs"], dtype=np.uint8),
                actions=rs.randint(0, cfg["n_act"], n).astype(np.uint8), advantages=rs.randn(n).astype(np.float32),
                returns=rs.randn(n).astype(np.float32), idx=rs.permutation(n)[:cfg["batch"]].astype(np.int32),
                old_noise=rs.rand(n, cfg["n_act"]).astype(np.float32))


CLIP, V_COEFF, ENT_COEFF = 0.2, 0.5, 0.01


@functools.lru_cache(maxsize=None)
def reference_step(name, kind, gather, dtype=np.float64):
    """The whole step in plain PyTorch on the CPU (float64): dict(prob, value, old_prob, losses (3), grads [per reference
    tensor], margin).  Computed once per variant and shared."""
    cfg, arr = CASES[name], case_arrays(name)
    rp, pos = [], 0
    policy_shapes = [s for _, s in _layout(name)]
    for shape in policy_shapes:
        m = int(np.prod(shape))
        rp.append(torch.from_numpy(arr["flat"][pos:pos + m].reshape(shape).astype(dtype)).requires_grad_())
        pos += m
    rows = arr["idx"].astype(np.int64) if gather else np.arange(cfg["batch"])
    x = torch.from_numpy(arr["obs"][rows].astype(dtype)) * dtype(np.float32(1. / 255))
    prob, value, taps = rr.ref_net(rp, cfg["channels"], cfg["blocks"], len(cfg["hidden"]), cfg["n_act"], x)
    # the behaviour policy of the PPO variant: near the current one, so that ratios fall on both sides of the clip
    old = 0.7 * prob.detach().numpy().astype(np.float32) + 0.3 * arr["old_noise"][rows] / arr["old_noise"][rows].sum(1, keepdims=True)
    old_full = np.full((arr["obs"].shape[0], cfg["n_act"]), 1.0 / cfg["n_act"], np.float32)
    old_full[rows] = old
    pick = lambda a: torch.from_numpy(a[rows].astype(dtype))                                   # noqa: E731
    losses = rr.pg_loss(prob, value, kind, torch.from_numpy(arr["actions"][rows].astype(np.int64)), pick(arr["advantages"]),
                        pick(arr["returns"]), torch.from_numpy(old.astype(dtype)), CLIP, V_COEFF, ENT_COEFF)
    grads = torch.autograd.grad(sum(losses), rp)
    return dict(prob=prob.detach().numpy(), value=value.detach().numpy(), old_prob=old_full,
                losses=np.array([float(t.detach()) for t in losses]), grads=[g.numpy() for g in grads],
                margin=rr.branch_margin(taps), names=[n for n, _ in _layout(name)])


def _layout(name):
    from accel_rl_amd.policies.atari_resnet_policy import AtariResnetPolicy
    cfg = CASES[name]
    return AtariResnetPolicy(channels=cfg["channels"], blocks_per_section=cfg["blocks"],
                             hidden_sizes=cfg["hidden"]).reference_layout(cfg["obs"], cfg["n_act"])


def _make_policy(name):
    from accel_rl_amd.policies.atari_resnet_policy import AtariResnetPolicy
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    cfg = CASES[name]
    set_seed(5)
    policy = AtariResnetPolicy(channels=cfg["channels"], blocks_per_section=cfg["blocks"], hidden_sizes=cfg["hidden"])
    policy.initialize(EnvSpec(UintBox(cfg["obs"]), Discrete(cfg["n_act"])), device=DEV)
    return policy


def test_parameters_round_trip_and_lead_with_the_conv_stack():
    policy = _make_policy("paper")
    assert policy.param_short_names == [n for n, _ in _layout("paper")]
    first = policy.get_param_values()
    assert first.size == policy.n_params == sum(int(np.prod(s)) for _, s in _layout("paper"))
    pos = 0
    for name, shape in _layout("paper"):
        t = first[pos:pos + int(np.prod(shape))]
        pos += t.size
        if name.endswith("b"):
            assert (t == 0).all(), name                        # biases start at 0
        elif len(shape) == 4:
            a = np.sqrt(6. / ((shape[0] + shape[1]) * 9))
            assert np.abs(t).max() <= a and np.abs(t).max() > 0.5 * a, name     # Glorot-uniform
    flat = case_arrays("paper")["flat"]
    policy.set_param_values(flat)
    np.testing.assert_array_equal(policy.get_param_values(), flat)
    np.testing.assert_array_equal(policy.bucket_to_reference(policy.flat_params), flat)
    n_conv2 = 2 * 15
    assert policy.grad_split_offset == policy._offsets[n_conv2]
    assert all(policy._offsets[k] < policy.grad_split_offset for k in range(n_conv2))
    assert all(policy._offsets[k] >= policy.grad_split_offset for k in range(n_conv2, len(policy._offsets)))
    assert not policy.serve_supported() and not policy._u8 and not policy._wt


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_three_forward_paths_give_the_same_bits(name):
    """prob_value, prob_value_rows in passes of 3 over 7 rows and the training forward (the probabilities of the rows a
    gathered minibatch picks, read back through an A2C loss's gradient-free outputs) on the same rows."""
    cfg = CASES[name]
    policy = _make_policy(name)
    policy.set_param_values(case_arrays(name)["flat"])
    rs = np.random.RandomState(4)
    obs = _dev(rs.randint(0, 256, size=(7,) + cfg["obs"], dtype=np.uint8))
    prob, value = (t.clone() for t in policy.prob_value(obs))
    assert prob.shape == (7, cfg["n_act"]) and float(prob.std()) > 0
    assert torch.allclose(prob.sum(dim=1), torch.ones(7, device=DEV), atol=1e-5)
    rows_prob, rows_value = policy.prob_value_rows(obs, rows_per_pass=3, tag="rows")
    assert torch.equal(rows_prob, prob) and torch.equal(rows_value, value)
    sel = _dev(np.array([6, 0, 3, 4], np.int32))
    sel_prob, sel_value = policy.prob_value(obs, sel)
    assert torch.equal(sel_prob, prob[sel.long()]) and torch.equal(sel_value, value[sel.long()])
    # the training forward: its hidden activations through the inference head
    x = policy._scaled(obs, sel)
    acts, hids = policy._trunk(x)
    t_prob = torch.empty((4, cfg["n_act"]), device=DEV)
    t_value = torch.empty(4, device=DEV)
    from accel_rl_amd import _lib
    _lib.pg_head_infer(hids[-1], policy.params[-2], policy.params[-1], t_prob, t_value)
    assert torch.equal(t_prob, prob[sel.long()]) and torch.equal(t_value, value[sel.long()])
    mb = dict(observations=obs, idx=sel, actions=_dev(rs.randint(0, cfg["n_act"], 7).astype(np.uint8)),
              advantages=_dev(rs.randn(7).astype(np.float32)), returns=_dev(rs.randn(7).astype(np.float32)), old_prob=prob)
    loss4 = policy.loss_and_grads(mb, 0, 0.0, V_COEFF, ENT_COEFF, torch.ones(1, device=DEV))
    want_ent = -ENT_COEFF * float((-(prob[sel.long()].double() * torch.log(prob[sel.long()].double() + 1e-8)).sum(1)).mean())
    assert torch.isfinite(loss4).all() and abs(float(loss4[2]) - want_ent) <= 1e-5 * abs(want_ent)
    again_prob, again_value = policy.prob_value(obs)            # the training pass left the parameters and the result alone
    assert torch.equal(again_prob, prob) and torch.equal(again_value, value)


@pytest.mark.parametrize("kind,gather", [(0, True), (0, False), (1, True), (1, False)],
                         ids=["a2c-idx", "a2c-rows", "ppo-idx", "ppo-rows"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_training_step_matches_float64_autograd(name, kind, gather):
    """loss_and_grads against float64 autograd of tests/resnet_ref.py:ref_net on the reference layout, at the whole-step
    tolerance of the other policies' tests (test_pqn_gpu.py: rtol 2e-3, atol 2e-5 max |.|; the gradients: max over the
    whole gradient).  The inputs keep every rectifier input and every pool window's lead further than BRANCH_MARGIN
    (relative to the layer's max |.|) from a tie, asserted on the float64 reference alone: float32 takes the same
    branches."""
    cfg, arr = CASES[name], case_arrays(name)
    ref = reference_step(name, kind, gather)
    assert ref["margin"] > rr.BRANCH_MARGIN, ref["margin"]
    policy = _make_policy(name)
    policy.set_param_values(arr["flat"])
    batch = cfg["batch"]
    obs = _dev(arr["obs"] if gather else arr["obs"][:batch])
    idx = _dev(arr["idx"]) if gather else None
    rows = arr["idx"].astype(np.int64) if gather else np.arange(batch)
    cut = (lambda a: a) if gather else (lambda a: a[:batch])
    mb = dict(observations=obs, idx=idx, actions=_dev(cut(arr["actions"])), advantages=_dev(cut(arr["advantages"])),
              returns=_dev(cut(arr["returns"])), old_prob=_dev(cut(ref["old_prob"])), valids=None)
    policy.flat_grads.fill_(NAN)
    loss4 = policy.loss_and_grads(mb, kind, CLIP, V_COEFF, ENT_COEFF, torch.ones(1, device=DEV))
    got_flat = policy.bucket_to_reference(policy.flat_grads)
    prob, value = policy.prob_value(obs, idx)

    def close(got, want, what):
        scale = np.abs(want).max()
        err = np.abs(got - want).max()
        print("%s %s kind %d gather %d: %s max err %.3g of max |.| %.3g" % (name, what, kind, gather, what, err, scale))
        return np.allclose(got, want, rtol=2e-3, atol=2e-5 * scale)

    assert close(_host(prob), ref["prob"], "prob") and close(_host(value), ref["value"], "value")
    assert close(_host(loss4)[:3], ref["losses"], "losses")
    assert abs(float(loss4[3]) - ref["losses"].sum()) <= 2e-3 * np.abs(ref["losses"]).sum()
    if kind == 1:
        ratio = ref["prob"][np.arange(batch), arr["actions"][rows]] / ref["old_prob"][rows][np.arange(batch), arr["actions"][rows]]
        assert (np.abs(np.abs(ratio - 1) - CLIP) > 1e-3).all()  # no row on the surrogate's kinks
    want_flat = np.concatenate([g.reshape(-1) for g in ref["grads"]])
    assert np.isfinite(got_flat).all() and got_flat.size == want_flat.size
    scale, pos = max(np.abs(want_flat).max(), 1e-3), 0
    for gname, want in zip(ref["names"], ref["grads"]):
        got = got_flat[pos:pos + want.size].reshape(want.shape)
        pos += want.size
        print("%-12s max |want| %.3g max err %.3g" % (gname, np.abs(want).max(), np.abs(got - want).max()))
        assert np.abs(want).max() > 0, gname                   # every tensor takes part
        assert np.allclose(got, want, rtol=2e-3, atol=2e-5 * scale), (gname, np.abs(got - want).max(), scale)


# ---- learners -----------------------------------------------------------------------------------------------------------

def _train(algo_name, use_graph, n_itr=5):
    """A2C or IMPALA(epochs=2) on the synthetic pong, 8 envs x horizon 5, the default AtariResnetPolicy."""
    from accel_rl_amd.algos.pg import IMPALA
    from accel_rl_amd.algos.pg.a2c import A2C
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_resnet_policy import AtariResnetPolicy
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game="pong"), horizon=5, n_parallel=2, envs_per=2,
                            max_path_length=25, max_decorrelation_steps=0, device=DEV)
    if algo_name == "a2c":
        algo = A2C(use_graph=use_graph)
    else:
        algo = IMPALA(optimizer_args=dict(epochs=2, minibatch_size=20), vtrace_lambda=0.95, rows_per_pass=16,
                      use_graph=use_graph)
    policy = AtariResnetPolicy()
    log = dict(infos=[])
    initialize, optimize = algo.initialize, algo.optimize_policy

    def recording_initialize(*a, **kw):
        initialize(*a, **kw)
        log["first"] = policy.get_param_values()

    def recording_optimize(itr, samples):
        out = optimize(itr, samples)
        log["infos"].append(out[1])
        return out
    algo.initialize, algo.optimize_policy = recording_initialize, recording_optimize
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=40 * (n_itr - 1), seed=9, log_interval_steps=40)
    runner.train()
    torch.cuda.synchronize()
    log["infos"] = [{k: _host(v).copy() for k, v in info.items()} for info in log["infos"]]
    return algo, policy, log


@pytest.mark.parametrize("algo_name", ["a2c", "impala"])
def test_learners_train_and_replayed_iterations_equal_eager_ones(algo_name):
    """Five iterations of 40 steps: the third is captured, the rest replayed; the same seeded run made eagerly ends in the
    same parameters and returned the same diagnostics, bit for bit."""
    algo, policy, log = _train(algo_name, True)
    assert algo._graph is not None and len(log["infos"]) == 5
    final = policy.get_param_values()
    assert policy.n_params == 1164759 and np.isfinite(final).all() and not np.array_equal(final, log["first"])
    for info in log["infos"]:
        assert all(np.isfinite(v).all() for v in info.values()) and (info["GradNorm"] > 0).all()
    algo_e, policy_e, log_e = _train(algo_name, False)
    assert algo_e._graph is None and np.array_equal(log["first"], log_e["first"])
    np.testing.assert_array_equal(policy_e.get_param_values(), final)
    for a, b in zip(log["infos"], log_e["infos"]):
        assert sorted(a) == sorted(b)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
