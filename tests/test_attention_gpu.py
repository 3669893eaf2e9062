"""The relational policy on the GPU: the attention and coordinate kernels (csrc/attention.hip), AtariRelationalPolicy's
forward paths, one whole training step against float64 autograd, and captured against eager learners.  The bar everywhere is
the project's whole-step bar: rtol 2e-3, atol 2e-5 of max |want|."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_ref as rr
from test_attention_host import coords_bwd32, coords_fwd32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
E_ARG, E_RANGE, E_ALIGN = -1, -2, -3
TAIL = 8


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


def close(got, want, what=""):
    scale = np.abs(want).max()
    print("%s max err %.3g of max |.| %.3g" % (what, np.abs(got - want).max(), scale))
    return np.allclose(got, want, rtol=2e-3, atol=2e-5 * scale)


# ---- the kernels --------------------------------------------------------------------------------------------------------

def attention64(qkv, dout, scale):
    """float64: (out [B, N, H d], lse [B, H, N], dqkv) of qkv [B, N, 3, H, d]."""
    t = torch.from_numpy(qkv.astype(np.float64)).requires_grad_()
    q, k, v = (t[:, :, i].transpose(1, 2) for i in range(3))                                   # [B, H, N, d]
    s = scale * q @ k.transpose(2, 3)
    out = (torch.softmax(s, dim=3) @ v).transpose(1, 2).flatten(2)
    dqkv, = torch.autograd.grad(out, t, torch.from_numpy(dout.astype(np.float64)))
    return out.detach().numpy(), torch.logsumexp(s, dim=3).detach().numpy(), dqkv.numpy()


def _padded(n):
    """A NaN-filled buffer of n + TAIL floats and its 16-byte aligned view of n."""
    buf = torch.full((n + TAIL,), NAN, device=DEV)
    return buf, buf[:n]


def run_attention(L, qkv, dout, scale):
    b, n, _, h, d = qkv.shape
    bufs = [_padded(m) for m in (b * n * h * d, b * h * n, qkv.size)]
    (_, out), (_, lse), (_, dqkv) = bufs
    out, lse, dqkv = out.view(b, n, h * d), lse.view(b, h, n), dqkv.view(qkv.shape)
    qd = _dev(qkv)
    L.attn_fwd(qd, out, lse, scale)
    L.attn_bwd(qd, out, lse, _dev(dout), dqkv, scale)
    torch.cuda.synchronize()
    assert all(torch.isnan(buf[-TAIL:]).all() for buf, _ in bufs)
    return out, lse, dqkv


# (B, H) = (400, 3): 1200 work items on at most ARL_ATTN_MAX_GRID = 1024 workgroups -- the grid-stride walk wraps
@pytest.mark.parametrize("n,d,h,b", [(n, d, h, b) for n in (1, 2, 31, 32, 33, 63, 64) for d in (4, 32, 36, 64)
                                     for h, b in ((1, 1), (3, 5), (1, 5), (3, 1))] + [(2, 4, 3, 400)])
def test_attention_matches_float64_inside_its_buffers_twice(L, n, d, h, b):
    rs = np.random.RandomState(1000 * n + 10 * d + h + b)
    peaked = 2.0 if (n + d // 4) % 3 == 0 else 1.0             # some rows of P close to one-hot
    qkv = (peaked * rs.randn(b, n, 3, h, d)).astype(np.float32)
    dout = rs.randn(b, n, h * d).astype(np.float32)
    scale = d ** -0.5
    want = attention64(qkv, dout, scale)
    got = run_attention(L, qkv, dout, scale)
    for g, w, what in zip(got, want, ("out", "lse", "dqkv")):
        assert close(_host(g), w, "N %d d %d H %d B %d %s" % (n, d, h, b, what)), what
    inference = torch.full_like(got[0], NAN)
    L.attn_fwd(_dev(qkv), inference, None, scale)
    assert torch.equal(inference, got[0])                       # without lse: the same output
    assert all(torch.equal(x, y) for x, y in zip(run_attention(L, qkv, dout, scale), got))     # a second run: the same bits


def test_attention_refusals_write_nothing(L):
    lib = L.load()
    b, n, h, d = 2, 5, 2, 8
    qkv, dout = torch.zeros(b * n * 3 * h * d + 4, device=DEV), torch.zeros(b * n * h * d + 4, device=DEV)
    out, lse, dqkv = (torch.full((m + 4,), NAN, device=DEV) for m in (b * n * h * d, b * h * n, b * n * 3 * h * d))
    p = lambda t: t.data_ptr()                                  # noqa: E731

    def fwd(q_=p(qkv), o_=p(out), l_=p(lse), b_=b, n_=n, h_=h, d_=d, s_=1.0):
        return lib.arl_attn_fwd(q_, o_, l_, b_, n_, h_, d_, s_, None)

    def bwd(q_=p(qkv), o_=p(dout), l_=p(qkv), g_=p(dout), dq_=p(dqkv), b_=b, n_=n, h_=h, d_=d, s_=1.0):
        return lib.arl_attn_bwd(q_, o_, l_, g_, dq_, b_, n_, h_, d_, s_, None)

    for kw in (dict(n_=0), dict(n_=65), dict(d_=0), dict(d_=6), dict(d_=68), dict(h_=0), dict(h_=5, d_=64), dict(b_=0),
               dict(b_=2 ** 24 + 1)):
        assert fwd(**kw) == E_RANGE and bwd(**kw) == E_RANGE, kw
    for kw in (dict(q_=None), dict(o_=None), dict(s_=float("inf")), dict(o_=p(qkv))):
        assert fwd(**kw) == E_ARG, kw
    for kw in (dict(q_=None), dict(o_=None), dict(l_=None), dict(g_=None), dict(dq_=None), dict(s_=NAN), dict(dq_=p(qkv))):
        assert bwd(**kw) == E_ARG, kw
    assert fwd(q_=p(qkv) + 4) == E_ALIGN and fwd(l_=p(lse) + 2) == E_ALIGN and bwd(dq_=p(dqkv) + 4) == E_ALIGN
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in (out, lse, dqkv))


@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 3, 5, 8), (3, 9, 7, 64)], ids=lambda s: "x".join(map(str, s)))
def test_coordinate_kernels_equal_the_restatement_bit_for_bit(L, shape):
    rs = np.random.RandomState(sum(shape))
    x, g = rs.randn(*shape).astype(np.float32), rs.randn(*shape).astype(np.float32)
    d_y = rs.randn(*shape[:3], shape[3] + 4).astype(np.float32)
    d_y[..., :shape[3]].reshape(-1)[::5] = -g.reshape(-1)[::5]                                 # exact zeros among the sums
    mask = np.where(rs.rand(*shape) < 0.3, np.float32(-0.0), np.abs(x)) * np.where(rs.rand(*shape) < 0.2, -1, 1).astype(np.float32)
    want_y = coords_fwd32(x)
    ybuf, y = _padded(want_y.size)
    L.entity_coords_fwd(_dev(x), y.view(want_y.shape))
    assert torch.isnan(ybuf[-TAIL:]).all()
    np.testing.assert_array_equal(_host(y).reshape(want_y.shape), want_y)
    np.testing.assert_array_equal(np.signbit(_host(y).reshape(want_y.shape)), np.signbit(want_y))
    for m in (None, mask):
        want = coords_bwd32(g, d_y, m)
        for alias in (False, True):
            gd = _dev(g)
            buf, fresh = _padded(g.size)
            g_in = gd if alias else fresh.view(shape)
            L.entity_coords_bwd(gd, _dev(d_y), _dev(m), g_in)
            np.testing.assert_array_equal(_host(g_in), want, err_msg=str((m is None, alias)))
            np.testing.assert_array_equal(np.signbit(_host(g_in)), np.signbit(want))
            assert alias or (torch.isnan(buf[-TAIL:]).all() and np.array_equal(_host(gd), g))


# ---- policy -------------------------------------------------------------------------------------------------------------

CASES = dict(      # 35 positions, two blocks of two heads of 4; 12 positions, one block of one head of 36
    a=dict(obs=(4, 9, 7), batch=3, trunk=dict(conv_filters=(8,), conv_filter_sizes=(3,), conv_strides=(1,), conv_pads=((0, 0),)),
           net=dict(n_heads=2, head_dim=4, n_blocks=2, hidden_sizes=(64,)), n_act=6, seed=1),
    b=dict(obs=(4, 9, 7), batch=3, trunk=dict(conv_filters=(20,), conv_filter_sizes=(3,), conv_strides=(2,), conv_pads=((0, 0),)),
           net=dict(n_heads=1, head_dim=36, n_blocks=1, hidden_sizes=(64,)), n_act=6, seed=1))
CLIP, V_COEFF, ENT_COEFF = 0.2, 0.5, 0.01


def _new_policy(name):
    from accel_rl_amd.policies import AtariRelationalPolicy
    return AtariRelationalPolicy(**CASES[name]["trunk"], **CASES[name]["net"])


def _make_policy(name):
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    set_seed(5)
    policy = _new_policy(name)
    policy.initialize(EnvSpec(UintBox(CASES[name]["obs"]), Discrete(CASES[name]["n_act"])), device=DEV)
    policy.set_param_values(case_arrays(name)["flat"])
    return policy


@functools.lru_cache(maxsize=None)
def case_arrays(name):
    """Everything random of a whole-step case, from its seed alone: parameters of realistic scale in the reference layout,
    u8 observations (three rows more than the batch, for the gathered variant) and the minibatch's targets."""
    cfg = CASES[name]
    rs = np.random.RandomState(2000 + cfg["seed"])
    layout = _new_policy(name).reference_layout(cfg["obs"], cfg["n_act"])
    flat = []
    for _, shape in layout:
        if len(shape) == 4:
            a = np.sqrt(6. / ((shape[0] + shape[1]) * shape[2] * shape[3]))
            t = rs.uniform(-a, a, size=shape)
        else:
            t = rs.randn(*shape) / np.sqrt(shape[0]) if len(shape) == 2 else 0.05 * rs.randn(*shape)
        flat.append(t.astype(np.float32).reshape(-1))
    n = cfg["batch"] + 3
    return dict(flat=np.concatenate(flat), layout=layout, obs=rs.randint(0, 256, size=(n,) + cfg["obs"], dtype=np.uint8),
                actions=rs.randint(0, cfg["n_act"], n).astype(np.uint8), advantages=rs.randn(n).astype(np.float32),
                returns=rs.randn(n).astype(np.float32), idx=rs.permutation(n)[:cfg["batch"]].astype(np.int32),
                old_noise=rs.rand(n, cfg["n_act"]).astype(np.float32))


def ref_net(rp, cfg, x):
    """float64: x [B, C, H, W] scaled observations -> (prob, value, taps: every tensor a rectifier reads)."""
    taps, k = [], [0]

    def conv(a, stride=1, pad=(0, 0)):
        y = F.conv2d(a, rp[k[0]].flip(2, 3), rp[k[0] + 1], stride=stride, padding=pad)
        k[0] += 2
        return y
    for st, pad in zip(cfg["trunk"]["conv_strides"], cfg["trunk"]["conv_pads"]):
        x = conv(x, st, pad)
        taps.append(x)
        x = F.relu(x)
    b, c, h, w = x.shape
    heads, d, n = cfg["net"]["n_heads"], cfg["net"]["head_dim"], h * w
    axis = lambda m: (2 * torch.arange(m, dtype=x.dtype) - (m - 1)) / max(m - 1, 1)            # noqa: E731
    coords = torch.stack([axis(w)[None, :].expand(h, w), axis(h)[:, None].expand(h, w), torch.zeros(h, w, dtype=x.dtype),
                          torch.zeros(h, w, dtype=x.dtype)])[None].expand(b, 4, h, w)
    for _ in range(cfg["net"]["n_blocks"]):
        qkv = conv(torch.cat([F.relu(x), coords], dim=1)).view(b, 3, heads, d, n)
        q, key, v = (qkv[:, i].transpose(2, 3) for i in range(3))                              # [B, H, N, d]
        a = torch.softmax(q @ key.transpose(2, 3) / np.sqrt(d), dim=3) @ v
        x = x + conv(a.transpose(2, 3).reshape(b, heads * d, h, w))
        taps.append(x)
    x = F.relu(x).flatten(1)
    for _ in cfg["net"]["hidden_sizes"]:
        pre = x @ rp[k[0]] + rp[k[0] + 1]
        taps.append(pre)
        x, k[0] = F.relu(pre), k[0] + 2
    logits, value = x @ rp[k[0]] + rp[k[0] + 1], (x @ rp[k[0] + 2] + rp[k[0] + 3])[:, 0]
    assert k[0] + 4 == len(rp)
    return torch.softmax(logits, dim=1), value, taps


@functools.lru_cache(maxsize=None)
def reference_step(name, kind, gather):
    """The whole step in float64 on the CPU, computed once per variant and shared."""
    cfg, arr = CASES[name], case_arrays(name)
    rp, pos = [], 0
    for _, shape in arr["layout"]:
        m = int(np.prod(shape))
        rp.append(torch.from_numpy(arr["flat"][pos:pos + m].reshape(shape).astype(np.float64)).requires_grad_())
        pos += m
    rows = arr["idx"].astype(np.int64) if gather else np.arange(cfg["batch"])
    x = torch.from_numpy(arr["obs"][rows].astype(np.float64)) * np.float64(np.float32(1. / 255))
    prob, value, taps = ref_net(rp, cfg, x)
    old = 0.7 * prob.detach().numpy().astype(np.float32) + 0.3 * arr["old_noise"][rows] / arr["old_noise"][rows].sum(1, keepdims=True)
    old_full = np.full((arr["obs"].shape[0], cfg["n_act"]), 1.0 / cfg["n_act"], np.float32)
    old_full[rows] = old
    pick = lambda a: torch.from_numpy(a[rows].astype(np.float64))                              # noqa: E731
    losses = rr.pg_loss(prob, value, kind, torch.from_numpy(arr["actions"][rows].astype(np.int64)), pick(arr["advantages"]),
                        pick(arr["returns"]), torch.from_numpy(old.astype(np.float64)), CLIP, V_COEFF, ENT_COEFF)
    grads = torch.autograd.grad(sum(losses), rp)
    margin = min(float(t.detach().abs().min() / t.detach().abs().max()) for t in taps)
    return dict(prob=prob.detach().numpy(), value=value.detach().numpy(), old_prob=old_full, margin=margin,
                losses=np.array([float(t.detach()) for t in losses]), grads=[g.numpy() for g in grads])


@pytest.mark.parametrize("kind,gather", [(0, True), (0, False), (1, True), (1, False)],
                         ids=["a2c-idx", "a2c-rows", "ppo-idx", "ppo-rows"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_training_step_matches_float64_autograd(name, kind, gather):
    """loss_and_grads against float64 autograd of ref_net on the reference layout.  The seeds keep every rectifier input
    further than 1e-5 of its layer's max |.| from zero, asserted on the float64 reference alone (margins found: a 1.6e-4
    gathered and in rows; b 7.0e-4, 3.1e-4): float32 takes the same branches."""
    cfg, arr = CASES[name], case_arrays(name)
    ref = reference_step(name, kind, gather)
    assert ref["margin"] > rr.BRANCH_MARGIN, ref["margin"]
    policy = _make_policy(name)
    batch = cfg["batch"]
    obs = _dev(arr["obs"] if gather else arr["obs"][:batch])
    idx = _dev(arr["idx"]) if gather else None
    cut = (lambda a: a) if gather else (lambda a: a[:batch])
    mb = dict(observations=obs, idx=idx, actions=_dev(cut(arr["actions"])), advantages=_dev(cut(arr["advantages"])),
              returns=_dev(cut(arr["returns"])), old_prob=_dev(cut(ref["old_prob"])), valids=None)
    policy.flat_grads.fill_(NAN)
    loss4 = policy.loss_and_grads(mb, kind, CLIP, V_COEFF, ENT_COEFF, torch.ones(1, device=DEV))
    got_flat = policy.bucket_to_reference(policy.flat_grads)
    prob, value = policy.prob_value(obs, idx)
    assert close(_host(prob), ref["prob"], "prob") and close(_host(value), ref["value"], "value")
    assert close(_host(loss4)[:3], ref["losses"], "losses")
    want_flat = np.concatenate([g.reshape(-1) for g in ref["grads"]])
    assert np.isfinite(got_flat).all() and got_flat.size == want_flat.size
    scale, pos = max(np.abs(want_flat).max(), 1e-3), 0
    for (gname, _), want in zip(arr["layout"], ref["grads"]):
        got = got_flat[pos:pos + want.size].reshape(want.shape)
        pos += want.size
        assert np.abs(want).max() > 0, gname                   # every tensor takes part
        assert np.allclose(got, want, rtol=2e-3, atol=2e-5 * scale), (gname, np.abs(got - want).max(), scale)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_three_forward_paths_give_the_same_bits(L, name):
    policy = _make_policy(name)
    obs = _dev(np.random.RandomState(4).randint(0, 256, size=(7,) + CASES[name]["obs"], dtype=np.uint8))
    prob, value = (t.clone() for t in policy.prob_value(obs))
    assert float(prob.std()) > 0 and torch.allclose(prob.sum(dim=1), torch.ones(7, device=DEV), atol=1e-5)
    rows_prob, rows_value = policy.prob_value_rows(obs, rows_per_pass=3, tag="rows")
    assert torch.equal(rows_prob, prob) and torch.equal(rows_value, value)
    sel = _dev(np.array([6, 0, 3, 4], np.int32))
    policy._bits_pass = True                                    # the training forward: with lse
    acts, hids = policy._trunk(policy._scaled(obs, sel))
    assert all(torch.isfinite(blk["lse"]).all() for blk in acts[1])
    t_prob, t_value = torch.empty((4, policy.n_act), device=DEV), torch.empty(4, device=DEV)
    L.pg_head_infer(hids[-1], policy.params[-2], policy.params[-1], t_prob, t_value)
    assert torch.equal(t_prob, prob[sel.long()]) and torch.equal(t_value, value[sel.long()])


# ---- learners -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo_name", ["a2c", "impala"])
def test_learners_train_and_replayed_iterations_equal_eager_ones(algo_name, monkeypatch):
    """A2C and IMPALA(epochs=2) on the synthetic pong, 8 envs x 5 steps, the default network (63 positions): five
    iterations, the third captured and the rest replayed; the same seeded run made eagerly ends in the same parameters
    and returned the same diagnostics, bit for bit.  The seeded run is test_resnet_gpu's, given this policy."""
    import accel_rl_amd.policies.atari_resnet_policy as module
    from accel_rl_amd.policies import AtariRelationalPolicy
    from test_resnet_gpu import _train
    monkeypatch.setattr(module, "AtariResnetPolicy", AtariRelationalPolicy)
    algo, policy, log = _train(algo_name, True)
    assert algo._graph is not None and len(log["infos"]) == 5 and policy._conv_out == (64, 9, 7)
    final = policy.get_param_values()
    assert np.isfinite(final).all() and not np.array_equal(final, log["first"])
    for info in log["infos"]:
        assert all(np.isfinite(v).all() for v in info.values()) and (info["GradNorm"] > 0).all()
    algo_e, policy_e, log_e = _train(algo_name, False)
    assert algo_e._graph is None and np.array_equal(log["first"], log_e["first"])
    np.testing.assert_array_equal(policy_e.get_param_values(), final)
    for a, b in zip(log["infos"], log_e["infos"]):
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
