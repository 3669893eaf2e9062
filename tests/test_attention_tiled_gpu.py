"""More than 64 positions on the GPU: the key-tiled attention kernels (arl_attn_tiled_fwd / _bwd, csrc/attention.hip) against
float64 at their tile edges, their refusals, one whole training step of AtariRelationalPolicy(max_positions=128) against
float64 autograd, and a captured against an eager learner on spec 1's own trunk.  Everything shared is
tests/test_attention_gpu.py's; the bar is its `close`: rtol 2e-3, atol 2e-5 of max |want|."""
import functools
import types

import numpy as np
import pytest
import torch

import test_attention_gpu as tag
from test_attention_gpu import DEV, E_ALIGN, E_ARG, E_RANGE, NAN, L, _dev, _host, attention64, close      # noqa: F401

pytestmark = pytest.mark.gpu

# ---- the kernels --------------------------------------------------------------------------------------------------------

# (n, d, h, b) = (65, 4, 3, 400): 2400 forward and 1200 backward items on at most ARL_ATTN_MAX_GRID = 1024 workgroups
SHAPES = [(n, d, h, b) for n in (1, 64, 65, 108, 128, 129, 255, 256) for d in (4, 32, 36, 64) for h, b in ((1, 1), (3, 2))]
KERNEL_CASES = ([s + (False,) for s in SHAPES + [(65, 4, 3, 400)]] + [s + (True,) for s in SHAPES if s[0] >= 128])


@pytest.mark.parametrize("n,d,h,b,ramp", KERNEL_CASES)
def test_tiled_attention_matches_float64_inside_its_buffers_twice(L, n, d, h, b, ramp):
    rs = np.random.RandomState(1000 * n + 10 * d + h + b)
    qkv = rs.randn(b, n, 3, h, d).astype(np.float32)
    if ramp:                    # the running maximum rises in every key tile; the early tiles' weights underflow
        qkv[:, :, 1] *= (1 + 2 * (np.arange(n) // 64)).astype(np.float32)[None, :, None, None]
    dout = rs.randn(b, n, h * d).astype(np.float32)
    scale = d ** -0.5
    tiled = types.SimpleNamespace(attn_fwd=L.attn_tiled_fwd, attn_bwd=L.attn_tiled_bwd)        # run_attention's two calls
    want = attention64(qkv, dout, scale)
    got = tag.run_attention(tiled, qkv, dout, scale)            # asserts the NaN tails behind the three buffers
    for g, w, what in zip(got, want, ("out", "lse", "dqkv")):
        assert close(_host(g), w, "N %d d %d H %d B %d ramp %d %s" % (n, d, h, b, ramp, what)), what
    inference = torch.full_like(got[0], NAN)
    L.attn_tiled_fwd(_dev(qkv), inference, None, scale)
    assert torch.equal(inference, got[0])                       # without lse: the same output
    assert all(torch.equal(x, y) for x, y in zip(tag.run_attention(tiled, qkv, dout, scale), got))      # again: the same bits


def test_tiled_refusals_write_nothing(L):
    lib = L.load()
    b, n, h, d = 2, 70, 2, 8
    qkv, dout = torch.zeros(b * n * 3 * h * d + 4, device=DEV), torch.zeros(b * n * h * d + 4, device=DEV)
    out, lse, dqkv = (torch.full((m + 4,), NAN, device=DEV) for m in (b * n * h * d, b * h * n, b * n * 3 * h * d))
    p = lambda t: t.data_ptr()                                  # noqa: E731

    def fwd(q_=p(qkv), o_=p(out), l_=p(lse), n_=n):
        return lib.arl_attn_tiled_fwd(q_, o_, l_, b, n_, h, d, 1.0, None)

    def bwd(q_=p(qkv), dq_=p(dqkv), n_=n):
        return lib.arl_attn_tiled_bwd(q_, p(dout), p(qkv), p(dout), dq_, b, n_, h, d, 1.0, None)

    for n_ in (0, 257):
        assert fwd(n_=n_) == E_RANGE and bwd(n_=n_) == E_RANGE, n_
    assert fwd(q_=None) == E_ARG and bwd(dq_=None) == E_ARG                 # a null pointer
    assert fwd(o_=p(qkv)) == E_ARG and bwd(dq_=p(qkv)) == E_ARG             # an output over an input
    assert fwd(q_=p(qkv) + 4) == E_ALIGN and fwd(l_=p(lse) + 2) == E_ALIGN and bwd(dq_=p(dqkv) + 4) == E_ALIGN
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in (out, lse, dqkv))


# ---- policy -------------------------------------------------------------------------------------------------------------

tag.CASES.update(   # 70 positions, two blocks of two heads of 4; 117 positions, one block of one head of 36
    c=dict(obs=(4, 12, 9), batch=3, trunk=dict(conv_filters=(8,), conv_filter_sizes=(3,), conv_strides=(1,), conv_pads=((0, 0),)),
           net=dict(n_heads=2, head_dim=4, n_blocks=2, hidden_sizes=(64,), max_positions=128), n_act=6, seed=1),
    d=dict(obs=(4, 15, 11), batch=3, trunk=dict(conv_filters=(20,), conv_filter_sizes=(3,), conv_strides=(1,), conv_pads=((0, 0),)),
           net=dict(n_heads=1, head_dim=36, n_blocks=1, hidden_sizes=(64,), max_positions=128), n_act=6, seed=2))


@pytest.mark.parametrize("kind,gather", [(0, True), (0, False), (1, True), (1, False)],
                         ids=["a2c-idx", "a2c-rows", "ppo-idx", "ppo-rows"])
@pytest.mark.parametrize("name", ["c", "d"])
def test_training_step_matches_float64_autograd_past_64_positions(name, kind, gather):
    """The whole-step test of tests/test_attention_gpu.py on cases c and d (margins on the float64 reference, gathered and
    in rows: c 7.2e-5, 1.0e-4; d 4.4e-5, 1.8e-5, asserted there above 1e-5).  Seed 3 of either case falls under it."""
    assert tag._new_policy(name).positions(tag.CASES[name]["obs"]) == dict(c=(10, 7), d=(13, 9))[name]
    tag.test_training_step_matches_float64_autograd(name, kind, gather)


# ---- learners -----------------------------------------------------------------------------------------------------------

def test_a2c_on_spec_1_trains_and_replayed_iterations_equal_eager_ones(monkeypatch):
    """A2C on the synthetic pong, 8 envs x 5 steps, spec 1's own trunk (108 positions): five iterations, the third
    captured and the rest replayed; the same seeded run made eagerly ends in the same parameters and diagnostics."""
    import accel_rl_amd.policies.atari_resnet_policy as module
    from accel_rl_amd.policies import AtariRelationalPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from test_resnet_gpu import _train
    spec1 = {k: v for k, v in cnn_specs[1].items() if k != "hidden_sizes"}
    monkeypatch.setattr(module, "AtariResnetPolicy", functools.partial(AtariRelationalPolicy, **spec1, max_positions=128))
    algo, policy, log = _train("a2c", True)
    assert algo._graph is not None and len(log["infos"]) == 5 and policy._conv_out == (64, 12, 9)
    final = policy.get_param_values()
    assert np.isfinite(final).all() and not np.array_equal(final, log["first"])
    algo_e, policy_e, log_e = _train("a2c", False)
    assert algo_e._graph is None and np.array_equal(log["first"], log_e["first"])
    np.testing.assert_array_equal(policy_e.get_param_values(), final)
    for a, b in zip(log["infos"], log_e["infos"]):
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
