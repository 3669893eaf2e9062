"""IMPALA without a GPU: the V-trace yardstick of tests/vtrace_ref.py against the paper's sum written without the
recurrence and against float64 GAE(lambda) on on-policy data, the refusals of arl_vtrace_scan that need no device, the
constructor refusals of IMPALA, its refusals at initialize and its defaults."""
import ctypes

import numpy as np
import pytest

import vtrace_ref as vr

NAN, INF = float("nan"), float("inf")


# ---- the restatement against an independent form ----------------------------------------------------------------------

def _paper_sum(c, discount, lam, rho_bar, c_bar, pg_rho_bar):
    """vs_t = V_t + sum_{k >= t} (prod_{t <= i < k} g_i lambda min(c_bar, ratio_i)) delta_k,
    delta_k = min(rho_bar, ratio_k) (r_k + g_k V_{k+1} - V_k), g_i = 0 at a done else discount (V_T = the bootstrap);
    adv_t = min(pg_rho_bar, ratio_t) (r_t + g_t vs_{t+1} - V_t), vs_T = the bootstrap.  Float64 on unrounded values, every
    vs_t from its own sum: no value is carried from one step to the next."""
    ratio = vr.ratios64(c["prob"], c["old_prob"], c["actions"])
    n_env, horizon = ratio.shape
    v = np.concatenate([c["values"].astype(np.float64), c["last_values"].astype(np.float64)[:, None]], axis=1)
    r = c["rewards"].astype(np.float64)
    g = np.where(c["dones"] != 0, 0.0, discount)
    delta = np.minimum(ratio, rho_bar) * (r + g * v[:, 1:] - v[:, :-1])
    trace = g * lam * np.minimum(ratio, c_bar)
    vs = v.copy()
    for e in range(n_env):
        for t in range(horizon):
            vs[e, t] = v[e, t] + sum(np.prod(trace[e, t:k]) * delta[e, k] for k in range(t, horizon))
    adv = np.minimum(ratio, pg_rho_bar) * (r + g * vs[:, 1:] - v[:, :-1])
    return vs[:, :-1], adv


@pytest.mark.parametrize("lam", [0.0, 0.95, 1.0])
@pytest.mark.parametrize("bars", [(0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0), (2.0, 0.5, 1.0)])
def test_the_walk_equals_the_papers_sum(lam, bars):
    c = vr.rollout(11, 7, 9, 5, p_done=0.2)
    c["dones"][0, 0] = c["dones"][1, -1] = 1
    c["dones"][2, 3:5] = 1
    ratio = vr.ratios64(c["prob"], c["old_prob"], c["actions"])
    assert all((ratio < b).any() and (ratio > b).any() for b in bars)           # every bar cuts some steps, not all
    vs, adv, stats = vr.vtrace_walk(ratio, c["values"], c["last_values"], c["rewards"], c["dones"], 0.97, lam, *bars)
    want_vs, want_adv = _paper_sum(c, 0.97, lam, *bars)
    for got, want in ((vs, want_vs), (adv, want_adv)):
        assert (np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), np.abs(got - want).max()
    assert np.abs(stats[:, 0] - ratio.sum(axis=1)).max() <= 1e-5 * ratio.sum(axis=1).max()      # (fp32 storage)
    np.testing.assert_array_equal(stats[:, 1], (ratio > bars[0]).sum(axis=1))
    r32, a32, _ = vr.vtrace_ref(c["prob"], c["old_prob"], c["actions"], c["values"], c["last_values"], c["rewards"],
                                c["dones"], 0.97, lam, *bars)
    np.testing.assert_array_equal(r32, vs.astype(np.float32))
    np.testing.assert_array_equal(a32, adv.astype(np.float32))


def test_a_done_cuts_the_trace_and_the_bootstrap():
    c = vr.rollout(12, 3, 8, 4, p_done=0.0)
    c["dones"][:, 4] = 1
    args = (0.99, 0.9, 1.0, 1.0, 1.0)
    ret, adv, _ = vr.vtrace_ref(c["prob"], c["old_prob"], c["actions"], c["values"], c["last_values"], c["rewards"],
                                c["dones"], *args)
    other = dict(c, values=c["values"].copy(), rewards=c["rewards"].copy(), last_values=c["last_values"] + 5)
    other["values"][:, 5:] += 3.0
    other["rewards"][:, 5:] -= 2.0
    ret2, adv2, _ = vr.vtrace_ref(other["prob"], other["old_prob"], other["actions"], other["values"],
                                  other["last_values"], other["rewards"], other["dones"], *args)
    np.testing.assert_array_equal(ret2[:, :5], ret[:, :5])
    np.testing.assert_array_equal(adv2[:, :5], adv[:, :5])
    assert not np.array_equal(ret2[:, 5:], ret[:, 5:])


# ---- on-policy identity -----------------------------------------------------------------------------------------------

def _close_as_two_roundings(a, b):
    """Both sides are float64 results rounded to fp32 once: at most the two neighbouring floats apart."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    return (np.abs(a - b) <= 2.0 ** -22 * np.maximum(np.abs(a), np.abs(b)) + 1e-12).all()


@pytest.mark.parametrize("lam", [0.0, 0.95, 1.0])
def test_on_policy_with_unit_bars_is_gae(lam):
    c = vr.rollout(13, 7, 9, 6, p_done=0.2, on_policy=True)
    ratio = vr.ratios64(c["prob"], c["old_prob"], c["actions"])
    assert (ratio == 1.0).all()
    ret, adv, stats = vr.vtrace_ref(c["prob"], c["old_prob"], c["actions"], c["values"], c["last_values"], c["rewards"],
                                    c["dones"], 0.99, lam, 1.0, 1.0, 1.0)
    gae_adv, gae_ret = vr.gae64(c["values"], c["last_values"], c["rewards"], c["dones"], 0.99, lam)
    assert _close_as_two_roundings(ret, gae_ret)
    if lam == 1.0:
        assert _close_as_two_roundings(adv, gae_adv)
    else:                                       # the advantage bootstraps from vs_{t+1}, GAE's from its own lambda-sum
        assert not _close_as_two_roundings(adv, gae_adv)
    np.testing.assert_array_equal(stats, np.array([[9.0, 0.0]] * 7, np.float32))       # a ratio AT the bar is not above it


# ---- the entry point's refusals: before any HIP call, so they run without a device -------------------------------------

def test_scan_refusals_need_no_device():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    lib = _lib.load()
    n_env, horizon, n_act = 3, 4, 6
    steps = n_env * horizon
    f = lambda n: (ctypes.c_float * n)()                        # noqa: E731  (host memory: a refused call reads none of it)
    prob, old, val, last, rew, ret, adv, stats = f(steps * n_act), f(steps * n_act), f(steps), f(n_env), f(steps), \
        f(steps), f(steps), f(2 * n_env)
    act, done = (ctypes.c_uint8 * steps)(), (ctypes.c_uint8 * steps)()
    p = ctypes.addressof

    def scan(pr=p(prob), ol=p(old), ac=p(act), va=p(val), la=p(last), re=p(rew), do=p(done), g=0.99, lam=1.0, rho=1.0,
             cb=1.0, pg=1.0, n=n_env, t=horizon, a=n_act, out_r=p(ret), out_a=p(adv), st=p(stats)):
        return lib.arl_vtrace_scan(pr, ol, ac, va, la, re, do, g, lam, rho, cb, pg, n, t, a, out_r, out_a, st, None)

    for k in ("pr", "ol", "ac", "va", "la", "re", "do", "out_r", "out_a"):
        assert scan(**{k: None}) == -1 and b"null" in lib.arl_last_error(), k
    for kw in (dict(n=0), dict(n=-1), dict(n=2 ** 31), dict(t=0), dict(t=4097), dict(a=0), dict(a=19)):
        assert scan(**kw) == -2, kw
    for kw in (dict(g=-0.01), dict(g=1.01), dict(g=NAN), dict(g=INF), dict(lam=-0.01), dict(lam=1.01), dict(lam=NAN),
               dict(rho=0.0), dict(rho=-1.0), dict(rho=NAN), dict(rho=INF), dict(cb=0.0), dict(cb=NAN), dict(cb=INF),
               dict(pg=0.0), dict(pg=-0.5), dict(pg=NAN), dict(pg=INF)):
        assert scan(**kw) == -1, kw
    for kw in (dict(out_r=p(rew)), dict(out_a=p(val) + 8), dict(out_r=p(prob) + 16), dict(out_a=p(old)), dict(st=p(last)),
               dict(out_r=p(act)), dict(st=p(done)), dict(out_a=p(ret)), dict(st=p(ret) + 8), dict(st=p(adv))):
        assert scan(**kw) == -1 and b"overlap" in lib.arl_last_error(), kw
    spare = f(steps * n_act + 4)
    for k in ("pr", "ol", "va", "la", "re", "out_r", "out_a", "st"):
        assert scan(**{k: p(spare) + 2}) == -3, k
    assert all(x == 0 for x in ret) and all(x == 0 for x in adv) and all(x == 0 for x in stats)


# ---- IMPALA: constructor, initialize, defaults ------------------------------------------------------------------------

def _spec(**kw):
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    return dict(dict(cnn_specs[0], hidden_sizes=[64]), **kw)


@pytest.mark.parametrize("kw", [dict(discount=1.5), dict(discount=-0.1), dict(discount=NAN), dict(vtrace_lambda=-0.1),
                                dict(vtrace_lambda=1.01), dict(vtrace_lambda=NAN), dict(rho_bar=0.0), dict(rho_bar=INF),
                                dict(c_bar=-1.0), dict(c_bar=NAN), dict(pg_rho_bar=0.0), dict(pg_rho_bar=None),
                                dict(v_loss_coeff=NAN), dict(ent_loss_coeff=INF), dict(rows_per_pass=0),
                                dict(rows_per_pass=2.5), dict(lr_schedule="cosine"),
                                dict(optimizer_args=dict(epochs=0))])
def test_constructor_refusals(kw):
    from accel_rl_amd.algos.pg import IMPALA
    with pytest.raises(ValueError):
        IMPALA(**kw)


def test_standardize_adv_is_not_offered():
    from accel_rl_amd.algos.pg import IMPALA
    with pytest.raises(TypeError):
        IMPALA(standardize_adv=True)
    assert IMPALA().standardize_adv is False


def test_initialize_refusals():
    from accel_rl_amd.algos.pg import IMPALA
    from accel_rl_amd.optimizers.single import PpoOptimizer, VtraceOptimizer
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.atari_lstm_policy import AtariLstmPolicy

    class ManyGpus(VtraceOptimizer):
        parallelism_tag = property(lambda self: "synchronous")

    feed_forward = AtariCnnPolicy(**_spec())
    recurrent = AtariLstmPolicy(**_spec())
    assert recurrent.recurrent and not feed_forward.recurrent
    with pytest.raises(NotImplementedError, match="recurrent.*section E"):
        IMPALA().initialize(recurrent, None, 40, 5, True)
    with pytest.raises(NotImplementedError, match="mid_batch_reset.*section E"):
        IMPALA().initialize(feed_forward, None, 40, 5, False)
    with pytest.raises(NotImplementedError, match="single GPU.*section E"):
        IMPALA(OptimizerCls=ManyGpus).initialize(feed_forward, None, 40, 5, True)
    with pytest.raises(TypeError, match="_epoch_hook"):       # an optimizer that would never compute the targets
        IMPALA(OptimizerCls=PpoOptimizer, optimizer_args=dict(minibatch_size=8)).initialize(feed_forward, None, 40, 5, True)


def test_defaults_table():
    from accel_rl_amd.algos.pg import IMPALA
    from accel_rl_amd.algos.pg.impala import IMPALA as same
    from accel_rl_amd.optimizers.single import PpoOptimizer, VtraceOptimizer
    assert IMPALA is same
    algo = IMPALA()
    opt = algo.optimizer
    assert type(opt) is VtraceOptimizer and isinstance(opt, PpoOptimizer) and opt.parallelism_tag == "single"
    assert (algo.discount, algo.vtrace_lambda, algo.rho_bar, algo.c_bar, algo.pg_rho_bar) == (0.99, 1.0, 1.0, 1.0, 1.0)
    assert (algo.v_loss_coeff, algo.ent_loss_coeff, algo.lr_schedule, algo.rows_per_pass) == (0.5, 0.01, None, 1024)
    assert (opt._epochs, opt._minibatch_size, opt._learning_rate, opt._grad_norm_clip) == (1, None, 7e-4, 40)
    assert opt._update_method.name == "rmsprop" and opt._epoch_hook is None
    assert algo.loss_kind == 0 and algo.need_extra_obs is True and algo.use_graph is True
    assert algo.opt_info_keys == ["GradNorm", "RhoMean", "RhoClipFrac"]
    custom = IMPALA(vtrace_lambda=0.95, rho_bar=2.0, optimizer_args=dict(epochs=4, minibatch_size=64))
    assert (custom.vtrace_lambda, custom.rho_bar, custom.optimizer._epochs, custom.optimizer._minibatch_size) == \
        (0.95, 2.0, 4, 64)


def test_the_optimizer_calls_the_hook_at_the_start_of_every_epoch(monkeypatch):
    """VtraceOptimizer.device_updates without a device: the launches are replaced by recorders; 3 epochs of 40 // 16 = 2
    minibatches call the hook before minibatches 0, 2 and 4; minibatch_size None becomes the whole batch."""
    import torch
    from accel_rl_amd import _lib
    from accel_rl_amd.optimizers import update_methods
    from accel_rl_amd.optimizers.single import VtraceOptimizer
    calls = []
    monkeypatch.setattr(_lib, "copy_bytes", lambda dst, src, stream=None: dst.copy_(src))
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)

    class Target(object):
        device = torch.device("cpu")

    def make(minibatch_size, epochs):
        opt = VtraceOptimizer(learning_rate=1e-3, update_method=update_methods.rmsprop, update_method_args=dict(),
                              epochs=epochs, minibatch_size=minibatch_size)
        opt._input_names, opt._idx_host, opt._target = ["x"], None, Target()
        opt._losses = lambda mb: (None, None, None, calls.append(("mb", tuple(mb["idx"].tolist()))))
        opt._apply_update = lambda avg: calls.append(("update",))
        opt._recent_grad_norms = lambda count: count
        opt._set_updates_per_call = lambda count: None
        opt._epoch_hook = lambda epoch: calls.append(("hook", epoch))
        return opt
    np.random.seed(3)
    opt = make(16, 3)
    opt.prepare_host(40)
    _, count = opt.device_updates([None])
    assert count == 6 and [c[0] for c in calls] == ["hook", "mb", "update", "mb", "update"] * 3
    assert [c[1] for c in calls if c[0] == "hook"] == [0, 1, 2]
    rows = [c[1] for c in calls if c[0] == "mb"]
    assert all(len(r) == 16 for r in rows) and not set(rows[0]) & set(rows[1])          # one permutation per epoch
    del calls[:]
    whole = make(None, 2)
    whole.prepare_host(40)
    assert whole._minibatch_size == 40 and whole._n_minibatches == 2
    whole.device_updates([None])
    assert [c[0] for c in calls] == ["hook", "mb", "update"] * 2
    assert all(sorted(c[1]) == list(range(40)) for c in calls if c[0] == "mb")
