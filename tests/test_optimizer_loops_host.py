"""CPU-only: what the optimizer classes share.  (1) The one minibatch loop (optimizers/single.py
`PpoOptimizer._minibatches`) as every class drives it: the exact sequence of epoch hook / minibatch / gradient share /
update / dual step, the keys each minibatch dict carries, and `_hole` put back to None after a backward pass that
raises.  2 epochs x 2 minibatches of 4 rows on a batch of 8 (trajectories: horizon 2), a fake target on the CPU, the
launches replaced by recorders.  The expected sequences are written out by hand from the classes' contracts.  (2) The
one optimiser-state builder (optimizers/base.py `BaseOptimizer._new_state`) under the main bucket, FQF's fraction range
and SAC's ranges: every pointer of the ArlOptState against the tensor that owns it."""
import types

import numpy as np
import pytest
import torch

from accel_rl_amd import _lib
from accel_rl_amd.optimizers import update_methods
from accel_rl_amd.optimizers.base import NORM_LOG_LEN, BaseOptimizer

ROWS, MB, EPOCHS, HORIZON = 8, 4, 2, 2


class _Target(object):
    device = torch.device("cpu")

    def traj_minibatch(self, mb):               # (the policy's: one launch that adds the rows' indices and states)
        return mb


class _Boom(Exception):
    pass


def _make(monkeypatch, cls, events, fail_at=None, sync_ranks=None, **kw):
    """A `cls` as far as its loop needs it, without a bucket.  The loss callable plays the policy: it records the
    minibatch, takes every hook the minibatch offers, and raises at minibatch number `fail_at`."""
    monkeypatch.setattr(_lib, "copy_bytes", lambda dst, src, stream=None: dst.copy_(src))
    monkeypatch.setattr(_lib, "vmpo_dual_step", lambda *a: events.append(("dual",)))
    monkeypatch.setattr(_lib, "corun_job", lambda *a: ("job",) + a[-2:])
    monkeypatch.setattr(BaseOptimizer, "_apply_update", lambda self, avg_factor=1.0: events.append(("update", avg_factor)))
    opt = cls(learning_rate=1e-3, update_method=update_methods.adam, update_method_args=dict(), epochs=EPOCHS,
              minibatch_size=MB, **kw)
    opt._input_names, opt._idx_host, opt._target = ["x"], None, _Target()
    opt._horizon = HORIZON                      # (read by TrajPpoOptimizer alone)
    opt._recent_grad_norms = lambda count: count
    opt._set_updates_per_call = lambda count: None
    opt._share_grad = lambda: events.append(("share",))
    if hasattr(cls, "_epoch_hook"):             # (VtraceOptimizer's: the algorithm sets it)
        opt._epoch_hook = lambda epoch: events.append(("hook", epoch))
    if sync_ranks:
        opt.init_comm(None, 0, sync_ranks)
        opt._share_grad_async = lambda tail: events.append(("share_async", tail))
    # what the co-run hook itself reads (BaseOptimizer._corun_hook): the first update of a call, no hole fixed yet
    opt._kernel_args, opt._n_updates, opt._hole, opt._hole_count, opt._call_hole = (0.9, 0.999, 1e-8), 0, None, 0, None
    opt._opt_state, opt._step_pp, opt._norm_parts = types.SimpleNamespace(norm_log_len=4), None, None
    opt._noclip_state = lambda: None
    opt._lr_mult = opt.duals = opt.temp4 = opt._dual_slot0 = opt._dual_slot1 = opt._dual_step_count = None
    seen = []

    def losses(mb):
        k = len(seen)
        seen.append(mb)
        events.append(("mb", k))
        if "dense_w_hook" in mb:
            assert mb["dense_w_hook"](0, 4) == ("job", 0, 4) and opt._hole == (0, 4)
        if "split_hook" in mb:
            mb["split_hook"]()
        if k == fail_at:
            raise _Boom()
        return (None, None, None, 10. + k)
    opt._losses = losses
    return opt, seen


def _run(monkeypatch, cls, **kw):
    """-> (events of one prepare_host + device_updates, the minibatch dicts, the optimizer); then the same call with a
    backward pass that raises at its second minibatch must leave `_hole` None."""
    events = []
    opt, seen = _make(monkeypatch, cls, events, **kw)
    np.random.seed(5)
    opt.prepare_host(ROWS)
    assert opt._n_minibatches == 4 and opt._idx_host.dtype == torch.int32
    losses, count = opt.device_updates([torch.arange(ROWS)])
    assert losses == [10., 11., 12., 13.] and count == 4 and opt._hole is None
    assert torch.equal(opt._idx_dev, opt._idx_host)
    failing, _ = _make(monkeypatch, cls, [], fail_at=1, **kw)
    failing.prepare_host(ROWS)
    with pytest.raises(_Boom):
        failing.device_updates([torch.arange(ROWS)])
    assert failing._hole is None
    return events, seen, opt


def _per_minibatch(*after_mb):
    return [e for k in range(4) for e in (("mb", k),) + after_mb]


def _rows_partition_each_epoch(seen):
    for mb in seen:
        assert mb["idx"].dtype == torch.int32 and mb["idx"].numel() == MB
    for e in range(EPOCHS):
        assert sorted(seen[2 * e]["idx"].tolist() + seen[2 * e + 1]["idx"].tolist()) == list(range(ROWS))


@pytest.mark.parametrize("kw,hook", [(dict(), True), (dict(grad_norm_clip=0.5), False), (dict(corun_update=False), False)])
def test_ppo_offers_the_corun_hook_only_without_a_clip_and_with_the_switch_on(monkeypatch, kw, hook):
    from accel_rl_amd.optimizers.single import PpoOptimizer
    kw = dict(kw)
    if "corun_update" in kw:
        monkeypatch.setattr(PpoOptimizer, "corun_update", kw.pop("corun_update"))
    events, seen, _ = _run(monkeypatch, PpoOptimizer, **kw)
    assert events == _per_minibatch(("share",), ("update", 1.0))
    assert all(set(mb) == {"x", "idx"} | ({"dense_w_hook"} if hook else set()) for mb in seen)
    _rows_partition_each_epoch(seen)


def test_vmpo_is_ppo_plus_a_dual_step_after_every_update(monkeypatch):
    from accel_rl_amd.optimizers.single import VmpoOptimizer
    events, seen, _ = _run(monkeypatch, VmpoOptimizer)
    assert events == _per_minibatch(("share",), ("update", 1.0), ("dual",))
    assert all(set(mb) == {"x", "idx", "dense_w_hook"} for mb in seen)
    _rows_partition_each_epoch(seen)


def test_vtrace_calls_the_epoch_hook_and_never_offers_the_corun_hook(monkeypatch):
    from accel_rl_amd.optimizers.single import VtraceOptimizer
    events, seen, opt = _run(monkeypatch, VtraceOptimizer)    # (no norm clip: PpoOptimizer itself would offer the hook)
    step = [("share",), ("update", 1.0)]
    assert opt._grad_norm_clip is None
    assert events == [("hook", 0), ("mb", 0)] + step + [("mb", 1)] + step + \
        [("hook", 1), ("mb", 2)] + step + [("mb", 3)] + step
    assert all(set(mb) == {"x", "idx"} for mb in seen)
    _rows_partition_each_epoch(seen)


def test_traj_minibatches_carry_segment_numbers_and_no_hook(monkeypatch):
    from accel_rl_amd.optimizers.single import TrajPpoOptimizer
    events, seen, opt = _run(monkeypatch, TrajPpoOptimizer)
    assert events == _per_minibatch(("share",), ("update", 1.0))
    assert all(set(mb) == {"x", "idx", "traj", "horizon"} and mb["idx"] is None and mb["horizon"] == HORIZON
               for mb in seen)
    assert tuple(opt._idx_host.shape) == (4, MB // HORIZON)
    for e in range(EPOCHS):
        assert sorted(seen[2 * e]["traj"].tolist() + seen[2 * e + 1]["traj"].tolist()) == list(range(ROWS // HORIZON))


def test_sync_ppo_overlapped_and_plain(monkeypatch):
    from accel_rl_amd.optimizers.sync import SyncPpoOptimizer
    assert SyncPpoOptimizer._overlap_allreduce is True
    events, seen, _ = _run(monkeypatch, SyncPpoOptimizer, sync_ranks=2)
    # the policy's split hook starts the tail's all-reduce inside the backward pass; the head's follows it
    assert events == _per_minibatch(("share_async", True), ("share_async", False), ("update", 0.5))
    assert all(set(mb) == {"x", "idx", "split_hook"} for mb in seen)
    _rows_partition_each_epoch(seen)
    monkeypatch.setattr(SyncPpoOptimizer, "_overlap_allreduce", False)          # (as the benchmark's N = 1 line sets it)
    events, seen, _ = _run(monkeypatch, SyncPpoOptimizer, sync_ranks=2)
    assert events == _per_minibatch(("share",), ("update", 0.5))
    assert all(set(mb) == {"x", "idx"} for mb in seen)


def test_no_minibatch_and_minibatch_size_none(monkeypatch):
    from accel_rl_amd.optimizers.single import PpoOptimizer, VmpoOptimizer
    events = []
    opt, seen = _make(monkeypatch, PpoOptimizer, events)
    opt._minibatch_size = 16                    # larger than the batch: the tail is dropped, nothing is left
    opt.prepare_host(ROWS)
    assert opt._n_minibatches == 0 and opt.device_updates([torch.arange(ROWS)]) == ([], []) and not events and not seen
    opt, _ = _make(monkeypatch, PpoOptimizer, events)
    opt._minibatch_size = None                  # plain PPO: no "whole batch" rule
    with pytest.raises(TypeError):
        opt.prepare_host(ROWS)
    opt, _ = _make(monkeypatch, VmpoOptimizer, events)
    opt._minibatch_size = None
    opt.prepare_host(ROWS)
    assert opt._minibatch_size == ROWS and opt._n_minibatches == EPOCHS


# ---- the state builder ------------------------------------------------------------------------------------------------

def _bucket(n, **extra):
    """A fake policy on the CPU: a flat fp32 parameter bucket and its gradient bucket."""
    return types.SimpleNamespace(device=torch.device("cpu"), flat_params=torch.zeros(n), flat_grads=torch.zeros(n), **extra)


def _check_state(st, n, params, grads, lr_mult, adam, norm_log_len, slot_len, first=0):
    """Every field of the ArlOptState `st` against the tensors it keeps (`st.tensors`)."""
    t = st.tensors
    assert st.n_params == n and st.norm_log_len == norm_log_len == t["norm_log"].numel()
    assert st.params == params.data_ptr() + 4 * first and st.grads == grads.data_ptr() + 4 * first
    assert st.slot0 == t["slot0"].data_ptr() and t["slot0"].numel() == slot_len
    if adam:
        assert st.slot1 == t["slot1"].data_ptr() and t["slot1"].numel() == slot_len
        assert t["slot1"].data_ptr() != t["slot0"].data_ptr()
    else:
        assert st.slot1 is None and t["slot1"] is None                      # a null pointer: rmsprop has one slot
    assert st.step_count == t["step_count"].data_ptr() and t["step_count"].numel() == 1
    assert st.lr_mult == lr_mult.data_ptr() and t["lr_mult"] is lr_mult
    assert st.partials == t["partials"].data_ptr() and t["partials"].numel() == _lib.OPT_PARTIALS
    assert t["partials"].dtype == torch.float64 and st.grad_norm_log == t["norm_log"].data_ptr()
    assert all(t[k].dtype == torch.float32 and not t[k].any() for k in ("slot0", "step_count", "norm_log"))


@pytest.mark.parametrize("method,want", [(update_methods.adam, (0.9, 0.999, 1e-8)), (update_methods.rmsprop, (0.9, 0.0, 1e-6))])
def test_main_bucket_state(method, want):
    from accel_rl_amd.optimizers.single import A2cOptimizer
    target, opt = _bucket(20), A2cOptimizer(1e-3, method)
    opt.initialize(["x"], None, None, target, lr_mult=0.5)
    st = opt._opt_state
    assert opt._lr_mult.tolist() == [0.5] and opt._kernel_args == want and NORM_LOG_LEN == 64
    _check_state(st, 20, target.flat_params, target.flat_grads, opt._lr_mult, method.name == "adam", 64, 20)
    assert opt._slot0 is st.tensors["slot0"] and opt._slot1 is st.tensors["slot1"]
    assert opt._step_count is st.tensors["step_count"] and opt._norm_log is st.tensors["norm_log"]
    assert opt.parallelism_tag == "single" and opt._avg_factor() == 1.0 and opt._share_grad() is None


def test_fqf_fraction_range_state():
    from accel_rl_amd.optimizers.dqn import FqfOptimizer
    off, n = 8, 20
    target = _bucket(n, frac_offset=off)
    lr_mult = torch.ones(1)
    opt = FqfOptimizer(1e-4, update_methods.adam)           # the fraction layer's own rule: the paper's RMSprop
    opt._setup_bucket(target, lr_mult)
    assert opt._opt_state.n_params == off and opt._opt_state.params == target.flat_params.data_ptr()
    assert opt._opt_state.norm_log_len == 64 and opt._slot0.numel() == n and opt._lr_mult is lr_mult
    _check_state(opt._frac_state, n - off, target.flat_params, target.flat_grads, lr_mult, False, 1, n - off, first=off)
    assert opt._frac_slot0 is opt._frac_state.tensors["slot0"] and opt._frac_slot1 is None
    assert opt._frac_step_count is opt._frac_state.tensors["step_count"] and opt._frac_kernel_args == (0.95, 0.0, 1e-5)
    both = FqfOptimizer(1e-4, update_methods.adam, fraction_args=dict(update_method=update_methods.adam))
    both._setup_bucket(target, lr_mult)
    _check_state(both._frac_state, n - off, target.flat_params, target.flat_grads, lr_mult, True, 1, n - off, first=off)


def test_sac_range_states():
    from accel_rl_amd.optimizers.dqn import SacOptimizer
    from accel_rl_amd.policies.dqn.atari_sac_discrete_policy import AtariSacDiscretePolicy
    target = object.__new__(AtariSacDiscretePolicy)         # (only what _setup_bucket reads; nothing is launched)
    target.__dict__.update(vars(_bucket(12)), q1=_bucket(3), q2=_bucket(16), log_alpha=torch.zeros(4),
                           log_alpha_grad=torch.zeros(4))
    lr_mult = torch.ones(1)
    opt = SacOptimizer(3e-4, update_methods.adam, alpha_args=dict(update_method=update_methods.rmsprop))
    opt._setup_bucket(target, lr_mult)
    assert len(opt._ranges) == 3 and opt._ranges[0] is opt._opt_state
    _check_state(opt._ranges[0], 12, target.flat_params, target.flat_grads, lr_mult, True, 64, 12)
    _check_state(opt._ranges[1], 3, target.q1.flat_params, target.q1.flat_grads, lr_mult, True, 1, 4)
    _check_state(opt._ranges[2], 16, target.q2.flat_params, target.q2.flat_grads, lr_mult, True, 1, 16)
    _check_state(opt._alpha_state, 1, target.log_alpha, target.log_alpha_grad, lr_mult, False, 1, 4)
