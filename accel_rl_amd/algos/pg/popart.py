"""PopArt (van Hasselt et al. 2016, "Learning values across many orders of magnitude"; Hessel et al. 2018, "Multi-task
deep reinforcement learning with PopArt", for the actor-critic form; the reference has none; PAPERS.md restates both from
memory, with what is recalled and what is chosen): adaptive normalisation of the value targets for the on-policy
learners.  The network's value output becomes a NORMALISED value n; running first and second moments (mu, nu) of the
return targets live on the device; the unnormalised value of a state is sigma n + mu with sigma = sqrt(nu - mu^2),
clamped.  After every update of the statistics the value row of W_head and its bias are rewritten so that sigma n + mu of
every state is what it was ("preserving outputs precisely"), and the loss then regresses n onto (G - mu) / sigma.

The head kernel, the served step, the sampler's record and the scans are untouched; the loop -- host / device split,
warm-up, hipGraph capture, diagnostics ring -- is AdvActorCriticBase's.  The mixin hooks in at two places.  _scan_values:
arl_popart_denorm on the recorded and the bootstrap values, into buffers of its own (the sampler's buffer is never
written), so the return / advantage scans run on unnormalised values as ever.  After the scan: one arl_popart_step on
opt["returns"] / opt["advantages"] -- batch moments, statistics, preservation, targets normalised in place.  Advantages
are divided by sigma' (unless standardize_adv has already made them unit-scale).  A2C, PPO and V-MPO scan in
process_samples, IMPALA in its epoch hook: one PopArt step per epoch's retargeting there.

The preservation step writes flat_params before the first minibatch, so the rollout's stored activations are withdrawn
(_reuse_granted is False; DESIGN.md 36 names keeping them as the follow-up)."""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.algos.pg.a2c import A2C
from accel_rl_amd.algos.pg.impala import IMPALA
from accel_rl_amd.algos.pg.ppo import PPO
from accel_rl_amd.algos.pg.vmpo import VMPO


def _finite(x):
    return isinstance(x, (int, float, np.floating, np.integer)) and not isinstance(x, bool) and bool(np.isfinite(x))


class PopArtMixin(object):
    """Over AdvActorCriticBase; PopArtA2C, PopArtPPO, PopArtVMPO and PopArtIMPALA are this plus the plain learner."""

    def __init__(self, beta=3e-4, sigma_min=1e-4, sigma_max=1e6, popart_init=(0.0, 1.0), **kwargs):
        if not (_finite(beta) and 0 <= beta <= 1):
            raise ValueError("beta must lie in [0, 1], got %r" % (beta,))
        if not (_finite(sigma_min) and _finite(sigma_max) and 0 < sigma_min <= sigma_max):
            raise ValueError("0 < sigma_min <= sigma_max, both finite; got %r, %r" % (sigma_min, sigma_max))
        if not (isinstance(popart_init, (tuple, list)) and len(popart_init) == 2 and all(_finite(x) for x in popart_init)):
            raise ValueError("popart_init must be a pair (mu, sigma) of finite numbers, got %r" % (popart_init,))
        if not sigma_min <= popart_init[1] <= sigma_max:
            raise ValueError("popart_init: sigma must lie in [sigma_min, sigma_max] = [%r, %r], got %r" %
                             (sigma_min, sigma_max, popart_init[1]))
        super().__init__(**kwargs)
        self.beta, self.sigma_min, self.sigma_max = float(beta), float(sigma_min), float(sigma_max)
        self.popart_init = (float(popart_init[0]), float(popart_init[1]))
        self._pa_stats = None

    def initialize(self, policy, env_spec, sample_size, horizon, mid_batch_reset):
        name = type(self).__name__
        if policy.recurrent:
            raise NotImplementedError("%s: recurrent policies are not built -- the value row is found in AtariCnnPolicy's "
                                      "output layers only (INTEGRATION.md, section E)" % name)
        if self.optimizer.parallelism_tag != "single":
            raise NotImplementedError("%s: single GPU only, got a %r optimizer (%s): per-rank statistics would rewrite "
                                      "the ranks' value rows differently and their parameters would diverge "
                                      "(INTEGRATION.md, section E)" %
                                      (name, self.optimizer.parallelism_tag, type(self.optimizer).__name__))
        try:
            head = policy.value_head()
        except (AttributeError, NotImplementedError) as e:
            raise NotImplementedError("%s: %s has no value_head() -- the preservation step rewrites the value row of "
                                      "W_head[(A + 1), hid] and its bias in place (%s) (INTEGRATION.md, section E)" %
                                      (name, type(policy).__name__, e))
        rows = int(sample_size)
        if rows > _lib.POPART_MAX_ROWS or head[0].numel() > _lib.POPART_MAX_HID:
            raise ValueError("%s: %d rows, a %d-wide value row; arl_popart_step takes at most %d rows and %d columns "
                             "(INTEGRATION.md, section E)" % (name, rows, head[0].numel(), _lib.POPART_MAX_ROWS,
                                                              _lib.POPART_MAX_HID))
        super().initialize(policy, env_spec, sample_size, horizon, mid_batch_reset)
        dev = policy.device
        self._pa_head = head
        mu, sigma = self.popart_init
        # (mu, nu, sigma, n_updates), and everything else the two launches write: allocated here, so the captured graph
        # keeps its addresses
        self._pa_stats = torch.tensor([mu, sigma * sigma + mu * mu, sigma, 0.], dtype=torch.float64, device=dev)
        self._pa_value = torch.zeros(rows, dtype=torch.float32, device=dev)
        self._pa_last = torch.zeros(self._n_env, dtype=torch.float32, device=dev)
        self._pa_diag = torch.zeros(2, dtype=torch.float32, device=dev)       # (PopArtMu, PopArtSigma) of the last step

    def _reuse_granted(self, samples_data):
        """Never: the preservation step writes the value row before the first minibatch (the head's inputs -- the stored
        activations -- would still be right; telling the writer contract so is the follow-up of DESIGN.md 36)."""
        return False

    # ---- device work (captured) ----
    def _device_optimize(self, itr, samples_data):
        opt_data, infos = super()._device_optimize(itr, samples_data)
        stats = self._pa_diag.clone()
        return opt_data, dict(infos, PopArtMu=stats[0:1], PopArtSigma=stats[1:2])

    def _scan_values(self, values, last_values):
        """sigma n + mu of the recorded and the bootstrap values, under the statistics as they stand (those every one of
        these forwards ran under: the statistics and the head change together, in _popart_step alone)."""
        _lib.popart_denorm(values.reshape(-1), last_values.reshape(-1), self._pa_stats, self._pa_value, self._pa_last)
        return self._pa_value.view(values.shape), self._pa_last.view(last_values.shape)

    def _popart_step(self, opt):
        adv = None if self.standardize_adv else opt["advantages"].reshape(-1)
        valids = opt["valids"].reshape(-1) if self._use_valids else None
        _lib.popart_step(opt["returns"].reshape(-1), adv, valids, self.beta, self.sigma_min, self.sigma_max,
                         self._pa_stats, self._pa_head[0], self._pa_head[1], self._pa_diag)
        self._params_written()

    def process_samples(self, itr, samples_data):
        opt = super().process_samples(itr, samples_data)
        self._popart_step(opt)
        return opt

    # ---- host side ----
    def popart_state(self):
        """dict(mu, nu, sigma, n_updates) as host floats (a device read: for snapshots, not for the loop)."""
        mu, nu, sigma, n = self._require_stats().cpu().tolist()
        return dict(mu=mu, nu=nu, sigma=sigma, n_updates=n)

    def set_popart_state(self, mu, nu, sigma, n_updates):
        """Put a snapshot's statistics back (the head that goes with them is part of the policy's parameters)."""
        if not (all(_finite(x) for x in (mu, nu, sigma, n_updates)) and sigma > 0 and n_updates >= 0):
            raise ValueError("set_popart_state: mu, nu, sigma, n_updates finite, sigma > 0, n_updates >= 0")
        stats = self._require_stats()
        stats.copy_(torch.tensor([mu, nu, sigma, n_updates], dtype=torch.float64))

    def unnormalize(self, values):
        """sigma n + mu (float32) for callers of policy.value, whose output is the normalised value."""
        stats = self._require_stats()
        return (stats[2] * values.double() + stats[0]).float()

    def _require_stats(self):
        if self._pa_stats is None:
            raise RuntimeError("%s: the statistics live on the policy's device and exist once initialize() has run" %
                               type(self).__name__)
        return self._pa_stats

    @property
    def opt_info_keys(self):
        return super().opt_info_keys + ["PopArtMu", "PopArtSigma"]


class PopArtA2C(PopArtMixin, A2C):
    """Single GPU, feed-forward policies"""


class PopArtPPO(PopArtMixin, PPO):
    """Single GPU, feed-forward policies; the targets are normalised once per call, before the first epoch"""


class PopArtVMPO(PopArtMixin, VMPO):
    """Single GPU, feed-forward policies; the temperature sees advantages in units of sigma'"""


class PopArtIMPALA(PopArtMixin, IMPALA):
    """Single GPU, feed-forward policies; one PopArt step per epoch's retargeting"""

    def process_samples(self, itr, samples_data):
        return IMPALA.process_samples(self, itr, samples_data)      # (nothing before the epochs: _retarget)

    def _retarget(self, epoch):
        super()._retarget(epoch)            # (prob_value_rows -> _scan_values -> arl_vtrace_scan)
        self._popart_step(self._opt_buf)
