"""RND (Burda et al. 2018, "Exploration by Random Network Distillation"; the reference has none; PAPERS.md restates it
from memory, with what is recalled and what is chosen): an exploration bonus for the on-policy learners.  A predictor
network is trained to reproduce a fixed random network's embedding of the next frame; its error, divided by a running
standard deviation of the discounted bonus stream, is added to the environment's reward.

The single-head form: ONE reward stream r = ext_coeff * r_ext + int_coeff * r_int, one discount, the environment's own
dones, the existing return / advantage scans (DESIGN.md 32 has why, and what the paper's two value heads would touch).

The loop -- host / device split, warm-up, hipGraph capture, diagnostics ring -- is AdvActorCriticBase's; the mixin hooks
in at two places.  process_samples: arl_rnd_obs_stats on the batch -> the bonus pass over all rows (arl_rnd_obs_prepare
-> target trunk -> predictor trunk -> arl_rnd_error) -> arl_rnd_reward_mix -> the parent's process_samples on a shallow
copy of samples_data whose rewards are the mix (the sampler's buffer is never written).  _losses: the parent's policy
loss, then one predictor update on the leading ceil(update_proportion * B) indices of the minibatch -- the minibatch
lists are random permutations, so this is the paper's random subset without a mask or another draw.  The frame of a
transition is the newest plane of its NEXT observation; after a mid-batch reset that is the new episode's first frame,
as in the public PPO + RND implementations."""
import math

import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.algos.pg.a2c import A2C
from accel_rl_amd.algos.pg.ppo import PPO
from accel_rl_amd.optimizers.base import BaseOptimizer
from accel_rl_amd.policies.rnd_network import RndNetwork

RND_ARG_KEYS = ("conv_filters", "conv_filter_sizes", "conv_strides", "conv_pads", "embedding_size", "predictor_hidden",
                "rnd_seed", "learning_rate", "update_method", "update_method_args")


def _finite(x):
    return isinstance(x, (int, float, np.floating, np.integer)) and not isinstance(x, bool) and bool(np.isfinite(x))


class PredictorOptimizer(BaseOptimizer):
    """The flat-bucket update on the predictor's parameters: arl_opt_step without a clip (its two-launch form keeps no
    per-call state, so it sits inside another optimizer's call).  Slots and step count are allocated at initialize():
    a captured graph keeps its addresses."""

    def __init__(self, learning_rate, update_method, update_method_args=None):
        self._set_update_rule(learning_rate, update_method, update_method_args,
                              grad_norm_clip=0.)        # arl_opt_step: clip <= 0 is "no clip"

    def initialize(self, target, lr_mult):
        self._setup_bucket(target, lr_mult)

    def step(self):
        self._apply_update(1.0)


class RndMixin(object):
    """Over AdvActorCriticBase; RndPPO and RndA2C are this plus PPO / A2C."""

    def __init__(self, int_coeff=1.0, ext_coeff=2.0, int_discount=0.99, update_proportion=0.25, rnd_args=None,
                 rnd_rows_per_pass=1024, **kwargs):
        for name, c in (("int_coeff", int_coeff), ("ext_coeff", ext_coeff)):
            if not _finite(c):
                raise ValueError("%s must be finite, got %r" % (name, c))
        if not (_finite(int_discount) and 0 <= int_discount <= 1):
            raise ValueError("int_discount must lie in [0, 1], got %r" % (int_discount,))
        if not (_finite(update_proportion) and 0 < update_proportion <= 1):
            raise ValueError("update_proportion must lie in (0, 1], got %r" % (update_proportion,))
        if rnd_rows_per_pass is not None and not (isinstance(rnd_rows_per_pass, (int, np.integer)) and
                                                  not isinstance(rnd_rows_per_pass, bool) and rnd_rows_per_pass >= 1):
            raise ValueError("rnd_rows_per_pass must be None (one pass) or an integer >= 1")
        args = dict(rnd_args or dict())
        unknown = sorted(set(args) - set(RND_ARG_KEYS))
        if unknown:
            raise ValueError("rnd_args: unknown keys %s (%s)" % (unknown, ", ".join(RND_ARG_KEYS)))
        super().__init__(**kwargs)
        self.int_coeff, self.ext_coeff, self.int_discount = float(int_coeff), float(ext_coeff), float(int_discount)
        self.update_proportion, self.rnd_rows_per_pass = float(update_proportion), rnd_rows_per_pass
        # the predictor's optimiser: the policy optimizer's rule and rate unless rnd_args says otherwise
        opt = self.optimizer
        if "update_method" in args:                 # (another rule does not inherit the policy's arguments)
            args.setdefault("update_method_args", dict())
        self._rnd_opt = PredictorOptimizer(args.pop("learning_rate", opt._learning_rate),
                                           args.pop("update_method", opt._update_method),
                                           args.pop("update_method_args", dict(opt._update_args)))
        self.rnd = RndNetwork(**args)               # (validates the network's sizes and rnd_seed)

    def initialize(self, policy, env_spec, sample_size, horizon, mid_batch_reset):
        name = type(self).__name__
        if policy.recurrent:
            raise NotImplementedError("%s: recurrent policies are not built -- the predictor trains on rows, not "
                                      "trajectories (INTEGRATION.md, section E)" % name)
        if not mid_batch_reset:
            raise NotImplementedError("%s: mid_batch_reset=False is not built -- rows that `valids` masks out would "
                                      "enter the observation and bonus statistics (INTEGRATION.md, section E)" % name)
        if self.optimizer.parallelism_tag != "single":
            raise NotImplementedError("%s: single GPU only, got a %r optimizer (%s): per-rank statistics are another "
                                      "algorithm (INTEGRATION.md, section E)" %
                                      (name, self.optimizer.parallelism_tag, type(self.optimizer).__name__))
        rows, n_env = int(sample_size), int(sample_size) // int(horizon)
        if rows > _lib.RND_MIX_MAX_ROWS or n_env > _lib.RND_MIX_MAX_ENVS:
            raise ValueError("%s: %d rows of %d envs; arl_rnd_reward_mix takes at most %d rows of %d envs "
                             "(INTEGRATION.md, section E)" % (name, rows, n_env, _lib.RND_MIX_MAX_ROWS,
                                                              _lib.RND_MIX_MAX_ENVS))
        super().initialize(policy, env_spec, sample_size, horizon, mid_batch_reset)
        dev = policy.device
        self.rnd.initialize(env_spec, n_env, device=dev)
        self._rnd_opt.initialize(self.rnd, self._lr_mult)
        bs = getattr(self.optimizer, "_minibatch_size", None)
        self._rnd_rows = int(math.ceil(self.update_proportion * (rows if bs is None else min(int(bs), rows))))
        f32 = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)     # noqa: E731
        self._rnd_err, self._r_mix, self._rnd_diag = f32(rows), f32(rows), f32(2)
        self._mix_ws = torch.zeros(rows, dtype=torch.float64, device=dev)
        # (RndLoss of the call's last update, IntRewMean, IntRewStd); allocated here, so the captured graph keeps
        # writing the same block
        self._rnd_stats = f32(3)
        self._rnd_extra = None

    # ---- device work (captured) ----
    def _device_optimize(self, itr, samples_data):
        opt_data, infos = super()._device_optimize(itr, samples_data)
        self._rnd_stats[1:3].copy_(self._rnd_diag)
        stats = self._rnd_stats.clone()
        return opt_data, dict(infos, RndLoss=stats[0:1], IntRewMean=stats[1:2], IntRewStd=stats[2:3])

    def bonus_pass(self, samples_data, rows_per_pass=None):
        """err f32[rows]: the predictor's error on every row's next frame, under the statistics as they stand."""
        return self.rnd.errors(samples_data["observations"], samples_data["extra_observations"], self._rnd_err,
                               rows_per_pass)

    def process_samples(self, itr, samples_data):
        obs, extra = samples_data["observations"], samples_data["extra_observations"]
        self._rnd_extra = extra
        self.rnd.update_obs_stats(obs, extra)
        self.bonus_pass(samples_data, self.rnd_rows_per_pass)
        _lib.rnd_reward_mix(self._rnd_err, samples_data["rewards"].reshape(-1), self._n_env, self._horizon, self.rnd.rho,
                            self.rnd.rew_moments, self.int_discount, self.ext_coeff, self.int_coeff, self._r_mix,
                            self._rnd_diag, self._mix_ws)
        mixed = dict(samples_data)                  # shallow: the sampler's buffer keeps its rewards
        mixed["rewards"] = self._r_mix.view(samples_data["rewards"].shape)
        return super().process_samples(itr, mixed)

    def _losses(self, mb):
        """The parent's policy loss and gradient, then one predictor update on the leading rows of the minibatch."""
        loss4 = super()._losses(mb)
        idx = mb.get("idx")
        if idx is not None:
            idx = idx[:self._rnd_rows]
        loss = self.rnd.loss_and_grads(mb["observations"], self._rnd_extra, idx)
        self._rnd_opt.step()
        self._rnd_stats[0:1].copy_(loss)
        return loss4

    @property
    def opt_info_keys(self):
        return super().opt_info_keys + ["RndLoss", "IntRewMean", "IntRewStd"]


class RndPPO(RndMixin, PPO):
    """Single GPU, feed-forward policies"""


class RndA2C(RndMixin, A2C):
    """Single GPU, feed-forward policies; one update per batch, so the predictor trains on the whole batch"""

    def __init__(self, update_proportion=1.0, **kwargs):
        if update_proportion != 1:
            raise ValueError("RndA2C trains the predictor on the whole batch (A2C's one update has no index list to "
                             "take a leading part of): update_proportion must be 1, got %r" % (update_proportion,))
        super().__init__(update_proportion=1.0, **kwargs)
