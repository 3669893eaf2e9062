"""NGU's episodic novelty bonus (Badia et al. 2020, "Never Give Up"; the reference has none; PAPERS.md restates it from
memory, with what is recalled and what is chosen) on top of RND, for the on-policy learners.  RND's bonus is lifelong:
it decays once a state has been seen in any episode.  The episodic bonus is large the first time an EPISODE visits a
place and small on a revisit: the k nearest neighbours of the next frame's embedding in a per-env memory of the current
episode's embeddings, through an inverse kernel, multiplied by RND's error as a clipped modulator.

process_samples: RND's observation statistics and bonus pass (the per-row error) -> NguEmbedding.embed -> arl_epi_knn
(search, then append; resets and ring eviction inside the rollout modelled exactly) -> arl_epi_mix, which stands where
arl_rnd_reward_mix stands in RND -> AdvActorCriticBase's process_samples on a shallow copy whose rewards are the mix.
_losses: RND's (the policy update and the predictor update), then one update of the embedding and its inverse-dynamics
head on the same leading rows of the minibatch (NguEmbedding.loss_and_grads), through a second PredictorOptimizer.

Single reward stream, single value head, as RND here.  csrc/episodic.hip; include/accel_rl_hip.h states every expression."""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.algos.pg.a2c import A2C
from accel_rl_amd.algos.pg.ppo import PPO
from accel_rl_amd.algos.pg.rnd import PredictorOptimizer, RndMixin, _finite
from accel_rl_amd.policies.ngu_network import NguEmbedding, _int_in

NGU_ARG_KEYS = ("conv_filters", "conv_filter_sizes", "conv_strides", "conv_pads", "embedding_size", "head_hidden", "seed")


class NguMixin(RndMixin):
    """Over AdvActorCriticBase; NguPPO and NguA2C are this plus PPO / A2C."""

    def __init__(self, memory_size=1024, k=10, eps=1e-3, c=1e-3, xi=8e-3, s_max=8.0, mod_clip=5.0, ngu_args=None,
                 **kwargs):
        if not _int_in(memory_size, 1, _lib.EPI_MAX_MEMORY):
            raise ValueError("memory_size must be an integer in 1 .. %d, got %r" % (_lib.EPI_MAX_MEMORY, memory_size))
        if not _int_in(k, 1, _lib.EPI_MAX_K):
            raise ValueError("k must be an integer in 1 .. %d, got %r" % (_lib.EPI_MAX_K, k))
        for name, v, ok in (("eps", eps, lambda x: x > 0), ("c", c, lambda x: x >= 0), ("xi", xi, lambda x: x >= 0),
                            ("s_max", s_max, lambda x: x > 0), ("mod_clip", mod_clip, lambda x: x >= 1)):
            if not (_finite(v) and ok(v)):
                raise ValueError("%s: finite, eps > 0, c >= 0, xi >= 0, s_max > 0, mod_clip >= 1; got %r" % (name, v))
        args = dict(ngu_args or dict())
        unknown = sorted(set(args) - set(NGU_ARG_KEYS))
        if unknown:
            raise ValueError("ngu_args: unknown keys %s (%s)" % (unknown, ", ".join(NGU_ARG_KEYS)))
        super().__init__(**kwargs)
        self.memory_size, self.k = int(memory_size), int(k)
        self.eps, self.c, self.xi, self.s_max, self.mod_clip = float(eps), float(c), float(xi), float(s_max), float(mod_clip)
        self.ngu = NguEmbedding(self.rnd, **args)           # (validates embedding_size, head_hidden and seed)
        ropt = self._rnd_opt                                # the embedding's optimiser: the predictor's rule and rate
        self._ngu_opt = PredictorOptimizer(ropt._learning_rate, ropt._update_method, dict(ropt._update_args))

    def initialize(self, policy, env_spec, sample_size, horizon, mid_batch_reset):
        n_env = int(sample_size) // int(horizon)
        if n_env > _lib.EPI_MAX_ENVS:
            raise ValueError("%s: %d envs; arl_epi_knn takes at most %d (INTEGRATION.md, section E)" %
                             (type(self).__name__, n_env, _lib.EPI_MAX_ENVS))
        super().initialize(policy, env_spec, sample_size, horizon, mid_batch_reset)     # (RND's refusals)
        dev, rows = policy.device, int(sample_size)
        self.ngu.initialize(env_spec, n_env, self.memory_size, device=dev)
        # allocated here, so the captured graph keeps reading and writing the same blocks
        self._emb = torch.zeros((rows, self.ngu.embedding_size), dtype=torch.float32, device=dev)
        self._knn = torch.zeros((rows, self.k), dtype=torch.float64, device=dev)
        self._knn_m = torch.zeros(rows, dtype=torch.int32, device=dev)
        self._epi_diag = torch.zeros(3, dtype=torch.float32, device=dev)
        self._ngu_opt.initialize(self.ngu, self._lr_mult)
        self._ngu_batch = None

    # ---- device work (captured) ----
    def _device_optimize(self, itr, samples_data):
        opt_data, infos = super()._device_optimize(itr, samples_data)
        infos = {k: v for k, v in infos.items() if k not in ("IntRewMean", "IntRewStd")}   # (arl_rnd_reward_mix's)
        diag = self._epi_diag.clone()
        inv = self.ngu.loss2.clone()
        return opt_data, dict(infos, EpiRewMean=diag[0:1], ModMean=diag[1:2], InvDynLoss=inv[0:1], InvDynAcc=inv[1:2])

    def episodic_pass(self, samples_data):
        """knn f64[rows, k] and m i32[rows] of the batch; the episodes' memories move on to the state after it."""
        obs, extra = samples_data["observations"], samples_data["extra_observations"]
        self.ngu.embed(obs, extra, self._emb, self.rnd_rows_per_pass)
        dones = samples_data["dones"].reshape(-1)
        if dones.dtype != torch.uint8:
            dones = dones.to(torch.uint8)
        _lib.epi_knn(self._emb, dones, self._n_env, self._horizon, self.ngu.mem, self.ngu.n_ins, self.k, self._knn,
                     self._knn_m)
        return self._knn, self._knn_m

    def process_samples(self, itr, samples_data):
        obs, extra = samples_data["observations"], samples_data["extra_observations"]
        self._rnd_extra = extra
        self._ngu_batch = (samples_data["actions"], samples_data["dones"])
        self.rnd.update_obs_stats(obs, extra)
        self.bonus_pass(samples_data, self.rnd_rows_per_pass)
        self.episodic_pass(samples_data)
        _lib.epi_mix(self._knn, self._knn_m, self._rnd_err, samples_data["rewards"].reshape(-1), self.ngu.dist_mean,
                     self.ngu.err_moments, self.eps, self.c, self.xi, self.s_max, self.mod_clip, self.ext_coeff,
                     self.int_coeff, self._r_mix, self._epi_diag)
        mixed = dict(samples_data)                  # shallow: the sampler's buffer keeps its rewards
        mixed["rewards"] = self._r_mix.view(samples_data["rewards"].shape)
        return super(RndMixin, self).process_samples(itr, mixed)

    def _losses(self, mb):
        """RND's (policy, then predictor), then one update of the embedding and its head on the same leading rows."""
        loss4 = super()._losses(mb)
        idx = mb.get("idx")
        if idx is not None:
            idx = idx[:self._rnd_rows]
        self.ngu.loss_and_grads(mb["observations"], self._rnd_extra, idx, *self._ngu_batch)
        self._ngu_opt.step()
        return loss4

    @property
    def opt_info_keys(self):
        keys = [k for k in super().opt_info_keys if k not in ("IntRewMean", "IntRewStd")]
        return keys + ["EpiRewMean", "ModMean", "InvDynLoss", "InvDynAcc"]


class NguPPO(NguMixin, PPO):
    """Single GPU, feed-forward policies"""


class NguA2C(NguMixin, A2C):
    """Single GPU, feed-forward policies; one update per batch, so RND's predictor trains on the whole batch"""

    def __init__(self, update_proportion=1.0, **kwargs):
        if update_proportion != 1:
            raise ValueError("NguA2C trains RND's predictor on the whole batch (A2C's one update has no index list to "
                             "take a leading part of): update_proportion must be 1, got %r" % (update_proportion,))
        super().__init__(update_proportion=1.0, **kwargs)
