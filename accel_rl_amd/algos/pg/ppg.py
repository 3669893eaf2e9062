"""Phasic Policy Gradient, single-network variant (Cobbe, Hilton, Klimov, Schulman 2020, "Phasic Policy Gradient"; the
reference has none; PAPERS.md restates it with the differences).  Policy and value share one trunk, as in every learner
here, and PPG keeps their objectives from interfering by training them in two phases:

- the POLICY phase, every iteration, is PPO whose value loss stops at the last shared layer: it trains the head's value
  row and bias, nothing of it reaches the trunk (loss kind 2, csrc/ppg.hip: arl_ppg_head_loss_parts, ARL_PPG_POLICY);
- the AUXILIARY phase, after every n_pi-th iteration, distils value information into the trunk: e_aux epochs over the
  last n_pi rollouts on  aux_v_loss_coeff * mean((V - R)^2) + beta_clone * mean(KL(pi_old || pi)),  pi_old being the
  network's own output on those rollouts at the start of the phase (loss kind 3, ARL_PPG_AUX).

The policy phase is AdvActorCriticBase's loop with PpoOptimizer's minibatches, one captured graph after two eager calls.
After it the rollout's observations and returns go into slot (call number % n_pi) of a memory of n_pi * sample_size rows
(two stream-ordered arl_copy_bytes outside the graph).  The auxiliary phase runs inside the same optimize_policy call:
AtariCnnPolicy.prob_value_rows over the whole memory, then a SECOND PpoOptimizer on the same flat parameter bucket --
its own Adam moments and step count, the policy phase's are not touched -- draws minibatches from the memory by idx.  Its
shapes are static, so it is a second graph under the same discipline (two eager phases, the third captured).  Its host
draws are made only in iterations that have an auxiliary phase, before anything is enqueued.

Defaults: the policy phase's as recalled from the paper -- one epoch, Adam, clip 0.2, entropy coefficient 0.01, value
coefficient 0.5, GAE lambda 0.95 -- on BasePPO's other defaults; n_pi 32, e_aux 6, beta_clone 1, auxiliary minibatches
of an eighth of the memory."""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.algos.pg.ppo import BasePPO
from accel_rl_amd.optimizers.base import NORM_LOG_LEN
from accel_rl_amd.optimizers.single import PpoOptimizer
from accel_rl_amd.util.misc import capture_graph


def _count(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool) and x >= 1


def _coeff(x):
    return isinstance(x, (int, float, np.floating, np.integer)) and bool(np.isfinite(x)) and x >= 0


class PPG(BasePPO):
    """Single GPU, feed-forward policies"""

    def __init__(self, n_pi=32, e_aux=6, beta_clone=1.0, aux_v_loss_coeff=0.5, aux_minibatch_size=None,
                 aux_optimizer_args=None, rows_per_pass=1024, OptimizerCls=PpoOptimizer, optimizer_args=None,
                 v_loss_coeff=0.5, ent_loss_coeff=0.01, **kwargs):
        for name, n in (("n_pi", n_pi), ("e_aux", e_aux)):
            if not _count(n):
                raise ValueError("%s must be an integer >= 1, got %r" % (name, n))
        for name, c in (("beta_clone", beta_clone), ("aux_v_loss_coeff", aux_v_loss_coeff)):
            if not _coeff(c):
                raise ValueError("%s must be finite and >= 0, got %r" % (name, c))
        if aux_minibatch_size is not None and not _count(aux_minibatch_size):
            raise ValueError("aux_minibatch_size must be None (an eighth of the memory) or an integer >= 1")
        if rows_per_pass is not None and not _count(rows_per_pass):
            raise ValueError("rows_per_pass must be None (one pass) or an integer >= 1")
        for key in ("epochs", "minibatch_size"):
            if key in (aux_optimizer_args or dict()):
                raise ValueError("aux_optimizer_args: %s is set by e_aux / aux_minibatch_size" % key)
        args = dict(epochs=1)
        args.update(optimizer_args or dict())
        super().__init__(OptimizerCls=OptimizerCls, optimizer_args=args, v_loss_coeff=v_loss_coeff,
                         ent_loss_coeff=ent_loss_coeff, **kwargs)
        self.n_pi, self.e_aux = int(n_pi), int(e_aux)
        self.beta_clone, self.aux_v_loss_coeff = float(beta_clone), float(aux_v_loss_coeff)
        self.aux_minibatch_size, self.rows_per_pass = aux_minibatch_size, rows_per_pass
        self._aux_args = dict(learning_rate=self.optimizer._learning_rate, update_method=self.optimizer._update_method,
                              update_method_args=dict(self.optimizer._update_args), grad_norm_clip=None, shuffle=True)
        aux = dict(aux_optimizer_args or dict())
        if "update_method" in aux:                  # (another rule does not inherit the policy phase's arguments)
            aux.setdefault("update_method_args", dict())
        self._aux_args.update(aux)

    loss_kind = 2

    def initialize(self, policy, env_spec, sample_size, horizon, mid_batch_reset):
        if policy.recurrent:
            raise NotImplementedError("PPG: recurrent policies are not built -- the auxiliary phase walks stored rows, "
                                      "not trajectories (INTEGRATION.md, section E)")
        if not mid_batch_reset:
            raise NotImplementedError("PPG: mid_batch_reset=False is not built -- the PPG head kernel takes no `valids` "
                                      "(INTEGRATION.md, section E)")
        if self.optimizer.parallelism_tag != "single":
            raise NotImplementedError("PPG: single GPU only, got a %r optimizer (%s) (INTEGRATION.md, section E)" %
                                      (self.optimizer.parallelism_tag, type(self.optimizer).__name__))
        if not hasattr(policy, "prob_value_rows"):
            raise TypeError("the policy must provide prob_value_rows (the no-grad forward over the stored rollouts); "
                            "got %s" % type(policy).__name__)
        rows = self.n_pi * int(sample_size)
        bs = rows // 8 if self.aux_minibatch_size is None else int(self.aux_minibatch_size)
        updates = self.e_aux * (rows // bs) if bs >= 1 else 0
        if updates < 1 or updates > NORM_LOG_LEN:
            raise ValueError("PPG: an auxiliary phase of e_aux * (n_pi * sample_size // aux_minibatch_size) = %d * (%d // "
                             "%d) = %d updates; one optimizer call takes 1 to %d (INTEGRATION.md, section E)" %
                             (self.e_aux, rows, bs, updates, NORM_LOG_LEN))
        super().initialize(policy, env_spec, sample_size, horizon, mid_batch_reset)
        dev = policy.device
        self._aux_opt = PpoOptimizer(epochs=self.e_aux, minibatch_size=bs, **self._aux_args)
        self._aux_opt.initialize(inputs=["observations", "returns", "old_prob"], losses=self._aux_losses,
                                 constraints=None, target=policy, lr_mult=self._lr_mult)
        self._aux_per_epoch = rows // bs
        self._mem_rows = rows
        obs_shape = tuple(env_spec.observation_space.shape)
        self._mem_obs = torch.zeros((rows,) + obs_shape, dtype=torch.uint8, device=dev)
        self._mem_ret = torch.zeros(rows, dtype=torch.float32, device=dev)
        # (clone, v_loss) means of the last completed auxiliary phase's final epoch; the policy-phase graph appends a
        # copy to the diagnostics ring.  Allocated here, so both graphs keep addressing the same block.
        self._aux_stats = torch.zeros(2, dtype=torch.float32, device=dev)
        self._aux_acc = torch.zeros(4, dtype=torch.float32, device=dev)
        self._calls = 0
        self._aux_phases = 0
        self._aux_graph = None

    def optimize_policy(self, itr, samples_data):
        aux_now = (self._calls + 1) % self.n_pi == 0
        if aux_now:
            if self._done_event is not None:        # (the pinned index buffer may still be read by the previous phase)
                self._done_event.synchronize()
            self._aux_opt.prepare_host(self._mem_rows)
        out = super().optimize_policy(itr, samples_data)
        n, slot = self._batch_size, self._calls % self.n_pi
        _lib.copy_bytes(self._mem_obs[slot * n:(slot + 1) * n], samples_data["observations"])
        _lib.copy_bytes(self._mem_ret[slot * n:(slot + 1) * n], self._opt_buf["returns"])
        self._calls += 1
        if aux_now:
            self._enqueue_aux()
        self._done_event.record(torch.cuda.current_stream(self.policy.device))
        return out

    def _device_optimize(self, itr, samples_data):
        opt_data, infos = super()._device_optimize(itr, samples_data)
        stats = self._aux_stats.clone()             # as they stand BEFORE this call's auxiliary phase, eager or replayed
        return opt_data, dict(GradNorm=infos["GradNorm"], AuxVLoss=stats[1:2], AuxCloneLoss=stats[0:1])

    # ---- auxiliary phase ----
    def _enqueue_aux(self):
        self._aux_phases += 1
        if not self.use_graph or self._aux_phases <= 2:
            return self._device_aux()
        if self._aux_graph is None:
            torch.cuda.synchronize(self.policy.device)
            graph = torch.cuda.CUDAGraph()
            with capture_graph(graph):
                self._device_aux()
            self._aux_graph = graph
        self._aux_graph.replay()

    def _device_aux(self):
        """pi_old of every stored row from the parameters as they stand, then e_aux epochs of minibatches drawn from the
        memory; the final epoch's mean losses go to _aux_stats."""
        old_prob, _ = self.policy.prob_value_rows(self._mem_obs, self.rows_per_pass, tag="ppg_aux")
        self._aux_acc.zero_()
        self._aux_k = 0
        self._aux_opt.device_updates((self._mem_obs, self._mem_ret, old_prob))
        torch.mul(self._aux_acc[:2], 1. / self._aux_per_epoch, out=self._aux_stats)

    def _aux_losses(self, mb):
        loss4 = self.policy.loss_and_grads(mb, 3, 0., self.aux_v_loss_coeff, 0., self._lr_mult, None,
                                           beta_clone=self.beta_clone)
        self._aux_k += 1
        if self._aux_k > (self.e_aux - 1) * self._aux_per_epoch:
            self._aux_acc.add_(loss4)
        return loss4

    @property
    def opt_info_keys(self):
        return ["GradNorm", "AuxVLoss", "AuxCloneLoss"]
