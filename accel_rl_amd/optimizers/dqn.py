"""DQN-family optimizer (reference: accel_rl/optimizers/single/dqn_optimizer.py:11-54): one gradient
step per call on a replay minibatch, optional conv-gradient scaling and global-norm clip, adam / rmsprop
on the flat bucket (csrc/optim.hip).  `loss` is a callable(minibatch tuple) -> (priority f32[B], loss scalar) that leaves
the gradient in the policy's flat bucket (the algorithm builds it)."""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.optimizers.base import BaseOptimizer, kernel_args, sub_args
from accel_rl_amd.util.misc import capture_graph


class DqnOptimizer(BaseOptimizer):
    """use_graph: after two eager calls the whole update (three forward passes, loss, backward, optimiser
    step: ~60 launches) is replayed from one hipGraph over static input buffers -- at the reference's
    batch size of 32 the update is launch-bound, not compute-bound."""

    def __init__(self, learning_rate, update_method, update_method_args=None, grad_norm_clip=None,
                 scale_conv_grads=False, use_graph=True):
        self._scale_conv_grads = scale_conv_grads      # dueling networks: conv gradients x 2^-1/2 (:34-36)
        self._set_update_rule(learning_rate, update_method, update_method_args, grad_norm_clip)
        self._use_graph = use_graph
        self._static = self._graph = self._graph_out = None
        self._ring, self._pack_rows = None, 0
        self._calls = 0

    def initialize(self, inputs, loss, target, priority_expr=None, givens=None, lr_mult=1):
        self._input_names = list(inputs)
        self._loss_fn = loss
        self._setup_bucket(target, lr_mult)
        self._set_updates_per_call(1)

    def optimize(self, inputs):
        if not self._use_graph:
            return self._step(inputs)
        static = self._stage(inputs)
        self._calls += 1
        if self._graph is None:
            if self._calls <= 2:                                  # warm-up: buffers, kernel attributes
                return self._step(static)
            if self._pack_rows:                                   # (allocated here: not from the capture's private pool)
                dev = self._target.device
                self._ring = torch.zeros((self.STATS_RING, 2 * self._pack_rows), dtype=torch.float32, device=dev)
                self._ring_count = torch.zeros(1, dtype=torch.int32, device=dev)
                self._ring_replays = 0
            torch.cuda.synchronize(self._target.device)
            graph = torch.cuda.CUDAGraph()
            with capture_graph(graph):
                self._graph_out = self._step(static)
            self._graph = graph
        self._graph.replay()
        priority, loss = self._graph_out          # graph-owned: valid until the next replay
        if self._ring is not None and loss.dim() == 1:     # the graph left [loss rows | priorities] in a ring slot: no launch here
            slot = self._ring_replays % self._ring.shape[0]
            self._ring_replays += 1
            return priority, self._ring[slot]
        return priority, loss.clone()

    STATS_RING = 1024           # updates whose statistics stay readable (one optimize_policy call enqueues at most this many)

    def _step(self, inputs):
        priority, loss = self._loss_fn(inputs)
        if loss.dim() == 1:                            # per-row losses (the loss is their sum)
            b = loss.numel()
            capturing = loss.is_cuda and torch.cuda.is_current_stream_capturing()
            packed = (priority.dim() == 1 and priority.numel() == b and loss.is_contiguous() and priority.is_contiguous()
                      and priority.data_ptr() == loss.data_ptr() + 4 * b)
            self._pack_rows = b if packed else 0           # (the warm-up calls tell optimize() how wide the ring is)
            if capturing and packed and self._ring is not None and self._ring.shape[1] == 2 * b:
                # inside the graph the statistics of an update are ONE ring append of both rows (the loss's sum and the
                # downsampled priorities are taken from the ring after the update loop: algos/dqn/dqn.py)
                _lib.ring_append(torch.as_strided(loss, (2 * b,), (1,)), self._ring, self._ring_count)
            else:
                loss = loss.sum()
        if self._scale_conv_grads:                     # the conv tensors lead the bucket (optimizers/util.py:122-126)
            self._target.flat_grads[:self._target.grad_split_offset].mul_(float(np.float32(2 ** -0.5)))
        self._apply_update(1.0)
        self._finish_updates(1)
        return priority, loss

    def _stage(self, inputs):
        """Copy one minibatch into the static buffers the graph reads (host arrays -- the importance
        weights -- through a pinned mirror guarded by an event)."""
        dev = self._target.device
        in_place = [isinstance(x, torch.Tensor) and getattr(x, "_arl_static", False) for x in inputs]
        if self._static is None or any(tuple(s.shape) != tuple(np.shape(x)) or (keep and s is not x)
                                       for s, x, keep in zip(self._static, inputs, in_place)):
            assert self._graph is None, "the replay minibatch changed shape or buffers after graph capture"
            self._static, self._pinned = [], []
            for x, keep in zip(inputs, in_place):
                if keep:                                          # the replay buffer's own static outputs
                    self._static.append(x)
                    self._pinned.append(None)
                elif isinstance(x, torch.Tensor):
                    self._static.append(torch.empty_like(x, device=dev))
                    self._pinned.append(None)
                else:
                    x = np.asarray(x, np.float32)
                    self._static.append(torch.empty(x.shape, dtype=torch.float32, device=dev))
                    self._pinned.append(torch.empty(x.shape, dtype=torch.float32).pin_memory())
            self._stage_event = torch.cuda.Event()
        else:
            self._stage_event.synchronize()                       # the previous upload has left the pinned mirrors
        copied = False
        for s, p, x in zip(self._static, self._pinned, inputs):
            if s is x:
                continue
            copied = True
            if p is None:
                s.copy_(x, non_blocking=True)
            else:
                p.copy_(torch.from_numpy(np.asarray(x, np.float32)))
                s.copy_(p, non_blocking=True)
        if copied:
            self._stage_event.record(torch.cuda.current_stream(dev))
        return tuple(self._static)


class FqfOptimizer(DqnOptimizer):
    """DqnOptimizer for a policy whose flat bucket ends in a fraction-proposal layer (AtariFqfPolicy.frac_offset): the
    bucket is updated as two ranges, each with its own ArlOptState, slots, step count and norm log.  [0, frac_offset)
    takes exactly DqnOptimizer's update; the fraction layer takes one arl_opt_step without clipping at its own
    learning_rate / update_method / update_method_args (fraction_args; defaults: the FQF paper's RMSprop, learning rate
    2.5e-9, rho 0.95, epsilon 1e-5).  Both updates sit inside the captured graph."""

    def __init__(self, learning_rate, update_method, update_method_args=None, grad_norm_clip=None,
                 scale_conv_grads=False, use_graph=True, fraction_args=None):
        super().__init__(learning_rate, update_method, update_method_args=update_method_args,
                         grad_norm_clip=grad_norm_clip, scale_conv_grads=scale_conv_grads, use_graph=use_graph)
        from accel_rl_amd.optimizers import update_methods
        frac = sub_args(fraction_args, dict(learning_rate=2.5e-9, update_method=update_methods.rmsprop,
                                            update_method_args=None), TypeError, "unexpected fraction_args: %s")
        self._frac_learning_rate, self._frac_method = frac["learning_rate"], frac["update_method"]
        args = frac["update_method_args"]
        if args is None:
            args = dict(rho=0.95, epsilon=1e-5) if self._frac_method.name == "rmsprop" else dict()
        self._frac_args = self._frac_method.resolve(**args)

    def _setup_bucket(self, target, lr_mult, givens=None):
        off = getattr(target, "frac_offset", None)
        if off is None:
            raise TypeError("FqfOptimizer updates a policy with a fraction layer (AtariFqfPolicy), got %s" %
                            type(target).__name__)
        super()._setup_bucket(target, lr_mult, givens)
        n = target.flat_params.numel() - off
        assert 0 < off and off % 4 == 0 and n > 0
        self._frac_offset = off
        self._opt_state.n_params = off                  # the main range: everything before the fraction layer
        # (norm log of 1: one update per call, _set_updates_per_call(1))
        st = self._new_state(n, target.flat_params, target.flat_grads, self._frac_method, self._lr_mult, 1, first=off)
        self._frac_state = st
        self._frac_slot0, self._frac_slot1, self._frac_step_count = \
            st.tensors["slot0"], st.tensors["slot1"], st.tensors["step_count"]
        self._frac_kernel_args = kernel_args(self._frac_method, self._frac_args)

    def _apply_update(self, avg_factor=1.0):
        super()._apply_update(avg_factor)
        b1, b2, eps = self._frac_kernel_args
        _lib.opt_step(self._frac_state, self._frac_method.kernel_id, self._frac_learning_rate, avg_factor, 0.0, b1, b2, eps)


class SacOptimizer(DqnOptimizer):
    """DqnOptimizer for AtariSacDiscretePolicy: four ranges -- the actor's bucket, the two critics' buckets and log_alpha
    -- each with its own ArlOptState, slots, step count and norm log, each updated by one arl_opt_step inside the
    captured update.  learning_rate, update_method, update_method_args and grad_norm_clip apply to the three networks
    (the clip per network, on that network's own gradient norm); the temperature takes
    alpha_args=dict(learning_rate, update_method, update_method_args) (default: the networks' learning rate and method)
    and is never clipped.  All four gradients were taken at the parameters as they stood before any of the four
    updates (AtariSacDiscretePolicy.sac_loss_and_grads)."""

    def __init__(self, learning_rate, update_method, update_method_args=None, grad_norm_clip=None,
                 scale_conv_grads=False, use_graph=True, alpha_args=None):
        if scale_conv_grads:
            raise NotImplementedError("scale_conv_grads belongs to dueling networks, which SAC-Discrete does not build")
        super().__init__(learning_rate, update_method, update_method_args=update_method_args,
                         grad_norm_clip=grad_norm_clip, scale_conv_grads=False, use_graph=use_graph)
        alpha = sub_args(alpha_args, dict(learning_rate=learning_rate, update_method=update_method,
                                          update_method_args=None), TypeError, "unexpected alpha_args: %s")
        self._alpha_learning_rate, self._alpha_method = alpha["learning_rate"], alpha["update_method"]
        args = alpha["update_method_args"]
        if args is None:                    # the networks' arguments where the method is theirs, else the method's defaults
            args = (update_method_args or dict()) if self._alpha_method is update_method else dict()
        self._alpha_kernel_args = kernel_args(self._alpha_method, self._alpha_method.resolve(**args))

    def _setup_bucket(self, target, lr_mult, givens=None):
        from accel_rl_amd.policies.dqn.atari_sac_discrete_policy import AtariSacDiscretePolicy
        if not isinstance(target, AtariSacDiscretePolicy):
            raise TypeError("SacOptimizer updates an AtariSacDiscretePolicy (actor, two critics, log_alpha), got %s" %
                            type(target).__name__)
        super()._setup_bucket(target, lr_mult, givens)  # the actor: DqnOptimizer's own state
        # (norm logs of 1: one update per call, _set_updates_per_call(1); slots of at least 4 entries)
        self._ranges = [self._opt_state]
        for critic in (target.q1, target.q2):
            n = critic.flat_params.numel()
            self._ranges.append(self._new_state(n, critic.flat_params, critic.flat_grads, self._update_method,
                                                self._lr_mult, 1, slot_len=max(n, 4)))
        self._alpha_state = self._new_state(1, target.log_alpha, target.log_alpha_grad, self._alpha_method,
                                            self._lr_mult, 1, slot_len=4)

    def _apply_update(self, avg_factor=1.0):
        b1, b2, eps = self._kernel_args
        for st in self._ranges:
            _lib.opt_step(st, self._update_method.kernel_id, self._learning_rate, avg_factor, self._grad_norm_clip,
                          b1, b2, eps)
        b1, b2, eps = self._alpha_kernel_args
        _lib.opt_step(self._alpha_state, self._alpha_method.kernel_id, self._alpha_learning_rate, avg_factor, 0.0,
                      b1, b2, eps)
        self._n_updates += 1
