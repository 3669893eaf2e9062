"""Single-GPU optimizers (reference: accel_rl/optimizers/single/a2c_optimizer.py:11-50,
single/ppo_optimizer.py:11-75)."""
import numpy as np
import torch

from accel_rl_amd import _lib

from accel_rl_amd.optimizers.base import BaseOptimizer, iterate_mb_idxs, iterate_traj_idxs, kernel_args, sub_args


class A2cOptimizer(BaseOptimizer):
    """One gradient step on the whole batch."""

    def __init__(self, learning_rate, update_method, update_method_args=None, grad_norm_clip=None):
        self._set_update_rule(learning_rate, update_method, update_method_args, grad_norm_clip)

    def initialize(self, inputs, losses, constraints, target, givens=None, lr_mult=1):
        self._input_names = list(inputs)
        self._losses = losses
        self._setup_bucket(target, lr_mult, givens)

    def optimize(self, inputs):
        self.prepare_host(len(inputs[0]))
        return self.device_updates(inputs)

    def prepare_host(self, data_length):
        self._set_updates_per_call(1)

    def device_updates(self, inputs):
        minibatch = dict(zip(self._input_names, inputs))
        minibatch["idx"] = None
        loss = self._backward(self._losses, minibatch)
        self._share_grad()
        self._apply_update(self._avg_factor())
        return loss, self._recent_grad_norms(1)


class PpoOptimizer(BaseOptimizer):
    """epochs x minibatches over a batch that stays resident in HBM; minibatch rows
    are selected by host-shuffled index vectors (np.random.shuffle, one
    permutation per epoch, tail dropped -- optimizers/util.py:8-18).

    The minibatch loop (`_minibatches`) is the only one: a subclass says where a minibatch's rows come from
    (`_epoch_minibatches`, `_minibatch`), what runs before a minibatch (`_before_minibatch`), whether the co-run hook is
    offered (`corun_update`) and whether minibatch_size None means the whole batch (`_none_is_whole_batch`)."""

    _none_is_whole_batch = False        # (plain PPO: minibatch_size is required)

    def __init__(self, learning_rate, update_method, update_method_args, epochs, minibatch_size,
                 grad_norm_clip=None, shuffle=True, num_slices=1):
        self._set_update_rule(learning_rate, update_method, update_method_args, grad_norm_clip)
        self._epochs = epochs
        self._minibatch_size = minibatch_size
        self._shuffle = shuffle

    def initialize(self, inputs, losses, constraints, target, givens=None, lr_mult=1):
        self._input_names = list(inputs)
        self._losses = losses
        self._setup_bucket(target, lr_mult, givens)
        self._idx_host = None

    def optimize(self, inputs):
        self.prepare_host(len(inputs[0]))
        return self.device_updates(inputs)

    # Split for hipGraph capture: everything that draws from the host RNG happens in
    # prepare_host(); device_updates() only enqueues static-shape device work.
    def prepare_host(self, data_length):
        """Minibatch permutations for ALL epochs up front, into one (pinned) int32 buffer: same
        RNG consumption order as the reference (np.random.shuffle once per epoch,
        optimizers/util.py:10-11; nothing else draws inside optimize)."""
        if self._minibatch_size is None and self._none_is_whole_batch:
            self._minibatch_size = int(data_length)         # (known at the first call)
        flat = [mb for _ in range(self._epochs) for mb in self._epoch_minibatches(data_length)]
        if self._idx_host is None:
            shape = (max(len(flat), 1), len(flat[0]) if flat else self._minibatch_size)
            self._idx_host = torch.zeros(shape, dtype=torch.int32)
            if torch.cuda.is_available():
                self._idx_host = self._idx_host.pin_memory()
            self._idx_dev = None                            # (its device twin: the first device_updates allocates it)
        self._n_minibatches = len(flat)
        self._set_updates_per_call(len(flat))
        if flat:
            self._idx_host.copy_(torch.from_numpy(np.stack(flat).astype(np.int32)))

    def _epoch_minibatches(self, data_length):
        """One epoch's rows of the index buffer (one draw from the host RNG): here the minibatches' row indices."""
        return iterate_mb_idxs(self._minibatch_size, data_length, self._shuffle)

    def device_updates(self, inputs):
        data = dict(zip(self._input_names, inputs))      # "_f_load": already on the device
        if not self._n_minibatches:
            return [], []
        if self._idx_dev is None:
            self._idx_dev = torch.zeros(tuple(self._idx_host.shape), dtype=torch.int32, device=self._target.device)
        _lib.copy_bytes(self._idx_dev, self._idx_host)
        if self._overlap_allreduce:
            return self._overlapped_minibatches(data)
        corun = self._corun_hook() if self.parallelism_tag == "single" else None

        def plain(mb):
            if corun is not None:
                mb["dense_w_hook"] = corun
            loss = self._backward(self._losses, mb)
            self._share_grad()
            return loss
        return self._minibatches(data, plain)

    def _minibatches(self, data, step):
        """The loop: per minibatch `step(mb)` leaves the (shared) gradient in the bucket and returns the loss, then
        the update."""
        losses = []
        try:
            for k in range(self._n_minibatches):
                self._before_minibatch(k)
                losses.append(step(self._minibatch(data, self._idx_dev[k])))
                self._apply_update(self._avg_factor())
        finally:
            self._hole = None           # (a backward pass that raised leaves no hole behind for the next call)
        return losses, self._recent_grad_norms(self._n_minibatches)

    def _before_minibatch(self, k):
        pass

    def _minibatch(self, data, idx):
        return dict(data, idx=idx)               # the kernels gather the minibatch's rows by idx themselves

    # Multi-GPU (`_overlap_allreduce`, set by the sync optimizers): minibatches are enqueued eagerly -- at ~550 us
    # of device work per minibatch the host stays far ahead, and a hipGraph per minibatch only added its launch
    # latency at every hand-over to RCCL's stream (measured at world size 1: 232 k -> 237 k env-steps/s without
    # the graphs).  The policy reports, through `split_hook`, the point of its backward pass from which the tail
    # of the gradient bucket (dense layers + heads: 98 % of the bytes for spec 1) is final: that tail's
    # all-reduce is issued there and runs on RCCL's stream underneath the conv layers' backward (~60 % of the
    # minibatch); the small head of the bucket follows, and the optimiser step waits for both.
    _overlap_allreduce = False

    def _overlapped_minibatches(self, data):
        def overlapped(mb):
            pending = []
            mb["split_hook"] = lambda: pending.append(self._share_grad_async(tail=True))
            loss = self._backward(self._losses, mb)
            pending.append(self._share_grad_async(tail=False) if pending else self._share_grad_async(None))
            self._wait_all(pending)
            return loss
        return self._minibatches(data, overlapped)

    @staticmethod
    def _wait_all(pending):
        for work in pending:
            if work is not None:
                work.wait()

    def _share_grad_async(self, tail):
        """All-reduce of the gradient bucket's tail (True), head (False) or all of it (None); a Work or None."""
        return None


class VtraceOptimizer(PpoOptimizer):
    """PpoOptimizer whose every epoch starts with a call back into the algorithm: `_epoch_hook(epoch)` runs before the
    first minibatch of each epoch, epoch 0 included (IMPALA recomputes its V-trace targets there from the parameters as
    they stand, into the tensors the minibatches gather from).  That is the one difference in the loop; besides it,
    minibatch_size None = the whole batch, one update per epoch, and the co-run hook is not offered."""

    _epoch_hook = None          # set by the algorithm (IMPALA.initialize); None: plain PpoOptimizer epochs
    _none_is_whole_batch = True
    corun_update = False

    def _before_minibatch(self, k):
        per_epoch = self._n_minibatches // self._epochs
        if k % per_epoch == 0 and self._epoch_hook is not None:
            self._epoch_hook(k // per_epoch)


class VmpoOptimizer(PpoOptimizer):
    """PpoOptimizer that also owns V-MPO's duals (eta, alpha).  The one difference in the loop: after the network's
    step of every minibatch, one arl_vmpo_dual_step moves both on the gradients the minibatch left behind -- temp4[1]
    (arl_vmpo_weights, which the algorithm points at `temp4`) and eps_alpha - loss4[2] (the head's mean KL) -- and
    projects them onto x >= 1e-8.  `duals`, their optimiser slots, their step count and `temp4` are allocated at
    initialize(), so a captured graph keeps its addresses.  dual_args = dict(learning_rate, update_method,
    update_method_args), each defaulting to the network's; the learning-rate multiplier is the network's.
    minibatch_size None = the whole batch."""

    _none_is_whole_batch = True

    def __init__(self, learning_rate, update_method, update_method_args, epochs, minibatch_size, dual_args=None,
                 dual_init=(1.0, 5.0), eps_alpha=0.005, **kwargs):
        super().__init__(learning_rate, update_method, update_method_args, epochs, minibatch_size, **kwargs)
        given = dict(dual_args or dict())
        if "update_method" in given:                # (another rule does not inherit the network's arguments)
            given.setdefault("update_method_args", dict())
        dual = sub_args(given, dict(learning_rate=learning_rate, update_method=update_method,
                                    update_method_args=update_method_args), ValueError,
                        "dual_args: unknown keys %s (learning_rate, update_method, update_method_args)")
        self._dual_lr, self._dual_method = dual["learning_rate"], dual["update_method"]
        self._dual_kernel_args = kernel_args(self._dual_method,
                                             self._dual_method.resolve(**(dual["update_method_args"] or dict())))
        self.dual_init = (float(dual_init[0]), float(dual_init[1]))
        self.eps_alpha = float(eps_alpha)

    def initialize(self, inputs, losses, constraints, target, givens=None, lr_mult=1):
        super().initialize(inputs, losses, constraints, target, givens=givens, lr_mult=lr_mult)
        dev = target.device
        self.duals = torch.tensor(self.dual_init, dtype=torch.float32, device=dev)
        self.temp4 = torch.zeros(4, dtype=torch.float32, device=dev)
        self._dual_slot0 = torch.zeros(2, dtype=torch.float32, device=dev)
        self._dual_slot1 = torch.zeros(2, dtype=torch.float32, device=dev) if self._dual_method.name == "adam" else None
        self._dual_step_count = torch.zeros(1, dtype=torch.float32, device=dev)
        self._loss4 = None

    def _backward(self, losses, minibatch):
        self._loss4 = losses(minibatch)             # (pi_loss, v_loss, mean KL, their sum): the dual step reads [2]
        return self._loss4[3]

    def _apply_update(self, avg_factor=1.0):
        super()._apply_update(avg_factor)
        b1, b2, eps = self._dual_kernel_args
        _lib.vmpo_dual_step(self.duals, self._dual_slot0, self._dual_slot1, self._dual_step_count, self._lr_mult,
                            self.temp4, self._loss4, self.eps_alpha, self._dual_method.kernel_id, self._dual_lr, b1, b2,
                            eps)


class AcerOptimizer(PpoOptimizer):
    """PpoOptimizer that also moves ACER's average network.  The one difference in the loop: after the network's step of
    every update, one arl_acer_avg_step moves the target's second bucket (`flat_target`, the average network) towards the
    parameters: avg = alpha avg + (1 - alpha) params.  `whole_batch_update` is one more update of the same kind -- the same
    slots and step count -- on data that is not the call's own (ACER's replayed trajectories); it needs a norm clip (the
    clip-free update closes its step count and norm log once per call, _finish_updates) and says so.  minibatch_size None = the
    whole batch; the co-run hook is not offered."""

    _none_is_whole_batch = True
    corun_update = False

    def __init__(self, learning_rate, update_method, update_method_args, epochs, minibatch_size, avg_alpha=0.99, **kwargs):
        super().__init__(learning_rate, update_method, update_method_args, epochs, minibatch_size, **kwargs)
        if not (isinstance(avg_alpha, (int, float, np.floating)) and 0 <= avg_alpha <= 1):
            raise ValueError("avg_alpha must lie in [0, 1], got %r" % (avg_alpha,))
        self.avg_alpha = float(avg_alpha)

    def _apply_update(self, avg_factor=1.0):
        super()._apply_update(avg_factor)
        _lib.acer_avg_step(self._target.flat_target, self._target.flat_params, self.avg_alpha)

    def whole_batch_update(self, inputs):
        """One update on all rows of `inputs` (the tuple order of initialize's names), no index; returns the loss."""
        if self._grad_norm_clip is None:
            raise NotImplementedError("whole_batch_update needs grad_norm_clip: the clip-free update is closed once per "
                                      "call (_finish_updates)")
        mb = dict(zip(self._input_names, inputs))
        mb["idx"] = None
        loss = self._backward(self._losses, mb)
        self._apply_update(self._avg_factor())
        return loss


class TrajPpoOptimizer(PpoOptimizer):
    """PPO for recurrent policies: epochs x minibatches of WHOLE trajectory segments (optimizers/util.py:21-32,
    iterate_traj_idxs; the reference's own PpoOptimizer slices rows and cuts trajectories apart).  `minibatch_size`
    keeps the reference's meaning -- rows -- so a minibatch is `minibatch_size // horizon` segments.  The one difference
    from PpoOptimizer: the index buffer holds segment numbers, not rows (one np.random.shuffle of the segments per
    epoch), and per minibatch one arl_traj_minibatch launch builds the row indices, the segments' stored initial states
    and 1 / sum(valids) on the device; the policy's forward / BPTT runs on those rows.  Static shapes, no host
    synchronisation: captured like PpoOptimizer's call."""

    trajectory_minibatches = True       # AdvActorCriticBase.initialize lets a recurrent policy through
    corun_update = False                # (a feed-forward-policy feature: the recurrent backward pass offers no hole)

    def initialize(self, inputs, losses, constraints, target, givens=None, lr_mult=1, horizon=None, data_length=None):
        if horizon is None or data_length is None:
            raise TypeError("TrajPpoOptimizer.initialize needs horizon and data_length (the algorithm passes them)")
        self._horizon = int(horizon)
        self.check_sizes(self._minibatch_size, int(data_length), self._horizon)
        super().initialize(inputs, losses, constraints, target, givens=givens, lr_mult=lr_mult)

    @staticmethod
    def check_sizes(minibatch_size, data_length, horizon):
        """iterate_traj_idxs' own condition, checked before the first update, with the numbers."""
        if horizon < 1 or minibatch_size < horizon or data_length % horizon or minibatch_size % horizon or \
                data_length % minibatch_size:
            raise ValueError("trajectory minibatches: minibatch_size (%d) and the batch (%d rows) must be multiples of "
                             "horizon (%d), and the batch a multiple of minibatch_size" %
                             (minibatch_size, data_length, horizon))

    def _epoch_minibatches(self, data_length):
        """The segment numbers of one epoch's minibatches: the same RNG consumption as the reference function."""
        return [segs for _, segs in iterate_traj_idxs(self._minibatch_size, data_length, self._horizon, self._shuffle)]

    def _minibatch(self, data, seg):
        """One arl_traj_minibatch launch: traj_idx, traj_state and inv_count of the chosen segments."""
        return self._target.traj_minibatch(dict(data, idx=None, traj=seg, horizon=self._horizon))
