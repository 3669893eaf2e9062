"""Rainbow (Hessel et al. 2018) with noisy nets: categorical + dueling + double DQN, 3-step returns, prioritized replay,
and exploration through the network's learned noise only -- the epsilon schedule is 0 throughout.  The reference stops
at EpsRainbow (accel_rl/algos/dqn/eps_rainbow.py:8-11: "Rainbow minus NoisyNets ... (NoisyNets are slow)"); here the
noise is drawn on the device inside the captured rollout and update graphs.  Every other default is EpsRainbow's.
Use with AtariNoisyNetCatDqnPolicy(dueling=True)."""
from accel_rl_amd.algos.dqn.eps_rainbow import EpsRainbow
from accel_rl_amd.policies.dqn.atari_noisy_net_cat_dqn_policy import AtariNoisyNetCatDqnPolicy


class Rainbow(EpsRainbow):

    def _get_default_sub_args(self):
        opt_args, _, priority_args = super()._get_default_sub_args()
        eps_greedy_args = dict(initial=0., final=0., eval=0., anneal_steps=1)
        return opt_args, eps_greedy_args, priority_args

    def build_loss(self, env_spec, policy):
        if not isinstance(policy, AtariNoisyNetCatDqnPolicy):
            raise TypeError("Rainbow explores through noisy nets: it needs an AtariNoisyNetCatDqnPolicy, got %s "
                            "(for epsilon-greedy exploration use EpsRainbow)" % type(policy).__name__)
        if bool(self.dueling_dqn) != bool(policy._dueling):
            raise ValueError("Rainbow(dueling_dqn=%s) needs AtariNoisyNetCatDqnPolicy(dueling=%s)" %
                             (bool(self.dueling_dqn), bool(self.dueling_dqn)))
        return super().build_loss(env_spec, policy)
