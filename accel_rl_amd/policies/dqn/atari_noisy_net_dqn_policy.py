"""Noisy-net DQN policy for Atari: conv stack -> noisy dense layers -> one Q value per action; a target network;
exploration through learned per-weight noise scales instead of epsilon-greedy.

Mirror of the reference's AtariNoisyNetDqnPolicy / NoisyNetDqnCnn / NoisyDenseLayer
(accel_rl/policies/dqn/atari_noisy_net_dqn_policy.py:20-148, policies/dqn/networks/noisy_net_dqn_cnn.py:11-137,
policies/dqn/layers/noisy_layer.py:15-147; the reference's policy file imports a network module that does not exist,
the network built here is NoisyNetDqnCnn).  Every hidden dense layer and the output layer "output_q" is a noisy layer:
the layer, its forward walk, backward pass, generator, parameter order and initial draws are NoisyLayers'
(policies/dqn/noisy_layers.py).  What is this policy's own: the output layer is AtariDqnPolicy's, n_actions units
padded to 32 rows, and the pass's noise is one arl_noisy_noise launch, whose `out_stride` zero-pads f(e_out) of that
layer.

Not built: factorized=False (per-row independent noise, B x fan_in x units normals per
call), dueling and shared-bias variants (the reference has none; noisy dueling and categorical networks:
AtariNoisyNetCatDqnPolicy), a noisy Munchausen agent.
"""
from accel_rl_amd import _lib
from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
from accel_rl_amd.policies.dqn.noisy_layers import NoisyLayers


class AtariNoisyNetDqnPolicy(NoisyLayers, AtariDqnPolicy):

    def __init__(self, conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=(), pixel_scale=255.,
                 epsilon=1, factorized=True, common_noise=False, sigma_0=0.4, use_mu_init=True,
                 initial_param_values=None, dueling=False, shared_last_bias=False):
        self._set_noisy(factorized, common_noise, sigma_0, use_mu_init)
        if dueling or shared_last_bias:
            raise NotImplementedError("noisy dueling / shared-bias networks are not built (INTEGRATION.md, section E)")
        super().__init__(conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=hidden_sizes,
                         pixel_scale=pixel_scale, epsilon=0, initial_param_values=initial_param_values)

    def _head_reference_init(self, fan, n_act):
        self._q_stride = (n_act + 31) // 32 * 32
        return list(self._out_ref), ["OutputW", "Outputb"]                # output_q (noisy_net_dqn_cnn.py:78-89)

    def _draw_noise(self, x_c, layers, b, tag):
        """One arl_noisy_noise launch: every layer's f(e_in), f(e_out) and the first one's x * f(e_in)."""
        units = [hs for hs, _ in self._hid_geom] + [self.n_act]
        _lib.noisy_noise(self._noise_state,
                         [(fein, feout, x_c if l == 0 else None, xs, fein.shape[1], units[l], feout.shape[1], l)
                          for l, (fein, feout, xs) in enumerate(layers)],
                         b, self._rows_per_draw(b, tag))

    def munchausen_loss_and_grads(self, *args, **kwargs):
        raise NotImplementedError("a noisy Munchausen agent is not built (INTEGRATION.md, section E)")
