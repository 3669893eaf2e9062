from accel_rl_amd.policies.dqn.atari_curl_dqn_policy import AtariCurlDqnPolicy  # noqa: F401
