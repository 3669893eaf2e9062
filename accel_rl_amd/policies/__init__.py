from accel_rl_amd.policies.atari_relational_policy import AtariRelationalPolicy  # noqa: F401
