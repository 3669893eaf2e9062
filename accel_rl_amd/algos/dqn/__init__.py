from accel_rl_amd.algos.dqn.curl import CURL  # noqa: F401
