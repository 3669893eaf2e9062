from accel_rl_amd.algos.pg.impala import IMPALA  # noqa: F401
