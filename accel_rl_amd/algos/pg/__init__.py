from accel_rl_amd.algos.pg.impala import IMPALA  # noqa: F401
from accel_rl_amd.algos.pg.ppg import PPG  # noqa: F401
from accel_rl_amd.algos.pg.vmpo import VMPO  # noqa: F401
from accel_rl_amd.algos.pg.rnd import RndA2C, RndPPO  # noqa: F401
from accel_rl_amd.algos.pg.acer import ACER  # noqa: F401
from accel_rl_amd.algos.pg.popart import PopArtA2C, PopArtIMPALA, PopArtPPO, PopArtVMPO  # noqa: F401
