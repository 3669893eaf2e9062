from accel_rl_amd.policies.atari_relational_policy import AtariRelationalPolicy  # noqa: F401
from accel_rl_amd.policies.atari_attn_memory_policy import AtariAttnMemoryPolicy  # noqa: F401
from accel_rl_amd.policies.atari_lru_policy import AtariLruPolicy  # noqa: F401
