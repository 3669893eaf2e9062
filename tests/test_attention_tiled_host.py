"""More than 64 positions in the relational policy, without a GPU: spec 1's own trunk under max_positions, the refusals
-- each raised before a device is touched -- and the argument checks of _lib's tiled attention wrappers."""
import pytest
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies import AtariRelationalPolicy
from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
from accel_rl_amd.spaces import Discrete, EnvSpec, UintBox

SPEC1 = {k: v for k, v in cnn_specs[1].items() if k != "hidden_sizes"}


def test_spec_1_layout():
    policy = AtariRelationalPolicy(**SPEC1, max_positions=128)
    assert policy.positions((4, 104, 80)) == (12, 9)
    assert dict(policy.reference_layout((4, 104, 80), 6)[:-4])["FC0W"] == (108 * 64, 256)


@pytest.mark.parametrize("max_positions", [0, 63, 257, 64.5, True])
def test_constructor_refusals(max_positions):
    with pytest.raises(NotImplementedError, match="section E"):
        AtariRelationalPolicy(max_positions=max_positions)


def test_initialize_refuses_475_positions_before_any_device(monkeypatch):
    def no_device(*a, **kw):
        raise AssertionError("a device tensor was asked for")
    monkeypatch.setattr(torch, "zeros", no_device)
    conv1 = {k: v[:1] for k, v in SPEC1.items()}                # spec 1's first convolution alone: 25 x 19
    with pytest.raises(NotImplementedError, match="25 x 19 positions.*1 .. 256.*section E"):
        AtariRelationalPolicy(**conv1, max_positions=256).initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(6)))


def test_lib_argument_checks():
    assert _lib.ATTN_TILED_MAX_POS == 256
    assert _lib.attn_tiled_shape_ok(256, 4, 64) and _lib.attn_tiled_shape_ok(1, 1, 4)
    assert not any(_lib.attn_tiled_shape_ok(*a) for a in ((257, 1, 4), (0, 1, 4), (8, 1, 6), (8, 5, 64)))
    qkv, out, lse = torch.zeros(2, 70, 3, 2, 4), torch.zeros(2, 70, 8), torch.zeros(2, 2, 70)
    for bad in (dict(qkv=torch.zeros(2, 70, 2, 2, 4)), dict(out=torch.zeros(2, 70, 4)), dict(lse=torch.zeros(2, 70, 2))):
        with pytest.raises(ValueError):
            _lib.attn_tiled_fwd(**dict(dict(qkv=qkv, out=out, lse=lse), **bad))
    with pytest.raises(TypeError):
        _lib.attn_tiled_fwd(qkv.double(), out)
    for call in (lambda: _lib.attn_tiled_bwd(qkv, out, None, out, qkv), lambda: _lib.attn_tiled_bwd(qkv, out, lse, out[:1], qkv)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: _lib.attn_tiled_fwd(qkv, out, lse), lambda: _lib.attn_tiled_bwd(qkv, out, lse, out, qkv)):
        with pytest.raises(RuntimeError, match="no CPU path"):  # shapes fine: the device check
            call()
