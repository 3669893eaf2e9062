"""The relational policy without a GPU: the NumPy restatements of the coordinate kernels (shared with
tests/test_attention_gpu.py), the parameter layout of AtariRelationalPolicy, its refusals -- each raised before a device is
touched -- and the argument checks of _lib's attention wrappers."""
import numpy as np
import pytest
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies import AtariRelationalPolicy
from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
from accel_rl_amd.spaces import Discrete, EnvSpec, UintBox


def coords_fwd32(x):
    """arl_entity_coords_fwd as include/accel_rl_hip.h states it: x f32[B][h][w][C] -> f32[B][h][w][C + 4]."""
    b, h, w, c = x.shape
    axis = lambda n: ((2 * np.arange(n) - (n - 1)).astype(np.float32) / np.float32(n - 1) if n > 1      # noqa: E731
                      else np.zeros(n, np.float32))
    y = np.zeros((b, h, w, c + 4), np.float32)
    y[..., :c] = x
    y[..., c] = axis(w)[None, None, :]
    y[..., c + 1] = axis(h)[None, :, None]
    return y


def coords_bwd32(g, d_y, mask):
    s = (g + d_y[..., :g.shape[3]]).astype(np.float32)
    return s if mask is None else np.where(mask > 0, s, np.float32(0))


def test_default_network_layout():
    policy = AtariRelationalPolicy()
    assert policy.positions((4, 104, 80)) == (9, 7) and not policy.serve_supported()
    layout = policy.reference_layout((4, 104, 80), 6)
    assert [n for n, _ in layout] == ["Conv0W", "Conv0b", "Conv1W", "Conv1b", "Conv2W", "Conv2b", "R0QkvW", "R0Qkvb", "R0OutW",
                                      "R0Outb", "FC0W", "FC0b", "OutputW", "Outputb", "OutputW", "Outputb"]
    shapes = dict(layout[:-4])
    assert shapes["Conv2W"] == (64, 64, 3, 3) and shapes["R0QkvW"] == (192, 68, 1, 1) and shapes["R0OutW"] == (64, 64, 1, 1)
    assert shapes["FC0W"] == (63 * 64, 256)
    two = AtariRelationalPolicy(n_blocks=2, n_heads=1, head_dim=36).reference_layout((4, 104, 80), 6)
    assert dict(two[:-4])["R1QkvW"] == (108, 68, 1, 1) and dict(two[:-4])["R1OutW"] == (64, 36, 1, 1)


@pytest.mark.parametrize("kw", [dict(n_blocks=0), dict(n_blocks=5), dict(n_blocks=1.5), dict(head_dim=0), dict(head_dim=6),
                                dict(head_dim=68), dict(n_heads=0), dict(n_heads=9), dict(n_heads=5, head_dim=64),
                                dict(hidden_sizes=())], ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_constructor_refusals(kw):
    with pytest.raises(NotImplementedError, match="section E"):
        AtariRelationalPolicy(**kw)


def test_initialize_refusals_come_before_any_device(monkeypatch):
    def no_device(*a, **kw):
        raise AssertionError("a device tensor was asked for")
    monkeypatch.setattr(torch, "zeros", no_device)
    spec1 = {k: v for k, v in cnn_specs[1].items() if k != "hidden_sizes"}
    with pytest.raises(NotImplementedError, match="12 x 9 positions.*section E"):       # spec 1 as it stands: 108 > 64
        AtariRelationalPolicy(**spec1).initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(6)))
    with pytest.raises(NotImplementedError, match="positions"):
        AtariRelationalPolicy().initialize(EnvSpec(UintBox((4, 30, 80)), Discrete(6)))      # an empty feature map


def test_lib_argument_checks():
    assert _lib.attn_shape_ok(64, 4, 64) and _lib.attn_shape_ok(1, 1, 4)
    assert not any(_lib.attn_shape_ok(*a) for a in ((65, 1, 4), (0, 1, 4), (8, 1, 6), (8, 1, 68), (8, 0, 4), (8, 5, 64)))
    qkv, out, lse = torch.zeros(2, 5, 3, 2, 4), torch.zeros(2, 5, 8), torch.zeros(2, 2, 5)
    for bad in (dict(qkv=torch.zeros(2, 5, 2, 2, 4)), dict(out=torch.zeros(2, 5, 4)), dict(lse=torch.zeros(2, 5, 2))):
        with pytest.raises(ValueError):
            _lib.attn_fwd(**dict(dict(qkv=qkv, out=out, lse=lse), **bad))
    with pytest.raises(TypeError):
        _lib.attn_fwd(qkv.double(), out)
    x = torch.zeros(1, 2, 3, 4)
    for call in (lambda: _lib.attn_bwd(qkv, out, None, out, qkv), lambda: _lib.attn_bwd(qkv, out, lse, out[:1], qkv),
                 lambda: _lib.entity_coords_fwd(x, torch.zeros(1, 2, 3, 4)),
                 lambda: _lib.entity_coords_bwd(x, torch.zeros(1, 2, 3, 8), torch.zeros(1, 2, 3, 8), x)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError, match="no CPU path"):                                  # shapes fine: the device check
        _lib.entity_coords_fwd(x, torch.zeros(1, 2, 3, 8))
